"""The K-sample importance-weighted bound end to end on the MI355X: the three eval_minibatch functions with num_samples
against the same objective in float64 (built here from oracle.torch_cpu_step.encoder / decoder with autograd), dp.TrainStep
with num_samples under two ranks, num_samples=1 against the call without the keyword, and one resumed command-line run.
The kernels on their own are tests/test_gpu_iw_kernels.py; the host side is tests/test_iw_cpu.py."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import cases
from helpers import rel_err
from iw_ref import iw_latent_formulas
from test_gpu_resume import _SMALL, _assert_same_state_files, _cli, _sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_G = 2e-5, 1e-4
B, SIDE, HID = 3, 12, 64
N = SIDE * SIDE


def _images(script, rs):
    """Three images nothing alike, so that a row decoded against another image's target or encoder output moves every
    number far beyond the tolerances: a dark one, a bright one, and one bright on its left half only."""
    C = 3 if script == "galaxy" else 1
    col = np.arange(N) % SIDE
    level = np.stack([np.full(N, 0.1), np.full(N, 0.9), np.where(col < SIDE // 2, 0.95, 0.05)])[:, :, None]
    y = np.clip(level + 0.05 * rs.normal(size=(B, N, C)), 0.0, 1.0)
    if script == "particles":
        return ((y[:, :, 0] - 0.5) * np.array([[1.0], [3.0], [6.0]])).astype(np.float32)
    return (y if script == "galaxy" else y[:, :, 0]).astype(np.float32)


def _reference(script, pp, qp, x, y, y_enc, r, K, offset, mask, ctf, dx_scale, theta_prior, z_scale):
    """(bound, log_p, kl) in the dtype of the parameters: encode once per image, K samples, rotate and shift the grid per
    sample (train_mnist.py:42-72), decode, score each sample against ITS image, log-mean-exp over an image's samples."""
    from oracle import torch_cpu_step as T
    z_mu, z_logstd = T.encoder(qp, y_enc.reshape(B, -1), "tanh", False)
    theta, dx, zc, log_ratio = iw_latent_formulas(torch.cat([z_mu, z_logstd], 1), r, K, True, True, script == "mnist",
                                                  dx_scale, z_scale, theta_prior)
    if offset is not None:
        theta = theta + offset.repeat_interleave(K)
    rot = torch.stack([torch.stack([torch.cos(theta), torch.sin(theta)], 1),
                       torch.stack([-torch.sin(theta), torch.cos(theta)], 1)], 1)
    xb = torch.bmm(x.expand(B * K, N, 2), rot) + dx.unsqueeze(1)
    y_hat = T.decoder(pp, xb.contiguous(), zc, "tanh").reshape(B * K, -1)
    target = y.repeat_interleave(K, 0).reshape(B * K, -1)
    if script == "particles":
        k = ctf.shape[-1]
        y_mu = F.conv2d(y_hat.reshape(1, B * K, SIDE, SIDE), ctf.repeat_interleave(K, 0), padding=k // 2, groups=B * K)
        diff = (y_mu.reshape(B * K, N) - target)[:, mask]
        loglik = -0.5 * (diff ** 2).sum(1)
    else:
        loglik = -F.binary_cross_entropy(y_hat, target, reduction="none").sum(1)
    bound = (torch.logsumexp((loglik + log_ratio).view(B, K), 1) - math.log(K)).mean()
    return bound, loglik.mean(), -log_ratio.mean(), y_hat


CASES = {"mnist": dict(K=4, z_dim=2, dx_scale=0.1, theta_prior=math.pi / 4, z_scale=1.0),
         "galaxy": dict(K=3, z_dim=3, dx_scale=0.1, theta_prior=math.pi, z_scale=0.5),
         "particles": dict(K=2, z_dim=2, dx_scale=0.2, theta_prior=0.5, z_scale=1.0)}


@pytest.mark.parametrize("script", sorted(CASES))
def test_eval_minibatch_with_samples_matches_float64(script):
    """eval_minibatch_mnist K = 4; eval_minibatch_galaxy K = 3 (C = 3, z_scale 0.5, augmentation with given angles: the images
    the encoder sees are oracle.pil_rotate's, the angle is added back to every sample's theta); eval_minibatch_particles
    K = 2 (CTF 5 x 5 per image, circular mask).  B = 3 unlike images of 12 x 12, hidden 64, two layers.  The three scalars to
    2e-5, y_hat of all B*K rows to 2e-5, every p_net and q_net gradient to 1e-4 of its largest entry.
    MI355X: scalars at most 5.8e-8, rows 1.3e-7, worst gradient 2.8e-6 (particles, p.latent_linear.weight)."""
    import spatial_vae.models as models
    from oracle import pil_rotate
    from spatial_vae_amd import elbo as E
    c = CASES[script]
    K, C = c["K"], 3 if script == "galaxy" else 1
    inf = c["z_dim"] + 3
    dev = torch.device("cuda:0")
    rs = np.random.RandomState({"mnist": 1, "galaxy": 2, "particles": 3}[script])
    torch.manual_seed(40 + K)
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(c["z_dim"], HID, n_out=C, num_layers=2, activation=nn.Tanh).to(dev)
        q_net = models.InferenceNetwork(N * C, inf, 32, num_layers=2, activation=nn.Tanh).to(dev)
    with torch.no_grad():                               # default initialisation leaves log-std near 0 and mu small: widen both
        last = [m for m in q_net.layers if isinstance(m, nn.Linear)][-1]
        last.bias.copy_(torch.from_numpy(np.concatenate([rs.uniform(-1, 1, inf), rs.uniform(-2.5, -0.5, inf)]).astype(np.float32)))
    y_np = _images(script, rs)
    r_np = rs.normal(size=(B * K, inf)).astype(np.float32)
    x_np = cases.coord_grid(SIDE, SIDE).astype(np.float32)
    offset = mask = ctf = None
    y_enc = y_np
    kw = dict(rotate=True, translate=True, dx_scale=c["dx_scale"], theta_prior=c["theta_prior"], num_samples=K,
              noise=torch.from_numpy(r_np).to(dev))
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    if script == "mnist":
        out = E.eval_minibatch_mnist(x, y, p_net, q_net, **kw)
    elif script == "galaxy":
        offset = np.array([0.7, 2.9, 5.1])
        y_enc = pil_rotate.augment_galaxy(y_np, offset)
        out = E.eval_minibatch_galaxy(x, y, p_net, q_net, z_scale=c["z_scale"], augment_rotation=True, offset=offset, **kw)
    else:
        ctf = (rs.normal(size=(B, 1, 5, 5)) / 5).astype(np.float32)
        ctf[:, 0, 2, 2] += 1.0
        rr, cc = np.divmod(np.arange(N), SIDE)
        mask = (rr - 5.5) ** 2 + (cc - 5.5) ** 2 <= 30.0
        out = E.eval_minibatch_particles(x, y, torch.from_numpy(mask).to(dev), torch.from_numpy(ctf).to(dev), p_net, q_net,
                                         z_scale=c["z_scale"], return_logits=True, **kw)
    (-out[0]).backward()
    torch.cuda.synchronize()
    f64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    pp = {k: v.detach().cpu().double().requires_grad_(True) for k, v in p_net.state_dict().items()}
    qp = {k: v.detach().cpu().double().requires_grad_(True) for k, v in q_net.state_dict().items()}
    sc = [float(np.float32(c[k])) for k in ("dx_scale", "theta_prior", "z_scale")]
    ref = _reference(script, pp, qp, f64(x_np), f64(y_np), f64(y_enc), f64(r_np), K, None if offset is None else f64(np.float32(offset)),
                     None if mask is None else torch.from_numpy(mask), None if ctf is None else f64(ctf), *sc)
    (-ref[0]).backward()
    got = [float(v.detach()) for v in out[:3]]
    want = [float(v.detach()) for v in ref[:3]]
    errs = [abs(g - w) / max(abs(w), 1.0 if i == 2 else 0.0) for i, (g, w) in enumerate(zip(got, want))]
    rows = out[3]                                       # y_hat (mnist, galaxy) or the decoder's pre-Sigmoid output (particles)
    assert rows.shape[0] == B * K
    e_rows = rel_err(rows.detach().cpu().numpy().reshape(B * K, -1), ref[3].detach().numpy()) if script != "particles" else 0.0
    g_err = {}
    for net, params, tag in ((p_net, pp, "p."), (q_net, qp, "q.")):
        for name, p in net.named_parameters():
            g_err[tag + name] = rel_err(p.grad.cpu().numpy(), params[name].grad.numpy())
    print("iw_step %s K%d scalars %s want %s errs %s rows %.2e worst grad %.2e (%s)" % (
        script, K, got, want, ["%.1e" % e for e in errs], e_rows, max(g_err.values()), max(g_err, key=g_err.get)))
    assert want[0] > want[1] - want[2] + 1e-3 * abs(want[0]) or K == 1      # the bound is not log_p - kl here
    assert all(e <= TOL for e in errs), (got, want)
    assert e_rows <= TOL
    assert all(e <= TOL_G for e in g_err.values()), g_err


def _step(dev, **kw):
    import spatial_vae.models as models
    from spatial_vae_amd import dp, elbo as E
    torch.manual_seed(9)
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(2, HID, num_layers=2, activation=nn.Tanh).to(dev)
        q_net = models.InferenceNetwork(N, 5, 32, num_layers=2, activation=nn.Tanh).to(dev)
    return dp.TrainStep(p_net, q_net, E.eval_minibatch_mnist, lr=1e-2, rotate=True, translate=True, dx_scale=0.1,
                        theta_prior=math.pi / 4, **kw)


def test_num_samples_one_is_the_call_without_the_keyword():
    """Three TrainStep updates with num_samples=1 (given to TrainStep, and given per call) against three without the keyword,
    same seeds and data: parameters, moments' effect and metrics equal bit for bit -- K = 1 takes the one-sample path.
    MI355X: equal."""
    from spatial_vae_amd import cli
    dev = torch.device("cuda:0")
    x = cli.coord_grid(SIDE, SIDE).to(dev)
    rs = np.random.RandomState(3)
    ys = [torch.from_numpy(rs.uniform(size=(b, N)).astype(np.float32)).to(dev) for b in (5, 4, 5)]
    rn = [torch.from_numpy(rs.normal(size=(b, 5)).astype(np.float32)).to(dev) for b in (5, 4, 5)]
    results = []
    for ctor, call in (({}, {}), ({"num_samples": 1}, {}), ({}, {"num_samples": 1})):
        step = _step(dev, **ctor)
        met = []
        for y, r in zip(ys, rn):
            step(x, y, noise=r, **call)
            met.append(step.metrics.clone())
        results.append((step.grads.flat_param.detach().cpu(), torch.stack(met).cpu()))
    for flat, met in results[1:]:
        assert torch.equal(flat, results[0][0]) and torch.equal(met, results[0][1])
    assert not torch.equal(results[0][0], _step(dev).grads.flat_param.detach().cpu())      # and the parameters did move


_DP_WORKER = r'''
import contextlib, io, math, os, sys
sys.path.insert(0, os.environ["SVAE_ROOT"])
import numpy as np, torch, torch.nn as nn, torch.distributed as dist
import spatial_vae.models as models
from spatial_vae_amd import dp, elbo as E, cli

K = 4
rank, world, local = dp.init_process_group(device_is_gpu=True)
dev = torch.device("cuda", local)
torch.cuda.set_device(dev)
torch.manual_seed(100 + rank)                       # rank 0's weights must win
with contextlib.redirect_stdout(io.StringIO()):
    p_net = models.SpatialGenerator(2, 64, num_layers=2, activation=nn.Tanh).to(dev)
    q_net = models.InferenceNetwork(144, 5, 32, num_layers=2, activation=nn.Tanh).to(dev)
step = dp.TrainStep(p_net, q_net, E.eval_minibatch_mnist, lr=1e-2, rotate=True, translate=True, dx_scale=0.1,
                    theta_prior=math.pi / 4, num_samples=K)
dp.shared_seed(dev)
x = cli.coord_grid(12, 12).to(dev)
rs = np.random.RandomState(7)
level = np.array([0.1, 0.9, 0.5, 0.3, 0.7])[:, None]
ys = [torch.from_numpy(np.clip(level + 0.2 * rs.normal(size=(5, 144)), 0, 1).astype(np.float32)).to(dev) for _ in range(3)]
noise = [torch.from_numpy(rs.normal(size=(5 * K, 5)).astype(np.float32)).to(dev) for _ in range(3)]
metrics = []
for y, r in zip(ys, noise):
    lo, hi = (0, 5) if world == 1 else ((0, 3), (3, 5))[rank]          # shards by image; noise rows [lo*K, hi*K)
    step(x, y[lo:hi], weight=(hi - lo) / 5, global_batch=5, noise=r[lo * K:hi * K])
    metrics.append(step.metrics.clone())
torch.cuda.synchronize()
flat, met = step.grads.flat_param.detach().cpu(), torch.stack(metrics).cpu()
if world == 1:
    torch.save({"flat": flat, "metrics": met}, os.environ["SVAE_DP_REF"])
    print("reference written", met[0].tolist())
else:
    ref = torch.load(os.environ["SVAE_DP_REF"], weights_only=True)
    both = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(both, flat)
    assert torch.equal(both[0], both[1]), "replicas diverged"
    perr = (flat - ref["flat"]).abs().max().item() / ref["flat"].abs().max().item()
    merr = ((met - ref["metrics"]).abs().max(1).values / ref["metrics"].abs().max(1).values).max().item()
    print("rank", rank, "param err %.3e metric err %.3e" % (perr, merr))
    assert perr < 2e-6 and merr < 2e-6, (perr, merr)
    dist.destroy_process_group()
'''


def test_two_ranks_with_four_samples_match_the_single_rank_run(tmp_path):
    """dp.TrainStep(num_samples=4), three updates on global minibatches of 5 images: two ranks sharing the GPU with 3 + 2
    images (noise rows [0, 12) and [12, 20) of the one global draw) against one rank.  Replicas bit-equal; parameters and the
    three metrics of every step within 2e-6.  MI355X: parameters 2.0e-7, metrics 7.6e-8 on both ranks."""
    script = tmp_path / "iw_dp_worker.py"
    script.write_text(_DP_WORKER)
    env = dict(os.environ, SVAE_ROOT=ROOT, SVAE_DP_REF=str(tmp_path / "ref.pt"), PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_SHARE_GPU", "SVAE_DP_BUCKETS", "SVAE_DP_LOWRANK"):
        env.pop(k, None)
    one = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stdout[-1500:] + one.stderr[-3000:]
    env["SVAE_SHARE_GPU"] = "1"
    code = ("import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
            "sys.exit(dp.launch_ranks(2, [%r], timeout=240))" % (ROOT, str(script)))
    two = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stdout[-1500:] + two.stderr[-3000:]
    lines = [l for l in two.stdout.splitlines() if l.startswith("rank")]
    print(one.stdout.strip().splitlines()[-1], lines)
    assert len(lines) == 2, lines


def test_resumed_run_with_samples_is_the_uninterrupted_run(tmp_path):
    """train_mnist.py --synthetic 200 --num_samples 3 --eval_num_samples 5 (minibatches of 64: a ragged last one of 8), four
    epochs, against the same run resumed from its epoch-2 state file: the rows of epochs 3 and 4 are the same strings, the
    final modules and state files (parameters, moments, step count, generator states) equal exactly.  MI355X: equal."""
    args = ["--synthetic", "200", "--seed", "5", "--minibatch_size", "64", "--num_samples", "3", "--eval_num_samples", "5"] + _SMALL
    cwd = str(tmp_path)
    a = _cli("train_mnist.py", args + ["--save_prefix", "a"], cwd)
    base = lambda p: str(tmp_path / ("outputs_" + p) / "trained" / p)
    stored = torch.load(base("a") + "_state_epoch2.ckpt", weights_only=True)["args"]
    assert stored["num_samples"] == 3 and stored["eval_num_samples"] == 5
    b = _cli("train_mnist.py", args + ["--save_prefix", "b", "--resume", base("a") + "_state_epoch2.ckpt"], cwd)
    assert len(a) == 1 + 8 and len(b) == 1 + 4 and a[0] == b[0]
    assert a[5:] == b[1:], (a[5:], b[1:])
    for f in ("train.txt", "val.txt"):
        assert (tmp_path / "outputs_a" / f).read_bytes() == (tmp_path / "outputs_b" / f).read_bytes(), f
    for tag in ("generator", "inference"):
        sa, sb = _sd(base("a") + "_%s_epoch4.sav" % tag), _sd(base("b") + "_%s_epoch4.sav" % tag)
        assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), tag
    _assert_same_state_files(base("a") + "_state_epoch4.ckpt", base("b") + "_state_epoch4.ckpt")
    # the bound beats the one-sample ELBO it generalises: column 1 is not column 2's negative minus column 3 any more
    e, g, k = (float(v) for v in a[-1].split("\t")[1:])
    assert e > -g - k
