"""The gradient guard (global-norm clipping, skipping a non-finite step) without a GPU: dp.TrainStep on the CPU path, where
torch.optim.Adam steps and the guard is spelt in torch ops, against plain modules + torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam; two gloo ranks; the flags, their place in state files, and a resumed command-line run.  The device form
(svae_grad_guard_norm / svae_adam_step_guarded) is tests/test_gpu_grad_guard.py."""
import argparse
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy_elbo(x, y, p_net, q_net, noise=None):
    q = q_net(y)
    mu, logstd = q[:, :2], q[:, 2:]
    z = mu + logstd.exp() * noise
    y_hat = p_net(z)
    log_p = -((y_hat - y) ** 2).sum(1).mean()
    kl = (-logstd + 0.5 * logstd.exp() ** 2 + 0.5 * mu ** 2 - 0.5).sum(1).mean()
    return log_p - kl, log_p, kl


def _toy_nets(seed):
    torch.manual_seed(seed)
    return (nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 5)),
            nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 4)))


def _packed(step):
    """The flat parameter buffer without its alignment gaps, in parameter order."""
    return torch.cat([step.grads.flat_param[o:o + p.numel()] for p, o in zip(step.grads.params, step.grads.offsets)]).detach()


def _ref_packed(nets):
    return torch.cat([p.detach().reshape(-1) for net in nets for p in net.parameters()])


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def test_trainstep_clips_like_clip_grad_norm_and_skips_a_nan_step_on_cpu():
    from spatial_vae_amd import dp
    gen = torch.Generator().manual_seed(11)
    sizes = (8, 5, 7, 6, 4, 8)
    ys = [torch.randn(b, 5, generator=gen) for b in sizes]
    rs = [torch.randn(b, 2, generator=gen) for b in sizes]
    # the threshold: half the first step's gradient norm, measured on plain modules -- that step certainly clips
    probe = _toy_nets(1)
    (-_toy_elbo(None, ys[0], *probe, noise=rs[0])[0]).backward()
    first = torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for net in probe for p in net.parameters()])).item()
    max_norm = 0.5 * first

    step = dp.TrainStep(*_toy_nets(1), _toy_elbo, lr=1e-2, clip_grad_norm=max_norm)
    assert step.guarded and isinstance(step.optim, torch.optim.Adam)
    ref = _toy_nets(1)
    params = [p for net in ref for p in net.parameters()]
    opt = torch.optim.Adam(params, lr=1e-2)
    norms = []

    def ref_step(y, r):
        opt.zero_grad()
        (-_toy_elbo(None, y, *ref, noise=r)[0]).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()

    for y, r in zip(ys[:4], rs[:4]):
        step(None, y, noise=r)
        ref_step(y, r)
    err = _rel(_packed(step), _ref_packed(ref))
    print("4 clipped steps: rel err %.3e, reference norms %s, threshold %.4g" % (err, norms, max_norm))
    assert err < 1e-6, err

    # a step whose gradient is not finite: nothing but the gradient buffer and the statistics may change
    st = step.optim.state[step.master]
    before = (step.grads.flat_param.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"]))
    bad = ys[4].clone()
    bad[1, 2] = float("nan")
    step(None, bad, noise=rs[4])
    assert torch.equal(step.grads.flat_param, before[0])
    assert torch.equal(st["exp_avg"], before[1]) and torch.equal(st["exp_avg_sq"], before[2])
    assert float(st["step"]) == before[3] == 4.0 and step.state_dict()["step"] == 4
    assert float(step.grads.flat.abs().max()) == 0.0 and step.aliased()

    # and the next clean step is the reference's next real step
    step(None, ys[5], noise=rs[5])
    ref_step(ys[5], rs[5])
    err = _rel(_packed(step), _ref_packed(ref))
    assert err < 1e-6, err
    assert float(st["step"]) == 5.0
    stats = step.guard_stats()
    clipped = sum(n > max_norm for n in norms)
    assert stats["steps"] == 6 and stats["skipped"] == 1 and stats["clipped"] == clipped >= 1
    assert abs(stats["max_norm"] - max(norms)) <= 1e-5 * max(norms)
    assert abs(stats["mean_norm"] - sum(norms) / len(norms)) <= 1e-5 * max(norms)
    assert step.guard_stats(reset=True) == stats and step.guard_stats()["steps"] == 0


def test_skip_nonfinite_alone_never_clips_and_inf_counts_as_nonfinite():
    from spatial_vae_amd import dp
    gen = torch.Generator().manual_seed(3)
    y, r = torch.randn(6, 5, generator=gen), torch.randn(6, 2, generator=gen)
    a = dp.TrainStep(*_toy_nets(2), _toy_elbo, lr=1e-2, skip_nonfinite=True)
    b = dp.TrainStep(*_toy_nets(2), _toy_elbo, lr=1e-2)
    assert a.guarded and not b.guarded
    for _ in range(3):
        a(None, y, noise=r)
        b(None, y, noise=r)
    assert torch.equal(a.grads.flat_param, b.grads.flat_param)       # coef is exactly 1
    keep = a.grads.flat_param.detach().clone()
    a(None, y * float("inf"), noise=r)
    assert torch.equal(a.grads.flat_param, keep)
    assert a.guard_stats() == dict(a.guard_stats(), steps=4, clipped=0, skipped=1)
    with pytest.raises(RuntimeError, match="guard_stats"):
        b.guard_stats()
    with pytest.raises(ValueError, match="clip_grad_norm"):
        dp.TrainStep(*_toy_nets(2), _toy_elbo, clip_grad_norm=0.0)


_DP_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["SVAE_ROOT"])
sys.path.insert(0, os.path.join(os.environ["SVAE_ROOT"], "tests"))
import torch, torch.nn as nn, torch.distributed as dist
from spatial_vae_amd import dp
from test_grad_guard_cpu import _toy_elbo, _toy_nets, _packed, _ref_packed, _rel

MAX_NORM = float(os.environ["SVAE_MAX_NORM"])
rank, world, _ = dp.init_process_group(device_is_gpu=False)
step = dp.TrainStep(*_toy_nets(100 + rank), _toy_elbo, lr=1e-2, clip_grad_norm=MAX_NORM)     # rank 0's weights win
gen = torch.Generator().manual_seed(1234)
sizes = [8, 5, 1, 6]                                # 4+4, 3+2 (ragged), 1+0 (rank 1 has NO rows), 3+3
batches = [torch.randn(b, 5, generator=gen) for b in sizes]
noises = [torch.randn(b, 2, generator=gen) for b in sizes]
ref = _toy_nets(100)
params = [p for net in ref for p in net.parameters()]
opt = torch.optim.Adam(params, lr=1e-2)
norms = []
for y, r in zip(batches, noises):
    lo, hi = dp.shard_bounds(y.size(0), rank, world)
    if y.size(0) == 5:
        assert (hi - lo) == (3, 2)[rank]
    step(None, y[lo:hi], weight=(hi - lo) / y.size(0), noise=r[lo:hi])
    opt.zero_grad()
    (-_toy_elbo(None, y, *ref, noise=r)[0]).backward()
    norms.append(float(torch.nn.utils.clip_grad_norm_(params, MAX_NORM)))
    opt.step()
assert any(n > MAX_NORM for n in norms), norms      # the threshold did clip
mine = step.grads.flat_param
both = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(both, mine)
assert torch.equal(both[0], both[1]), "replicas diverged"
gs = step.guard_stats()
vec = torch.tensor([gs["steps"], gs["clipped"], gs["skipped"], gs["mean_norm"], gs["max_norm"], gs["last_norm"]], dtype=torch.float64)
seen = [torch.empty_like(vec) for _ in range(world)]
dist.all_gather(seen, vec)
assert torch.equal(seen[0], seen[1]), "the ranks' guards saw different gradients"
assert gs["steps"] == 4 and gs["skipped"] == 0 and gs["clipped"] == sum(n > MAX_NORM for n in norms)
err = _rel(_packed(step), _ref_packed(ref))
print("rank", rank, "param err", err, "norms", norms)
assert err < 1e-6, err
dist.destroy_process_group()
'''


def test_two_gloo_ranks_clip_the_global_gradient_and_stay_bit_equal(tmp_path):
    """The guard runs after the all-reduce, so each rank clips by the norm of the GLOBAL gradient: ragged 3+2 and empty shards,
    replicas bit-equal, parameters within 1e-6 of the single-process run with clip_grad_norm_."""
    script = tmp_path / "guard_dp_worker.py"
    script.write_text(_DP_WORKER)
    # the four global gradients have norms 3.9, 5.0, 10.8 and 4.3 (printed by the worker): 4.5 clips two steps and leaves
    # two alone -- the worker asserts that it clips at all, whatever the figures
    env = dict(os.environ, SVAE_ROOT=ROOT, SVAE_MAX_NORM="4.5", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    code = ("import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
            "sys.exit(dp.launch_ranks(2, [%r]))" % (ROOT, str(script)))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.count("param err") == 2


# ---- the flags ----------------------------------------------------------------------------------------------------------------
def test_the_three_parsers_take_the_guard_flags_in_their_own_spelling():
    sys.path.insert(0, ROOT)
    import train_galaxy
    import train_mnist
    import train_particles
    for a in (train_mnist.mnist_arguments([]), train_galaxy.galaxy_arguments(["tr", "te"]),
              train_particles.particle_arguments(["tr", "te"])):
        assert a.clip_grad_norm is None and a.skip_nonfinite is False
    a = train_mnist.mnist_arguments(["--clip_grad_norm", "2.5", "--skip_nonfinite"])
    assert a.clip_grad_norm == 2.5 and a.skip_nonfinite is True
    a = train_galaxy.galaxy_arguments(["tr", "te", "--clip_grad_norm", "0.5"])
    assert a.clip_grad_norm == 0.5 and a.skip_nonfinite is False
    a = train_particles.particle_arguments(["tr", "te", "--clip-grad-norm", "2.5", "--skip-nonfinite"])
    assert a.clip_grad_norm == 2.5 and a.skip_nonfinite is True
    with pytest.raises(SystemExit):
        train_particles.particle_arguments(["tr", "te", "--clip_grad_norm", "2.5"])
    with pytest.raises(SystemExit):
        train_mnist.mnist_arguments(["--clip-grad-norm", "2.5"])


def _args(**over):
    base = dict(z_dim=2, learning_rate=1e-4, minibatch_size=64, save_prefix="a", num_epochs=4, seed=3, resume=None,
                checkpoint_interval=2, clip_grad_norm=None, skip_nonfinite=False)
    base.update(over)
    return argparse.Namespace(**base)


def test_resume_treats_a_file_without_the_guard_arguments_as_both_off():
    from spatial_vae_amd import cli
    old = {k: v for k, v in cli.plain_args(_args()).items() if k not in ("clip_grad_norm", "skip_nonfinite")}
    ck = {"args": old, "completed": 2}
    cli.check_resume_args(ck, _args(), "mnist")                                  # written before the flags existed: accepted
    with pytest.raises(cli.CheckpointError, match=r"\bclip_grad_norm\b"):
        cli.check_resume_args(ck, _args(clip_grad_norm=1.0), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\bskip_nonfinite\b"):
        cli.check_resume_args(ck, _args(skip_nonfinite=True), "mnist")
    ck = {"args": cli.plain_args(_args(clip_grad_norm=1.0, skip_nonfinite=True)), "completed": 2}
    cli.check_resume_args(ck, _args(clip_grad_norm=1.0, skip_nonfinite=True), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\bclip_grad_norm\b.*2\.0.*1\.0"):
        cli.check_resume_args(ck, _args(clip_grad_norm=2.0, skip_nonfinite=True), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\bclip_grad_norm\b"):
        cli.check_resume_args(ck, _args(skip_nonfinite=True), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\bskip_nonfinite\b"):
        cli.check_resume_args(ck, _args(clip_grad_norm=1.0), "mnist")


# ---- the command line, resumed, with a CPU stand-in for the ELBO ---------------------------------------------------------------
_FLOW_WORKER = r'''
import sys, os, io, contextlib
sys.path.insert(0, os.environ["SVAE_ROOT"])
import numpy as np, torch, torch.nn as nn
from spatial_vae_amd import cli, dp, elbo as E
import train_mnist

def toy(x, y, p_net, q_net, rotate=None, translate=None, dx_scale=None, theta_prior=None, noise=None):
    q = q_net(y); mu, ls = q[:, :2], q[:, 2:]
    z = mu + ls.exp() * noise
    yh = torch.sigmoid(p_net(z))
    log_p = -((yh - y) ** 2).sum(1).mean()
    kl = (-ls + 0.5 * ls.exp() ** 2 + 0.5 * mu ** 2 - 0.5).sum(1).mean()
    return log_p - kl, log_p, kl, yh
E.eval_minibatch_mnist = toy
cli.pick_device = lambda d, world=1, local=0: torch.device("cpu")

def build(args, device):
    tr = cli.synthetic_images("mnist", args.synthetic, 28, 28, 1, 0)
    te = cli.synthetic_images("mnist", args.synthetic // 4, 28, 28, 1, 1)
    y_train = torch.from_numpy(tr).float().div(255).view(-1, 784); y_test = torch.from_numpy(te).float().div(255).view(-1, 784)
    p = nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 784))
    q = nn.Sequential(nn.Linear(784, 8), nn.Tanh(), nn.Linear(8, 4)); q.latent_dim = 2
    return dict(y_train=y_train, y_test=y_test, n=28, m=28, p_net=p, q_net=q, rotate=False, translate=False, table=["Epoch", "ELBO", "BCE loss", "KL"])

def run(extra):
    args = train_mnist.mnist_arguments(["--synthetic", "200", "--seed", "5", "--minibatch_size", "64", "--num_epochs", "4", "--progress_every", "0",
                                        "--save_interval", "100", "--checkpoint_interval", "2", "-l", "1e-2"] + extra)
    buf, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
        cli.train_main("mnist", args, build)
    return [l for l in buf.getvalue().splitlines() if "\t" in l], [l for l in err.getvalue().splitlines() if l.startswith("# grad norm:")]

CLIP = ["--clip_grad_norm", os.environ["SVAE_CLIP"], "--skip_nonfinite"]
a, ga = run(["--save_prefix", "a"] + CLIP)
b, gb = run(["--save_prefix", "b", "--resume", "outputs_a/trained/a_state_epoch2.ckpt"] + CLIP)
print(a); print(b); print("\n".join(ga))
assert a[5:] == b[1:] and len(b) == 5
assert len(ga) == 4 and ga[2:] == gb
assert open("outputs_a/train.txt").read() == open("outputs_b/train.txt").read()
fa, fb = (torch.load("outputs_%s/trained/%s_state_epoch4.ckpt" % (p, p), weights_only=True) for p in "ab")
for g in ("p_net", "q_net"):
    for k in fa["train_step"][g]:
        assert torch.equal(fa["train_step"][g][k], fb["train_step"][g][k])
        assert torch.equal(fa["train_step"]["exp_avg_sq"][g][k], fb["train_step"]["exp_avg_sq"][g][k])
assert torch.equal(fa["rng"]["torch"], fb["rng"]["torch"]) and torch.equal(fa["rng"]["numpy_keys"], fb["rng"]["numpy_keys"])
assert fa["train_step"]["step"] == fb["train_step"]["step"] == 16
assert fa["args"]["clip_grad_norm"] == float(os.environ["SVAE_CLIP"]) and fa["args"]["skip_nonfinite"] is True
plain, _ = run(["--save_prefix", "p"])
assert plain != a                                   # the clipped run is another trajectory: the threshold did something
for bad in (["--clip_grad_norm", "7.0", "--skip_nonfinite"], ["--clip_grad_norm", os.environ["SVAE_CLIP"]], []):
    try:
        run(["--save_prefix", "c", "--resume", "outputs_a/trained/a_state_epoch2.ckpt"] + bad); raise AssertionError
    except SystemExit as e:
        print("refused:", e)
print("FLOW OK")
'''


def test_train_main_resumes_bit_for_bit_with_clipping_on_cpu(tmp_path):
    """tests/test_checkpoint_cpu.py's resume flow with --clip_grad_norm and --skip_nonfinite: run B continues run A's epoch-2
    state file to exactly A's rows, files, parameters, moments, step count and generator states; each epoch prints its
    `# grad norm:` line with some steps clipped; the options travel in the state file and a differing value is refused."""
    script = tmp_path / "guard_flow_worker.py"
    script.write_text(_FLOW_WORKER)
    # the stand-in's gradient norms grow from ~9 to ~25 over these 16 steps (its `# grad norm:` lines: max 13.4 in the first
    # epoch, means 18 to 24 afterwards): 16 leaves the first epoch alone and clips most later steps
    env = dict(os.environ, SVAE_ROOT=ROOT, SVAE_CLIP="16", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_SHARE_GPU", "SVAE_DP_SOLO"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(script)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FLOW OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    lines = re.findall(r"# grad norm: mean (\S+) max (\S+) clipped (\d+)/(\d+) skipped (\d+)", out.stdout)
    assert len(lines) == 4 and all(int(n) == 4 and int(s) == 0 for _, _, _, n, s in lines)
    assert sum(int(c) for _, _, c, _, _ in lines) > 0
    assert sum(int(c) for _, _, c, _, _ in lines) < 16                 # some steps clipped, not all
