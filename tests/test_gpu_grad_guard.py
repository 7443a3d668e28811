"""The gradient guard on the MI355X: svae_grad_guard_norm (fixed-order double sum of squares, control record) against
float64, ops.FlatAdam's guarded mode and dp.TrainStep(clip_grad_norm=...) against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam, two ranks sharing cuda:0, and the command line with --clip_grad_norm (stderr line, bit-for-bit resume).
NaN and inf are ordinary float data here: nothing in this file faults.  The CPU half is tests/test_grad_guard_cpu.py."""
import copy
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases as C
from helpers import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 300                                                          # seconds per child process
INF = float("inf")


def _guard_norm(g, max_norm=INF, lr=1e-3, betas=(0.9, 0.999), control=None):
    """One svae_grad_guard_norm call on a workspace filled with NaN bytes; returns (record, raw control tensor)."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    n = g.numel()
    ws_bytes = L.svae_grad_guard_workspace_bytes(n)
    assert ws_bytes == 8 * -(-n // _chunk(n))
    ws = torch.full((max(ws_bytes, 256),), 0xFF, dtype=torch.uint8, device=g.device)
    assert L.svae_grad_guard_control_bytes() == ctypes.sizeof(_lib.GuardControl) == 72
    if control is None:
        control = torch.zeros(9, dtype=torch.int64, device=g.device)          # all zero bytes = a fresh record
    with torch.cuda.device(g.device):
        _lib.check(L.svae_grad_guard_norm(g.data_ptr(), n, max_norm, lr, betas[0], betas[1], control.data_ptr(), ws.data_ptr(),
                                          ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)))
    rec = _lib.GuardControl()
    ctypes.memmove(ctypes.byref(rec), control.cpu().numpy().tobytes(), ctypes.sizeof(rec))
    return rec, control


def _chunk(n):
    """include/svae.h: 4096 floats per chunk, doubled until the buffer is at most 4096 chunks -- a function of n only."""
    c = 4096
    while -(-n // c) > 4096:
        c *= 2
    return c


def _within_4_spacings(total, want):
    return abs(float(total) - want) <= 4 * float(np.spacing(np.float32(want)))


@pytest.mark.parametrize("n", [1, 5, 64, 1023, 4099, 1000003])
def test_norm_matches_float64_and_is_reproducible(n):
    """A lone scalar tail (1), a vector body with a tail (5), one chunk, many chunks (245) and a chunk that is only a tail
    (4099 = 4096 + 3).  The only fp32 roundings are the final conversion and the sqrt: 4 fp32 spacings."""
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(n)
    g = (torch.randn(n, generator=gen) * 10.0 ** ((torch.arange(n) % 7) - 3).float()).to(dev)      # stripes 1e-3 ... 1e3
    want = math.sqrt(float((g.cpu().double() ** 2).sum()))
    rec, raw = _guard_norm(g)
    print("n %d: total %.9g float64 %.17g" % (n, rec.total, want))
    assert _within_4_spacings(rec.total, want)
    assert rec.finite == 1 and rec.apply == 1 and rec.t == 1 and rec.coef == 1.0
    assert (rec.steps, rec.clipped, rec.skipped) == (1, 0, 0) and rec.norm_max == rec.total and rec.norm_sum == rec.total
    # both corrections are formed in double and rounded once: one fp32 spacing
    assert abs(rec.step_size - float(np.float32(1e-3)) / (1.0 - float(np.float32(0.9)))) <= float(np.spacing(np.float32(rec.step_size)))
    assert abs(rec.sqrt_bc2 - math.sqrt(1.0 - float(np.float32(0.999)))) <= float(np.spacing(np.float32(rec.sqrt_bc2)))
    _, again = _guard_norm(g)
    assert torch.equal(raw, again)                                   # the same call on a fresh record: the same bits
    # with a threshold: clip_grad_norm_'s coefficient in fp32, and the record goes on counting
    max_norm = 0.25 * want
    rec2, _ = _guard_norm(g, max_norm=max_norm, control=raw)
    coef = np.float32(max_norm) / (np.float32(rec.total) + np.float32(1e-6))
    assert abs(rec2.coef - float(coef)) <= float(np.spacing(coef)) and rec2.t == 2 and (rec2.steps, rec2.clipped) == (2, 1)
    assert rec2.total == rec.total


def test_norm_accumulates_in_double_and_flags_what_leaves_the_float_range():
    dev = torch.device("cuda:0")
    g = torch.full((1000,), 1e25, device=dev)                        # squares of 1e50: beyond fp32, far inside double
    rec, _ = _guard_norm(g, max_norm=1.0)
    print("1000 x 1e25: total %.9g" % rec.total)
    assert rec.finite == 1 and rec.apply == 1 and _within_4_spacings(rec.total, 1e25 * math.sqrt(1000.0))
    assert 0.0 < rec.coef < 1e-26 and rec.clipped == 1
    g = torch.zeros(10007, device=dev)
    g[[3, 4100, 9000, 10006]] = 3e38                                 # norm 6e38 > FLT_MAX, each entry finite
    rec, _ = _guard_norm(g, max_norm=1.0)
    assert rec.finite == 0 and rec.apply == 0 and rec.t == 0 and (rec.steps, rec.clipped, rec.skipped) == (1, 0, 1)
    assert math.isinf(rec.total) and rec.norm_sum == 0.0 and rec.norm_max == 0.0
    for bad, where in ((float("nan"), 5000), (INF, 10006), (-INF, 0)):
        g = torch.ones(10007, device=dev)
        g[where] = bad
        rec, _ = _guard_norm(g)
        assert rec.finite == 0 and rec.apply == 0 and rec.t == 0 and rec.skipped == 1, bad


def _ulp_ok(an, bn):
    return (np.abs(an - bn) <= 4 * np.spacing(np.maximum(np.abs(bn), np.float32(5e-3)))).all()


def test_guarded_flat_adam_matches_clip_grad_norm_and_torch_adam():
    """Five gradients randn * 10^(i-2) -- norms ~3.2, 32, 316, 3162, 31623 against a threshold of 50: two unclipped, three
    clipped, none within a factor 1.5 of it -- with two poisoned steps in between (NaN in the vector body, inf in the scalar
    tail), which torch's side simply does not take."""
    from spatial_vae_amd.ops import FlatAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n = 100003
    w0 = torch.randn(n, device=dev)
    a, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone())
    oa = FlatAdam([a], lr=1e-3, zero_grad=True, max_grad_norm=50.0, skip_nonfinite=True)
    ob = torch.optim.Adam([b], lr=1e-3)
    clean = [torch.randn_like(w0) * (10.0 ** (i - 2)) for i in range(5)]
    nan_g, inf_g = torch.randn_like(w0), torch.randn_like(w0)
    nan_g[4096 * 3 + 8] = float("nan")
    inf_g[n - 1] = INF
    assert (n - 1) >= (n // 4) * 4                                   # the last element is in the scalar tail
    plan = [clean[0], clean[1], nan_g, clean[2], clean[3], inf_g, clean[4]]
    norms = []
    for g in plan:
        a.grad = g.clone()
        poisoned = g is nan_g or g is inf_g
        if poisoned:
            st = oa.state[a]
            keep = (a.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        oa.step()
        assert float(a.grad.abs().max()) == 0.0                      # cleared behind the update, applied or not
        if poisoned:
            assert torch.equal(a.detach(), keep[0]) and torch.equal(st["exp_avg"], keep[1]) and torch.equal(st["exp_avg_sq"], keep[2])
            continue
        norms.append(math.sqrt(float((g.double() ** 2).sum())))
        b.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([b], 50.0)
        ob.step()
    torch.cuda.synchronize()
    assert all(x > 75.0 or x < 50.0 / 1.5 for x in norms) and sum(x > 50.0 for x in norms) == 3, norms
    st = oa.state[a]
    assert torch.is_tensor(st["step"]) and st["step"].is_cuda and st["step"].dtype == torch.int64 and st["step"].numel() == 1
    assert int(st["step"]) == 5
    an, bn = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    print("guarded FlatAdam vs torch: rel err %.3e" % rel_err(an, bn))
    assert rel_err(an, bn) < 1e-6
    assert _ulp_ok(an, bn)
    assert np.abs(an - w0.cpu().numpy()).max() > 1e-3
    gs = oa.guard_stats()
    assert (gs["steps"], gs["clipped"], gs["skipped"]) == (7, 3, 2), gs
    assert abs(gs["max_norm"] - max(norms)) <= 1e-6 * max(norms)
    assert abs(gs["mean_norm"] - sum(norms) / 5) <= 1e-6 * max(norms)
    assert oa.guard_stats(reset=True) == gs
    gs = oa.guard_stats()
    assert (gs["steps"], gs["clipped"], gs["skipped"], gs["max_norm"]) == (0, 0, 0, 0.0) and int(st["step"]) == 5


def test_skip_nonfinite_alone_is_plain_flat_adam_on_finite_gradients():
    """coef is exactly 1; the bias corrections are formed on the device (double, then rounded, as the host forms them for
    svae_adam_step), so the bar is the 4-ulp one and not bit equality."""
    from spatial_vae_amd.ops import FlatAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    w0 = torch.randn(100003, device=dev)
    a, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(w0.clone())
    oa, ob = FlatAdam([a], lr=1e-3, skip_nonfinite=True), FlatAdam([b], lr=1e-3)
    for i in range(3):
        g = torch.randn_like(w0) * (10.0 ** (i - 1))
        a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    an, bn = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert _ulp_ok(an, bn) and rel_err(an, bn) < 1e-6
    assert float(a.grad.abs().max()) > 0                             # zero_grad off: the gradient is left alone
    gs = oa.guard_stats()
    assert (gs["steps"], gs["clipped"], gs["skipped"]) == (3, 0, 0) and int(oa.state[a]["step"]) == 3 == ob.state[b]["step"]
    with pytest.raises(RuntimeError, match="guard_stats"):
        ob.guard_stats()
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdam([a], max_grad_norm=-1.0)


ACT = {"tanh": nn.Tanh, "leakyrelu": nn.LeakyReLU, "relu": nn.ReLU, "sigmoid": nn.Sigmoid}


def _nets(case, inp, device):
    import spatial_vae.models as models
    p_net = models.SpatialGenerator(case["z_dim"], case["H"], n_out=case["n_out"], num_layers=case["L"],
                                    activation=ACT[case["act"]], softplus=case["softplus"], resid=case["resid"],
                                    expand_coords=case["expand_coords"], bilinear=case["bilinear"])
    q_net = models.InferenceNetwork(case["n"] * case["m"], C.inf_dim(case), case["q_hidden"], num_layers=case["q_layers"],
                                    activation=ACT[case["act"]], resid=case["resid"])
    p_net.load_state_dict({k: torch.from_numpy(v) for k, v in inp["p_state"].items()})
    q_net.load_state_dict({k: torch.from_numpy(v) for k, v in inp["q_state"].items()})
    return p_net.to(device), q_net.to(device)


def test_train_step_with_clipping_matches_clip_grad_norm_and_torch_adam():
    from spatial_vae_amd import dp, elbo as E, ops
    case = C.CASES_BY_NAME["mnist_rt"]
    inp = C.build_inputs(case)
    dev = torch.device("cuda:0")
    p1, q1 = _nets(case, inp, dev)
    p2, q2 = copy.deepcopy(p1), copy.deepcopy(q1)
    p3, q3 = copy.deepcopy(p1), copy.deepcopy(q1)
    x = torch.from_numpy(inp["x_coord"]).to(dev)
    y = torch.from_numpy(inp["y"]).to(dev)
    r = torch.from_numpy(inp["r"]).to(dev)
    kw = dict(rotate=True, translate=True, dx_scale=case["dx_scale"], theta_prior=case["theta_prior"])
    # the threshold: half the first step's norm, from a plain backward -- that step clips, and so do the next two unless
    # three steps at lr 1e-3 halve the gradient (the reference run's norms are printed and asserted below)
    (-E.eval_minibatch_mnist(x, y, p3, q3, noise=r, **kw)[0]).backward()
    first = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1) for p in list(p3.parameters()) + list(q3.parameters())])))
    max_norm = 0.5 * first
    step = dp.TrainStep(p1, q1, E.eval_minibatch_mnist, lr=1e-3, clip_grad_norm=max_norm, **kw)
    assert isinstance(step.optim, ops.FlatAdam) and step.optim.guarded
    params = list(p2.parameters()) + list(q2.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    norms = []
    for _ in range(3):
        step(x, y, noise=r)
        elbo = E.eval_minibatch_mnist(x, y, p2, q2, noise=r, **kw)[0]
        (-elbo).backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
        opt.zero_grad()
    torch.cuda.synchronize()
    print("norms %s threshold %.6g" % (norms, max_norm))
    assert all(v > max_norm for v in norms), (norms, max_norm)       # every step clipped
    for (k, a), (_, b) in zip(list(p1.named_parameters()) + list(q1.named_parameters()),
                              list(p2.named_parameters()) + list(q2.named_parameters())):
        assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 2e-5, k
    assert step.grads.flat.numel() == step.grads.n and float(step.grads.flat.abs().max()) == 0.0   # padding included
    gs = step.guard_stats()
    assert (gs["steps"], gs["clipped"], gs["skipped"]) == (3, 3, 0) and step.state_dict()["step"] == 3 and step.aliased()
    assert abs(gs["max_norm"] - max(norms)) <= 2e-5 * max(norms)
    with pytest.raises(RuntimeError, match="fused_adam"):
        dp.TrainStep(p3, q3, E.eval_minibatch_mnist, lr=1e-3, fused_adam=True, clip_grad_norm=1.0, **kw)
    with pytest.raises(RuntimeError, match="fused_adam"):
        dp.TrainStep(p3, q3, E.eval_minibatch_mnist, lr=1e-3, fused_adam=True, skip_nonfinite=True, **kw)


def _env(**extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_SHARE_GPU", "SVAE_DP_SOLO", "SVAE_DP_BUCKETS", "SVAE_DP_LOWRANK"):
        env.pop(k, None)
    env.update(extra)
    return env


def test_two_ranks_on_one_gpu_clip_alike_and_match_the_single_rank_run(tmp_path):
    """tests/grad_guard_child.py: shards 4+4, 5+3, 1+0 (EMPTY), 3+3.  The guard sits behind the all-reduce, so both ranks clip
    by the norm of the same global gradient: replicas bit-equal, parameters within 2e-6 of the one-rank run (the bar of
    tests/test_gpu_dp.py), and the two control records tell the same story."""
    child = os.path.join(ROOT, "tests", "grad_guard_child.py")
    env = _env(SVAE_GUARD_REF=str(tmp_path / "ref.pt"))
    one = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=LIMIT)
    assert one.returncode == 0, one.stdout[-1500:] + one.stderr[-3000:]
    env["SVAE_SHARE_GPU"] = "1"
    code = ("import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
            "sys.exit(dp.launch_ranks(2, [%r], timeout=%d))" % (ROOT, child, LIMIT - 30))
    two = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=LIMIT)
    assert two.returncode == 0, two.stdout[-1500:] + two.stderr[-3000:]
    stats = {int(r): json.loads(s) for r, s in re.findall(r"^rank (\d) stats (\{.*\})$", two.stdout, re.M)}
    solo = json.loads(re.search(r"^rank 0 stats (\{.*\})$", one.stdout, re.M).group(1))
    print(solo, stats)
    assert sorted(stats) == [0, 1] and stats[0] == stats[1]
    assert stats[0]["steps"] == 4 and stats[0]["skipped"] == 0 and stats[0]["clipped"] >= 1
    assert (stats[0]["clipped"], stats[0]["threshold"]) == (solo["clipped"], solo["threshold"])
    assert abs(stats[0]["max_norm"] - solo["max_norm"]) <= 2e-6 * solo["max_norm"]


# ---- the command line ----------------------------------------------------------------------------------------------------------
# The issue's run with a measured threshold.  Unclipped (threshold 1e9) its two passes of three steps print, on an MI355X,
# `mean 1537.56 max 1658.2` and `mean 1119.94 max 1230.74` (with every step clipped, at 1.0: 1537.44 / 1658.2 and 1116.49 /
# 1229.48 -- Adam barely cares about the gradient's scale).  1150 lies under the second pass's largest norm and above its mean,
# hence above its smallest: both passes clip, the second one not every step.
CLI_ARGS = ["--synthetic", "96", "--minibatch_size", "32", "--num_epochs", "2", "--seed", "3", "--checkpoint_interval", "1"]
CLI_CLIP = "1150"


def _cli(args, cwd):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_mnist.py")] + args, cwd=cwd, env=_env(), capture_output=True,
                         text=True, timeout=LIMIT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    rows = [l for l in out.stdout.splitlines() if "\t" in l]
    guard = re.findall(r"^# grad norm: mean (\S+) max (\S+) clipped (\d+)/(\d+) skipped (\d+)$", out.stderr, re.M)
    return rows, guard


def test_command_line_clips_reports_and_resumes_bit_for_bit(tmp_path):
    cwd = str(tmp_path)
    clip = ["--clip_grad_norm", CLI_CLIP]
    a, ga = _cli(CLI_ARGS + clip + ["--save_prefix", "a"], cwd)
    print(ga)
    assert len(a) == 1 + 4 and len(ga) == 2
    for mean, top, clipped, steps, skipped in ga:
        assert int(steps) == 3 and int(skipped) == 0 and int(clipped) > 0 and float(mean) <= float(top)
    assert sum(int(g[2]) for g in ga) < 6                             # some steps clipped, not all
    base = lambda p: str(tmp_path / ("outputs_" + p) / "trained" / p)  # noqa: E731
    b, gb = _cli(CLI_ARGS + clip + ["--save_prefix", "b", "--resume", base("a") + "_state_epoch1.ckpt"], cwd)
    assert len(b) == 1 + 2 and a[3:] == b[1:], (a, b)
    assert gb == ga[1:]
    fa, fb = (torch.load(base(p) + "_state_epoch2.ckpt", weights_only=True) for p in "ab")
    assert fa["train_step"]["step"] == fb["train_step"]["step"] == 6
    assert fa["args"]["clip_grad_norm"] == float(CLI_CLIP) and fa["args"]["skip_nonfinite"] is False
    for group in ("p_net", "q_net"):
        for k, v in fa["train_step"][group].items():
            assert torch.equal(v, fb["train_step"][group][k]), (group, k)
            for m in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(fa["train_step"][m][group][k], fb["train_step"][m][group][k]), (m, group, k)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_mnist.py")] + CLI_ARGS +
                         ["--clip_grad_norm", "2.0", "--save_prefix", "c", "--resume", base("a") + "_state_epoch1.ckpt"],
                         cwd=cwd, env=_env(), capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 1 and "clip_grad_norm" in out.stderr and "Traceback" not in out.stderr
