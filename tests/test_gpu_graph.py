"""Every entry point that takes a stream under HIP graph capture and replay, and dp.TrainStep.capture against the eager step.

include/svae.h says what a captured call means: the launches are recorded with the addresses and host numbers of the
capture, the host tables are updated at enqueue time only, and everything that should differ between replays must be device
data.  A launch that escaped the capture, a host constant baked in where device data was meant, or state carried from one
replay to the next shows here as a replay that differs from the eager default-stream result of the same inputs
(tests/test_gpu_streams.py's baselines, themselves held to float64 there).

Captures are linear: one capture stream, nothing forks or joins inside."""
import contextlib
import ctypes
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import stream_cases as S
from decoder_abi import SENTINEL
from test_gpu_streams import _dev, _eager, _fresh, _handle, assert_bit_equal, assert_clean, baseline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ME = "tests/test_gpu_graph.py"
CAPTURED = [n for n in S.NAMES if not set(S.make_case(n).entry_points) & set(S.NOT_CAPTURABLE)]


def _captured(case):
    """One eager warm call (the once-per-kernel hipFuncSetAttribute; scratch at its size), the inputs restored, the outputs
    refilled with the sentinel, then the case's calls recorded into a graph.  Asserts that the capture executed nothing."""
    S.statuses_ok(case.enqueue(_handle(torch.cuda.current_stream())))
    torch.cuda.synchronize()
    case.stage_to_real()
    case.fill_outputs()
    torch.cuda.synchronize()
    before, _ = case.collect()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcs = case.enqueue(_handle(torch.cuda.current_stream()))
    S.statuses_ok(rcs)
    torch.cuda.synchronize()
    after, bad = case.collect()
    assert not bad, (case.name, bad)
    assert_bit_equal(case.name, after, before, "after the capture alone (it must execute nothing)")
    for k, a in after.items():
        if k not in case.state and a.dtype.kind == "f":
            assert (a == SENTINEL).all(), (case.name, k, "written during capture")
    return g


def _replay(case, g):
    case.stage_to_real()                    # the in-place cases start every replay from their inputs; a no-op copy elsewhere
    case.fill_outputs()
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert_clean(case, out, bad)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. every case under replay
# ---------------------------------------------------------------------------------------------------------------------
def test_not_capturable_entries_are_stated():
    assert len(S.NOT_CAPTURABLE) <= 3 and all(isinstance(r, str) and r for r in S.NOT_CAPTURABLE.values())


@pytest.mark.parametrize("name", CAPTURED)
def test_every_case_under_replay(name):
    """Captured with input set A in its buffers: a replay equals baseline A; with set B written over the inputs in place, the
    eager default-stream result of B; a second replay of B the same again.  Scratch is NOT cleared in between: whatever the
    calls carry from one run to the next in their workspace, `saved` or a record would show."""
    case = _fresh(name)
    g = _captured(case)
    assert_bit_equal(name, _replay(case, g), baseline(name), "replayed with set A")
    case.load(1)
    assert_bit_equal(name, _replay(case, g), baseline(name, 1), "replayed with set B")
    assert_bit_equal(name, _replay(case, g), baseline(name, 1), "replayed with set B a second time")


def test_the_guarded_pair_advances_its_count_inside_the_graph():
    """svae_grad_guard_norm -> svae_adam_step_guarded: three replays equal three eager call pairs, record included -- t,
    step_size and sqrt_bc2 live on the device and advance per replay.  A fourth replay on a gradient holding one inf leaves
    param, both moments and t alone, clears the gradient and counts a skipped step."""
    cases = eager, graph = [_fresh("guard_clip") for _ in range(2)]
    g = _captured(graph)
    assert S.Guard.record(graph.collect()[0]["control"]).t == 3                 # the warm call was undone, the capture ran nothing
    rs = np.random.RandomState(5)
    for i in range(3):
        grad = torch.from_numpy(rs.normal(size=eager.n).astype(np.float32)).to(_dev())
        for c in cases:
            c.real["grad"].copy_(grad)
        want = _eager(eager)
        g.replay()
        torch.cuda.synchronize()
        got, bad = graph.collect()
        assert not bad
        assert_bit_equal("guard_clip", got, want, "replay %d against eager call pair %d" % (i, i))
        rec = S.Guard.record(got["control"])
        assert rec.t == 4 + i and rec.apply == 1 and rec.steps == 1 + i
        # the values themselves are pinned by the equality with the eager pair; this only says that they are step t's (formed
        # in double from the float arguments and rounded to float, as here: two float spacings cover a last-bit difference)
        for got_v, want_v in ((rec.step_size, S.LR / (1 - S.BETA1 ** rec.t)), (rec.sqrt_bc2, math.sqrt(1 - S.BETA2 ** rec.t))):
            assert abs(got_v - want_v) <= 2 * np.spacing(np.float32(want_v)), (i, got_v, want_v)
    before = got
    grad[77] = float("inf")
    graph.real["grad"].copy_(grad)
    g.replay()
    torch.cuda.synchronize()
    after, bad = graph.collect()
    assert not bad
    for k in ("param", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), k
    rec = S.Guard.record(after["control"])
    assert rec.t == 6 and rec.apply == 0 and rec.finite == 0 and rec.skipped == 1 and rec.steps == 4
    assert (after["grad"] == 0).all()


def test_kmeans_replays_advance_the_record_they_are_not_handed_afresh():
    """One replay on set B and a zero record equals baseline B.  Replays WITHOUT restoring the record advance its count -- the
    iterations live on the device -- and three of them equal three eager call sequences on one record, count included."""
    name = "kmeans_N600_D3_k4"
    case = _fresh(name)
    g = _captured(case)
    assert (case.collect()[0]["rec"] == 0).all()
    assert_bit_equal(name, _replay(case, g), baseline(name), "replayed with set A")
    case.load(1)                                    # set B, and the record back to zero bytes
    assert_bit_equal(name, _replay(case, g), baseline(name, 1), "replayed with set B against the eager result of B")
    for n in (2, 3):
        g.replay()
        torch.cuda.synchronize()
        out, bad = case.collect()
        assert not bad and out["rec"][0] == 2 * n, (n, out["rec"])
        assert np.array_equal(out["seed_index"], baseline(name, 1)["seed_index"])
    # the same calls made eagerly on a record that already counts: equal to the replays, count included
    eager = _fresh(name, 1)
    for _ in range(3):
        want = _eager(eager)
    assert_bit_equal(name, out, want, "three replays against three eager sequences")


def test_the_mixture_steps_alone_in_a_second_graph():
    """After one replay on set B (svae_gmm_init zeroes the record itself), a second graph holding one update step alone,
    replayed twice on what the first left: the record's count advances to 3 and 4 -- the iterations live on the device -- and
    everything equals the same calls made eagerly, which the reference confirms."""
    import gmm_ref as G
    from stream_cases_analysis import GMM_REG, GMM_TOL
    name = "gmm_N600_D3_k4"
    case = _fresh(name)
    g = _captured(case)
    assert (case.collect()[0]["rec"] == 0).all()
    assert_bit_equal(name, _replay(case, g), baseline(name), "replayed with set A")
    case.load(1)                                    # set B: x, label_in and the centres
    assert_bit_equal(name, _replay(case, g), baseline(name, 1), "replayed with set B against the eager result of B")
    one = torch.cuda.CUDAGraph()
    with torch.cuda.graph(one):
        rc = case.step(1)(_handle(torch.cuda.current_stream()))
    S.statuses_ok([rc])
    torch.cuda.synchronize()
    assert case.collect()[0]["rec"][0] == 2         # captured, not run
    for n in (3, 4):
        one.replay()
        torch.cuda.synchronize()
        out, bad = case.collect()
        assert not bad and out["rec"][0] == n, (n, out["rec"])
    eager = _fresh(name, 1)
    _eager(eager)
    want = _eager(eager, [eager.step(1), eager.step(1)])
    assert_bit_equal(name, out, want, "two replayed steps against two eager ones")
    ref = eager.inputs(1)
    state = G.init(ref["x"], ref["label_in"], ref["mean"], GMM_REG)
    for update in (1, 1, 0, 1, 1):
        state = G.step(ref["x"], state, update, GMM_REG, GMM_TOL)
    assert state["iterations"] == 4 and np.abs(out["mean"] - state["mean"]).max() <= 1e-10 * max(1.0, np.abs(state["mean"]).max())


@pytest.mark.parametrize("zero_grad", [0, 1])
def test_adam_steps_number_is_a_captured_constant(zero_grad):
    """svae_adam_step takes the step number as a host argument: a graph captured at step 9 applies step 9's bias corrections
    on every replay (include/svae.h says so), equal to an eager call with 9 and different from one with 10."""
    eager, graph = S.Adam(zero_grad).alloc(_dev()), S.Adam(zero_grad).alloc(_dev())
    for c in (eager, graph):
        c.step = 9
        c.load(0)
        c.stage_to_real()
    g = _captured(graph)
    want = _eager(eager)
    for _ in range(2):
        assert_bit_equal(graph.name, _replay(graph, g), want, "replayed, captured at step 9")
    eager.step = 10
    eager.stage_to_real()
    assert not np.array_equal(_eager(eager)["param"], want["param"])
    graph.step = 10                                     # the host number was read at capture: changing it now changes nothing
    assert_bit_equal(graph.name, _replay(graph, g), want, "replayed after the host number changed")


# ---------------------------------------------------------------------------------------------------------------------
# b. the captured training step equals the eager one
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "mnist_bce": dict(script="mnist", n=8, B=6, z=2, H=64, L=2, C=1),
    # svae_gaussian_loglik refuses a CTF together with the two-channel (fit-noise) decoder, as the reference has no result for
    # it: the particle step runs once with C = 2 and the mask, once with C = 1, the mask and 11 x 11 CTF filters
    "particles_fit_noise": dict(script="particles", n=12, B=5, z=3, H=96, L=3, C=2),
    "particles_ctf": dict(script="particles", n=12, B=5, z=3, H=96, L=3, C=1, ctf=11),
}


def _twin(cfg, **kw):
    import spatial_vae.models as models
    from spatial_vae_amd import dp, elbo as E
    torch.manual_seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(cfg["z"], cfg["H"], n_out=cfg["C"], num_layers=cfg["L"], activation=nn.Tanh).to(_dev())
        q_net = models.InferenceNetwork(cfg["n"] ** 2, cfg["z"] + 3, 32, num_layers=2, activation=nn.Tanh).to(_dev())
    fn = E.eval_minibatch_mnist if cfg["script"] == "mnist" else E.eval_minibatch_particles
    return dp.TrainStep(p_net, q_net, fn, lr=1e-3, rotate=True, translate=True, dx_scale=0.1, theta_prior=math.pi, **kw)


def _data(cfg):
    """(grid, the step's batch arguments, six noise draws) on the device."""
    import cases
    from spatial_vae_amd import cli, ops
    from stream_cases import random_table
    dev, rs = _dev(), np.random.RandomState(12)
    n, B = cfg["n"], cfg["B"]
    x = cli.coord_grid(n, n).to(dev)
    if cfg["script"] == "mnist":
        batch = (torch.from_numpy((np.floor(rs.uniform(size=(B, n * n)) * 255) / 255).astype(np.float32)).to(dev),)
    else:
        y = torch.from_numpy(rs.normal(size=(B, n * n)).astype(np.float32)).to(dev)
        mask = torch.from_numpy(np.asarray(cases.circular_mask(n, n)).reshape(-1)).to(dev)
        ctf = ops.ctf_filter(random_table(B, 3), cfg["ctf"], cfg["ctf"], device=dev).unsqueeze(1) if cfg.get("ctf") else None
        batch = (y, mask, ctf)
    noise = [torch.from_numpy(rs.normal(size=(B, cfg["z"] + 3)).astype(np.float32)).to(dev) for _ in range(4)]
    return x, batch, noise


def _state(step):
    torch.cuda.synchronize()
    st = step.optim.state[step.master]
    return [t.detach().clone() for t in (step.grads.flat_param, st["exp_avg"], st["exp_avg_sq"], step.metrics[:3])]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_captured_step_equals_the_eager_step(name):
    """Two TrainStep(fused_adam=True) twins from identical weights: one runs capture(warmup=3) and three replays, the other six
    eager steps on the same batch and noise (the noise tensor is the one handed to capture(), refilled in place before each
    replay).  Parameters, both Adam moments and the three metrics are bit-equal after the warm-up and after every replay."""
    cfg = CONFIGS[name]
    x, batch, noise = _data(cfg)
    eager, graph = _twin(cfg, fused_adam=True), _twin(cfg, fused_adam=True)
    assert torch.equal(eager.grads.flat_param, graph.grads.flat_param)
    start = graph.grads.flat_param.detach().clone()
    static_noise = noise[0].clone()
    for _ in range(3):
        eager(x, *batch, noise=noise[0])
    assert graph.capture(x, *batch, warmup=3, noise=static_noise) is graph
    # (the captured step's metrics live in the graph's own memory and hold nothing before the first replay)
    for a, b, what in zip(_state(graph)[:3], _state(eager)[:3], ("parameters", "exp_avg", "exp_avg_sq")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "after the warm-up", what)
    assert not torch.equal(start, graph.grads.flat_param)
    for i in (1, 2, 3):
        static_noise.copy_(noise[i])
        eager(x, *batch, noise=noise[i])
        graph(x, *batch)
        got, want = _state(graph), _state(eager)
        assert bool(torch.isfinite(got[3]).all())
        for a, b, what in zip(got, want, ("parameters", "exp_avg", "exp_avg_sq", "metrics")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, "replay %d" % i, what)
    assert float(graph.optim.state[graph.master]["step"]) == 6.0


def test_a_captured_step_refuses_what_it_cannot_replay():
    cfg = CONFIGS["mnist_bce"]
    x, batch, noise = _data(cfg)
    step = _twin(cfg, fused_adam=True).capture(x, *batch, warmup=1, noise=noise[0].clone())
    step(x, *batch)
    step(x, *batch, global_batch=cfg["B"])                                  # bench.py passes it; it does not change the step
    with pytest.raises(RuntimeError, match="fixed arguments"):
        step(x, *batch, weight=0.5)
    with pytest.raises(RuntimeError, match="fixed arguments"):
        step(x, *batch, noise=noise[1])
    with pytest.raises(RuntimeError, match="shape"):
        step(x, batch[0][:3])
    with pytest.raises(RuntimeError, match="shape"):
        step(x, batch[0][:1])                                               # one row would broadcast into the static batch
    with pytest.raises(RuntimeError, match="batch tensors"):
        step(x)


# ---------------------------------------------------------------------------------------------------------------------
# c. capture() checks what it needs
# ---------------------------------------------------------------------------------------------------------------------
def test_capture_needs_the_capturable_optimiser():
    """The default step's ops.FlatAdam hands svae_adam_step the step number from the host: captured, it would replay step 4's
    bias corrections forever.  capture() raises and names fused_adam=True; so it does for the guarded step."""
    from spatial_vae_amd import ops
    cfg = CONFIGS["mnist_bce"]
    x, batch, noise = _data(cfg)
    step = _twin(cfg)
    assert isinstance(step.optim, ops.FlatAdam)
    with pytest.raises(RuntimeError, match="fused_adam=True"):
        step.capture(x, *batch, noise=noise[0])
    assert step._graph is None
    before = step.grads.flat_param.detach().clone()
    step(x, *batch, noise=noise[0])                                          # still an eager step
    assert not torch.equal(before, step.grads.flat_param)
    guarded = _twin(cfg, clip_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="fused_adam=True"):
        guarded.capture(x, *batch, noise=noise[0])


# ---------------------------------------------------------------------------------------------------------------------
# fp16x3 child, bench smoke
# ---------------------------------------------------------------------------------------------------------------------
FP16X3_SUBJECTS = ["test_the_captured_step_equals_the_eager_step[mnist_bce]",
                   "test_every_case_under_replay[decoder_rank1_tanh]",
                   "test_every_case_under_replay[decoder_rank1_tanh_bce]",
                   "test_every_case_under_replay[decoder_z0_sigmoid_w128]"]


def test_capture_and_replay_pass_in_fp16x3_mode():
    """One fresh process under SVAE_GEMM=fp16x3 (the amax memset nodes and atomicMax scales live there) repeats the MNIST-like
    captured step and the split-eligible decoder cases under replay."""
    if os.environ.get("SVAE_GEMM") == "fp16x3":
        return                                              # this IS the child
    env = dict(os.environ, SVAE_GEMM="fp16x3")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] +
                         [ME + "::" + t for t in FP16X3_SUBJECTS], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert "%d passed" % len(FP16X3_SUBJECTS) in out.stdout and "failed" not in out.stdout, tail


def test_bench_runs_from_a_graph():
    from test_gpu_bench import _bench
    d = _bench(["--gpus", "1", "--config", "1", "--steps", "3", "--warmup", "2", "--graph"])
    assert d["value"] > 0 and d["steps"] == 3
