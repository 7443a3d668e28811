"""The mixture calls (include/svae_gmm.h) off the default stream and under graph capture and replay: init, two update steps,
one labelling step, as one row of the kind tests/stream_cases.py holds (that file's Case is the base; the table itself is not
extended).  The baseline is first held to tests/gmm_ref.py, so the comparisons are between live numbers."""
import functools

import numpy as np
import pytest
import torch

import gmm_ref as G
import kmeans_ref as K
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu
REG, TOL = 1e-6, 1e-12


@functools.lru_cache(maxsize=None)
def _inputs(seed, N, D, k):
    """Overlapping blobs (planted centres randn * 0.6, noise 0.35), so that EM is still moving after a handful of steps, and
    their k-means start: three steps of kmeans_ref.fit."""
    rs = np.random.RandomState(60 + seed)
    planted = rs.randn(k, D) * 0.6
    x = (planted[rs.randint(0, k, size=N)] + 0.35 * rs.randn(N, D)).astype(np.float32)
    km = K.fit(x, k, rs.rand(k), 3)
    return x, km["label"].astype(np.int32), km["centres"]


class GmmCase(S.Case):
    """N = 600 (three chunks, the last of 88 points), D = 3, k = 4.  The record is the calls' to advance, and `mean` arrives
    holding the k-means centres and leaves holding the mixture's means: both are state."""
    name, entry_points, has_reference = "gmm_N600_D3_k4", ("svae_gmm_init", "svae_gmm_step"), True
    state = ("rec", "mean")
    N, D, k = 600, 3, 4

    def inputs(self, seed):
        x, label_in, centres = _inputs(seed, self.N, self.D, self.k)
        return {"x": x, "label_in": label_in, "mean": centres.copy(), "rec": np.zeros(6, np.int64)}

    def _outputs(self):
        return {"weight": ((self.k,), np.float64), "var": ((self.k, self.D), np.float64), "resp": ((self.N, self.k), np.float64),
                "label": ((self.N,), np.int32), "loglik_point": ((self.N,), np.float64)}

    def _scratch_bytes(self):
        from spatial_vae_amd import _lib
        return {"ws": _lib.lib().svae_gmm_workspace_bytes(self.N, self.D, self.k)}

    def step(self, update):
        p, ws = self.ptr, self.scratch["ws"]
        return lambda st: self.L.svae_gmm_step(p("x"), self.N, self.D, self.k, update, REG, TOL, p("weight"), p("mean"), p("var"), p("resp"),
                                               p("label"), p("loglik_point"), p("rec"), ws.ptr, ws.nbytes, st)

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        init = lambda st: self.L.svae_gmm_init(p("x"), self.N, self.D, self.k, p("label_in"), REG, p("weight"), p("mean"), p("var"), p("resp"),
                                               p("rec"), ws.ptr, ws.nbytes, st)
        return [init, self.step(1), self.step(1), self.step(0)]

    def check(self, out, seed=0, iters=2):
        i = self.inputs(seed)
        want = G.fit(i["x"], i["label_in"], i["mean"], iters, REG, TOL)
        assert want["iterations"] == iters and want["converged_at"] == 0        # still moving: a further step would advance it
        assert np.array_equal(out["label"], want["label"])
        for key in ("weight", "mean", "var", "resp", "loglik_point"):
            assert np.abs(out[key] - want[key]).max() <= 1e-10 * max(1.0, np.abs(want[key]).max()), key
        rec = out["rec"]
        assert rec[:4].tolist() == [iters, 0, self.N, 0]
        loglik, previous = rec[4:].view(np.float64)
        assert abs(loglik - want["loglik"]) <= 1e-10 * abs(want["loglik"]) and abs(previous - want["previous"]) <= 1e-10 * abs(want["previous"])


def _fresh(seed):
    case = GmmCase().alloc(_dev())
    case.load(seed)
    case.zero_scratch()
    case.stage_to_real()
    return case


def _eager(case, calls=None):
    S.statuses_ok([call(_handle(torch.cuda.current_stream())) for call in (case.steps() if calls is None else calls)])
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    return out


@pytest.fixture(scope="module")
def baselines():
    """The default-stream results of input sets A and B, each held to the reference; computed once."""
    out = []
    for seed in (0, 1):
        case = _fresh(seed)
        got = _eager(case)
        case.check(got, seed)
        out.append(got)
    assert not np.array_equal(out[0]["mean"], out[1]["mean"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs,
    workspace and outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = GmmCase().alloc(_dev())
    case.load(1)
    case.stage_to_real()
    case.load(0)
    case.poison()
    torch.cuda.synchronize()
    s = side_streams()[0]
    torch.cuda._sleep(delay_cycles())               # the default stream is busy
    busy = torch.cuda.Event()
    busy.record()
    behind_a_delay(case, s)
    rcs = case.enqueue(_handle(s))
    done = torch.cuda.Event()
    done.record(s)
    still_pending = not done.query() and not busy.query()
    S.statuses_ok(rcs)
    torch.cuda.synchronize()
    assert still_pending, "inconclusive: the %g ms delays had already run out when the last call returned" % DELAY_MS
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[0], "on a side stream")


def test_captured_and_replayed_on_a_second_input_set(baselines):
    """Captured with set A in the buffers (the capture executes nothing), replayed: baseline A.  Set B written over the inputs:
    one replay equals the eager result of B (svae_gmm_init zeroes the record itself).  A second graph holding one update step
    alone, replayed twice on what the first left: the record's count advances to 3 and 4 -- the iterations live on the device --
    and everything equals the same calls made eagerly, which the reference confirms."""
    case = _fresh(0)
    S.statuses_ok(case.enqueue(_handle(torch.cuda.current_stream())))      # one eager warm call
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
    assert not bad, bad
    assert_bit_equal(case.name, after, before, "after the capture alone (it must execute nothing)")
    assert (after["rec"] == 0).all()
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[0], "replayed with set A")
    case.load(1)
    case.stage_to_real()                            # set B: x, label_in and the centres
    case.fill_outputs()
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[1], "replayed with set B against the eager result of B")
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
    eager = _fresh(1)
    _eager(eager)
    want = _eager(eager, [eager.step(1), eager.step(1)])
    assert_bit_equal(case.name, out, want, "two replayed steps against two eager ones")
    ref = eager.inputs(1)
    state = G.init(ref["x"], ref["label_in"], ref["mean"], REG)
    for update in (1, 1, 0, 1, 1):
        state = G.step(ref["x"], state, update, REG, TOL)
    assert state["iterations"] == 4 and np.abs(out["mean"] - state["mean"]).max() <= 1e-10 * max(1.0, np.abs(state["mean"]).max())
