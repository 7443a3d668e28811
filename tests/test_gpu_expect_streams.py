"""The two launches of include/svae_expect.h off the default stream and under graph capture and replay: svae_pose_expect, then
svae_expect_sums_update on what it wrote, as one row of the kind tests/stream_cases.py holds (that file's Case is the base; the
table itself is not extended).  The baseline is first held to tests/expect_ref.py, so the comparisons are between live
numbers."""
import numpy as np
import pytest
import torch

import expect_ref as X
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu
INV_SIGMA2 = 1.5


class ExpectCase(S.Case):
    """tests/expect_ref.py's second shape (17 x 13 x 3, A = 2, S = 3, M = 3: five references) with weight and prior; the soft sums
    fold the five references into three classes on top of start values.  Set B is set A's images in reverse order with other
    start values: other numbers of equal shapes."""
    name, entry_points, has_reference = "expect_17x13x3_M3_sums", ("svae_pose_expect", "svae_expect_sums_update"), True
    state = ("sum", "count")
    n_classes = 3

    def __init__(self):
        self.f = X.fixture(1, True, True)

    def inputs(self, seed):
        f = self.f
        rs = np.random.RandomState(7 + seed)
        order = slice(None, None, -1) if seed else slice(None)
        N = f["rows"] * f["cols"]
        return {"y": f["y"][order].copy(), "ref": f["ref"], "weight": f["weight"], "log_prior": f["log_prior"],
                "cand": f["cand"][order].copy(), "pose": f["pose"][order].copy(), "target": np.array([0, 1, 2, 2, 5], np.int32),
                "sum": rs.normal(size=(self.n_classes, N, f["C"])), "count": np.floor(rs.uniform(0, 5, size=(self.n_classes, N)))}

    def _outputs(self):
        f = self.f
        B, M, N = f["B"], f["M"], f["rows"] * f["cols"]
        return {"contrib": ((B, M, N, f["C"]), np.float64), "cover_w": ((B, M, N), np.float64), "class_post": ((B, M), np.float64),
                "log_evidence": ((B,), np.float64), "best": ((B, 4), np.int32)}

    def _scratch_bytes(self):
        from spatial_vae_amd import _lib
        f = self.f
        return {"ws": _lib.lib().svae_pose_expect_workspace_bytes(f["B"], f["n_ref"], f["M"], f["rows"], f["cols"], f["C"], f["A"], f["S"])}

    def steps(self):
        from spatial_vae_amd import _lib
        p, f, ws = self.ptr, self.f, self.scratch["ws"]
        N = f["rows"] * f["cols"]
        return [lambda st: self.L.svae_pose_expect(p("y"), p("ref"), p("weight"), p("log_prior"), p("cand"), p("pose"), f["B"], f["n_ref"],
                                                   f["M"], f["rows"], f["cols"], f["C"], f["A"], float(f["step"]), f["S"],
                                                   _lib.ALIGN_INTERP["bicubic"], INV_SIGMA2, p("contrib"), p("cover_w"), p("class_post"),
                                                   p("log_evidence"), p("best"), ws.ptr, ws.nbytes, st),
                lambda st: self.L.svae_expect_sums_update(p("contrib"), p("cover_w"), p("cand"), p("target"), f["B"], f["M"], N, f["C"],
                                                          f["n_ref"], self.n_classes, p("sum"), p("count"), st)]

    def check(self, out, seed=0):
        """tests/test_gpu_expect.py's bounds against expect_ref; the sums against its walk added to the start values."""
        i, f = self.inputs(seed), self.f
        want = X.pose_expect(i["y"], i["ref"], i["weight"], i["log_prior"], i["cand"], i["pose"], f["rows"], f["cols"], f["A"], f["step"],
                             f["S"], INV_SIGMA2)
        assert want["gap"].min() > 1e-9 and np.array_equal(out["best"], want["best"])
        for k in ("contrib", "cover_w", "class_post"):
            assert np.abs(out[k] - want[k]).max() <= 1e-10 * np.abs(want[k]).max(), k
        assert (np.abs(out["log_evidence"] - want["log_evidence"]) <= 1e-10 * np.maximum(1.0, np.abs(want["log_evidence"]))).all()
        s, c = X.sums_update(i["sum"].copy(), i["count"].copy(), want["contrib"], want["cover_w"], i["cand"], i["target"], f["n_ref"])
        assert np.abs(out["sum"] - s).max() <= 1e-10 * np.abs(s).max() and np.abs(out["count"] - c).max() <= 1e-10 * np.abs(c).max()
        assert not np.array_equal(out["sum"], i["sum"])


def _fresh(seed):
    case = ExpectCase().alloc(_dev())
    case.load(seed)
    case.zero_scratch()
    case.stage_to_real()
    return case


@pytest.fixture(scope="module")
def baselines():
    """The default-stream results of input sets A and B, each held to the reference; computed once."""
    out = []
    for seed in (0, 1):
        case = _fresh(seed)
        S.statuses_ok(case.enqueue(_handle(torch.cuda.current_stream())))
        torch.cuda.synchronize()
        got, bad = case.collect()
        assert not bad, bad
        case.check(got, seed)
        out.append(got)
    assert not np.array_equal(out[0]["sum"], out[1]["sum"]) and not np.array_equal(out[0]["class_post"], out[1]["class_post"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs,
    workspace and outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = ExpectCase().alloc(_dev())
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
    """Captured with set A in the buffers (the capture executes nothing), replayed: baseline A.  Set B written over the inputs
    and the start values of the sums: one replay equals the eager result of B."""
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
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[0], "replayed with set A")
    case.load(1)
    case.stage_to_real()
    case.fill_outputs()
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[1], "replayed with set B against the eager result of B")
