"""The ring-correlation calls (include/svae_frc.h) off the default stream and under graph capture and replay: svae_frc, then
svae_frc_filter of the first half with weights the case holds, as one row of the kind tests/stream_cases.py holds (that file's
Case is the base; the table itself is not extended).  The baseline is first held to tests/frc_ref.py within
tests/test_gpu_frc.py's bounds, so the comparisons are between live numbers."""
import numpy as np
import pytest
import torch

import frc_ref as F
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu


class FrcCase(S.Case):
    """13 x 10 (odd by even, oblong; LDS form, so there is no workspace), 3 planes, the default mask (2, 3)."""
    name, entry_points, has_reference = "frc_13x10_P3", ("svae_frc", "svae_frc_filter"), True
    n, m, P = 13, 10, 3
    R = 6

    def inputs(self, seed):
        a, b = F.half_planes(70 + seed, self.n, self.m, self.P)
        rs = np.random.RandomState(700 + seed)
        return {"a": a.copy(), "b": b.copy(), "weight": rs.uniform(0.0, 1.0, size=(self.P, self.R))}

    def _outputs(self):
        return {"sums": ((self.P, self.R, 3), np.float64), "frc": ((self.P, self.R), np.float64), "ring_count": ((self.R,), np.int32),
                "filtered": ((self.P, self.n, self.m), np.float32)}

    def _scratch_bytes(self):
        return {"ws": self.L_bytes()}

    def L_bytes(self):
        from spatial_vae_amd import _lib
        return _lib.lib().svae_frc_workspace_bytes(self.P, self.n, self.m)

    def steps(self):
        p, ws = self.ptr, self.scratch.get("ws")
        radius, edge = F.default_mask(self.n, self.m)
        return [lambda st: self.L.svae_frc(p("a"), p("b"), self.P, self.n, self.m, radius, edge, p("sums"), p("frc"), p("ring_count"),
                                           ws.ptr if ws else None, ws.nbytes if ws else 0, st),
                lambda st: self.L.svae_frc_filter(p("a"), p("weight"), self.P, self.n, self.m, p("filtered"), ws.ptr if ws else None,
                                                  ws.nbytes if ws else 0, st)]

    def check(self, out, seed=0):
        from test_gpu_frc import TOL_FILTER, TOL_FRC, TOL_SUMS
        i = self.inputs(seed)
        sums, curve, counts = F.frc(i["a"], i["b"], self.n, self.m, *F.default_mask(self.n, self.m))
        assert np.array_equal(out["ring_count"], counts)
        scale = sums[..., 1:].reshape(self.P, -1).max(1)
        assert (np.abs(out["sums"] - sums).reshape(self.P, -1).max(1) / scale).max() <= TOL_SUMS
        assert np.abs(out["frc"] - curve).max() <= TOL_FRC
        want = F.filter_planes(i["a"], i["weight"], self.n, self.m)
        err = np.abs(out["filtered"] - want).reshape(self.P, -1).max(1) / np.abs(want).reshape(self.P, -1).max(1)
        assert err.max() <= TOL_FILTER


def _fresh(seed):
    case = FrcCase().alloc(_dev())
    case.load(seed)
    case.zero_scratch()
    case.stage_to_real()
    return case


def _eager(case):
    S.statuses_ok(case.enqueue(_handle(torch.cuda.current_stream())))
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
    assert not np.array_equal(out[0]["frc"], out[1]["frc"]) and np.array_equal(out[0]["ring_count"], out[1]["ring_count"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs and
    outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = FrcCase().alloc(_dev())
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
    one replay equals the eager result of B."""
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
