"""Multi-reference alignment (include/svae_classify.h) off the default stream and under graph capture and replay, as one row of
the kind tests/stream_cases.py holds (that file's Case is the base; the table itself is not extended).  Both launches of the
call, the norms and the search, go to the stream it is handed.  The baseline is first held to tests/classify_ref.py within
tests/test_gpu_refine.py's bounds, so the comparisons are between live numbers."""
import numpy as np
import pytest
import torch

import classify_ref as CR
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu


class ClassifyCase(S.Case):
    """17 x 13 x 2 (odd by odd, oblong; LDS form, the workspace holding the norms alone), 4 images of which one has no slot, five
    slots over six references (one all zero, one slot empty), a weight, A = 2, S = 1, bicubic."""
    name, entry_points, has_reference = "pose_classify_17x13x2_B4_M5", ("svae_pose_classify",), True
    rows, cols, C, B, M, n_ref, A, step, Sh = 17, 13, 2, 4, 5, 6, 2, 0.06, 1

    def inputs(self, seed):
        from spatial_vae_amd import elbo as E
        rs = np.random.RandomState(950 + seed)
        N = self.rows * self.cols
        y = rs.normal(size=(self.B, self.rows, self.cols, self.C))
        y = (y + np.roll(y, 1, 1) + np.roll(y, 1, 2)).reshape(self.B, N, self.C).astype(np.float32)
        pose = np.concatenate([rs.uniform(-3, 3, (self.B, 1)), rs.uniform(-0.1, 0.1, (self.B, 2))], 1).astype(np.float32)
        ref = rs.normal(size=(self.n_ref, N, self.C))
        ref[3] = 0.0
        cand = np.array([[0, 1, 2, 3, 4], [5, -1, 0, 1, 2], [-1, -1, -1, -1, -1], [4, 3, 5, 1, 0]], np.int32)
        return {"y": y, "ref": ref, "weight": E.refine_mask(self.rows, self.cols, self.Sh).reshape(-1), "cand": cand, "pose_in": pose}

    def _outputs(self):
        return {"choice": ((self.B,), np.int32), "ref_chosen": ((self.B,), np.int32), "cand_score": ((self.B, self.M), np.float64),
                "margin": ((self.B,), np.float64)}

    def _scratch_bytes(self):
        from spatial_vae_amd import _lib
        return {"ws": _lib.lib().svae_pose_classify_workspace_bytes(self.B, self.n_ref, self.M, self.rows, self.cols, self.C)}

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        return [lambda st: self.L.svae_pose_classify(p("y"), p("ref"), p("weight"), p("cand"), p("pose_in"), self.B, self.n_ref, self.M,
                                                     self.rows, self.cols, self.C, self.A, self.step, self.Sh, 1, p("choice"),
                                                     p("ref_chosen"), p("cand_score"), p("margin"), ws.ptr, ws.nbytes, st)]

    def check(self, out, seed=0):
        from test_gpu_refine import MARGIN, TOL_SCORE
        i = self.inputs(seed)
        want = CR.pose_classify(i["y"], i["ref"], i["weight"], i["cand"], i["pose_in"], self.rows, self.cols, self.A, self.step,
                                self.Sh, "bicubic")
        assert want["margin"][[0, 1, 3]].min() > MARGIN and want["choice"][2] == -1
        finite = np.isfinite(want["cand_score"])
        assert np.array_equal(np.isneginf(out["cand_score"]), ~finite)
        assert np.abs(out["cand_score"][finite] - want["cand_score"][finite]).max() <= TOL_SCORE
        assert np.array_equal(out["choice"], want["choice"]) and np.array_equal(out["ref_chosen"], want["ref_chosen"])
        assert out["margin"][2] == np.inf and np.abs(out["margin"][[0, 1, 3]] - want["margin"][[0, 1, 3]]).max() <= TOL_SCORE


def _fresh(seed):
    case = ClassifyCase().alloc(_dev())
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
    assert not np.array_equal(out[0]["cand_score"], out[1]["cand_score"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs and
    outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = ClassifyCase().alloc(_dev())
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
