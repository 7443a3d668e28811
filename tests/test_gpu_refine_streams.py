"""The pose search (include/svae_refine.h) off the default stream and under graph capture and replay, as one row of the kind
tests/stream_cases.py holds (that file's Case is the base; the table itself is not extended).  The baseline is first held to
tests/refine_ref.py within tests/test_gpu_refine.py's bounds, so the comparisons are between live numbers."""
import numpy as np
import pytest
import torch

import refine_ref as R
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu


class RefineCase(S.Case):
    """17 x 13 x 2 (odd by odd, oblong; LDS form, so there is no workspace), 4 images of which one is in no class, two
    references, a weight, A = 2, S = 1, bicubic."""
    name, entry_points, has_reference = "pose_search_17x13x2_B4", ("svae_pose_search",), True
    rows, cols, C, B, A, step, Sh = 17, 13, 2, 4, 2, 0.06, 1

    def inputs(self, seed):
        from spatial_vae_amd import elbo as E
        rs = np.random.RandomState(900 + seed)
        N = self.rows * self.cols
        y = rs.normal(size=(self.B, self.rows, self.cols, self.C))
        y = (y + np.roll(y, 1, 1) + np.roll(y, 1, 2)).reshape(self.B, N, self.C).astype(np.float32)
        pose = np.concatenate([rs.uniform(-3, 3, (self.B, 1)), rs.uniform(-0.1, 0.1, (self.B, 2))], 1).astype(np.float32)
        return {"y": y, "ref": rs.normal(size=(2, N, self.C)), "weight": E.refine_mask(self.rows, self.cols, self.Sh).reshape(-1),
                "ref_index": np.array([0, 1, -1, 1], np.int32), "pose_in": pose}

    def _outputs(self):
        nA, nS = 2 * self.A + 1, 2 * self.Sh + 1
        return {"pose_out": ((self.B, 3), np.float32), "score": ((self.B,), np.float64), "offset": ((self.B, 4), np.int32),
                "scores": ((self.B, nA, nS, nS), np.float64)}

    def _scratch_bytes(self):
        from spatial_vae_amd import _lib
        return {"ws": _lib.lib().svae_pose_search_workspace_bytes(self.B, self.rows, self.cols, self.C, self.A, self.Sh)}

    def steps(self):
        p, ws = self.ptr, self.scratch.get("ws")
        return [lambda st: self.L.svae_pose_search(p("y"), p("ref"), p("weight"), p("ref_index"), p("pose_in"), self.B, 2, self.rows,
                                                   self.cols, self.C, self.A, self.step, self.Sh, 1, p("pose_out"), p("score"),
                                                   p("offset"), p("scores"), ws.ptr if ws else None, ws.nbytes if ws else 0, st)]

    def check(self, out, seed=0):
        from test_gpu_refine import MARGIN, TOL_POSE, TOL_SCORE
        i = self.inputs(seed)
        want = R.pose_search(i["y"], i["ref"], i["weight"], i["ref_index"], i["pose_in"], self.rows, self.cols, self.A, self.step,
                             self.Sh, "bicubic")
        assert want["margin"][[0, 1, 3]].min() > MARGIN
        assert np.abs(out["scores"] - want["scores"]).max() <= TOL_SCORE and np.abs(out["score"] - want["score"]).max() <= TOL_SCORE
        assert np.array_equal(out["offset"], want["offset"]) and out["offset"][2].tolist() == [0, 0, 0, R.SKIPPED]
        assert np.abs(out["pose_out"].astype(np.float64) - want["pose"].astype(np.float64)).max() <= TOL_POSE


def _fresh(seed):
    case = RefineCase().alloc(_dev())
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
    assert not np.array_equal(out[0]["scores"], out[1]["scores"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs and
    outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = RefineCase().alloc(_dev())
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
