"""The PCA calls (include/svae_pca.h) off the default stream and under graph capture and replay: moments, eigen, project, as
one row of the kind tests/stream_cases.py holds (that file's Case is the base; the table itself is not extended).  The three
calls form a single chain on one stream, so the captured graph has no parallel branches.  The baseline is first held to
tests/pca_ref.py, so the comparisons are between live numbers."""
import functools

import numpy as np
import pytest
import torch

import pca_ref as R
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inputs(seed, N, D, G):
    return R.labelled(60 + seed, N, D, G)


class PcaCase(S.Case):
    """N = 600 (three chunks, the last of 88 points), D = 3, G = 4: two live groups, one of a single member, one empty; labels
    outside [0, G) and two non-finite rows.  P = 2 of the 3 components are projected."""
    name, entry_points, has_reference = "pca_N600_D3_G4", ("svae_pca_moments", "svae_pca_eigen", "svae_pca_project"), True
    N, D, G, P = 600, 3, 4, 2

    def inputs(self, seed):
        x, group = _inputs(seed, self.N, self.D, self.G)
        return {"x": x, "group": group}

    def _outputs(self):
        G, D = self.G, self.D
        return {"count": ((G,), np.int64), "mean": ((G, D), np.float64), "cov": ((G, D, D), np.float64),
                "eigenvalues": ((G, D), np.float64), "components": ((G, D, D), np.float64), "sweeps": ((G,), np.int32),
                "off_norm": ((G,), np.float64), "proj": ((self.N, self.P), np.float64)}

    def _scratch_bytes(self):
        from spatial_vae_amd import _lib
        return {"ws": _lib.lib().svae_pca_workspace_bytes(self.N, self.D, self.G)}

    def steps(self):
        p, ws, L = self.ptr, self.scratch["ws"], self.L
        N, D, G, P = self.N, self.D, self.G, self.P
        return [lambda st: L.svae_pca_moments(p("x"), N, D, G, p("group"), p("count"), p("mean"), p("cov"), ws.ptr, ws.nbytes, st),
                lambda st: L.svae_pca_eigen(p("cov"), D, G, p("eigenvalues"), p("components"), p("sweeps"), p("off_norm"), st),
                lambda st: L.svae_pca_project(p("x"), N, D, G, P, p("group"), p("count"), p("mean"), p("components"), p("proj"), st)]

    def check(self, out, seed=0):
        i = self.inputs(seed)
        want = R.fit(i["x"], i["group"], self.G, self.P)
        assert np.array_equal(out["count"], want["count"]) and np.array_equal(out["sweeps"], want["sweeps"])
        assert sorted(want["count"].tolist())[:2] == [0, 1] and (want["sweeps"] > 0).sum() == 2
        for key in ("mean", "cov", "eigenvalues", "components", "off_norm", "proj"):
            assert np.abs(out[key] - want[key]).max() <= 1e-10 * max(1.0, np.abs(want[key]).max()), key


def _fresh(seed):
    case = PcaCase().alloc(_dev())
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
    assert not np.array_equal(out[0]["mean"], out[1]["mean"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs,
    workspace and outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = PcaCase().alloc(_dev())
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
    and the outputs refilled: one replay equals the eager result of B, and a second replay changes no bit."""
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
    for what in ("replayed with set B against the eager result of B", "replayed once more"):
        g.replay()
        torch.cuda.synchronize()
        out, bad = case.collect()
        assert not bad, bad
        assert_bit_equal(case.name, out, baselines[1], what)
