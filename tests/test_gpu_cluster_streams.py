"""The k-means calls (include/svae_cluster.h) off the default stream and under graph capture and replay: seed, two update
steps, one assign-only step, as one row of the kind tests/stream_cases.py holds (that file's Case is the base; the table itself
is not extended).  The baseline is first held to tests/kmeans_ref.py bit for bit, so the comparisons are between live numbers."""
import numpy as np
import pytest
import torch

import kmeans_ref as K
import stream_cases as S
from test_gpu_streams import DELAY_MS, _dev, _handle, assert_bit_equal, behind_a_delay, delay_cycles, side_streams

pytestmark = pytest.mark.gpu


class KMeansCase(S.Case):
    """N = 600 (three chunks, the last of 88 points), D = 3, k = 4.  The record is the calls' to advance: state."""
    name, entry_points, has_reference = "kmeans_N600_D3_k4", ("svae_kmeans_seed", "svae_kmeans_step"), True
    state = ("rec",)
    N, D, k = 600, 3, 4

    def inputs(self, seed):
        x, u = K.blobs(40 + seed, self.N, self.D, self.k)
        return {"x": x, "u": u, "rec": np.zeros(6, np.int64)}

    def _outputs(self):
        return {"centres": ((self.k, self.D), np.float64), "label": ((self.N,), np.int32), "members": ((self.k,), np.int64),
                "seed_index": ((self.k,), np.int32)}

    def _scratch_bytes(self):
        return {"ws": self.L_bytes()}

    def L_bytes(self):
        from spatial_vae_amd import _lib
        return _lib.lib().svae_kmeans_workspace_bytes(self.N, self.D, self.k)

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        seed = lambda st: self.L.svae_kmeans_seed(p("x"), self.N, self.D, self.k, p("u"), p("centres"), p("seed_index"), ws.ptr, ws.nbytes, st)
        step = lambda update: (lambda st: self.L.svae_kmeans_step(p("x"), self.N, self.D, self.k, update, p("centres"), p("label"),
                                                                  p("members"), p("rec"), ws.ptr, ws.nbytes, st))
        return [seed, step(1), step(1), step(0)]

    def check(self, out, seed=0):
        i = self.inputs(seed)
        want = K.fit(i["x"], self.k, i["u"], 2)
        assert np.array_equal(out["label"], want["label"]) and np.array_equal(out["members"], want["members"])
        assert np.array_equal(out["seed_index"], want["seed_index"])
        assert np.array_equal(out["centres"].view(np.uint64), want["centres"].view(np.uint64))
        rec = out["rec"]
        assert rec[:5].tolist() == [2, want["changed"], want["converged_at"], self.N, want["empty"]]
        assert rec[5:].view(np.float64)[0] == want["inertia"]


def _fresh(seed):
    case = KMeansCase().alloc(_dev())
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
    assert not np.array_equal(out[0]["centres"], out[1]["centres"])
    return out


def test_on_a_side_stream_while_the_default_stream_is_busy(baselines):
    """The default stream sits in a delay kernel; the case runs on a side stream behind a delay of its own, with its inputs,
    workspace and outputs poisoned until copies on that stream replace them.  Bit-equal to the default-stream baseline."""
    delay_cycles()
    case = KMeansCase().alloc(_dev())
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
    and a fresh record: one replay equals the eager result of B.  Replays without restoring the record advance its count: the
    iterations live on the device."""
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
    case.stage_to_real()                            # set B, and the record back to zero bytes
    case.fill_outputs()
    g.replay()
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, bad
    assert_bit_equal(case.name, out, baselines[1], "replayed with set B against the eager result of B")
    for n in (2, 3):
        g.replay()
        torch.cuda.synchronize()
        out, bad = case.collect()
        assert not bad and out["rec"][0] == 2 * n, (n, out["rec"])
        assert np.array_equal(out["seed_index"], baselines[1]["seed_index"])
    # the same calls made eagerly on a record that already counts: equal to the replays, count included
    eager = _fresh(1)
    for _ in range(3):
        want = _eager(eager)
    assert_bit_equal(case.name, out, want, "three replays against three eager sequences")
