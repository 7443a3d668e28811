"""Every entry point that takes a stream, off the default stream (tests/stream_cases.py holds the callers).

include/svae.h promises that work is enqueued on `stream` and that the library is stateless: any number of streams.  Every
other GPU test hands it the default stream, so a launch or a hipMemsetAsync that went to stream 0, or device state shared
between two calls, would pass them all.  Here each case runs

  a. on a side stream behind a delay kernel, with its inputs, workspace and `saved` still poisoned while the host enqueues:
     the real inputs arrive by copies queued on that same stream, so anything the library sent elsewhere has run on poison
     (the analysis rows once more with the default stream held in a delay of its own, which no call may wait for);
  b. next to a second case on a second stream, the host calls interleaved;

and must reproduce its default-stream baseline bit for bit.  The baseline itself is first held to the float64 reference and
the bound of the case's own test file, so that the comparison is between live numbers.

The delay is torch.cuda._sleep, calibrated once to 100 ms: the host enqueues a case in well under 1 ms.  Each test asserts
that the event recorded behind the delay had NOT completed when the last call returned; if it had, the test fails as
inconclusive (it never skips).

Not every side stream will do.  The HIP runtime multiplexes its streams onto a few hardware queues (four by default), and a
queue executes in order: about one torch stream in four shares the default stream's queue, and a kernel that wrongly went
to stream 0 then still runs behind that stream's delay and copies -- the test would pass.  side_streams() therefore picks,
once per process, two streams that the hardware demonstrably runs BESIDE the default stream and beside each other (work on
one completes while the other sits in a delay kernel), and every test here uses those."""
import contextlib
import ctypes
import functools
import inspect
import io
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn as nn

import stream_cases as S
from decoder_abi import sentinel_hits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELAY_MS = 100.0
ME = "tests/test_gpu_streams.py"


def _dev():
    return torch.device("cuda:0")


def _handle(stream):
    return ctypes.c_void_p(stream.cuda_stream)


@functools.lru_cache(maxsize=None)
def delay_cycles():
    """torch.cuda._sleep's argument for DELAY_MS, from one timed call."""
    probe = 20_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(probe)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.05, "torch.cuda._sleep(%d) took %.4f ms: it does not delay" % (probe, ms)
    return int(probe * DELAY_MS / ms)


def _runs_beside(sleeper, other):
    """True when a small kernel on `other` completes while `sleeper` still sits in a 20 ms delay kernel."""
    probe = torch.zeros(8, device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(sleeper):
        torch.cuda._sleep(delay_cycles() // 5)
    asleep = torch.cuda.Event()
    asleep.record(sleeper)
    with torch.cuda.stream(other):
        probe.add_(1.0)
    done = torch.cuda.Event()
    done.record(other)
    t0 = time.perf_counter()
    while not done.query() and time.perf_counter() - t0 < 0.010:
        pass
    beside = done.query() and not asleep.query()
    torch.cuda.synchronize()
    return beside


@functools.lru_cache(maxsize=None)
def side_streams():
    """Two streams of torch's pool that run beside the default stream and beside each other in both directions."""
    default, found = torch.cuda.default_stream(_dev()), []
    for _ in range(16):
        s = torch.cuda.Stream()
        if _runs_beside(s, default) and all(_runs_beside(s, f) and _runs_beside(f, s) for f in found):
            found.append(s)
        if len(found) == 2:
            return tuple(found)
    pytest.fail("inconclusive: of 16 streams no two ran beside the default stream and each other (found %d)" % len(found))


def _fresh(name, seed=0):
    """The case allocated, input set `seed` in its staging copies and in its inputs, scratch zeroed."""
    case = S.make_case(name).alloc(_dev())
    case.load(seed)
    case.zero_scratch()
    case.stage_to_real()
    return case


def _eager(case, calls=None):
    """The case's calls (or `calls`) on the current stream, synchronised: its outputs, nothing written outside them."""
    S.statuses_ok([call(_handle(torch.cuda.current_stream())) for call in (case.steps() if calls is None else calls)])
    torch.cuda.synchronize()
    out, bad = case.collect()
    assert not bad, (case.name, bad)
    return out


@functools.lru_cache(maxsize=None)
def baseline(name, seed=0):
    """The case's outputs from the default stream with input set `seed`, scratch zeroed; computed once and shared."""
    out = _eager(_fresh(name, seed))
    for a in out.values():
        a.setflags(write=False)
    return out


def assert_bit_equal(name, got, want, what):
    assert set(got) == set(want)
    for k in want:
        a, b = np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)
        assert np.array_equal(a, b), "%s %s: %s differs from the default-stream baseline in %d bytes" % (name, what, k, int((a != b).sum()))


def assert_clean(case, out, bad):
    assert not bad, "%s: written outside %s" % (case.name, bad)
    for k, a in out.items():
        if a.dtype == np.float32 and k not in case.state:
            assert sentinel_hits(a) == 0, (case.name, k)


def behind_a_delay(case, stream):
    """On `stream`, without the host blocking: the delay, zeroes for workspace and `saved`, the device-to-device copies of the
    inputs.  The case's calls and the event are the caller's."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay_cycles())
        case.zero_scratch()
        case.stage_to_real()


def prepared(name):
    """The case allocated, input set A in its staging copies, everything the calls touch poisoned: float inputs -12345.5,
    integer inputs the valid values of set B, workspace and `saved` 0xA5, outputs the sentinel."""
    case = S.make_case(name).alloc(_dev())
    case.load(1)
    case.stage_to_real()
    case.load(0)
    case.poison()
    torch.cuda.synchronize()
    return case


# ---------------------------------------------------------------------------------------------------------------------
# baseline
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_the_default_stream_baseline_is_live(name):
    """Input set A on the default stream against the float64 reference and the bound of the case's own test file where one
    exists (case.has_reference); elsewhere finite, free of the sentinel and not constant.  A check that takes the seed (every
    row of tests/stream_cases_analysis.py) holds set B to its reference too.  Set B gives other numbers, in every output the
    case names in must_differ."""
    case = S.make_case(name)
    out = baseline(name)
    case.check({k: np.array(v) for k, v in out.items()})
    other = baseline(name, 1)
    if "seed" in inspect.signature(case.check).parameters:
        case.check({k: np.array(v) for k, v in other.items()}, seed=1)
    assert any(not np.array_equal(out[k], other[k]) for k in out), name
    for k in case.must_differ:
        assert not np.array_equal(out[k], other[k]), (name, k)


# ---------------------------------------------------------------------------------------------------------------------
# a. late producer on a side stream
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_late_producer_on_a_side_stream(name):
    """The case behind a delay on a side stream, everything it reads poisoned until copies on that stream replace it.
    MI355X: every case of S.NAMES equals its baseline (the rank1_tanh decoder case also in the fp16x3 child); with
    svae_colsum's launch moved to stream 0 in a scratch build the colsum case differs in 131 of 132 bytes."""
    want = baseline(name)
    delay_cycles()
    case = prepared(name)
    s = side_streams()[0]
    behind_a_delay(case, s)
    rcs = case.enqueue(_handle(s))
    done = torch.cuda.Event()
    done.record(s)
    still_pending = not done.query()
    S.statuses_ok(rcs)
    s.synchronize()
    assert still_pending, "inconclusive: the %g ms delay had already run out when the last call returned" % DELAY_MS
    out, bad = case.collect()
    assert_clean(case, out, bad)
    assert_bit_equal(name, out, want, "on a side stream")


@pytest.mark.parametrize("name", S.ANALYSIS_NAMES)
def test_on_a_side_stream_while_the_default_stream_is_busy(name):
    """As above, with the default stream in a delay kernel of its own that is still running when the last call returns: no
    call waited on the null stream or synchronised with it."""
    want = baseline(name)
    delay_cycles()
    case = prepared(name)
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
    assert_clean(case, out, bad)
    assert_bit_equal(name, out, want, "on a side stream")


# ---------------------------------------------------------------------------------------------------------------------
# b. two streams at once
# ---------------------------------------------------------------------------------------------------------------------
PAIRS = [("decoder_rank1_tanh", "decoder_stream_c2_L3"),
         ("decoder_leaky_resid_L4", "gaussian_ctf_n10_k9_lds_mask"),
         ("linear_17x130x33_tanh", "linear_5x49x24_leakyrelu"),
         ("guard_clip", "decoder_many_images"),
         ("iw_stream_B3_inf5_chunks_2_3", "align_3x9x9_sums")]


@pytest.mark.parametrize("first,second", PAIRS, ids=["%s+%s" % p for p in PAIRS])
def test_two_cases_on_two_streams_with_interleaved_calls(first, second):
    """Each case owns its buffers and its stream and sits behind its own delay; the host issues A's first call, B's first
    call, A's second, B's second ...  Both must equal their serial baselines bit for bit."""
    assert first in S.NAMES and second in S.NAMES
    want = [baseline(first), baseline(second)]
    delay_cycles()
    cases = [prepared(first), prepared(second)]
    streams = side_streams()
    assert streams[0].cuda_stream != streams[1].cuda_stream
    for c, s in zip(cases, streams):
        behind_a_delay(c, s)
    steps = [c.steps() for c in cases]
    rcs = []
    for i in range(max(len(st) for st in steps)):
        for st, s in zip(steps, streams):
            if i < len(st):
                rcs.append(st[i](_handle(s)))
    events = [torch.cuda.Event(), torch.cuda.Event()]
    for e, s in zip(events, streams):
        e.record(s)
    still_pending = [not e.query() for e in events]
    S.statuses_ok(rcs)
    torch.cuda.synchronize()
    assert all(still_pending), "inconclusive: a delay had already run out when the last call returned (%s)" % still_pending
    for c, w in zip(cases, want):
        out, bad = c.collect()
        assert_clean(c, out, bad)
        assert_bit_equal(c.name, out, w, "next to another stream")


def _posed_net(seed, hidden, layers):
    import spatial_vae_amd.models as M
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = M.SpatialGenerator(2, hidden, num_layers=layers, activation=nn.Tanh)
    return net.to(_dev())


def test_two_decoders_under_torch_streams_keep_their_scratch_apart():
    """The ops level: SpatialGenerator.forward_posed and its backward for two small nets, each under torch.cuda.stream on a
    stream of its own behind a delay, forward calls first and backward calls after.  Every .grad equals the serial run on the
    default stream bit for bit, and ops._ws_cache holds different buffers under the two stream handles."""
    import cases
    from spatial_vae_amd import ops
    dev = _dev()
    rs = np.random.RandomState(3)
    jobs = []
    for seed, (hidden, layers, n, B) in enumerate([(64, 2, 9, 5), (96, 3, 11, 4)]):
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
        jobs.append(dict(net=_posed_net(20 + seed, hidden, layers), grid=t(cases.coord_grid(n, n)), B=B,
                         theta=t(rs.uniform(-3, 3, B)), dx=t(0.1 * rs.normal(size=(B, 2))), z=t(rs.normal(size=(B, 2))),
                         w=t(rs.normal(size=(B, n * n, 1)) / (n * n))))

    def forward(j):
        return j["net"].forward_posed(j["grid"], j["B"], theta=j["theta"], dx=j["dx"], z=j["z"])

    def grads(j):
        out = [p.grad.clone() for p in j["net"].parameters()]
        for p in j["net"].parameters():
            p.grad = None
        return out

    serial = []
    for j in jobs:
        (forward(j).view_as(j["w"]) * j["w"]).sum().backward()
        serial.append(grads(j))
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) > 0 for gs in serial for g in gs)
    streams = side_streams()
    ys, events = [], []
    for j, s in zip(jobs, streams):
        with torch.cuda.stream(s):
            torch.cuda._sleep(delay_cycles())
            ys.append(forward(j))
    for j, s, y in zip(jobs, streams, ys):
        with torch.cuda.stream(s):
            (y.view_as(j["w"]) * j["w"]).sum().backward()
            events.append(torch.cuda.Event())
            events[-1].record(s)
    still_pending = [not e.query() for e in events]
    torch.cuda.synchronize()
    assert all(still_pending), "inconclusive: a delay had already run out when the last call returned (%s)" % still_pending
    for j, want in zip(jobs, serial):
        got = grads(j)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))
    by_stream = [{k[2]: t for k, t in ops._ws_cache.items() if k[1] == s.cuda_stream} for s in streams]
    assert by_stream[0] and set(by_stream[0]) == set(by_stream[1]), [sorted(map(str, b)) for b in by_stream]
    for key in by_stream[0]:
        a, b = by_stream[0][key], by_stream[1][key]
        assert a.data_ptr() + a.numel() <= b.data_ptr() or b.data_ptr() + b.numel() <= a.data_ptr(), key


# ---------------------------------------------------------------------------------------------------------------------
# c. the same in fp16x3 mode (the amax memset nodes and the atomicMax scales live there)
# ---------------------------------------------------------------------------------------------------------------------
FP16X3_SUBJECTS = ["test_late_producer_on_a_side_stream[decoder_rank1_tanh]",
                   "test_two_cases_on_two_streams_with_interleaved_calls[decoder_rank1_tanh+decoder_stream_c2_L3]",
                   "test_the_default_stream_baseline_is_live[decoder_rank1_tanh]",
                   "test_the_split_kernels_run_on_a_side_stream_when_the_mode_asks"]


def test_the_split_kernels_run_on_a_side_stream_when_the_mode_asks():
    """svae_path_counts around one rank1_tanh forward + backward on a side stream: under SVAE_GEMM=fp16x3 the split forward,
    data-gradient and weight-gradient kernels ran and no fp32 GEMM did; in fp32 mode the reverse."""
    from spatial_vae_amd import _lib
    case = prepared("decoder_rank1_tanh")
    s = side_streams()[0]
    behind_a_delay(case, s)
    _lib.path_counts(reset=True)
    S.statuses_ok(case.enqueue(_handle(s)))
    paths = {k: v for k, v in _lib.path_counts(reset=True).items() if v}
    s.synchronize()
    from test_gpu_decoder_abi import FP32, SPLIT          # the families tests/test_gpu_decoder_abi.py tells the modes by
    if os.environ.get("SVAE_GEMM") == "fp16x3":
        assert _lib.gemm_mode() == "fp16x3"
        assert all(paths.get(k, 0) > 0 for k in SPLIT + ("out_bwd_split",)) and not any(paths.get(k, 0) for k in FP32), paths
    else:
        assert not any(paths.get(k, 0) for k in SPLIT) and all(paths.get(k, 0) > 0 for k in FP32), paths


def test_the_decoder_cases_pass_in_fp16x3_mode():
    """One fresh process (the mode is read once per process) repeats the rank1_tanh case of (a), one decoder pair of (b), the
    baseline's float64 check and the path-count test under SVAE_GEMM=fp16x3."""
    if os.environ.get("SVAE_GEMM") == "fp16x3":
        return                                              # this IS the child
    env = dict(os.environ, SVAE_GEMM="fp16x3")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] +
                         [ME + "::" + t for t in FP16X3_SUBJECTS], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert "%d passed" % len(FP16X3_SUBJECTS) in out.stdout and "failed" not in out.stdout, tail
