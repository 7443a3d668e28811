"""The streaming K-sample scorer (include/svae_stream.h: svae_iw_stream_reset / _update / _finish, ops.IWStream) on its own,
against tests/iw_stream_ref.py: a plain float64 evaluation of the definitions from all samples at once, which knows nothing of
chunks.  Row b*K + k of a chunk is sample k of image b.

Bounds as in tests/test_gpu_iw_kernels.py, formed from the reference's own fp32 error and never from the kernel's output: a
column may be 4x as far from float64 as the fp32 numpy evaluation of the same definition on the same inputs, floor 8 * 2^-24;
errors are helpers.rel_err per column; angles (the weighted rotation and the best sample's) are compared as the wrapped
difference.  Each test prints its figures before it asserts."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from helpers import rel_err
from iw_stream_ref import coords, iw_stream_ref, wrap
from ref64 import U

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
BS, INFS = (1, 3, 257), (1, 3, 5, 12)
CHUNKINGS = ((1,), (5,), (1, 1, 1, 1, 1), (2, 64, 1, 65), (65, 2))


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bound(oracle_err):
    return max(4.0 * oracle_err, 8 * U)


def _poses(inf):
    return [(r, t) for r in (False, True) for t in (False, True) if int(r) + 2 * int(t) <= inf]


@functools.lru_cache(maxsize=None)
def _case(B, K, inf, rotate, translate, theta0=0.3):
    """loglik and log_ratio ~ N(0, 3^2) each, theta = theta0 + 0.5 normal, the other coordinates N(0, 1).  An image whose
    float64 weights would leave fewer than two above 1e-3 (K >= 2) or a resultant length below 0.1 is drawn again, from the
    same generator, until it has: a row with one dominant weight would hide a weighted-mean or atan2 error.  The float64
    reference and its fp32 twin are computed once per case and shared."""
    rs = np.random.RandomState(9000 + 1000 * inf + 37 * B + K + 5 * int(rotate) + 11 * int(translate))
    zd = inf - int(rotate) - 2 * int(translate)
    ll, lr, v = np.empty((B, K), np.float32), np.empty((B, K), np.float32), np.empty((B, K, inf), np.float32)
    for b in range(B):
        for _ in range(1000):
            l, r = (3.0 * rs.normal(size=K)).astype(np.float32), (3.0 * rs.normal(size=K)).astype(np.float32)
            vb = rs.normal(size=(K, inf)).astype(np.float32)
            if rotate:
                vb[:, 0] = (theta0 + 0.5 * rs.normal(size=K)).astype(np.float32)
            row, _, w = iw_stream_ref(l[None], r[None], vb[None], rotate)
            if ((w > 1e-3).sum() >= min(2, K)) and row[0, 5] >= 0.1:
                break
        ll[b], lr[b], v[b] = l, r, vb
    ref = iw_stream_ref(ll, lr, v, rotate)
    assert ((ref[2] > 1e-3).sum(1) >= min(2, K)).all() and (ref[0][:, 5] >= 0.1).all(), "a degenerate row would hide an error"
    f32 = iw_stream_ref(ll, lr, v, rotate, np.float32)
    theta = v[:, :, 0] if rotate else None
    dx = v[:, :, int(rotate):int(rotate) + 2] if translate else None
    zc = v[:, :, inf - zd:] if zd else None
    return ll, lr, theta, dx, zc, ref, f32


def _chunks(arr, c0, c1):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr[:, c0:c1])).to(_dev()).reshape(-1, *arr.shape[2:])


def _run(B, inf, rotate, translate, chunking, ll, lr, theta, dx, zc):
    from spatial_vae_amd import ops
    st = ops.IWStream(B, inf, _dev())
    c0 = 0
    for k in chunking:
        st.update(rotate, translate, False, 0.1, 1.0, math.pi, k, _chunks(ll, c0, c0 + k), _chunks(lr, c0, c0 + k),
                  _chunks(theta, c0, c0 + k), _chunks(dx, c0, c0 + k), _chunks(zc, c0, c0 + k))
        c0 += k
    per_image, out3 = st.finish()
    return per_image.cpu().numpy(), out3.cpu().numpy()


def _column_errors(got, ref, f32, inf, rotate):
    """{column: (error, bound)}; angle columns as wrapped differences over the largest reference angle."""
    out = {}
    for c in range(ref.shape[1]):
        if rotate and c in (6, 6 + inf):
            scale = max(np.abs(ref[:, c]).max(), 1e-30)
            e, o = np.abs(wrap(got[:, c] - ref[:, c])).max() / scale, np.abs(wrap(f32[:, c].astype(np.float64) - ref[:, c])).max() / scale
        else:
            e, o = rel_err(got[:, c], ref[:, c]), rel_err(f32[:, c], ref[:, c])
        out[c] = (float(e), _bound(float(o)))
    return out


@pytest.mark.parametrize("chunking", CHUNKINGS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("B", BS)
def test_stream_against_float64(B, chunking):
    """Every column of per_image and out3 for inf_dim in {1, 3, 5, 12} and every (rotate, translate) that fits (zd = 0
    included), the samples merged in the given chunks; (2, 64, 1, 65) has chunks on both sides of the 64-lane group.  One more
    case per (B, chunking) has theta0 = pi - 0.05, so the samples straddle the +-pi cut.
    MI355X: the worst error is 0.077 to 0.122 of its bound over the fifteen (B, chunking) cases (at most 5.8e-8 against 4.8e-7)."""
    K = sum(chunking)
    worst = (0.0, None)
    todo = [(inf, r, t, 0.3) for inf in INFS for r, t in _poses(inf)] + [(5, True, True, math.pi - 0.05)]
    for inf, rotate, translate, theta0 in todo:
        ll, lr, theta, dx, zc, ref, f32 = _case(B, K, inf, rotate, translate, theta0)
        per_image, out3 = _run(B, inf, rotate, translate, chunking, ll, lr, theta, dx, zc)
        assert per_image.shape == (B, 6 + 2 * inf)
        errs = _column_errors(per_image, ref[0], f32[0], inf, rotate)
        for i in range(3):
            errs["out3[%d]" % i] = (rel_err(out3[i:i + 1], ref[1][i:i + 1]), _bound(rel_err(f32[1][i:i + 1], ref[1][i:i + 1])))
        for c, (e, b) in errs.items():
            if e / b > worst[0]:
                worst = (e / b, (inf, rotate, translate, theta0, c, e, b))
        bad = {c: v for c, v in errs.items() if not v[0] <= v[1]}
        if bad:
            print("stream B%d %s inf%d r%d t%d theta0 %.2f: %s" % (B, chunking, inf, rotate, translate, theta0, bad))
        assert not bad, (inf, rotate, translate, theta0, bad)
        if not rotate:
            assert (per_image[:, 5] == 1.0).all()
        assert (per_image[:, 3] >= 1.0 - 8 * U).all() and (per_image[:, 3] <= K * (1 + 8 * U)).all()
    print("stream B%d chunks %s worst error/bound %.3f at %s" % (B, chunking, worst[0], worst[1]))


def _edge_inputs(levels, B=3, inf=5, k=4, seed=5):
    """Chunks of k samples whose a sit near the given levels (None = every log_ratio -inf); `levels` per chunk is a scalar or one
    entry per image."""
    rs = np.random.RandomState(seed)
    K = k * len(levels)
    ll = (-20.0 + rs.normal(size=(B, K))).astype(np.float32)
    lr = np.empty((B, K), np.float32)
    for c, lev in enumerate(levels):
        for b in range(B):
            lv = lev[b] if isinstance(lev, (tuple, list)) else lev
            lr[b, c * k:(c + 1) * k] = -np.inf if lv is None else (lv + 20.0 + rs.normal(size=k))
    v = rs.normal(size=(B, K, inf)).astype(np.float32)
    v[:, :, 0] = (0.3 + 0.5 * rs.normal(size=(B, K))).astype(np.float32)
    return ll, lr, v


@pytest.mark.parametrize("name,levels", [("low_then_high", (-800.0, 50.0)), ("high_then_low", (50.0, -800.0)),
                                         ("hole_in_the_middle", (-3.0, None, 2.0)), ("hole_first", (None, 1.0)),
                                         ("one_image_all_holes", ((1.0, None, -2.0), (0.0, None, 3.0)))])
def test_dynamic_range_across_chunks(name, levels):
    """B = 3, rotate and translate, inf_dim 5, chunks of 4: a near -800 then near +50 and the reverse (the far-lower chunk's
    sums must underflow to exactly 0: the weighted columns equal, bit for bit, those of the +50 chunk streamed alone -- a
    rescale in the wrong direction overflows, a missing square on s2 moves the sample size); a middle chunk and a first chunk
    whose a are all -inf; an image that is -inf throughout (bound -inf, sample size 0, R 0, weighted means 0, best = its first
    sample, best a = -inf).  No NaN anywhere; finite columns to 8 * 2^-24 of the float64 reference.
    MI355X: every case holds; the weighted columns of the +50 chunk are bit-equal with and without the -800 chunk."""
    B, inf, k = 3, 5, 4
    ll, lr, v = _edge_inputs(levels)
    ref, ref3, _ = iw_stream_ref(ll, lr, v, True)
    theta, dx, zc = v[:, :, 0], v[:, :, 1:3], v[:, :, 3:]
    got, got3 = _run(B, inf, True, True, (k,) * len(levels), ll, lr, theta, dx, zc)
    print("%s got\n%s\nref\n%s\nout3 %s ref %s" % (name, got, ref, got3, ref3))
    assert not np.isnan(got).any() and not np.isnan(got3).any()
    for c in range(ref.shape[1]):
        fin = np.isfinite(ref[:, c])
        assert np.array_equal(got[~fin, c], ref[~fin, c].astype(np.float32)), (c, got[:, c], ref[:, c])
        if fin.any():
            d = np.abs(wrap(got[fin, c] - ref[fin, c])) if c in (6, 6 + inf) else np.abs(got[fin, c] - ref[fin, c])
            assert (d <= 8 * U * max(np.abs(ref[fin, c]).max(), 1e-30)).all(), (c, got[:, c], ref[:, c])
    for i in range(3):
        if math.isfinite(ref3[i]):
            assert abs(got3[i] - ref3[i]) <= 8 * U * abs(ref3[i])
        else:
            assert got3[i] == np.float32(ref3[i])
    if name in ("low_then_high", "high_then_low"):
        hi = 1 if name == "low_then_high" else 0
        sl = slice(hi * k, (hi + 1) * k)
        alone, _ = _run(B, inf, True, True, (k,), ll[:, sl], lr[:, sl], theta[:, sl], dx[:, sl], zc[:, sl])
        cols = [3, 4, 5] + list(range(6, 6 + 2 * inf))
        assert np.array_equal(got[:, cols], alone[:, cols])
    if name == "one_image_all_holes":
        row = got[1]
        assert row[0] == -np.inf and row[3] == 0.0 and row[4] == -np.inf and row[5] == 0.0
        assert (row[6:6 + inf] == 0.0).all() and np.array_equal(row[6 + inf:], v[1, 0])


@functools.lru_cache(maxsize=None)
def _head_inputs(B, K):
    rs = np.random.RandomState(700 + 11 * B + K)
    ll = (-300.0 + 5.0 * rs.normal(size=(B, 1)) + 1.5 * rs.normal(size=(B, K))).astype(np.float32)
    lr = (-4.0 + 0.3 * rs.normal(size=(B, K))).astype(np.float32)
    return ll, lr


@pytest.mark.parametrize("K", [2, 5, 64, 65])
def test_one_chunk_agrees_with_iw_head(K):
    """B = 257, one chunk: finish's out3 against ops.iw_head's on the same inputs within 2 ulp of fp32 per element (both round
    one double; only the order of summation differs), and the sample size against 1 / sum_k w^2 of iw_head's weights, held to
    the file's bound (fp32 numpy sample size against float64).
    MI355X: 0 ulp on all three scalars at every K; sample size within 9.3e-8 (bounds 2.5e-5 and up)."""
    from spatial_vae_amd import ops
    B, inf = 257, 1
    ll, lr = _head_inputs(B, K)
    dev = _dev()
    l, r = torch.from_numpy(ll).to(dev).reshape(-1), torch.from_numpy(lr).to(dev).reshape(-1)
    head = torch.stack(list(ops.iw_head(l, r, K))).cpu().numpy()
    lg = l.clone().requires_grad_(True)
    (ops.iw_head(lg, r, K)[0] * B).backward()                    # d(B * bound)/d loglik = the softmax weights
    w = lg.grad.cpu().numpy().astype(np.float64).reshape(B, K)
    st = ops.IWStream(B, inf, dev)
    zc = torch.zeros(B * K, 1, device=dev)
    st.update(False, False, False, 0.1, 1.0, math.pi, K, l, r, None, None, zc)
    per_image, out3 = st.finish()
    per_image, out3 = per_image.cpu().numpy(), out3.cpu().numpy()
    ulps = np.abs(out3.astype(np.float64) - head.astype(np.float64)) / np.spacing(np.abs(head)).astype(np.float64)
    ref, _, _ = iw_stream_ref(ll, lr, np.zeros((B, K, 1), np.float32), False)
    f32, _, _ = iw_stream_ref(ll, lr, np.zeros((B, K, 1), np.float32), False, np.float32)
    e, b = rel_err(per_image[:, 3], 1.0 / (w * w).sum(1)), _bound(rel_err(f32[:, 3], ref[:, 3]))
    print("K%d out3 %s head %s ulps %s; ess error %.2e bound %.2e" % (K, out3, head, ulps, e, b))
    assert (ulps <= 2).all()
    assert e <= b


def _raw_state(L, B, inf, pad=32):
    n = L.svae_iw_stream_state_bytes(B, inf) // 8
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float64, device=_dev())
    return buf, buf[pad:pad + n], n, pad


@pytest.mark.parametrize("B,chunking", [(3, (5,)), (257, (2, 64, 1, 65))])
def test_determinism_and_containment(B, chunking):
    """The same chunking twice gives a bit-equal per_image and out3; finish twice without an update in between is bit-equal;
    the state, per_image and out3 sit inside sentinel-filled buffers and the sentinels are intact after reset, every update
    and both finishes.  MI355X: equal, sentinels intact."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    inf, rotate, translate = 12, True, True
    K = sum(chunking)
    ll, lr, theta, dx, zc, _, _ = _case(B, K, inf, rotate, translate)
    desc = _lib.LatentDesc(B, inf, 1, 1, 0, 0.1, 1.0, math.pi)
    assert L.svae_iw_stream_state_bytes(B, inf) % 8 == 0 and L.svae_iw_stream_state_bytes(B, inf) > 0
    runs = []
    for _ in range(2):
        buf, state, n, pad = _raw_state(L, B, inf)
        width = 6 + 2 * inf
        pi = [torch.full((B * width + 64,), SENTINEL, device=_dev()) for _ in range(2)]
        o3 = [torch.full((3 + 64,), SENTINEL, device=_dev()) for _ in range(2)]
        with torch.cuda.device(_dev()):
            _lib.check(L.svae_iw_stream_reset(state.data_ptr(), B, inf, _stream()))
            c0 = 0
            for k in chunking:
                t = [_chunks(a, c0, c0 + k) for a in (ll, lr, theta, dx, zc)]
                _lib.check(L.svae_iw_stream_update(state.data_ptr(), ctypes.byref(desc), k, *[a.data_ptr() for a in t], _stream()))
                c0 += k
                torch.cuda.synchronize()                                 # the chunk tensors stay alive until their kernel ran
            for i in range(2):
                _lib.check(L.svae_iw_stream_finish(state.data_ptr(), ctypes.byref(desc), pi[i].data_ptr(), o3[i].data_ptr(), _stream()))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:pad] == SENTINEL).all() and (host[pad + n:] == SENTINEL).all()
        pi, o3 = [t.cpu().numpy() for t in pi], [t.cpu().numpy() for t in o3]
        for i in range(2):
            assert (pi[i][B * width:] == SENTINEL).all() and (o3[i][3:] == SENTINEL).all()
            assert not (pi[i][:B * width] == SENTINEL).any()
        assert np.array_equal(pi[0], pi[1]) and np.array_equal(o3[0], o3[1])
        runs.append((pi[0], o3[0], host))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_invalid_calls_are_refused():
    """Argument checks only -- nothing here launches a kernel that could misbehave: K = 0, -1 and 1025, B*K >= 2^31, a null
    loglik / log_ratio / theta / dx / zc / state, an inf_dim and a B that disagree with the state's, a state that was never
    reset, finish before any update and finish with a null per_image all return SVAE_E_INVALID with a message, and leave the
    state and the outputs as they were; out3 = NULL is accepted.  ops.IWStream refuses CPU tensors.
    MI355X: every call refused as listed, buffers untouched."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    dev = _dev()
    B, inf, K = 2, 5, 3
    desc = _lib.LatentDesc(B, inf, 1, 1, 0, 0.1, 1.0, math.pi)
    buf, state, n, pad = _raw_state(L, B, inf)
    per_image = torch.full((B * (6 + 2 * inf),), SENTINEL, device=dev)
    out3 = torch.full((3,), SENTINEL, device=dev)
    t = {k: torch.zeros(B * 1025 * w, device=dev) for k, w in (("ll", 1), ("lr", 1), ("theta", 1), ("dx", 2), ("zc", 2))}
    p = {k: v.data_ptr() for k, v in t.items()}
    assert L.svae_iw_stream_state_bytes(0, inf) == 0 and L.svae_iw_stream_state_bytes(B, 0) == 0

    def update(d=desc, K=K, state=state.data_ptr(), **over):
        q = dict(p, **over)
        return L.svae_iw_stream_update(state, ctypes.byref(d), K, q["ll"], q["lr"], q["theta"], q["dx"], q["zc"], _stream())

    with torch.cuda.device(dev):
        assert L.svae_iw_stream_reset(None, B, inf, _stream()) == _lib.E_INVALID
        assert L.svae_iw_stream_reset(state.data_ptr(), 0, inf, _stream()) == _lib.E_INVALID
        # an address no reset was ever given: one double into this test's own buffer
        assert update(state=buf.data_ptr() + 8) == _lib.E_INVALID and b"never reset" in L.svae_last_error()
        _lib.check(L.svae_iw_stream_reset(state.data_ptr(), B, inf, _stream()))
        torch.cuda.synchronize()
        fresh = buf.clone()
        assert L.svae_iw_stream_finish(state.data_ptr(), ctypes.byref(desc), per_image.data_ptr(), out3.data_ptr(),
                                       _stream()) == _lib.E_INVALID
        assert b"no chunk" in L.svae_last_error()
        for bad in (0, -1, 1025):
            assert update(K=bad) == _lib.E_INVALID and b"K" in L.svae_last_error()
        huge = _lib.LatentDesc(1 << 22, inf, 1, 1, 0, 0.1, 1.0, math.pi)
        assert update(d=huge, K=1024) == _lib.E_INVALID and b"out of range" in L.svae_last_error()
        for name in ("ll", "lr", "theta", "dx", "zc"):
            assert update(**{name: None}) == _lib.E_INVALID and b"null" in L.svae_last_error(), name
        assert update(state=None) == _lib.E_INVALID
        for d in (_lib.LatentDesc(B, inf + 1, 1, 1, 0, 0.1, 1.0, math.pi), _lib.LatentDesc(B + 1, inf, 1, 1, 0, 0.1, 1.0, math.pi)):
            assert update(d=d) == _lib.E_INVALID and b"reset for" in L.svae_last_error()
        torch.cuda.synchronize()
        assert torch.equal(buf, fresh) and bool((per_image == SENTINEL).all()) and bool((out3 == SENTINEL).all())
        _lib.check(update())
        assert L.svae_iw_stream_finish(state.data_ptr(), ctypes.byref(desc), None, out3.data_ptr(), _stream()) == _lib.E_INVALID
        wrong = _lib.LatentDesc(B, inf + 1, 1, 1, 0, 0.1, 1.0, math.pi)
        assert L.svae_iw_stream_finish(state.data_ptr(), ctypes.byref(wrong), per_image.data_ptr(), None, _stream()) == _lib.E_INVALID
        torch.cuda.synchronize()
        assert bool((per_image == SENTINEL).all()) and bool((out3 == SENTINEL).all())
        _lib.check(L.svae_iw_stream_finish(state.data_ptr(), ctypes.byref(desc), per_image.data_ptr(), None, _stream()))
        torch.cuda.synchronize()
    assert bool((out3 == SENTINEL).all()) and not bool((per_image == SENTINEL).any())
    host = buf.cpu().numpy()
    assert (host[:pad] == SENTINEL).all() and (host[pad + n:] == SENTINEL).all()
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.IWStream(B, inf, "cpu")
    st = ops.IWStream(B, inf, dev)
    with pytest.raises(RuntimeError, match="HIP device"):
        st.update(True, True, False, 0.1, 1.0, math.pi, K, torch.zeros(B * K), t["lr"][:B * K], t["theta"][:B * K],
                  t["dx"][:2 * B * K].view(-1, 2), t["zc"][:2 * B * K].view(-1, 2))
    with pytest.raises(RuntimeError, match="no chunk"):
        st.finish()
