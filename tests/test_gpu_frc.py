"""The ring-correlation kernels (include/svae_frc.h: svae_frc, svae_frc_filter; ops.frc, ops.frc_filter) on the MI355X against
the float64 reference tests/frc_ref.py (np.fft), shape by shape, with and without the mask, then every refusal of the header
with the buffers prefilled and compared."""
import functools

import numpy as np
import pytest
import torch

import frc_ref as F

pytestmark = pytest.mark.gpu
TOL_SUMS = 1e-11    # of the plane's largest pa / pb entry: a length-len double DFT is ~len 2^-53 of the plane's norm
TOL_FRC = 1e-9      # absolute: the ratio's error is ~1e-13 at these sizes; four orders left for sincospi and sqrt
TOL_FILTER = 2e-6   # tests/test_gpu_ctfcorr.py's TOL: the same construction with one fp32 rounding
MIN_RING_POWER = 1e-6
# (n, m, planes): even square, odd by even and oblong, even square, config 5's box, the largest planes that stay in LDS (71 x 71:
# 32 n m + 16 (n + m) bytes in 160 KiB) and the first that take a workspace, a non-square workspace shape, and more planes
# than the 512 workgroups of the workspace form (the grid strides)
SHAPES = [(8, 8, 3), (13, 10, 3), (12, 12, 3), (40, 40, 5), (71, 71, 2), (72, 72, 2), (96, 90, 2), (72, 72, 515)]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(n, m, planes, masked):
    """The shared, read-only inputs and references of one shape: the half planes, the mask, the reference's sums, FRC, ring
    counts, weights and filtered first halves."""
    a, b = F.half_planes(n * m + planes, n, m, planes)
    radius, edge = F.default_mask(n, m) if masked else (0.0, 0.0)
    sums, curve, counts = F.frc(a, b, n, m, radius, edge)
    weights = F.weight(curve)
    filtered = F.filter_planes(a, weights, n, m)
    for x in (sums, curve, counts, weights, filtered):
        x.setflags(write=False)
    return {"a": a, "b": b, "radius": radius, "edge": edge, "sums": sums, "frc": curve, "count": counts, "weight": weights,
            "filtered": filtered}


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("n,m,planes", SHAPES)
def test_frc_matches_the_reference(n, m, planes, masked):
    """svae_frc against np.fft: the ring sums within 1e-11 of the plane's largest pa / pb entry, the FRC within 1e-9, the ring
    counts equal, a second run bit-equal; every ring of the reference keeps at least 1e-6 of the largest ring's power per
    frequency (a condition on the reference; 1.8e-5 at worst).  MI355X: sums at most 1.3e-15, FRC at most 1.0e-15 over all
    shapes."""
    from spatial_vae_amd import ops
    c = _case(n, m, planes, masked)
    kept = F.rings_keep_power(c["sums"], c["count"])
    assert kept >= MIN_RING_POWER, kept
    a, b = torch.tensor(c["a"]).to(DEV), torch.tensor(c["b"]).to(DEV)
    sums, curve, counts = ops.frc(a, b, n, m, c["radius"], c["edge"])
    again = ops.frc(a.reshape(planes, n * m), b.reshape(planes, n * m), n, m, c["radius"], c["edge"])
    R = min(n, m) // 2 + 1
    assert sums.shape == (planes, R, 3) and curve.shape == (planes, R) and counts.shape == (R,)
    assert sums.dtype == curve.dtype == torch.float64 and counts.dtype == torch.int32
    assert torch.equal(sums, again[0]) and torch.equal(curve, again[1]) and torch.equal(counts, again[2])
    sums, curve, counts = sums.cpu().numpy(), curve.cpu().numpy(), counts.cpu().numpy()
    scale = c["sums"][..., 1:].reshape(planes, -1).max(1)
    e_sums = float((np.abs(sums - c["sums"]).reshape(planes, -1).max(1) / scale).max())
    e_frc = float(np.abs(curve - c["frc"]).max())
    print("%dx%d planes=%d %s: sums %.2e of the largest power, frc %.2e (least ring power %.1e)"
          % (n, m, planes, "masked" if masked else "no mask", e_sums, e_frc, kept))
    assert np.array_equal(counts, c["count"])
    assert np.isfinite(sums).all() and np.isfinite(curve).all()
    assert e_sums <= TOL_SUMS and e_frc <= TOL_FRC


@pytest.mark.parametrize("n,m,planes", SHAPES)
def test_filter_matches_the_reference(n, m, planes):
    """svae_frc_filter with the reference's weights sqrt(2 f / (1 + f)) against np.fft: 2e-6 of each plane's largest magnitude;
    a second run gives the same bits; an all-zero row of weights gives a zero plane.  MI355X: at most 5.8e-8."""
    from spatial_vae_amd import ops
    c = _case(n, m, planes, True)
    weights = c["weight"].copy()
    weights[planes - 1] = 0.0
    x, w = torch.tensor(c["a"]).to(DEV), torch.from_numpy(weights).to(DEV)
    got = ops.frc_filter(x, w, n, m)
    again = ops.frc_filter(x.reshape(planes, n * m), w, n, m)
    assert got.shape == (planes, n, m) and got.dtype == torch.float32 and torch.equal(got, again)
    got = got.cpu().numpy().astype(np.float64)
    want = c["filtered"][:planes - 1]
    err = float((np.abs(got[:planes - 1] - want).reshape(planes - 1, -1).max(1) / np.abs(want).reshape(planes - 1, -1).max(1)).max())
    print("%dx%d planes=%d filter: %.2e of the plane maximum" % (n, m, planes, err))
    assert (got[planes - 1] == 0).all() and np.isfinite(got).all()
    assert err <= TOL_FILTER


def test_an_empty_half_gives_zero_everywhere():
    """pa pb == 0: the FRC is exactly 0 on every ring, so the weight and the filtered plane are too."""
    from spatial_vae_amd import elbo as E
    from spatial_vae_amd import ops
    n, m = 13, 10
    c = _case(n, m, 3, True)
    a = torch.tensor(c["a"]).to(DEV)
    b = a.clone()
    b[1] = 0.0
    sums, curve, _ = ops.frc(a, b, n, m, c["radius"], c["edge"])
    assert (curve[1] == 0).all() and (sums[1, :, 2] == 0).all() and (sums[1, :, 1] > 0).all()
    assert (curve[0] > 0.999999).all() and (curve[2] > 0.999999).all()
    filtered = ops.frc_filter(a, E.frc_weight(curve), n, m)
    assert (filtered[1] == 0).all() and not (filtered[0] == 0).all()


def _refused(rc, L, word=None):
    from spatial_vae_amd import _lib
    message = L.svae_last_error()
    assert rc == _lib.E_INVALID and message, (rc, message)
    if word is not None:
        assert word in message, message


def test_every_refusal_leaves_the_buffers_untouched():
    """Each SVAE_E_INVALID case of the header, through the raw entry points: the code, a message (naming the workspace where
    that is the reason), and every output still what it was prefilled with."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    n, m, P = 12, 10, 3
    R = min(n, m) // 2 + 1
    f64 = dict(dtype=torch.float64, device=DEV)
    a, b = torch.ones(P, n, m, **f64), torch.full((P, n, m), 2.0, **f64)
    sums, curve = torch.full((P, R, 3), 7.0, **f64), torch.full((P, R), 7.0, **f64)
    counts = torch.full((R,), 7, dtype=torch.int32, device=DEV)
    big_a, big_b = torch.ones(2, 72, 72, **f64), torch.ones(2, 72, 72, **f64)
    big_sums, big_curve = torch.full((2, 37, 3), 7.0, **f64), torch.full((2, 37), 7.0, **f64)
    big_counts = torch.full((37,), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(2 * 72 * 72 * 32, dtype=torch.uint8, device=DEV)
    A, B, S, C, K = a.data_ptr(), b.data_ptr(), sums.data_ptr(), curve.data_ptr(), counts.data_ptr()

    def frc(a=A, b=B, planes=P, n=n, m=m, radius=0.0, edge=0.0, sums=S, frc=C, ring_count=K, ws=None, ws_bytes=0):
        return L.svae_frc(a, b, planes, n, m, radius, edge, sums, frc, ring_count, ws, ws_bytes, None)

    assert L.svae_frc_workspace_bytes(2, 72, 72) == ws.numel() and L.svae_frc_workspace_bytes(P, n, m) == 0
    inf, nan = float("inf"), float("nan")
    for kw in (dict(n=1), dict(m=1), dict(n=1025), dict(m=1025), dict(n=0), dict(planes=0), dict(planes=-1),
               dict(planes=2048, n=1024, m=1024), dict(a=None), dict(b=None), dict(sums=None), dict(frc=None), dict(ring_count=None),
               dict(sums=A), dict(frc=A + 8), dict(ring_count=B), dict(sums=B + 8 * (P * n * m - 1)), dict(a=S), dict(b=C),
               dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(radius=3.0, edge=0.0), dict(radius=3.0, edge=-1.0),
               dict(radius=3.0, edge=nan), dict(radius=3.0, edge=inf)):
        _refused(frc(**kw), L)
    big = dict(a=big_a.data_ptr(), b=big_b.data_ptr(), planes=2, n=72, m=72, sums=big_sums.data_ptr(), frc=big_curve.data_ptr(),
               ring_count=big_counts.data_ptr())
    for kw in (dict(ws=None, ws_bytes=0), dict(ws=ws.data_ptr(), ws_bytes=ws.numel() - 1), dict(ws=None, ws_bytes=ws.numel()),
               dict(ws=ws.data_ptr() + 8, ws_bytes=ws.numel())):
        _refused(frc(**dict(big, **kw)), L, b"workspace")
    torch.cuda.synchronize()
    for t, v in ((sums, 7.0), (curve, 7.0), (counts, 7), (big_sums, 7.0), (big_curve, 7.0), (big_counts, 7), (a, 1.0), (b, 2.0)):
        assert (t == v).all()

    weight = torch.ones(P, R, **f64)
    out = torch.full((P + 1, n, m), 7.0, device=DEV)
    big_w, big_out = torch.ones(2, 37, **f64), torch.full((2, 72, 72), 7.0, device=DEV)
    W, O = weight.data_ptr(), out.data_ptr()

    def filt(x=A, weight=W, planes=P, n=n, m=m, out=O, ws=None, ws_bytes=0):
        return L.svae_frc_filter(x, weight, planes, n, m, out, ws, ws_bytes, None)

    assert L.svae_frc_filter_workspace_bytes(2, 72, 72) == ws.numel() and L.svae_frc_filter_workspace_bytes(P, n, m) == 0
    for kw in (dict(n=1), dict(m=1), dict(n=1025), dict(m=1025), dict(planes=0), dict(planes=-1), dict(planes=2048, n=1024, m=1024),
               dict(x=None), dict(weight=None), dict(out=None), dict(out=A), dict(out=A + 8 * (P * n * m) - 4), dict(out=W), dict(x=O)):
        _refused(filt(**kw), L)
    for kw in (dict(ws=None, ws_bytes=0), dict(ws=ws.data_ptr(), ws_bytes=ws.numel() - 1), dict(ws=None, ws_bytes=ws.numel()),
               dict(ws=ws.data_ptr() + 8, ws_bytes=ws.numel())):
        _refused(filt(x=big_a.data_ptr(), weight=big_w.data_ptr(), planes=2, n=72, m=72, out=big_out.data_ptr(), **kw), L, b"workspace")
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (big_out == 7.0).all() and (a == 1.0).all() and (weight == 1.0).all()
    # and the calls these were variations of are accepted
    assert frc() == 0 and frc(radius=3.0, edge=2.0) == 0 and filt() == 0
    assert frc(**dict(big, ws=ws.data_ptr(), ws_bytes=ws.numel())) == 0
    torch.cuda.synchronize()
    assert not (sums == 7.0).any() and not (curve == 7.0).any() and not (counts == 7).all()
    assert counts.cpu().numpy().tolist() == F.ring_count(n, m).tolist() and big_counts.cpu().numpy().tolist() == F.ring_count(72, 72).tolist()
    assert not (out[:P] == 7.0).any() and (out[P] == 7.0).all()
