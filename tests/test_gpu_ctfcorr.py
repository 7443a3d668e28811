"""The CTF-correction kernels (include/svae_ctfcorr.h: svae_ctf_apply, svae_ctf_power_update, svae_wiener_finish; ops.ctf_apply,
ops.CtfPower, ops.wiener_finish) on the MI355X against the float64 reference tests/ctfcorr_ref.py (np.fft), shape by shape, then
chained on the recovery example, then every refusal of the header with the buffers prefilled and compared."""
import functools
import os

import numpy as np
import pytest
import torch

from ctfcorr_ref import apply_ref, example_image, finish_ref, power_ref, random_table, transfer
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu
TOL = 2e-6          # doubles inside, one fp32 rounding at the end (tests/test_gpu_ctf.py's figure for the same construction)
TOL_POWER = 1e-10   # double sin / cos of arguments up to ~1e3 rad: ~1e-13 absolute per term, with a 100x margin
# (n, m, P): odd x even twice, even square, config 5's box with a ragged count, the largest planes that stay in LDS (71 x 71:
# 32 n m + 16 (n + m) bytes in 160 KiB) and the first that take a workspace, the workspace form of svae_ctf_filter's limit and
# a non-square one, more images than LDS workgroups' worth, and more images than the 512 workgroups of the workspace form
# (the grid strides)
SHAPES = [(7, 10, 5), (13, 10, 5), (12, 12, 6), (40, 40, 37), (71, 71, 3), (72, 72, 3), (81, 81, 3), (96, 90, 3), (12, 12, 700),
          (72, 72, 515)]
SCALES = [1.0, 1.5]
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(n, m, P, scale):
    """The shared, read-only inputs and references of one shape: table, images, labels (with -1 and an empty class 2), H, u."""
    table = random_table(P, n)
    rs = np.random.RandomState(1000 + n * m + P)
    y = rs.normal(size=(P, n, m)).astype(np.float32)
    label = rs.choice([-1, 0, 1, 3], size=P).astype(np.int32)
    label[:4] = [0, -1, 3, 1][:min(P, 4)]
    H, u = transfer(table, n, m, scale)
    for a in (table, y, label, H, u):
        a.setflags(write=False)
    return {"table": table, "y": y, "label": label, "H": H, "u": u}


def _plane_err(got, ref):
    """max over planes of max |got - ref| / max |ref| of the plane."""
    got, ref = got.astype(np.float64).reshape(len(ref), -1), ref.astype(np.float64).reshape(len(ref), -1)
    return float((np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())


def _signs_are_safe(c):
    """No flip may depend on the last bit of u: a condition on the reference, not a tolerance."""
    smallest = float(np.abs(c["u"]).min())
    assert smallest >= 1e-9, smallest
    return smallest


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,m,P", SHAPES)
def test_apply_matches_the_reference(n, m, P, scale):
    """svae_ctf_apply in both modes against np.fft: 2e-6 of each plane's largest magnitude; a second run gives the same bits.
    MI355X: the largest error over all shapes is 5.0e-8 (flip) and 1.4e-8 (multiply); most planes equal the rounded reference in
    every element."""
    from spatial_vae_amd import ops
    c = _case(n, m, P, scale)
    smallest = _signs_are_safe(c)
    y = torch.tensor(c["y"]).to(DEV)
    for mode in ("flip", "multiply"):
        got = ops.ctf_apply(y, c["table"], n, m, scale, mode)
        again = ops.ctf_apply(y.reshape(P, n * m), torch.tensor(c["table"]).to(DEV), n, m, scale, mode)
        assert got.shape == y.shape and got.dtype == torch.float32 and torch.equal(got.reshape(P, -1), again)
        err = _plane_err(got.cpu().numpy(), apply_ref(c["y"], c["table"], n, m, scale, mode))
        print("%dx%d P=%d scale %g %s: %.2e of the plane maximum (min |u| %.1e)" % (n, m, P, scale, mode, err, smallest))
        assert err <= TOL


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,m,P", SHAPES)
def test_flipping_twice_is_the_identity(n, m, P, scale):
    """s^2 = 1: two phase flips return the input within 2e-6 of each plane's largest magnitude (two fp32 roundings).
    MI355X: at most 6.0e-8."""
    from spatial_vae_amd import ops
    c = _case(n, m, P, scale)
    _signs_are_safe(c)
    y = torch.tensor(c["y"]).to(DEV)
    table = torch.tensor(c["table"]).to(DEV)
    twice = ops.ctf_apply(ops.ctf_apply(y, table, n, m, scale, "flip"), table, n, m, scale, "flip")
    err = _plane_err(twice.cpu().numpy(), c["y"])
    print("%dx%d P=%d scale %g flip twice: %.2e of the plane maximum" % (n, m, P, scale, err))
    assert err <= TOL


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n,m,P", SHAPES)
def test_power_update_matches_the_reference(n, m, P, scale):
    """svae_ctf_power_update against the float64 sums of H^2 by label (labels include -1 and class 2 stays empty): 1e-10 of the
    largest entry; one call equals two calls on the halves, bit for bit.  MI355X: at most 2.5e-14."""
    from spatial_vae_amd import ops
    c = _case(n, m, P, scale)
    _signs_are_safe(c)
    n_classes = 4
    label = torch.tensor(c["label"]).to(DEV)
    table = torch.tensor(c["table"]).to(DEV)
    whole = ops.CtfPower(n_classes, n, m, DEV, scale=scale)
    whole.update(table, label)
    halves = ops.CtfPower(n_classes, n, m, DEV, scale=scale)
    cut = P // 2
    halves.update(table[:cut], label[:cut])
    halves.update(c["table"][cut:], label[cut:])
    assert torch.equal(whole.result(), halves.result())
    got = whole.result().cpu().numpy()
    want = power_ref([(c["table"], c["label"])], n_classes, n, m, scale)
    assert got.shape == want.shape == (n_classes, n, m) and (got[2] == 0).all() and (want[2] == 0).all()
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("%dx%d P=%d scale %g power: %.2e of the largest entry" % (n, m, P, scale, err))
    assert err <= TOL_POWER


@pytest.mark.parametrize("n,m,P", SHAPES)
def test_wiener_finish_matches_the_reference(n, m, P):
    """svae_wiener_finish on P classes against np.fft: 2e-6 of the largest magnitude at lambda 1e-3 and 1.0, and at lambda 0
    with one denominator entry set to 0, which contributes 0 (as in the reference).  MI355X: at most 7.0e-13 (equal to the rounded reference in every element but at 72 x 72 with 515 classes)."""
    from spatial_vae_amd import ops
    rs = np.random.RandomState(n * 1000 + m + P)
    total = rs.normal(size=(P, n, m))
    den = rs.uniform(0.5, 6.0, size=(P, n, m))
    total_d = torch.from_numpy(total).to(DEV)
    for lam, zero in ((1e-3, False), (1.0, False), (0.0, True)):
        d = den.copy()
        if zero:
            d[P // 2, n // 2, 1] = 0.0
        got = ops.wiener_finish(total_d.reshape(P, n * m, 1), torch.from_numpy(d).to(DEV), lam, n, m)
        assert got.shape == (P, n, m) and got.dtype == torch.float32
        want = finish_ref(total, d, lam, n, m)
        got = got.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
        print("%dx%d classes=%d lambda %g: %.2e of the largest magnitude" % (n, m, P, lam, err))
        assert np.isfinite(got).all() and err <= TOL


def test_chain_recovers_the_image():
    """The recovery example on the device: six copies of the 40 x 40 image through the transfer functions of the golden table,
    identity pose, ctf_apply(multiply) -> ClassSums -> CtfPower -> wiener_finish at lambda 1e-3.  Each link is held to its own
    reference (the products to apply_ref at 2e-6 of the plane maximum, the sums to numpy's sum of those products at 1e-12, the
    denominator to power_ref at 1e-10) and the result to finish_ref of the chain's sum and denominator at 2e-6; it is closer to
    the image than the plain class average of the same copies (reference alone: 0.012 against 0.72 of the image's norm).  The
    distance to finish_ref of the all-float64 chain is printed, not bounded: den + lambda goes down to 2.4e-3 here, and moving
    three in ten of the fp32 products by one unit in the last place, which the 2e-6 of the first link allows, moves the quotient
    by 1.95e-6 of its maximum on its own.  MI355X: equal to finish_ref and to the float64 chain in every element; 0.0117 against 0.7223."""
    from spatial_vae_amd import ops
    table = np.loadtxt(os.path.join(GOLDEN_DIR, "ctf_table.txt"), ndmin=2)
    n = m = 40
    A = example_image()
    H, u = transfer(table, n, m)
    assert np.abs(u).min() >= 1e-9
    copies = np.fft.ifft2(H * np.fft.fft2(A)[None]).real.astype(np.float32)
    y = torch.from_numpy(copies).to(DEV).reshape(6, n * m)
    label = torch.zeros(6, dtype=torch.int32, device=DEV)
    g = ops.ctf_apply(y, table, n, m, 1.0, "multiply")
    g_ref = apply_ref(copies, table, n, m, 1.0, "multiply")
    assert _plane_err(g.cpu().numpy(), g_ref) <= TOL
    sums = ops.ClassSums(1, n * m, 1, DEV)
    sums.update(g, None, label)
    power = ops.CtfPower(1, n, m, DEV)
    power.update(table, label)
    total, den = sums.result()[0], power.result()
    want_total = g.cpu().numpy().astype(np.float64).sum(0).reshape(1, n * m, 1)
    assert np.abs(total.cpu().numpy() - want_total).max() <= 1e-12 * np.abs(want_total).max()
    den_ref = power_ref([(table, np.zeros(6, int))], 1, n, m)
    assert np.abs(den.cpu().numpy() - den_ref).max() <= TOL_POWER * den_ref.max()
    got = ops.wiener_finish(total, den, 1e-3, n, m).cpu().numpy().astype(np.float64)
    want = finish_ref(total.cpu().numpy(), den.cpu().numpy(), 1e-3, n, m)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    full = finish_ref(g_ref.astype(np.float64).sum(0)[None], den_ref, 1e-3, n, m)
    err_full = float(np.abs(got - full).max() / np.abs(full).max())

    def away(img):
        return float(np.sqrt(((img - A) ** 2).sum() / (A ** 2).sum()))

    plain = ops.ClassSums(1, n * m, 1, DEV)
    plain.update(y, None, label)
    plain_average = (plain.result()[0] / plain.result()[1][..., None]).cpu().numpy().reshape(n, m)
    print("chain: %.2e of the maximum from finish_ref, %.2e from the float64 chain; %.4f of the image's norm away, the plain "
          "average %.4f" % (err, err_full, away(got[0]), away(plain_average)))
    assert err <= TOL
    assert away(got[0]) < away(plain_average)


def _refused(rc, L, word=None):
    from spatial_vae_amd import _lib
    message = L.svae_last_error()
    assert rc == _lib.E_INVALID and message, (rc, message)
    if word is not None:
        assert word in message, message


def test_every_refusal_leaves_the_buffers_untouched():
    """Each SVAE_E_INVALID case of the header, through the raw entry points: the code, a message (naming the workspace where
    that is the reason), and out / den / average still what they were prefilled with.  SVAE_E_INVALID is -1 in svae.h; -2 is
    SVAE_E_WORKSPACE, which these entries do not use."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    n, m, B = 12, 10, 3
    y = torch.ones(B, n, m, device=DEV)
    out = torch.full((B + 1, n, m), 7.0, device=DEV)
    par = torch.from_numpy(random_table(B, 1)).to(DEV)
    big, big_out = torch.ones(2, 72, 72, device=DEV), torch.full((2, 72, 72), 7.0, device=DEV)
    ws = torch.zeros(2 * 72 * 72 * 32, dtype=torch.uint8, device=DEV)
    Y, O, T = y.data_ptr(), out.data_ptr(), par.data_ptr()

    def apply(y=Y, params=T, B=B, n=n, m=m, scale=1.0, mode=0, out=O, ws=None, ws_bytes=0):
        return L.svae_ctf_apply(y, params, B, n, m, scale, mode, out, ws, ws_bytes, None)

    assert L.svae_ctf_apply_workspace_bytes(2, 72, 72) == ws.numel() and L.svae_ctf_apply_workspace_bytes(B, n, m) == 0
    for kw in (dict(n=1), dict(m=1), dict(B=0), dict(B=-1), dict(B=2048, n=1024, m=1024), dict(n=10000, m=241), dict(mode=2),
               dict(mode=-1), dict(y=None), dict(out=None), dict(params=None), dict(out=Y), dict(out=Y + 4 * n * m), dict(y=O + 4 * n * m),
               dict(scale=0.0), dict(scale=float("nan"))):
        _refused(apply(**kw), L)
    for kw in (dict(ws=None, ws_bytes=0), dict(ws=ws.data_ptr(), ws_bytes=ws.numel() - 1), dict(ws=None, ws_bytes=ws.numel()),
               dict(ws=ws.data_ptr() + 8, ws_bytes=ws.numel())):
        _refused(apply(y=big.data_ptr(), B=2, n=72, m=72, out=big_out.data_ptr(), **kw), L, b"workspace")
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (big_out == 7.0).all() and (y == 1.0).all()

    den = torch.full((4, n, m), 7.0, dtype=torch.float64, device=DEV)
    lab = torch.zeros(B, dtype=torch.int32, device=DEV)
    D, Lb = den.data_ptr(), lab.data_ptr()

    def power(params=T, label=Lb, B=B, n=n, m=m, scale=1.0, n_classes=4, den=D):
        return L.svae_ctf_power_update(params, label, B, n, m, scale, n_classes, den, None)

    for kw in (dict(B=0), dict(n=1), dict(m=1), dict(n_classes=0), dict(n_classes=4097), dict(n=32768, m=32768, n_classes=2),
               dict(params=None), dict(label=None), dict(den=None), dict(scale=-1.0)):
        _refused(power(**kw), L)
    torch.cuda.synchronize()
    assert (den == 7.0).all()

    total = torch.ones(4, n, m, dtype=torch.float64, device=DEV)
    avg = torch.full((4, n, m), 7.0, device=DEV)
    big_sum, big_den = torch.ones(2, 72, 72, dtype=torch.float64, device=DEV), torch.ones(2, 72, 72, dtype=torch.float64, device=DEV)
    S, A = total.data_ptr(), avg.data_ptr()

    def finish(sum=S, den=D, lam=1.0, n_classes=4, n=n, m=m, average=A, ws=None, ws_bytes=0):
        return L.svae_wiener_finish(sum, den, lam, n_classes, n, m, average, ws, ws_bytes, None)

    for kw in (dict(lam=-1e-3), dict(lam=float("nan")), dict(lam=float("inf")), dict(n_classes=0), dict(n_classes=4097), dict(n=1),
               dict(m=1), dict(n=10000, m=241), dict(n=1024, m=1024, n_classes=2048), dict(sum=None), dict(den=None), dict(average=None)):
        _refused(finish(**kw), L)
    for kw in (dict(ws=None, ws_bytes=0), dict(ws=ws.data_ptr(), ws_bytes=ws.numel() - 1)):
        _refused(finish(sum=big_sum.data_ptr(), den=big_den.data_ptr(), average=big_out.data_ptr(), n=72, m=72, n_classes=2, **kw), L,
                 b"workspace")
    torch.cuda.synchronize()
    assert (avg == 7.0).all() and (den == 7.0).all() and (big_out == 7.0).all()
    # and the calls these were variations of are accepted
    assert apply() == 0 and power() == 0 and finish(lam=0.0) == 0
    torch.cuda.synchronize()
    assert not (out[:B] == 7.0).all() and (out[B] == 7.0).all() and not (avg == 7.0).all()
