"""The alignment kernels (include/svae_align.h: svae_align_images, svae_class_sums_update; ops.align_images, ops.ClassSums) on
the MI355X against tests/align_ref.py, the float64 numpy restatement of the header.

Values: |out - ref| <= 2^-23 |ref| + 1e-12 max|y|.  Both sides evaluate the same double expression and round to float once;
the device's double sin / cos may differ from numpy's in the last bits, which moves a source position by ~1e-15 pixel.  Coverage
is compared exactly; pixels whose reference source position lies within 1e-9 of a coverage threshold could be excluded, and each
test asserts from the reference alone that its inputs have none.  Each test prints its figures before it asserts."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from align_ref import align_ref, class_sums_ref, near_threshold, source_positions

pytestmark = pytest.mark.gpu
SHAPES = [(3, 9, 9, 1), (3, 12, 20, 3), (4, 28, 28, 1), (2, 2, 3, 1)]
INTERPS = ["bicubic", "bilinear"]
POSES = [(0.7, (0.12, -0.08)), (-2.3, (-0.1, 0.15))]
SENTINEL = -12345.5


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(B, rows, cols, C):
    """Images ~ U(-1, 2); image 0 at the identity, image 1 at an exact quarter turn (float32(pi/2), no shift), the others at
    random poses.  The float64 references of both interpolations are computed once per shape and shared."""
    rs = np.random.RandomState(100 * rows + cols + C)
    y = rs.uniform(-1, 2, size=(B, rows * cols, C)).astype(np.float32)
    theta = rs.uniform(-np.pi, np.pi, B).astype(np.float32)
    dx = rs.uniform(-0.25, 0.25, (B, 2)).astype(np.float32)
    theta[0], dx[0] = 0.0, 0.0
    theta[1], dx[1] = np.float32(np.pi / 2), 0.0
    fx, fy = source_positions(theta, dx, B, rows, cols)
    ref = {i: align_ref(y, theta, dx, rows, cols, i) for i in INTERPS}
    return y, theta, dx, ref, int(near_threshold(fx, fy, rows, cols).sum())


def _check(out, cover, ref, ref_cover, y, what):
    out, ref64 = out.astype(np.float64), ref.astype(np.float64)
    excess = np.abs(out - ref64) - (2.0 ** -23 * np.abs(ref64) + 1e-12 * np.abs(y).max())
    print("%s: max |out - ref| %.3e, %d of %d elements differ, covered %d of %d pixels" % (
        what, np.abs(out - ref64).max(), int((out != ref64).sum()), out.size, int(ref_cover.sum()), ref_cover.size))
    assert np.array_equal(cover, ref_cover)
    assert excess.max() <= 0


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("B,rows,cols,C", SHAPES)
def test_kernel_against_the_reference(B, rows, cols, C, interp):
    """A batch mixing the identity, an exact quarter turn and random poses: values within the bound, coverage exactly equal (no
    pixel of these inputs lies near a threshold), the identity image bit-equal to its input, uncovered pixels exactly 0, and
    theta / dx absent bit-equal to zeros.  MI355X: every shape and both interpolations hold, and no element differs from the
    reference at all."""
    from spatial_vae_amd import ops
    y, theta, dx, ref, near = _case(B, rows, cols, C)
    assert near == 0
    dev = _dev()
    yd, td, dd = (torch.from_numpy(a).to(dev) for a in (y, theta, dx))
    out, cover = ops.align_images(yd, td, dd, rows, cols, interp)
    assert out.shape == yd.shape and cover.shape == (B, rows * cols) and cover.dtype == torch.uint8
    out, cover = out.cpu().numpy(), cover.cpu().numpy()
    _check(out, cover, ref[interp][0], ref[interp][1], y, "%dx%dx%dx%d %s" % (B, rows, cols, C, interp))
    assert np.array_equal(out[0].view(np.uint32), y[0].view(np.uint32)) and cover[0].all()
    assert cover[1].all()                                           # a quarter turn maps the grid's square onto itself
    assert (out[cover == 0] == 0).all()
    zeros_t, zeros_d = torch.zeros(B, device=dev), torch.zeros(B, 2, device=dev)
    both = ops.align_images(yd, zeros_t, zeros_d, rows, cols, interp)
    assert torch.equal(both[0], yd) and bool(both[1].all())
    for t, d in ((None, dd), (td, None), (None, None)):
        a = ops.align_images(yd, t, d, rows, cols, interp)
        b = ops.align_images(yd, zeros_t if t is None else t, zeros_d if d is None else d, rows, cols, interp)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    again = ops.align_images(yd, td, dd, rows, cols, interp)
    assert np.array_equal(again[0].cpu().numpy().view(np.uint32), out.view(np.uint32))


def test_convention_against_the_decoder():
    """The decoder itself (SpatialGenerator, H = 64, 2 layers, default init, seeds 0-2, 28x28) drawn at a pose and un-posed: the
    posed output aligned at that pose agrees with the un-posed output over the covered pixels at least 10 times better than
    under theta negated, dx negated, or no pose at all.  MI355X: the ratio to the best wrong convention is 58.0 ... 74.3 over the
    six cases (error 1.4e-4 ... 3.1e-4 at the stated pose)."""
    import torch.nn as nn
    from spatial_vae_amd import cli, models, ops
    dev = _dev()
    rows = cols = 28
    x = cli.coord_grid(rows, cols).to(dev)
    worst = np.inf
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        p_net = models.SpatialGenerator(2, 64, num_layers=2, activation=nn.Tanh).to(dev)
        z = torch.randn(1, 2).to(dev)
        with torch.no_grad():
            canonical = p_net.forward_posed(x, 1, z=z).reshape(1, -1)
            for theta, dx in POSES:
                t, d = torch.tensor([theta], device=dev), torch.tensor([dx], device=dev)
                posed = p_net.forward_posed(x, 1, theta=t, dx=d, z=z).reshape(1, rows * cols, 1)
                err = {}
                for name, (tt, dd) in {"stated": (t, d), "theta negated": (-t, d), "dx negated": (t, -d), "no pose": (None, None)}.items():
                    aligned, cover = ops.align_images(posed, tt, dd, rows, cols, "bicubic")
                    on = cover.bool()
                    assert int(on.sum()) > rows * cols // 4
                    err[name] = float((aligned.reshape(1, -1) - canonical).abs()[on].max())
                ratio = min(err[k] for k in err if k != "stated") / err["stated"]
                print("seed %d pose (%g, %s): %s, ratio %.1f" % (seed, theta, dx, {k: "%.2e" % v for k, v in err.items()}, ratio))
                worst = min(worst, ratio)
    assert worst >= 10


def test_class_sums_are_the_reference_bit_for_bit():
    """n_classes = 3, labels with -1 and an out-of-range 3 among them, on what the align kernel wrote for 8 images of 12x20x3:
    one call, and two calls on the halves, are bit-equal to each other and to align_ref's sums in index order (float to double is
    exact); cover = NULL counts every pixel; a second run gives the same bits.  MI355X: holds."""
    from spatial_vae_amd import ops
    dev = _dev()
    B, rows, cols, C, n_classes = 8, 12, 20, 3, 3
    N = rows * cols
    rs = np.random.RandomState(11)
    y = torch.from_numpy(rs.normal(size=(B, N, C)).astype(np.float32)).to(dev)
    theta = torch.from_numpy(rs.uniform(-np.pi, np.pi, B).astype(np.float32)).to(dev)
    dx = torch.from_numpy(rs.uniform(-0.3, 0.3, (B, 2)).astype(np.float32)).to(dev)
    aligned, cover = ops.align_images(y, theta, dx, rows, cols, "bicubic")
    label = np.array([0, 2, -1, 1, 2, 2, 3, 0], np.int32)
    label_d = torch.from_numpy(label).to(dev)
    a_h, c_h = aligned.cpu().numpy(), cover.cpu().numpy()
    assert 0 < c_h.sum() < c_h.size

    def run(pieces, with_cover=True):
        sums = ops.ClassSums(n_classes, N, C, dev)
        for lo, hi in pieces:
            sums.update(aligned[lo:hi], cover[lo:hi] if with_cover else None, label_d[lo:hi])
        return tuple(t.cpu().numpy() for t in sums.result())

    one, two, again = run([(0, B)]), run([(0, 4), (4, B)]), run([(0, 4), (4, B)])
    ref = class_sums_ref([(a_h[:4], c_h[:4], label[:4]), (a_h[4:], c_h[4:], label[4:])], n_classes, N, C)
    for name, got in (("one call", one), ("two calls", two), ("second run", again)):
        assert got[0].shape == (n_classes, N, C) and got[1].shape == (n_classes, N) and got[0].dtype == np.float64
        assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)), name
        assert np.array_equal(got[1], ref[1]), name
    everywhere = run([(0, 3), (3, B)], with_cover=False)
    ref_all = class_sums_ref([(a_h, None, label)], n_classes, N, C)
    assert np.array_equal(everywhere[0].view(np.uint64), ref_all[0].view(np.uint64)) and np.array_equal(everywhere[1], ref_all[1])
    assert np.array_equal(ref_all[1][:, 0], [2, 1, 3])
    print("class sums: %d covered contributions, per class %s" % (int(ref[1].sum()), ref[1].sum(1)))


def test_invalid_calls_are_refused_and_touch_nothing():
    """Every SVAE_E_INVALID case of the header, straight through the C ABI: a message is recorded and aligned, cover, sum and
    count still hold what they held; ops.align_images refuses an unknown interpolation by name.  MI355X: every call refused."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    dev = _dev()
    B, rows, cols, C = 2, 4, 5, 2
    n = B * rows * cols * C
    y = torch.full((n + 8,), 0.5, device=dev)
    out = torch.full((n,), SENTINEL, device=dev)
    cover = torch.full((B * rows * cols,), 77, dtype=torch.uint8, device=dev)
    theta, dx = torch.zeros(B, device=dev), torch.zeros(B, 2, device=dev)

    def align(**kw):
        a = dict(y=y.data_ptr(), theta=theta.data_ptr(), dx=dx.data_ptr(), B=B, rows=rows, cols=cols, C=C, interp=1, aligned=out.data_ptr(),
                 cover=cover.data_ptr())
        a.update(kw)
        return L.svae_align_images(a["y"], a["theta"], a["dx"], a["B"], a["rows"], a["cols"], a["C"], a["interp"], a["aligned"], a["cover"],
                                   _stream())

    bad = [dict(rows=1), dict(cols=1), dict(rows=0), dict(C=0), dict(C=_lib.MAX_OUT + 1), dict(B=0), dict(B=-1),
           dict(B=1 << 15, rows=1 << 8, cols=1 << 8, C=1), dict(interp=2), dict(interp=-1), dict(y=None), dict(aligned=None),
           dict(aligned=y.data_ptr()), dict(aligned=y.data_ptr() + 16), dict(y=out.data_ptr() + 4 * (n - 1))]
    for kw in bad:
        assert align(**kw) == _lib.E_INVALID, kw
        assert b"svae_align_images" in L.svae_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((cover == 77).all()) and bool((y == 0.5).all())
    assert align() == _lib.OK and align(theta=None, dx=None, cover=None, interp=0) == _lib.OK
    with pytest.raises(RuntimeError, match="interp must be one of"):
        ops.align_images(y[:n].view(B, -1, C), None, None, rows, cols, "nearest")
    with pytest.raises(RuntimeError, match="does not hold"):
        ops.align_images(y[:n].view(B, -1, C), None, None, rows, cols + 1, "bicubic")

    N, n_classes = rows * cols, 3
    total = torch.full((n_classes * N * C,), 3.25, dtype=torch.float64, device=dev)
    count = torch.full((n_classes * N,), 7.0, dtype=torch.float64, device=dev)
    label = torch.zeros(B, dtype=torch.int32, device=dev)

    def update(**kw):
        a = dict(aligned=out.data_ptr(), cover=cover.data_ptr(), label=label.data_ptr(), B=B, N=N, C=C, n_classes=n_classes,
                 sum=total.data_ptr(), count=count.data_ptr())
        a.update(kw)
        return L.svae_class_sums_update(a["aligned"], a["cover"], a["label"], a["B"], a["N"], a["C"], a["n_classes"], a["sum"], a["count"],
                                        _stream())

    bad = [dict(B=0), dict(N=0), dict(C=0), dict(C=_lib.MAX_OUT + 1), dict(n_classes=0), dict(n_classes=4097), dict(B=1 << 20, N=1 << 11, C=1),
           dict(n_classes=4096, N=1 << 19, C=1), dict(aligned=None), dict(label=None), dict(sum=None), dict(count=None)]
    for kw in bad:
        assert update(**kw) == _lib.E_INVALID, kw
        assert b"svae_class_sums_update" in L.svae_last_error(), kw
    torch.cuda.synchronize()
    assert bool((total == 3.25).all()) and bool((count == 7.0).all())
    assert update() == _lib.OK and update(cover=None) == _lib.OK
    torch.cuda.synchronize()
    assert float(count[0]) == 7.0 + 2 * B and float(count[N]) == 7.0      # both images are of class 0, both calls counted them
