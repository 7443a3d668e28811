"""CPU-only: the binding of include/svae_align.h held to that header, the float64 reference of the alignment (tests/align_ref.py)
held to properties of the geometry it restates, the class-sum reference against a naive loop, and infer.py's new options: their
defaults and every refusal its argument parser makes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from align_ref import align_ref, class_sums_ref, covered, source_positions
from test_binding_cpu import binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(28, 28), (12, 20), (9, 9), (2, 3)]
INTERPS = ["bicubic", "bilinear"]
POSES = [(0.7, (0.12, -0.08)), (-2.3, (-0.1, 0.15))]


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_align_binding_matches_its_header():
    """What is include/svae_align.h's own (the rules every added header shares are tests/test_binding_cpu.py's): two functions
    and their argument names, no struct; the header's two constants are _lib.ALIGN_INTERP, and none of this adds an upper-case
    integer to the binding (those are svae.h's constants); the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_align.h")[1]
    assert _lib.HEADERS["svae_align.h"] is _lib.ALIGN_SIGNATURES
    assert H["structs"] == {} and len(H["functions"]) == 2
    assert H["constants"] == {"SVAE_ALIGN_" + k.upper(): v for k, v in _lib.ALIGN_INTERP.items()} == {"SVAE_ALIGN_BILINEAR": 0, "SVAE_ALIGN_BICUBIC": 1}
    assert [a[2] for a in H["functions"]["svae_align_images"][1]] == ["y", "theta", "dx", "B", "rows", "cols", "C", "interp", "aligned",
                                                                      "cover", "stream"]
    assert [a[2] for a in H["functions"]["svae_class_sums_update"][1]] == ["aligned", "cover", "label", "B", "N", "C", "n_classes", "sum",
                                                                           "count", "stream"]
    assert not [k for k in binding_constants(_lib) if "ALIGN" in k]
    assert ops._POINTER_ARGS["svae_align_images"] == (0, 1, 2, 8, 9) and ops._POINTER_ARGS["svae_class_sums_update"] == (0, 1, 2, 7, 8)


# ---------------------------------------------------------------- the reference, held to the geometry
def _images(rs, B, rows, cols, C=1):
    return rs.uniform(-1, 2, size=(B, rows * cols, C)).astype(np.float32)


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_identity_pose_is_bit_exact(rows, cols, interp):
    """theta = 0, dx = 0 (given, or absent) returns the input bit for bit and covers everything."""
    y = _images(np.random.RandomState(rows * cols), 2, rows, cols, 2)
    for theta, dx in ((np.zeros(2, np.float32), np.zeros((2, 2), np.float32)), (None, None)):
        out, cover = align_ref(y, theta, dx, rows, cols, interp)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), y.view(np.uint32)) and cover.all()


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("n", [28, 9, 2])
def test_quarter_turn_is_rot90(n, interp):
    """theta = pi/2 on a square image covers every pixel (the 1e-6 slack) and is np.rot90(img, 1) to 1e-12."""
    y = _images(np.random.RandomState(n), 1, n, n).astype(np.float64)
    out, cover = align_ref(y, np.array([np.pi / 2]), None, n, n, interp, dtype=np.float64)
    err = np.abs(out.reshape(n, n) - np.rot90(y.reshape(n, n), 1)).max()
    print("quarter turn %dx%d %s: max error %.2e" % (n, n, interp, err))
    assert cover.all() and err <= 1e-12


@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_constant_image_stays_constant_where_covered(rows, cols, interp):
    """Partition of unity: both weight sets sum to 1, so a constant image is that constant on covered pixels (to 1e-12) and 0
    on the others; random poses leave some of each."""
    rs = np.random.RandomState(5)
    B = 6
    theta, dx = rs.uniform(-np.pi, np.pi, B), rs.uniform(-0.3, 0.3, (B, 2))
    out, cover = align_ref(np.full((B, rows * cols, 1), 0.75), theta, dx, rows, cols, interp, dtype=np.float64)
    on = cover.astype(bool)
    assert on.any() and (~on).any()
    assert np.abs(out[..., 0][on] - 0.75).max() <= 1e-12 and (out[..., 0][~on] == 0).all()


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bilinear_reproduces_an_affine_image(rows, cols):
    """An image affine in (jx, jy) is reproduced by bilinear interpolation at the clamped source position, to 1e-12."""
    rs = np.random.RandomState(6)
    B = 5
    theta, dx = rs.uniform(-np.pi, np.pi, B), rs.uniform(-0.3, 0.3, (B, 2))
    jy, jx = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    img = 0.3 + 0.11 * jx - 0.07 * jy
    out, cover = align_ref(np.broadcast_to(img.reshape(1, -1, 1), (B, rows * cols, 1)), theta, dx, rows, cols, "bilinear", dtype=np.float64)
    fx, fy = source_positions(theta, dx, B, rows, cols)
    on = covered(fx, fy, rows, cols)
    assert np.array_equal(on.reshape(B, -1), cover.astype(bool))
    want = 0.3 + 0.11 * np.clip(fx, 0, cols - 1) - 0.07 * np.clip(fy, 0, rows - 1)
    assert np.abs(out.reshape(B, rows, cols) - want)[on].max() <= 1e-12


def scene(p):
    """A smooth scene without any symmetry, on the plane the decoder's grid spans."""
    x, y = p[..., 0], p[..., 1]
    return (np.exp(-((x - 0.25) ** 2 + (y + 0.2) ** 2) / 0.18) + 0.6 * np.exp(-((x + 0.35) ** 2 / 0.10 + (y - 0.3) ** 2 / 0.25))
            + 0.15 * x - 0.1 * y * x)


def grid(rows, cols):
    x0, x1 = np.meshgrid(np.linspace(-1, 1, cols), np.linspace(1, -1, rows))
    return np.stack([x0.ravel(), x1.ravel()], 1)


def observe(f, theta, dx, rows, cols):
    """What the decoder draws for a scene f at the pose (theta, dx): f at x'' = grid @ [[c, s], [-s, c]] + dx (svae_pose)."""
    c, s = np.cos(theta), np.sin(theta)
    return f(grid(rows, cols) @ np.array([[c, s], [-s, c]]) + np.asarray(dx))


def convention_errors(observed, canonical, theta, dx, rows, cols, interp="bicubic"):
    """Max error against the canonical image over the covered pixels, under the stated convention and three wrong ones."""
    out = {}
    for name, (t, d) in {"stated": (theta, dx), "theta negated": (-theta, dx), "dx negated": (theta, -np.asarray(dx)),
                         "no pose": (0.0, (0.0, 0.0))}.items():
        a, cover = align_ref(observed.reshape(1, -1, 1), np.array([t]), np.array([d]), rows, cols, interp, dtype=np.float64)
        on = cover[0].astype(bool)
        assert on.sum() > rows * cols // 4
        out[name] = np.abs(a[0, :, 0] - canonical)[on].max()
    return out


@pytest.mark.parametrize("theta,dx", POSES)
def test_convention_is_the_decoders(theta, dx):
    """A scene observed through the svae_pose formula, aligned at that pose, is the scene on the un-posed grid: the bicubic error
    over covered pixels is at least 10 times smaller than under theta negated, dx negated, or no pose at all (28x28)."""
    rows = cols = 28
    err = convention_errors(observe(scene, theta, dx, rows, cols), scene(grid(rows, cols)), theta, dx, rows, cols)
    print("pose (%g, %s): %s" % (theta, dx, {k: "%.2e" % v for k, v in err.items()}))
    for wrong in ("theta negated", "dx negated", "no pose"):
        assert err[wrong] >= 10 * err["stated"], (wrong, err)


def test_class_sum_reference_against_a_naive_loop():
    rs = np.random.RandomState(7)
    B, N, C, n_classes = 9, 5, 2, 3
    aligned = rs.normal(size=(B, N, C)).astype(np.float32)
    cover = (rs.uniform(size=(B, N)) > 0.3).astype(np.uint8)
    label = np.array([0, 2, -1, 1, 2, 2, 0, 5, 1])
    total, count = class_sums_ref([(aligned[:4], cover[:4], label[:4]), (aligned[4:], cover[4:], label[4:])], n_classes, N, C)
    for k in range(n_classes):
        for j in range(N):
            s, n = np.zeros(C), 0.0
            for b in range(B):
                if label[b] == k and cover[b, j]:
                    s = s + aligned[b, j].astype(np.float64)
                    n += 1
            assert np.array_equal(total[k, j], s) and count[k, j] == n
    assert count.sum() == cover[(label >= 0) & (label < n_classes)].sum()
    everywhere, n_all = class_sums_ref([(aligned, None, label)], n_classes, N, C)
    assert np.array_equal(n_all, np.repeat(np.bincount(label[(label >= 0) & (label < 3)], minlength=3)[:, None], N, 1))
    assert np.allclose(everywhere[2], aligned[label == 2].astype(np.float64).sum(0), rtol=0, atol=1e-12)


# ---------------------------------------------------------------- infer.py's new options
def test_new_options_default_to_off(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    a = _infer().infer_arguments(["mnist", "--state", str(state), "--out", "s.npz"])
    assert (a.aligned, a.recon, a.class_averages, a.labels, a.label_array) == (None, None, None, None, None)
    assert (a.pose, a.interp) == ("iw", "bicubic")
    labels = tmp_path / "l.npy"
    np.save(labels, np.array([0, 2, -1, 1], np.int16))
    a = _infer().infer_arguments(["mnist", "--state", str(state), "--out", "s.npz", "--aligned", "a.mrcs", "--recon", "r.npy", "--class_averages",
                                "c.npz", "--labels", str(labels), "--pose", "best", "--interp", "bilinear"])
    assert (a.aligned, a.recon, a.class_averages, a.pose, a.interp) == ("a.mrcs", "r.npy", "c.npz", "best", "bilinear")
    assert a.label_array.dtype == np.int64 and a.label_array.tolist() == [0, 2, -1, 1]
    a = _infer().infer_arguments(["mnist", "--state", str(state), "--out", "s.npz", "--class_averages", "c.npz", "--pose", "q"])
    assert (a.pose, a.interp, a.label_array) == ("q", "bicubic", None)


@pytest.mark.parametrize("extra,message", [
    (["--aligned", "a.png"], "--aligned must end in .npy or .mrcs"),
    (["--recon", "r.mrc"], "--recon must end in .npy or .mrcs"),
    (["--class_averages", "c.npy"], "--class_averages must end in .npz"),
    (["--labels", "{int1d}"], "--labels needs --class_averages"),
    (["--class_averages", "c.npz", "--labels", "{missing}"], "no such file"),
    (["--class_averages", "c.npz", "--labels", "{float1d}"], "must be an integer array"),
    (["--class_averages", "c.npz", "--labels", "{int2d}"], "must be 1-D"),
    (["--class_averages", "c.npz", "--labels", "{below}"], "below -1"),
    (["--class_averages", "c.npz", "--labels", "{many}"], "4097 classes"),
    (["--pose", "best"], "--pose needs one of"),
    (["--interp", "bilinear"], "--interp needs one of"),
])
def test_new_refusals_exit_with_code_2_before_the_library_is_loaded(tmp_path, extra, message):
    """Through the real command line in a fresh process: exit code 2, the reason on stderr, no output file, and the process
    never loaded the kernel library (a marker printed by an exit hook shows _lib's handle was still unset)."""
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    files = {"int1d": np.array([0, 1, 1]), "float1d": np.array([0.0, 1.0]), "int2d": np.zeros((3, 1), np.int64),
             "below": np.array([0, -2, 1]), "many": np.array([0, 4096])}
    for name, array in files.items():
        np.save(tmp_path / (name + ".npy"), array)
    names = dict({k: tmp_path / (k + ".npy") for k in files}, missing=tmp_path / "nope.npy")
    argv = ["mnist", "--state", str(state), "--out", "s.npz"] + [a.format(**names) for a in extra]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert message in out.stderr and "LIB True" in out.stderr
    assert sorted(os.listdir(tmp_path)) == sorted(["a.ckpt"] + [k + ".npy" for k in files])
