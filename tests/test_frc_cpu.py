"""CPU-only: the binding of include/svae_frc.h held to that header, the integer ring rule held to exact rationals, the float64
reference (tests/frc_ref.py) held to what a ring correlation means, elbo.py's three helpers held to that reference, and
infer.py's --frc options: their defaults and every refusal."""
import numpy as np
import pytest

import frc_ref as F
from test_binding_cpu import binding_constants, parse_added_header


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_frc_binding_matches_its_header():
    """What is include/svae_frc.h's own (the rules every added header shares are tests/test_binding_cpu.py's): four functions
    and their argument names, no constant and no struct; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_frc.h")[1]
    assert _lib.HEADERS["svae_frc.h"] is _lib.FRC_SIGNATURES
    assert H["constants"] == {} and not H["structs"] and len(H["functions"]) == 4
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_frc_workspace_bytes"] == names["svae_frc_filter_workspace_bytes"] == ["planes", "n", "m"]
    assert names["svae_frc"] == ["a", "b", "planes", "n", "m", "mask_radius", "mask_edge", "sums", "frc", "ring_count", "ws",
                                 "ws_bytes", "stream"]
    assert names["svae_frc_filter"] == ["x", "weight", "planes", "n", "m", "out", "ws", "ws_bytes", "stream"]
    assert not [k for k in binding_constants(_lib) if "FRC" in k]
    assert ops._POINTER_ARGS["svae_frc"] == (0, 1, 7, 8, 9, 10) and ops._POINTER_ARGS["svae_frc_filter"] == (0, 1, 5, 6)


def test_workspace_size_needs_no_gpu():
    """Host arithmetic, svae_ctfcorr.h's: 0 while 32 n m + 16 (n + m) bytes fit 160 KiB (up to 71 x 71), else 32 n m bytes for
    each of min(planes, 512) workgroups."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    for fn in (L.svae_frc_workspace_bytes, L.svae_frc_filter_workspace_bytes):
        assert fn(20, 40, 40) == 0 and fn(5, 71, 71) == 0 and fn(1, 13, 10) == 0
        assert fn(2, 72, 72) == 2 * 32 * 72 * 72 and fn(515, 72, 72) == 512 * 32 * 72 * 72 and fn(8, 256, 256) == 8 * 32 * 256 * 256


# ---------------------------------------------------------------- the ring rule
@pytest.mark.parametrize("n,m", [(8, 8), (9, 7), (13, 10), (40, 40), (96, 90)])
def test_the_integer_rule_is_the_rounded_radius(n, m):
    """The 64-bit rule against brute force on exact rationals, and against the double expression it replaces; every frequency is
    in exactly one ring or (at or beyond R) in none; ring 0 is the DC term alone on these boxes."""
    ring = F.ring_index(n, m)
    assert np.array_equal(ring, F.ring_index_rational(n, m))
    L, R = F.layout(n, m)
    rho = L * np.sqrt((F.signed(n)[:, None] / n) ** 2 + (F.signed(m)[None, :] / m) ** 2)
    assert np.array_equal(ring, np.floor(rho + 0.5).astype(np.int64))
    counts = F.ring_count(n, m)
    assert counts.shape == (R,) and counts.dtype == np.int32 and counts[0] == 1 and ring[0, 0] == 0
    assert counts.sum() + (ring >= R).sum() == n * m and (ring >= 0).all()
    assert (ring >= R).any() and ring.max() >= R        # the corners beyond Nyquist


def test_first_ring_counts():
    assert F.ring_count(40, 40)[:4].tolist() == [1, 8, 12, 16]
    assert F.ring_count(13, 10)[:4].tolist() == [1, 8, 14, 28]
    assert F.layout(13, 10) == (10, 6) and F.layout(9, 7) == (7, 4) and F.layout(40, 40) == (40, 21)


def test_ring_layout_is_the_references():
    from spatial_vae_amd import elbo as E
    for n, m in [(8, 8), (9, 7), (13, 10), (96, 90)]:
        L, R, freq = E.ring_layout(n, m)
        assert (L, R) == F.layout(n, m) and freq.shape == (R,) and freq.dtype == np.float64
        assert np.array_equal(freq, np.arange(R) / L) and freq[-1] <= 0.5


# ---------------------------------------------------------------- the reference, held to what a ring correlation means
def test_reference_frc_of_equal_opposite_and_scaled_planes():
    for n, m in [(13, 10), (40, 40)]:
        a, b = F.half_planes(5, n, m, 3)
        radius, edge = F.default_mask(n, m)
        for r, e in ((0.0, 0.0), (radius, edge)):
            _, same, counts = F.frc(a, a, n, m, r, e)
            assert np.abs(same - 1.0).max() <= 1e-12
            _, opposite, _ = F.frc(a, -a, n, m, r, e)
            assert np.abs(opposite + 1.0).max() <= 1e-12
            sums, curve, _ = F.frc(a, b, n, m, r, e)
            sums2, scaled, _ = F.frc(3.0 * a, 0.25 * b, n, m, r, e)
            assert np.abs(scaled - curve).max() <= 1e-12 and (np.abs(curve) <= 1 + 1e-12).all()
            assert np.allclose(sums2[..., 1], 9.0 * sums[..., 1], rtol=1e-12, atol=0)
            assert np.array_equal(counts, F.ring_count(n, m))
            assert curve[:, 1].min() > 0.9 and curve[:, -1].max() < 0.5     # signal at low frequency, noise at Nyquist
    zero = np.zeros((1, 8, 8))
    sums, curve, _ = F.frc(zero, np.ones((1, 8, 8)), 8, 8)
    assert (curve == 0).all() and sums[0, 0, 2] == 64.0 ** 2        # pa pb == 0: exactly 0


def test_reference_mask():
    w = F.mask(40, 40, 17.0, 3.0)
    d = np.hypot(*np.meshgrid(np.arange(40) - 19.5, np.arange(40) - 19.5))
    assert (w[d <= 17] == 1).all() and (w[d >= 20] == 0).all() and ((w > 0) & (w < 1))[(d > 17) & (d < 20)].all()
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1]) and (F.mask(9, 7, 0.0, 3.0) == 1).all()
    assert abs(F.mask(13, 10, 2.0, 2.0)[6, 7] - 0.5 * (1 + np.cos(np.pi * (np.hypot(0.0, 2.5) - 2.0) / 2.0))) <= 1e-15
    from spatial_vae_amd import elbo as E
    for n, m, r, e in [(40, 40, 17.0, 3.0), (13, 10, 2.0, 3.0), (9, 7, 0.0, 3.0), (13, 10, 1.0, 0.5)]:
        assert np.array_equal(E.frc_mask_weights(n, m, r, e), F.mask(n, m, r, e))


def test_reference_filter_is_a_band_limit():
    """Weight 1 on every ring: the frequencies beyond the last ring are removed and nothing else changes; on a plane that has
    none of those the filter returns the plane; the weights of one plane do not reach another."""
    for n, m in [(13, 10), (12, 12)]:
        L, R = F.layout(n, m)
        rs = np.random.RandomState(n)
        x = rs.normal(size=(2, n, m))
        inside = F.ring_index(n, m) < R
        limited = np.fft.ifft2(np.fft.fft2(x) * inside).real
        ones = np.ones((2, R))
        assert np.abs(F.filter_planes(x, ones, n, m) - limited).max() <= 1e-13
        assert np.abs(limited - x).max() > 1e-2
        assert np.abs(F.filter_planes(limited, ones, n, m) - limited).max() <= 1e-13
        w = np.stack([np.ones(R), np.zeros(R)])
        got = F.filter_planes(x, w, n, m)
        assert np.abs(got[0] - limited[0]).max() <= 1e-13 and (got[1] == 0).all()
        only_dc = np.zeros((2, R))
        only_dc[:, 0] = 1
        assert np.abs(F.filter_planes(x, only_dc, n, m) - x.mean(axis=(1, 2), keepdims=True)).max() <= 1e-13


def test_weight():
    import torch
    from spatial_vae_amd import elbo as E
    f = np.array([[1.0, 0.5, 0.143, 0.0, -0.2, 1e-300]])
    want = F.weight(f)
    assert want[0, 0] == 1.0 and want[0, 3] == 0.0 and want[0, 4] == 0.0 and abs(want[0, 1] - np.sqrt(2 / 3)) <= 1e-16
    got = E.frc_weight(torch.from_numpy(f))
    assert got.dtype == torch.float64 and np.abs(got.numpy() - want).max() <= 1e-15 and np.isfinite(got.numpy()).all()
    assert (got.numpy()[0, 3:5] == 0).all()


# ---------------------------------------------------------------- the resolution
def test_resolution_on_hand_made_curves():
    from spatial_vae_amd import elbo as E
    L = 40
    for fn in (F.resolution, E.frc_resolution):
        # an interior crossing: between ring 2 (0.6) and ring 3 (0.1) the line meets 0.5 at 2 + 0.1/0.5 = 2.2 rings
        res, never = fn(np.array([1.0, 0.9, 0.6, 0.1, 0.3, 0.0]), 0.5, L)
        assert not never and abs(res - 40 / 2.2) <= 1e-12
        res, never = fn(np.array([1.0, 0.9, 0.6, 0.1, 0.3, 0.0]), 0.143, L)
        assert not never and abs(res - 40 / (2 + (0.6 - 0.143) / 0.5)) <= 1e-12
        # the first ring below counts, not a later one
        res, never = fn(np.array([1.0, 0.4, 0.9, 0.1]), 0.5, L)
        assert not never and abs(res - 40 / ((1.0 - 0.5) / 0.6)) <= 1e-12
        # never below: the last ring, flagged
        assert fn(np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.5]), 0.5, L) == (40 / 5, True)
        # below at ring 0 (an empty half gives an all-zero curve): NaN
        for curve in (np.zeros(6), np.array([0.1, 0.9, 0.9]), np.array([np.nan, 1.0])):
            res, never = fn(curve, 0.143, L)
            assert np.isnan(res) and not never
    a = np.array([1.0, 0.93, 0.51, 0.2, 0.0])
    assert E.frc_resolution(a, 0.143, 9) == F.resolution(a, 0.143, 9)


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


def test_frc_options_default_to_off_and_fill_in(tmp_path):
    infer = _infer()
    base = _base(tmp_path)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz"])
    assert (a.frc, a.frc_mask_radius, a.frc_mask_edge) == (False, None, None)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz", "--frc"])
    assert (a.frc, a.frc_mask_radius, a.frc_mask_edge) == (True, None, 3.0)
    assert infer.frc_mask_radius(a, 40, 40) == 17.0 and infer.frc_mask_radius(a, 28, 28) == 11.0
    assert infer.frc_mask_radius(a, 13, 10) == 2.0 and infer.frc_mask_radius(a, 6, 9) == 1.0
    assert (infer.frc_mask_radius(a, 40, 40), a.frc_mask_edge) == F.default_mask(40, 40)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz", "--frc", "--frc_mask_radius", "0", "--frc_mask_edge", "1.5"])
    assert (a.frc_mask_radius, a.frc_mask_edge) == (0.0, 1.5) and infer.frc_mask_radius(a, 40, 40) == 0.0
    a = infer.infer_arguments(base + ["--class_averages", "c.npz", "--frc", "--frc_mask_radius", "9.5"])
    assert infer.frc_mask_radius(a, 40, 40) == 9.5 and a.frc_mask_edge == 3.0
    help_text = " ".join(infer_help().split())
    assert "--frc_mask_radius" in help_text and "a convention" in help_text.split("--frc_mask_radius")[1]


def infer_help():
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        _infer().infer_arguments(["--help"])
    return buf.getvalue()


REFUSALS = [
    (["--frc"], "--frc needs --class_averages"),
    (["--frc_mask_radius", "5"], "--frc_mask_radius needs --frc"),
    (["--frc_mask_edge", "2"], "--frc_mask_edge needs --frc"),
    (["--class_averages", "c.npz", "--frc_mask_edge", "2"], "--frc_mask_edge needs --frc"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_radius", "-1"], "--frc_mask_radius must be a finite number >= 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_radius", "inf"], "--frc_mask_radius must be a finite number >= 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_radius", "nan"], "--frc_mask_radius must be a finite number >= 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_edge", "-2"], "--frc_mask_edge must be a finite number > 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_edge", "0"], "--frc_mask_edge must be a finite number > 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_edge", "inf"], "--frc_mask_edge must be a finite number > 0"),
    (["--class_averages", "c.npz", "--frc", "--frc_mask_edge", "nan"], "--frc_mask_edge must be a finite number > 0"),
    (["--class_averages", "c.npz", "--frc", "--labels", "{many}"], "--frc keeps two sums per class: at most 2048 classes"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_frc_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    np.save(tmp_path / "many.npy", np.array([0, 2048, 1]))
    argv = _base(tmp_path) + [a.format(many=tmp_path / "many.npy") for a in extra]
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_a_box_above_1024_is_refused_against_the_split(tmp_path, capsys):
    infer = _infer()
    base = dict(images=4, n=8, m=8, channels=1, rotate=True, translate=True, inf_dim=6, z_scale=1, split="test", ctf_rows=None)
    args = infer.infer_arguments(_base(tmp_path) + ["--class_averages", "c.npz", "--frc"])
    assert infer.check_request(args, infer.SplitFacts(**base)) is None
    assert infer.check_request(args, infer.SplitFacts(**dict(base, n=1024, m=1024))) is None
    for shape in (dict(n=1025, m=1025), dict(n=8, m=1025), dict(n=1025)):
        with pytest.raises(SystemExit) as e:
            infer.check_request(args, infer.SplitFacts(**dict(base, **shape)))
        err = capsys.readouterr().err
        assert e.value.code == 2 and err.startswith("infer.py: ") and "at most 1024x1024" in err
    plain = infer.infer_arguments(_base(tmp_path) + ["--class_averages", "c.npz"])
    assert infer.check_request(plain, infer.SplitFacts(**dict(base, n=1025, m=1025))) is None
