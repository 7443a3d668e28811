"""CPU-only: the binding of include/svae_refine.h held to that header, the float64 reference (tests/refine_ref.py) held to
properties of what it restates (the identity search, the shift identity, recovery of a known pose on an analytic image),
elbo.py's host helpers, and infer.py's --refine options: their defaults and every refusal."""
import numpy as np
import pytest

import align_ref as AR
import refine_ref as R
from test_binding_cpu import binding_constants, parse_added_header


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_refine_binding_matches_its_header():
    """What is include/svae_refine.h's own (the rules every added header shares are tests/test_binding_cpu.py's): two
    functions and their argument names, no constant and no struct; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_refine.h")[1]
    assert _lib.HEADERS["svae_refine.h"] is _lib.REFINE_SIGNATURES
    assert H["constants"] == {} and not H["structs"] and len(H["functions"]) == 2
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_pose_search_workspace_bytes"] == ["B", "rows", "cols", "C", "A", "S"]
    assert names["svae_pose_search"] == ["y", "ref", "weight", "ref_index", "pose_in", "B", "n_ref", "rows", "cols", "C", "A", "step",
                                         "S", "interp", "pose_out", "score", "offset", "scores", "ws", "ws_bytes", "stream"]
    assert not [k for k in binding_constants(_lib) if "REFINE" in k]
    assert ops._POINTER_ARGS["svae_pose_search"] == (0, 1, 2, 3, 4, 14, 15, 16, 17, 18)


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: 0 while 8 (rows cols C + (2A+1)(2S+1)^2 + 8) bytes fit 160 KiB, else that many doubles without the 8,
    rounded up to 256 bytes, for each of min(B, 512) workgroups; 0 for sizes the search refuses."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_pose_search_workspace_bytes
    assert fn(100, 40, 40, 1, 5, 2) == 0 and fn(5, 24, 24, 1, 32, 8) == 0 and fn(1, 71, 72, 4, 0, 0) == 0
    limit = 160 * 1024 // 8
    for B, rows, cols, C, A, S in [(3, 256, 256, 1, 5, 2), (600, 144, 143, 1, 1, 1), (2, 72, 72, 4, 0, 0)]:
        doubles = rows * cols * C + (2 * A + 1) * (2 * S + 1) ** 2
        assert doubles + 8 > limit
        assert fn(B, rows, cols, C, A, S) == min(B, 512) * ((doubles + 31) // 32 * 32) * 8
    assert fn(0, 40, 40, 1, 5, 2) == 0 and fn(3, 2000, 256, 1, 5, 2) == 0 and fn(3, 256, 256, 5, 5, 2) == 0
    assert fn(3, 256, 256, 1, 33, 2) == 0 and fn(3, 256, 256, 1, 5, 9) == 0


def lds_plane_limit(A, S):
    """The largest rows * cols * C the LDS form takes at a search of (A, S): 160 KiB of doubles less the volume and the 8."""
    return 160 * 1024 // 8 - 8 - (2 * A + 1) * (2 * S + 1) ** 2


def test_the_lds_limit_is_where_the_header_puts_it():
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_pose_search_workspace_bytes
    top = lds_plane_limit(1, 1)                             # 20445 doubles of plane
    assert top == 20445
    assert 71 * 72 * 4 == 20448 > top and fn(1, 71, 72, 4, 1, 1) > 0        # three doubles too many
    assert 71 * 71 * 4 <= top and fn(1, 71, 71, 4, 1, 1) == 0
    assert 101 * 101 * 2 <= top < 101 * 102 * 2 and fn(1, 101, 101, 2, 1, 1) == 0 and fn(1, 101, 102, 2, 1, 1) > 0


# ---------------------------------------------------------------- the reference, held to what it restates
def _random_case(seed, B, rows, cols, C):
    rs = np.random.RandomState(seed)
    y = rs.normal(size=(B, rows * cols, C)).astype(np.float32)
    ref = rs.normal(size=(2, rows * cols, C))
    pose = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)
    return y, ref, pose


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_an_empty_neighbourhood_returns_the_pose(interp):
    """A = S = 0: one candidate, which wins; no axis has a neighbour or more than one entry, so the pose comes back bit for bit
    with flags 0, whatever `step` is; the score is the plain normalised correlation of the aligned image with the reference."""
    y, ref, pose = _random_case(1, 4, 9, 7, 2)
    idx = np.array([0, 1, 1, 0], np.int32)
    for step in (0.1, float("nan")):
        out = R.pose_search(y, ref, None, idx, pose, 9, 7, 0, step, 0, interp)
        assert out["pose"].tobytes() == pose.tobytes() and (out["offset"] == 0).all() and out["scores"].shape == (4, 1, 1, 1)
    al, _ = AR.align_ref(y, pose[:, 0], pose[:, 1:], 9, 7, interp, dtype=np.float64)
    want = [(al[b] * ref[idx[b]]).sum() / np.sqrt((ref[idx[b]] ** 2).sum() * (al[b] ** 2).sum()) for b in range(4)]
    assert np.abs(out["score"] - want).max() <= 1e-14 and np.isinf(out["margin"]).all()


def test_skipped_images_keep_their_pose():
    y, ref, pose = _random_case(2, 5, 8, 8, 1)
    ref[1] = 0.0
    pose[3, 1] = np.nan
    pose[4, 0] = np.inf
    idx = np.array([-1, 1, 2, 0, 0], np.int32)
    out = R.pose_search(y, ref, None, idx, pose, 8, 8, 2, 0.05, 1)
    assert out["pose"].tobytes() == pose.tobytes() and (out["score"] == 0).all() and (out["scores"] == 0).all()
    assert (out["offset"] == [0, 0, 0, R.SKIPPED]).all()
    w = np.zeros(64)                                        # a weight that removes the whole reference: skipped as well
    out = R.pose_search(y[:1], ref, w, np.zeros(1, np.int32), pose[:1], 8, 8, 2, 0.05, 1)
    assert out["offset"][0].tolist() == [0, 0, 0, R.SKIPPED]


@pytest.mark.parametrize("rows,cols", [(12, 12), (9, 14)])
def test_a_shift_of_the_candidate_is_the_alignment_at_the_shifted_pose(rows, cols):
    """The identity the header states: Q for (sx, sy) equals align_ref at (theta, dx0 + sx/a, dx1 + sy/bq) wherever the latter's
    taps stay inside the box.  Bilinear at a dx of whole pixels: the two source positions then differ by the rotated whole
    shift only up to rounding (1e-12), and the pixels compared are those both cover with the 2 x 2 taps at least one pixel
    inside the border, so no clamp acts in either."""
    rs = np.random.RandomState(rows)
    y = rs.normal(size=(1, rows * cols, 2)).astype(np.float32)
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    compared = 0
    for theta in (0.0, 0.4, -2.0):
        pose = np.array([[theta, 2.0 / a, -1.0 / bq]])
        P = R.candidate_planes(y, pose, rows, cols, 0, 0.0, "bilinear")[0, 0]
        for sx, sy in [(1, 0), (0, 1), (-2, 1), (2, -2), (-1, -1)]:
            Q = R.shifted(P, sx, sy)
            moved = np.array([[theta, pose[0, 1] + sx / a, pose[0, 2] + sy / bq]])
            want, _ = AR.align_ref(y, moved[:, 0], moved[:, 1:], rows, cols, "bilinear", dtype=np.float64)
            fx, fy = AR.source_positions(moved[:, 0], moved[:, 1:], 1, rows, cols)
            inner = ((fx >= 1) & (fx <= cols - 2) & (fy >= 1) & (fy <= rows - 2))[0]
            jy, jx = np.nonzero(inner)
            inside = (jy + sy >= 0) & (jy + sy < rows) & (jx - sx >= 0) & (jx - sx < cols)
            jy, jx = jy[inside], jx[inside]
            assert len(jy) >= 4
            compared += len(jy)
            assert np.abs(Q[jy, jx] - want.reshape(rows, cols, 2)[jy, jx]).max() <= 1e-12
    assert compared > 200


RECOVERY_SEED = 100


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_reference_recovers_a_known_pose_on_an_analytic_image(interp):
    """Five off-centre Gaussians on the [-1, 1] grid, evaluated exactly at the posed coordinates (no resampling, no noise), in
    boxes of 24 x 24, 17 x 17 and 17 x 13; six draws each start within 2.8 steps and 2 pixels of the truth, A = 6, step 4
    degrees, S = 3, the canonical image as the reference, no weight.  The refined pose is within 1 step and 0.25 pixels of the
    truth and no winner is flagged at an edge.  Observed over the 18 draws (starting errors up to 2.64 steps, 1.98 px): bicubic
    0.673 steps, 0.069 px; bilinear 0.673 steps, 0.071 px.  What limits the angle is the half-pixel residue of the whole-pixel
    shifts, which a small rotation partly absorbs."""
    worst = np.zeros(2)
    for i, (rows, cols) in enumerate(R.RECOVERY_BOXES):
        y, ref, true, start = R.recovery_case(rows, cols, RECOVERY_SEED + i)
        e_angle, e_shift = R.recovery_errors(start, true, rows, cols)
        assert e_angle.max() <= 3 and e_shift.max() <= 2 and e_angle.max() > 2 and e_shift.max() > 1.5
        out = R.pose_search(y, ref, None, np.zeros(len(y), np.int32), start, rows, cols, R.RECOVERY["A"], R.RECOVERY["step"],
                            R.RECOVERY["S"], interp)
        e_angle, e_shift = R.recovery_errors(out["pose"], true, rows, cols)
        worst = np.maximum(worst, [e_angle.max(), e_shift.max()])
        assert (out["offset"][:, 3] == 0).all(), out["offset"]
    print("recovery (%s): %.3f steps, %.3f px" % (interp, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 0.25


def test_parabola():
    assert R.parabola(0.0, 1.0, 0.0) == 0.0 and R.parabola(0.5, 1.0, 0.0) == pytest.approx(-1.0 / 6.0)
    assert R.parabola(1.0, 1.0, 0.0) == -0.5 and R.parabola(0.0, 1.0, 1.0) == 0.5      # clamped at half a step
    assert R.parabola(1.0, 1.0, 1.0) == 0.0 and R.parabola(np.nan, 1.0, 0.0) == 0.0     # flat, or a NaN neighbour: no move


# ---------------------------------------------------------------- elbo.py's host helpers
def test_refine_mask_is_the_frc_mask_drawn_in_by_the_shift():
    from spatial_vae_amd import elbo as E
    import frc_ref as F
    for n, m, S in [(40, 40, 2), (28, 28, 0), (17, 13, 3), (256, 256, 8)]:
        radius = max(min(n, m) / 2.0 - 3.0 - S, 1.0)
        w = E.refine_mask(n, m, S)
        assert w.shape == (n, m) and w.dtype == np.float64 and np.array_equal(w, F.mask(n, m, radius, 3.0))
        if radius > 1:      # radius + edge = min(n, m)/2 - S: no weighted pixel in the S rows and columns along the border
            assert (w[:S] == 0).all() and (w[:, :S] == 0).all() and (w[n - S:] == 0).all() and (w[:, m - S:] == 0).all()
            assert w[n // 2, m // 2] == 1
    assert "convention" in E.refine_mask.__doc__


def test_initial_pose_is_what_align_minibatch_aligns_at():
    """(B, 3) fp32 = theta, dx0, dx1 of the chosen estimate; a coordinate the model does not infer is 0."""
    import torch
    from spatial_vae_amd import elbo as E
    rs = np.random.RandomState(0)
    for rotate, translate in [(True, True), (True, False), (False, True), (False, False)]:
        inf_dim = (1 if rotate else 0) + (2 if translate else 0) + 3
        lay = E.row_layout(rotate, translate, inf_dim)
        per_image = torch.from_numpy(rs.normal(size=(4, lay.width)).astype(np.float32))
        q_mu = torch.from_numpy(rs.normal(size=(4, inf_dim)).astype(np.float32))
        for pose, rows_of in (("iw", per_image[:, lay.iw]), ("best", per_image[:, lay.best]), ("q", q_mu)):
            got = E.initial_pose(per_image, q_mu, rotate, translate, pose)
            assert got.shape == (4, 3) and got.dtype == torch.float32
            assert torch.equal(got[:, 0], rows_of[:, 0] if rotate else torch.zeros(4))
            assert torch.equal(got[:, 1:], rows_of[:, lay.dx] if translate else torch.zeros(4, 2))


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


def test_refine_options_default_to_off_and_fill_in(tmp_path):
    infer = _infer()
    base = _base(tmp_path)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz"])
    assert (a.refine, a.refine_angles, a.refine_step, a.refine_shift) == (None, None, None, None)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz", "--refine", "3"])
    assert (a.refine, a.refine_angles, a.refine_step, a.refine_shift) == (3, 5, 2.0, 2)
    a = infer.infer_arguments(base + ["--class_averages", "c.npz", "--frc", "--refine", "10", "--refine_angles", "0", "--refine_step",
                                      "0.5", "--refine_shift", "8"])
    assert (a.refine, a.refine_angles, a.refine_step, a.refine_shift) == (10, 0, 0.5, 8)
    a = infer.infer_arguments(["particles", "--state", base[2], "--out", "s.npz", "--class_averages", "c.npz", "--ctf_correct", "flip",
                               "--refine", "1", "--refine_angles", "32", "--refine_shift", "0"])
    assert (a.refine, a.refine_angles, a.refine_shift, a.ctf_correct) == (1, 32, 0, "flip")


C = ["--class_averages", "c.npz"]
REFUSALS = [
    (["--refine", "2"], "--refine needs --class_averages"),
    (["--aligned", "a.npy", "--refine", "2"], "--refine needs --class_averages"),
    (C + ["--refine", "0"], "--refine must be in [1, 10]"),
    (C + ["--refine", "11"], "--refine must be in [1, 10]"),
    (C + ["--refine_angles", "3"], "--refine_angles needs --refine"),
    (C + ["--refine_step", "1.0"], "--refine_step needs --refine"),
    (C + ["--refine_shift", "1"], "--refine_shift needs --refine"),
    (["--refine_shift", "1"], "--refine_shift needs --refine"),
    (C + ["--refine", "1", "--refine_angles", "-1"], "--refine_angles must be in [0, 32]"),
    (C + ["--refine", "1", "--refine_angles", "33"], "--refine_angles must be in [0, 32]"),
    (C + ["--refine", "1", "--refine_shift", "-1"], "--refine_shift must be in [0, 8]"),
    (C + ["--refine", "1", "--refine_shift", "9"], "--refine_shift must be in [0, 8]"),
    (C + ["--refine", "1", "--refine_step", "0"], "--refine_step must be a finite number > 0"),
    (C + ["--refine", "1", "--refine_step", "-2"], "--refine_step must be a finite number > 0"),
    (C + ["--refine", "1", "--refine_step", "inf"], "--refine_step must be a finite number > 0"),
    (C + ["--refine", "1", "--refine_step", "nan"], "--refine_step must be a finite number > 0"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_refine_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_wiener_references_are_refused_by_the_parser(tmp_path, capsys):
    argv = ["particles", "--state", _base(tmp_path)[2], "--out", "s.npz"] + C + ["--ctf_correct", "wiener", "--refine", "1"]
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(argv)
    assert e.value.code == 2 and "--refine does not take --ctf_correct wiener" in capsys.readouterr().err


def test_a_model_without_a_pose_is_refused_against_the_model(tmp_path, capsys):
    infer = _infer()
    base = dict(images=4, n=8, m=8, channels=1, rotate=True, translate=True, inf_dim=6, z_scale=1, split="test", ctf_rows=None)
    args = infer.infer_arguments(_base(tmp_path) + C + ["--refine", "1"])
    for rotate, translate in [(True, True), (True, False), (False, True)]:
        assert infer.check_request(args, infer.SplitFacts(**dict(base, rotate=rotate, translate=translate))) is None
    with pytest.raises(SystemExit) as e:
        infer.check_request(args, infer.SplitFacts(**dict(base, rotate=False, translate=False, inf_dim=3)))
    err = capsys.readouterr().err
    assert e.value.code == 2 and err.startswith("infer.py: ") and "this model infers neither" in err
    with pytest.raises(SystemExit) as e:
        infer.check_request(args, infer.SplitFacts(**dict(base, n=1025)))
    assert e.value.code == 2 and "at most 1024x1024" in capsys.readouterr().err
    plain = infer.infer_arguments(_base(tmp_path) + C)
    assert infer.check_request(plain, infer.SplitFacts(**dict(base, rotate=False, translate=False, inf_dim=3))) is None
