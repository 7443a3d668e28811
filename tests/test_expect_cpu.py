"""CPU-only: the binding of include/svae_expect.h held to that header, the workspace formula on both sides of the LDS limit, the
float64 reference (tests/expect_ref.py) held to what a posterior means and to the room the device bounds of the kernel tests
rely on, and infer.py's --refine_soft options: their defaults and every refusal."""
import numpy as np
import pytest

import classify_ref as CR
import expect_ref as X
import refine_ref as R
from test_binding_cpu import binding_constants, parse_added_header


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_expect_binding_matches_its_header():
    """What is include/svae_expect.h's own (the rules every added header shares are tests/test_binding_cpu.py's): exactly
    three functions and their argument names, no constant and no struct; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_expect.h")[1]
    assert _lib.HEADERS["svae_expect.h"] is _lib.EXPECT_SIGNATURES
    assert H["constants"] == {} and not H["structs"] and len(H["functions"]) == 3
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_pose_expect_workspace_bytes"] == ["B", "n_ref", "M", "rows", "cols", "C", "A", "S"]
    assert names["svae_pose_expect"] == ["y", "ref", "weight", "log_prior", "cand", "pose_in", "B", "n_ref", "M", "rows", "cols", "C", "A",
                                         "step", "S", "interp", "inv_sigma2", "contrib", "cover_w", "class_post", "log_evidence", "best",
                                         "ws", "ws_bytes", "stream"]
    assert names["svae_expect_sums_update"] == ["contrib", "cover_w", "cand", "target", "B", "M", "N", "C", "n_ref", "n_classes", "sum",
                                                "count", "stream"]
    assert not [k for k in binding_constants(_lib) if "EXPECT" in k]
    assert ops._POINTER_ARGS["svae_pose_expect"] == (0, 1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 22)
    assert ops._POINTER_ARGS["svae_expect_sums_update"] == (0, 1, 2, 3, 10, 11)
    assert ops._POINTER_ARGS["svae_pose_expect_workspace_bytes"] == ()
    assert ops.PoseExpect._fields == ("contrib", "cover_w", "class_post", "log_evidence", "best")
    assert callable(ops.ClassSums.update_soft)


def up32(v):
    return (v + 31) // 32 * 32


def doubles(M, rows, cols, C, A, S):
    return rows * cols * C + rows * cols + M * (2 * A + 1) * (2 * S + 1) ** 2


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: h alone, 8 roundup32(n_ref), while 8 (N C + N + M nA nS^2 + 40) bytes fit 160 KiB; above that also
    roundup32(N C + N + M nA nS^2) doubles for each of min(B, 512) workgroups; 0 for sizes the call refuses."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_pose_expect_workspace_bytes
    limit = 160 * 1024 // 8
    for B, n_ref, M, rows, cols, C, A, S in [(100, 8, 8, 40, 40, 1, 5, 2), (5, 3, 1, 24, 24, 1, 3, 2), (5, 5, 3, 17, 13, 3, 2, 3),
                                             (5, 66, 64, 9, 8, 1, 0, 0), (700, 2, 2, 64, 64, 3, 1, 1)]:
        assert doubles(M, rows, cols, C, A, S) + 40 <= limit
        assert fn(B, n_ref, M, rows, cols, C, A, S) == 8 * up32(n_ref)
    for B, n_ref, M, rows, cols, C, A, S in [(5, 9, 7, 9, 8, 1, 32, 8), (5, 4, 2, 72, 72, 4, 1, 1), (600, 2, 2, 144, 143, 1, 0, 0),
                                             (3, 70, 64, 40, 40, 1, 5, 2)]:
        d = doubles(M, rows, cols, C, A, S)
        assert d + 40 > limit
        assert fn(B, n_ref, M, rows, cols, C, A, S) == 8 * (up32(n_ref) + min(B, 512) * up32(d))
    # the limit moved once by the plane and its coverage (C = 1, M = 1, A = S = 0: 2 N + 1 + 40 doubles) ...
    assert 2 * 101 * 101 + 1 + 40 <= limit < 2 * 101 * 102 + 1 + 40
    assert fn(2, 1, 1, 101, 101, 1, 0, 0) == 8 * 32 and fn(2, 1, 1, 101, 102, 1, 0, 0) == 8 * (32 + 2 * up32(2 * 101 * 102 + 1))
    # ... and once by the volume: 40 x 40 x 1 leaves 20480 - 3200 - 40 = 17240 doubles, 62 volumes of A = 5, S = 2 (275 each)
    assert 3200 + 62 * 275 + 40 <= limit < 3200 + 63 * 275 + 40
    assert fn(3, 70, 62, 40, 40, 1, 5, 2) == 8 * up32(70)
    assert fn(3, 70, 63, 40, 40, 1, 5, 2) == 8 * (up32(70) + 3 * up32(3200 + 63 * 275))
    # refused sizes
    for bad in [(0, 3, 3, 40, 40, 1, 1, 1), (3, 0, 3, 40, 40, 1, 1, 1), (3, 3, 0, 40, 40, 1, 1, 1), (3, 3, 65, 40, 40, 1, 1, 1),
                (3, 3, 3, 1, 40, 1, 1, 1), (3, 3, 3, 40, 1025, 1, 1, 1), (3, 3, 3, 40, 40, 0, 1, 1), (3, 3, 3, 40, 40, 5, 1, 1),
                (3, 3, 3, 40, 40, 1, -1, 1), (3, 3, 3, 40, 40, 1, 33, 1), (3, 3, 3, 40, 40, 1, 1, -1), (3, 3, 3, 40, 40, 1, 1, 9),
                (1 << 20, 3, 3, 1024, 1024, 1, 1, 1), (3, 1 << 20, 3, 1024, 1024, 1, 1, 1), (1 << 10, 3, 64, 256, 256, 1, 1, 1)]:
        assert fn(*bad) == 0, bad
    assert fn((1 << 10) - 1, 3, 32, 256, 256, 1, 1, 1) > 0          # B M N C just under 2^31


# ---------------------------------------------------------------- the reference, held to what a posterior means
def _random_case(seed, B, rows, cols, C, n_ref=3):
    rs = np.random.RandomState(seed)
    y = rs.normal(size=(B, rows * cols, C)).astype(np.float32)
    ref = rs.normal(size=(n_ref, rows * cols, C))
    pose = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)
    return y, ref, pose


def test_flat_posterior_at_zero_precision():
    """inv_sigma2 = 0 with no prior: every live entry has p = 1 / (live nA nS^2): exactly where that count is a power of two,
    within 1e-15 otherwise; class_post rows sum to 1 within 1e-12; the first entry is the maximum."""
    y, ref, pose = _random_case(11, 2, 8, 8, 1, n_ref=5)
    cand = np.array([[0, 3, 1, 4], [2, 2, -1, 0]], np.int32)          # 4 live slots; 2 live slots
    got = X.pose_expect(y, ref, None, None, cand, pose, 8, 8, 0, 0.1, 0, 0.0)               # 4 and 2 entries: powers of two
    assert np.array_equal(got["class_post"], [[0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.0, 0.5]])
    assert np.array_equal(got["log_evidence"], np.log([4.0, 2.0])) and np.array_equal(got["best"], [[0, 0, 0, 0], [0, 0, 0, 0]])
    got = X.pose_expect(y, ref, None, None, cand, pose, 8, 8, 1, 0.1, 1, 0.0)               # 27 entries per slot
    assert np.abs(got["class_post"] - [[0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.0, 0.5]]).max() <= 1e-15
    assert np.abs(got["class_post"].sum(1) - 1).max() <= 1e-12
    assert np.array_equal(got["best"], [[0, -1, -1, -1], [0, -1, -1, -1]])
    assert np.abs(got["log_evidence"] - np.log([108.0, 54.0])).max() <= 1e-14
    assert np.abs(got["cover_w"]).max() <= 0.5 + 1e-15


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_large_precision_is_one_hot_on_the_classifier_winner(interp):
    """The planted three-class case at inv_sigma2 = 1e6: class_post is one-hot on classify_ref's winner for every image."""
    y, ref, cand, start = X.planted_one_hot()
    p = CR.PLANTED
    want = CR.pose_classify(y, ref, None, cand, start, p["rows"], p["cols"], p["A"], p["step"], p["S"], interp)
    got = X.pose_expect(y, ref, None, None, cand, start, p["rows"], p["cols"], p["A"], p["step"], p["S"], 1e6, interp)
    assert np.array_equal(got["class_post"].argmax(1), want["choice"]) and np.array_equal(got["best"][:, 0], want["choice"])
    assert np.array_equal(got["class_post"].max(1), np.ones(len(y))) and np.array_equal(np.sort(got["class_post"], 1)[:, :2], np.zeros((len(y), 2)))


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_one_slot_one_pose_is_the_aligned_image(interp):
    """M = 1, A = S = 0: p = 1, contrib is P_0 and cover_w its coverage, exactly; log_evidence is L itself."""
    y, ref, pose = _random_case(5, 3, 9, 7, 2)
    idx = np.array([[0], [2], [1]], np.int32)
    got = X.pose_expect(y, ref, None, None, idx, pose, 9, 7, 0, 0.0, 0, 0.37, interp)
    P = R.candidate_planes(y, pose, 9, 7, 0, 0.0, interp)[:, 0].reshape(3, 63, 2)
    cover = X.coverage_planes(y, pose, 9, 7, 0, 0.0, interp)[:, 0].reshape(3, 63)
    assert np.array_equal(got["contrib"][:, 0], P) and np.array_equal(got["cover_w"][:, 0], cover)
    assert np.array_equal(got["class_post"], np.ones((3, 1))) and 0 < cover.sum() < cover.size
    for b in range(3):
        L = 0.37 * ((ref[idx[b, 0]] * P[b]).sum() - 0.5 * (ref[idx[b, 0]] ** 2).sum())
        assert abs(got["log_evidence"][b] - L) <= 1e-12 * abs(L)


def test_dead_slots_and_skipped_images():
    """A repeated slot and a slot whose prior is -inf are dead (zero rows, zero posterior); an image with no live slot, a NaN
    pose or a NaN pixel is skipped: zeros everywhere and best = (-1, 0, 0, 0)."""
    y, ref, pose = _random_case(4, 5, 8, 8, 1, n_ref=4)
    pose[3, 1] = np.nan
    y[4, 27, 0] = np.nan
    with np.errstate(divide="ignore"):
        prior = np.log(np.array([0.5, 0.25, 0.0, 0.25]))
    cand = np.array([[1, 1, 0], [2, 3, 7], [-1, 4, 2], [0, 1, 3], [0, 1, 3]], np.int32)
    got = X.pose_expect(y, ref, None, prior, cand, pose, 8, 8, 1, 0.05, 1, 0.01)
    assert got["class_post"][0, 1] == 0 and not got["contrib"][0, 1].any() and not got["cover_w"][0, 1].any()
    assert got["class_post"][0, 0] > 0 and got["class_post"][0, 2] > 0 and abs(got["class_post"][0].sum() - 1) <= 1e-12
    assert np.array_equal(got["class_post"][1], [0.0, 1.0, 0.0]) and got["best"][1, 0] == 1       # -inf prior, live, out of range
    assert not got["contrib"][1, [0, 2]].any() and got["contrib"][1, 1].any()
    for b in (2, 3, 4):
        assert not got["class_post"][b].any() and got["log_evidence"][b] == 0 and np.array_equal(got["best"][b], [-1, 0, 0, 0])
        assert not got["contrib"][b].any() and not got["cover_w"][b].any()


def test_reference_sums_update_folds_and_skips():
    rs = np.random.RandomState(0)
    contrib, cover_w = rs.normal(size=(3, 2, 6, 1)), rs.uniform(size=(3, 2, 6))
    cand = np.array([[0, 3], [2, -1], [1, 9]], np.int32)
    halves = X.sums_update(np.zeros((4, 6, 1)), np.zeros((4, 6)), contrib, cover_w, cand, None, 4)
    full = X.sums_update(np.zeros((2, 6, 1)), np.zeros((2, 6)), contrib, cover_w, cand, np.arange(4) >> 1, 4)
    assert np.abs(full[0] - (halves[0][0::2] + halves[0][1::2])).max() <= 1e-15
    assert np.abs(full[1] - (halves[1][0::2] + halves[1][1::2])).max() <= 1e-15
    assert np.array_equal(halves[0][3], contrib[0, 1]) and np.array_equal(halves[1][2], cover_w[1, 0])
    few = X.sums_update(np.zeros((1, 6, 1)), np.zeros((1, 6)), contrib, cover_w, cand, np.array([0, 5, -1, 0]), 4)
    assert np.array_equal(few[0][0], contrib[0, 0] + contrib[0, 1])      # targets 5 and -1 are skipped


# ---------------------------------------------------------------- the bounds the device tests rely on
@pytest.mark.parametrize("index", range(len(X.SHAPES)), ids=X.SHAPE_IDS)
def test_fixture_spreads_and_gaps(index):
    """For every fixture the device tests run (both interps, with and without weight and prior): at the inv_sigma2 the rule
    picks, max L - min L of every image that is not skipped lies in [5, 50] -- wherever the volume has more than one entry: the
    posterior is neither flat nor one-hot -- and the largest L leads the second by more than 1e-9, so the device test compares
    `best` for every image; rows of class_post sum to 1 within 1e-12; image 3 is skipped and image 1 has its repeat dead."""
    rows, cols, C, A, S, M = X.SHAPES[index]
    for interp in ("bicubic", "bilinear"):
        for weighted in (True, False):
            for prior in (True, False):
                f = X.fixture(index, weighted, prior)
                inv = X.pick_inv_sigma2(f, interp)
                got = X.run(f, inv, interp)
                ran = [b for b in range(f["B"]) if b != 3]
                assert got["best"][3, 0] == -1 and (got["best"][ran, 0] >= 0).all()
                spread, gap = got["spread"][ran], got["gap"][ran]
                print("%s %s w=%d p=%d: inv_sigma2 %g, spread %.3g..%.3g, least gap %.3g"
                      % (X.SHAPE_IDS[index], interp, weighted, prior, inv, spread.min(), spread.max(), gap.min()))
                several = [i for i, b in enumerate(ran) if (f["cand"][b] >= 0).sum() * (2 * A + 1) * (2 * S + 1) ** 2 > 1]
                assert len(several) == len(ran)
                assert (spread >= X.SPREAD[0]).all() and (spread <= X.SPREAD[1]).all()
                assert (gap > 1e-9).all()
                assert np.abs(got["class_post"][ran].sum(1) - 1).max() <= 1e-12
                if M > 1:
                    assert got["class_post"][1, M - 1] == 0 and not got["contrib"][1, M - 1].any()


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


C = ["--class_averages", "c.npz"]
RR = C + ["--refine", "1", "--reassign"]


def test_refine_soft_options_default_to_off(tmp_path):
    infer = _infer()
    base = _base(tmp_path)
    a = infer.infer_arguments(base + RR)
    assert a.refine_soft is False and a.refine_soft_classes is None and a.refine_soft_sigma2 is None
    a = infer.infer_arguments(base + RR + ["--refine_soft"])
    assert a.refine_soft is True and a.refine_soft_classes == 8 and a.refine_soft_sigma2 is None
    a = infer.infer_arguments(base + RR + ["--frc", "--refine_soft", "--refine_soft_classes", "64", "--refine_soft_sigma2", "0.25"])
    assert a.refine_soft_classes == 64 and a.refine_soft_sigma2 == 0.25
    assert infer.infer_arguments(base + RR + ["--refine_soft", "--refine_soft_classes", "1"]).refine_soft_classes == 1
    assert infer.INFER_MAX_SOFT_CLASSES == 64


REFUSALS = [
    (C + ["--refine_soft"], "--refine_soft needs --refine"),
    (["--refine_soft"], "--refine_soft needs --refine"),
    (C + ["--refine", "1", "--refine_soft"], "--refine_soft needs --reassign"),
    (RR + ["--refine_soft_classes", "4"], "--refine_soft_classes needs --refine_soft"),
    (RR + ["--refine_soft_sigma2", "1.0"], "--refine_soft_sigma2 needs --refine_soft"),
    (RR + ["--refine_soft", "--refine_soft_classes", "0"], "--refine_soft_classes must be in [1, 64] (got 0)"),
    (RR + ["--refine_soft", "--refine_soft_classes", "65"], "--refine_soft_classes must be in [1, 64] (got 65)"),
    (RR + ["--refine_soft", "--refine_soft_sigma2", "0"], "--refine_soft_sigma2 must be a finite number > 0"),
    (RR + ["--refine_soft", "--refine_soft_sigma2", "-1"], "--refine_soft_sigma2 must be a finite number > 0"),
    (RR + ["--refine_soft", "--refine_soft_sigma2", "inf"], "--refine_soft_sigma2 must be a finite number > 0"),
    (RR + ["--refine_soft", "--refine_soft_sigma2", "nan"], "--refine_soft_sigma2 must be a finite number > 0"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_refine_soft_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err
