"""CPU-only: the binding of include/svae_classify.h held to that header, the workspace formula on both sides of the LDS limit,
the float64 reference (tests/classify_ref.py) held to properties of what it restates and to its planted-truth case, and
infer.py's --reassign options: their defaults and every refusal."""
import numpy as np
import pytest

import classify_ref as CR
import refine_ref as R
from test_binding_cpu import binding_constants, parse_added_header


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_classify_binding_matches_its_header():
    """What is include/svae_classify.h's own (the rules every added header shares are tests/test_binding_cpu.py's): exactly two
    functions and their argument names, no constant and no struct; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_classify.h")[1]
    assert _lib.HEADERS["svae_classify.h"] is _lib.CLASSIFY_SIGNATURES
    assert H["constants"] == {} and not H["structs"] and len(H["functions"]) == 2
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_pose_classify_workspace_bytes"] == ["B", "n_ref", "M", "rows", "cols", "C"]
    assert names["svae_pose_classify"] == ["y", "ref", "weight", "cand", "pose_in", "B", "n_ref", "M", "rows", "cols", "C", "A", "step",
                                           "S", "interp", "choice", "ref_chosen", "cand_score", "margin", "ws", "ws_bytes", "stream"]
    assert not [k for k in binding_constants(_lib) if "CLASSIFY" in k]
    assert ops._POINTER_ARGS["svae_pose_classify"] == (0, 1, 2, 3, 4, 15, 16, 17, 18, 19)
    assert ops._POINTER_ARGS["svae_pose_classify_workspace_bytes"] == ()


def up32(v):
    return (v + 31) // 32 * 32


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: the norms alone, 8 roundup32(n_ref), while 8 (rows cols C + M + 8) bytes fit 160 KiB; above that also
    roundup32(rows cols C + M) doubles for each of min(B, 512) workgroups; 0 for sizes the call refuses."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_pose_classify_workspace_bytes
    limit = 160 * 1024 // 8
    for B, n_ref, M, rows, cols, C in [(100, 3, 3, 40, 40, 1), (5, 1, 1, 24, 24, 1), (1, 33, 24, 71, 72, 4), (7, 8192, 4096, 9, 8, 1)]:
        assert rows * cols * C + M + 8 <= limit
        assert fn(B, n_ref, M, rows, cols, C) == 8 * up32(n_ref)
    for B, n_ref, M, rows, cols, C in [(3, 4, 4, 256, 256, 1), (600, 2, 2, 144, 143, 1), (2, 2, 2, 72, 72, 4), (5, 70, 64, 128, 128, 2)]:
        assert rows * cols * C + M + 8 > limit
        assert fn(B, n_ref, M, rows, cols, C) == 8 * (up32(n_ref) + min(B, 512) * up32(rows * cols * C + M))
    # the limit moved once by the plane (M = 1: 20471 doubles of plane fit, 20472 do not) ...
    assert 71 * 72 * 4 + 1 + 8 <= limit < 72 * 72 * 4 + 1 + 8
    assert fn(2, 1, 1, 71, 72, 4) == 8 * 32 and fn(2, 1, 1, 72, 72, 4) == 8 * (32 + 2 * up32(72 * 72 * 4 + 1))
    assert 101 * 101 * 2 + 1 + 8 <= limit < 101 * 102 * 2 + 1 + 8
    assert fn(1, 1, 1, 101, 101, 2) == 8 * 32 and fn(1, 1, 1, 101, 102, 2) == 8 * (32 + up32(101 * 102 * 2 + 1))
    # ... and once by M: 71 x 72 x 4 = 20448 doubles of plane leave room for 24 maxima
    plane = 71 * 72 * 4
    assert plane + 24 + 8 == limit
    assert fn(3, 400, 24, 71, 72, 4) == 8 * up32(400)
    assert fn(3, 400, 25, 71, 72, 4) == 8 * (up32(400) + 3 * up32(plane + 25))
    # refused sizes
    for bad in [(0, 3, 3, 40, 40, 1), (3, 0, 3, 40, 40, 1), (3, 3, 0, 40, 40, 1), (3, 3, 4097, 40, 40, 1), (3, 3, 3, 1, 40, 1),
                (3, 3, 3, 40, 1025, 1), (3, 3, 3, 40, 40, 0), (3, 3, 3, 40, 40, 5), (1 << 20, 3, 3, 1024, 1024, 1),
                (3, 1 << 20, 3, 1024, 1024, 1), (1 << 20, 3, 4096, 2, 2, 1)]:
        assert fn(*bad) == 0, bad
    assert fn((1 << 19) - 1, 3, 4096, 2, 2, 1) > 0          # B M just under 2^31


# ---------------------------------------------------------------- the reference, held to what it restates
def _random_case(seed, B, rows, cols, C, n_ref=3):
    rs = np.random.RandomState(seed)
    y = rs.normal(size=(B, rows * cols, C)).astype(np.float32)
    ref = rs.normal(size=(n_ref, rows * cols, C))
    pose = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.2, 0.2, (B, 2))], 1).astype(np.float32)
    return y, ref, pose


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_one_slot_is_the_pose_search(interp):
    """M = 1: cand_score is refine_ref.pose_search's score, the choice slot 0 and the margin infinite."""
    y, ref, pose = _random_case(3, 4, 9, 7, 2)
    idx = np.array([0, 2, 1, 0], np.int32)
    got = CR.pose_classify(y, ref, None, idx[:, None], pose, 9, 7, 2, 0.07, 1, interp)
    want = R.pose_search(y, ref, None, idx, pose, 9, 7, 2, 0.07, 1, interp)
    assert got["cand_score"].shape == (4, 1) and np.array_equal(got["cand_score"][:, 0], want["score"])
    assert (got["choice"] == 0).all() and np.array_equal(got["ref_chosen"], idx) and np.isinf(got["margin"]).all()
    assert got["choice"].dtype == np.int32 and got["ref_chosen"].dtype == np.int32


def test_duplicates_empty_slots_and_zero_references():
    y, ref, pose = _random_case(4, 5, 8, 8, 1, n_ref=4)
    ref[2] = 0.0
    pose[4, 1] = np.nan
    cand = np.array([[1, 1, 0, 1],          # a duplicate never wins: the first of equals does
                     [-1, 2, 3, 7],         # empty (below and above the range) and all-zero slots: -inf, never the winner
                     [-1, 4, 2, -5],        # nothing live
                     [2, 0, -1, -1],        # one live slot: an infinite margin
                     [0, 1, 3, 0]], np.int32)       # a non-finite pose: nothing live
    got = CR.pose_classify(y, ref, None, cand, pose, 8, 8, 1, 0.05, 1)
    s = got["cand_score"]
    assert s[0, 0] == s[0, 1] == s[0, 3] and got["choice"][0] in (0, 2)
    if got["choice"][0] == 0:
        assert got["margin"][0] == 0.0 and got["ref_chosen"][0] == 1
    only = CR.pose_classify(y[:1], ref, None, np.array([[1, 1]], np.int32), pose[:1], 8, 8, 1, 0.05, 1)
    assert only["choice"][0] == 0 and only["margin"][0] == 0.0 and only["cand_score"][0, 0] == only["cand_score"][0, 1]
    assert np.isneginf(s[1, [0, 1, 3]]).all() and np.isfinite(s[1, 2]) and got["choice"][1] == 2 and got["ref_chosen"][1] == 3
    assert np.isinf(got["margin"][1]) and got["margin"][1] > 0
    for b in (2, 4):
        assert np.isneginf(s[b]).all() and got["choice"][b] == -1 and got["ref_chosen"][b] == -1 and got["margin"][b] == np.inf
    assert np.isneginf(s[3, [0, 2, 3]]).all() and got["choice"][3] == 1 and got["ref_chosen"][3] == 0 and got["margin"][3] == np.inf
    w = np.zeros(64)                                        # a weight that removes every reference: nothing live anywhere
    got = CR.pose_classify(y, ref, w, cand, pose, 8, 8, 1, 0.05, 1)
    assert np.isneginf(got["cand_score"]).all() and (got["choice"] == -1).all() and np.isinf(got["margin"]).all()


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_reference_assigns_every_planted_image_to_its_class(interp):
    """Three analytic classes (the blobs, their mirror image, the blobs less two), twelve images at known poses whose starts are
    off by up to 2.8 steps and 2 pixels, every third with a wrong starting label; scored against the three canonical images the
    reference picks the true class for every image.  Observed least classification margin: 0.0063 bicubic, 0.0060 bilinear: seven orders above
    the 1e-9 the device test asks of it before it compares winners."""
    y, ref, true, label, start = CR.planted_case()
    assert sorted(np.bincount(true).tolist()) == [4, 4, 4] and (label[::3] != true[::3]).all() and (label != true).sum() == 4
    p = CR.PLANTED
    cand = np.tile(np.arange(3, dtype=np.int32), (len(y), 1))
    got = CR.pose_classify(y, ref, None, cand, start, p["rows"], p["cols"], p["A"], p["step"], p["S"], interp)
    print("planted (%s): least margin %.3g, scores of the winners %.4f..%.4f"
          % (interp, got["margin"].min(), got["cand_score"].max(1).min(), got["cand_score"].max(1).max()))
    assert np.array_equal(got["choice"], true) and np.array_equal(got["ref_chosen"], true)
    assert got["margin"].min() > 1e-9


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


C = ["--class_averages", "c.npz"]


def test_reassign_options_default_to_off(tmp_path):
    infer = _infer()
    base = _base(tmp_path)
    a = infer.infer_arguments(base + C)
    assert a.reassign is False and a.reassign_labels is None
    a = infer.infer_arguments(base + C + ["--refine", "2"])
    assert a.reassign is False and a.reassign_labels is None
    a = infer.infer_arguments(base + C + ["--refine", "2", "--reassign"])
    assert a.reassign is True and a.reassign_labels is None and a.refine == 2
    a = infer.infer_arguments(base + C + ["--frc", "--refine", "1", "--reassign", "--reassign_labels", "new.npy"])
    assert a.reassign is True and a.reassign_labels == "new.npy"
    assert infer.INFER_MAX_REASSIGN_CLASSES == 4096


REFUSALS = [
    (C + ["--reassign"], "--reassign needs --refine"),
    (["--reassign"], "--reassign needs --refine"),
    (C + ["--reassign_labels", "l.npy"], "--reassign_labels needs --reassign"),
    (C + ["--refine", "1", "--reassign_labels", "l.npy"], "--reassign_labels needs --reassign"),
    (C + ["--refine", "1", "--reassign", "--reassign_labels", "l.npz"], "--reassign_labels must end in .npy"),
    (C + ["--refine", "1", "--reassign", "--reassign_labels", "labels"], "--reassign_labels must end in .npy"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_reassign_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_more_classes_than_the_kernel_takes_slots_are_refused(tmp_path, capsys, monkeypatch):
    """--labels already stops at 4096 classes, the kernel's M limit; the check of its own is seen with the limit lowered."""
    infer = _infer()
    labels = tmp_path / "l.npy"
    np.save(labels, np.array([0, 1, 2, -1]))
    argv = _base(tmp_path) + C + ["--labels", str(labels), "--refine", "1", "--reassign"]
    assert infer.infer_arguments(argv).reassign is True
    monkeypatch.setattr(infer, "INFER_MAX_REASSIGN_CLASSES", 2)
    assert infer.infer_arguments(argv[:-1]).reassign is False       # only --reassign is held to it
    with pytest.raises(SystemExit) as e:
        infer.infer_arguments(argv)
    assert e.value.code == 2 and "at most 2 classes (got 3)" in capsys.readouterr().err
