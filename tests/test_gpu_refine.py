"""The pose search (include/svae_refine.h: svae_pose_search; ops.pose_search) on the MI355X against the float64 reference
tests/refine_ref.py: the whole score volume, the winners, the refined poses, shape by shape through both memory forms and both
interpolations; bit-equality of repeated and of split calls; every refusal of the header with the buffers prefilled and compared;
and the recovery of a known pose on the analytic image of tests/test_refine_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import refine_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
# Scores lie in [-1, 1]; a sum of at most a few thousand doubles carries ~1e-13 and a last-place difference in sin / cos moves
# a source position by ~1e-15: that estimate with three orders of margin.
TOL_SCORE = 1e-10
MARGIN = 1e-9       # the winner is compared wherever the reference's best beats its second best by more than this
TOL_POSE = 1e-6
# (rows, cols, C, A, step, S, weighted).  The first two stay in LDS (8 (rows cols C + (2A+1)(2S+1)^2 + 8) bytes within 160 KiB);
# 71 x 72 x 4 = 20448 doubles of plane with a volume of 45 is the smallest box of four channels that does not (71 x 71 x 4 =
# 20164 does: 20164 + 45 + 8 <= 20480 < 20448 + 45 + 8) and goes through the workspace; the last has the largest search the
# header takes, 65 angles by 17 x 17 shifts, most of which move the whole 9 x 8 box out of itself; the row after it is a volume of
# one entry (A = S = 0): three of the four waves get no shift, no edge flag can be set and the reference's margin is +inf.
SHAPES = [(24, 24, 1, 3, 0.05, 2, True), (17, 13, 3, 2, 0.08, 3, False), (71, 72, 4, 2, 0.03, 1, True), (9, 8, 1, 32, 0.02, 8, False),
          (9, 8, 1, 0, 0.1, 0, True)]
REF_INDEX = np.array([0, 1, -1, 2, 1], np.int32)        # two references, one image in no class, one all-zero reference


@functools.lru_cache(maxsize=None)
def _case(rows, cols, C, A, step, S, weighted, interp):
    """The shared, read-only inputs and reference results of one shape: B = 5 smooth random images, references that are other
    poses of images 0 and 1 plus noise (so the volume has a peak to find), the mask of elbo.refine_mask or none."""
    from spatial_vae_amd import elbo as E
    import align_ref as AR
    rs = np.random.RandomState(rows * cols + C + A)
    B = len(REF_INDEX)
    y = rs.normal(size=(B, rows, cols, C))
    y = (y + np.roll(y, 1, 1) + np.roll(y, 1, 2) + np.roll(y, (1, 1), (1, 2))).reshape(B, rows * cols, C).astype(np.float32)
    y[4] = y[1]
    pose = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.15, 0.15, (B, 2))], 1).astype(np.float32)
    near = pose.astype(np.float64) + np.concatenate([rs.uniform(-A, A, (B, 1)) * step, rs.uniform(-S, S, (B, 2)) / ((cols - 1) / 2.0)], 1)
    aligned, _ = AR.align_ref(y, near[:, 0], near[:, 1:], rows, cols, interp, dtype=np.float64)
    ref = np.stack([aligned[0], aligned[1], np.zeros_like(aligned[0])]) + np.concatenate([0.1 * rs.normal(size=(2, rows * cols, C)),
                                                                                           np.zeros((1, rows * cols, C))])
    weight = E.refine_mask(rows, cols, S).reshape(-1) if weighted else None
    want = R.pose_search(y, ref, weight, REF_INDEX, pose, rows, cols, A, step, S, interp)
    for x in (y, ref, pose) + tuple(want.values()):
        x.setflags(write=False)
    return {"y": y, "ref": ref, "weight": weight, "pose": pose, "want": want}


def _search(c, rows, cols, A, step, S, interp, lo=0, hi=None, scores=True):
    from spatial_vae_amd import ops
    dev = lambda a: None if a is None else torch.tensor(a[lo:hi] if a.shape[0] == len(REF_INDEX) else a).to(DEV)
    weight = None if c["weight"] is None else torch.tensor(c["weight"]).to(DEV)
    return ops.pose_search(dev(c["y"]), torch.tensor(c["ref"]).to(DEV), weight, torch.tensor(REF_INDEX[lo:hi]).to(DEV), dev(c["pose"]),
                           rows, cols, A, step, S, interp, return_scores=scores)


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
@pytest.mark.parametrize("rows,cols,C,A,step,S,weighted", SHAPES)
def test_pose_search_matches_the_reference(rows, cols, C, A, step, S, weighted, interp):
    """The whole score volume within 1e-10, every winner equal (the reference's margin over its second best exceeds 1e-9 for
    every image of every case: asserted, so nothing is left out), pose_out within 1e-6, the winning score within 1e-10; the
    image in no class and the image of the all-zero reference come back skipped with their pose bit for bit; a second run and
    the two halves [0, 2) and [2, 5) are bit-equal to the one call; without the volume the other outputs are the same bits.
    MI355X: volume at most 3.4e-16 over all cases, every pose_out equal to the reference's in every bit; least margin 2.3e-4."""
    from spatial_vae_amd import _lib
    c = _case(rows, cols, C, A, step, S, weighted, interp)
    want = c["want"]
    uses_ws = _lib.lib().svae_pose_search_workspace_bytes(5, rows, cols, C, A, S) > 0
    assert uses_ws == ((rows, cols, C) == (71, 72, 4))
    got = _search(c, rows, cols, A, step, S, interp)
    assert got.pose.shape == (5, 3) and got.pose.dtype == torch.float32 and got.score.shape == (5,) and got.score.dtype == torch.float64
    assert got.offset.shape == (5, 4) and got.offset.dtype == torch.int32
    assert got.scores.shape == (5, 2 * A + 1, 2 * S + 1, 2 * S + 1) and got.scores.dtype == torch.float64
    again = _search(c, rows, cols, A, step, S, interp)
    first, second = _search(c, rows, cols, A, step, S, interp, 0, 2), _search(c, rows, cols, A, step, S, interp, 2, 5)
    bare = _search(c, rows, cols, A, step, S, interp, scores=False)
    assert bare.scores is None
    for name in ("pose", "score", "offset", "scores"):
        t = getattr(got, name)
        assert torch.equal(t.view(torch.uint8), getattr(again, name).view(torch.uint8)), name
        halves = torch.cat([getattr(first, name), getattr(second, name)])
        assert torch.equal(t.view(torch.uint8), halves.view(torch.uint8)), name
        if name != "scores":
            assert torch.equal(t.view(torch.uint8), getattr(bare, name).view(torch.uint8)), name
    pose, score, offset, scores = (t.cpu().numpy() for t in got)
    live = np.array([0, 1, 4])
    margin = want["margin"][live].min()
    e_vol = float(np.abs(scores - want["scores"]).max())
    e_score = float(np.abs(score - want["score"]).max())
    e_pose = float(np.abs(pose.astype(np.float64) - want["pose"].astype(np.float64)).max())
    print("%dx%dx%d A=%d S=%d %s %s: volume %.2e, score %.2e, pose %.2e; least margin %.1e; flags %s"
          % (rows, cols, C, A, S, interp, "workspace" if uses_ws else "LDS", e_vol, e_score, e_pose, margin, offset[:, 3].tolist()))
    assert np.isfinite(scores).all() and np.abs(scores).max() <= 1 + 1e-12
    assert margin > MARGIN, want["margin"]
    assert e_vol <= TOL_SCORE and e_score <= TOL_SCORE
    assert np.array_equal(offset, want["offset"])
    assert e_pose <= TOL_POSE
    for b in (2, 3):                                        # skipped: no class, and an all-zero reference
        assert offset[b].tolist() == [0, 0, 0, R.SKIPPED] and score[b] == 0 and (scores[b] == 0).all()
        assert pose[b].tobytes() == c["pose"][b].tobytes()
    assert (offset[live, 3] & R.SKIPPED == 0).all() and (score[live] > 0).all()


def test_non_finite_poses_and_images_are_skipped():
    """A NaN or infinite pose component: skipped, pose_out the same bits.  An image that holds a NaN gives NaN scores only, and
    a NaN never wins: skipped too."""
    c = _case(17, 13, 3, 2, 0.08, 3, False, "bicubic")
    from spatial_vae_amd import ops
    y, pose = torch.tensor(c["y"]).to(DEV), torch.tensor(c["pose"]).to(DEV)
    pose[0, 0], pose[1, 2] = float("nan"), float("inf")
    y[4, 7, 1] = float("nan")
    idx = torch.zeros(5, dtype=torch.int32, device=DEV)
    got = ops.pose_search(y, torch.tensor(c["ref"]).to(DEV), None, idx, pose, 17, 13, 2, 0.08, 3, return_scores=True)
    offset = got.offset.cpu().numpy()
    assert offset[[0, 1, 4]].tolist() == [[0, 0, 0, R.SKIPPED]] * 3 and (offset[[2, 3], 3] & R.SKIPPED == 0).all()
    assert torch.equal(got.pose.view(torch.int32)[[0, 1, 4]], pose.view(torch.int32)[[0, 1, 4]])
    assert (got.score[[0, 1, 4]] == 0).all() and (got.scores[:2] == 0).all() and torch.isnan(got.scores[4]).any()


def _refused(rc, L, word=None):
    from spatial_vae_amd import _lib
    message = L.svae_last_error()
    assert rc == _lib.E_INVALID and message, (rc, message)
    if word is not None:
        assert word in message, message


def test_every_refusal_leaves_the_buffers_untouched():
    """Each SVAE_E_INVALID case of the header, through the raw entry point: the code, a message (naming the workspace where that
    is the reason), and every output still what it was prefilled with; the calls these were variations of are accepted."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    B, rows, cols, C, A, S = 3, 10, 8, 2, 2, 1
    f64 = dict(dtype=torch.float64, device=DEV)

    def buffers(B, rows, cols, C, A, S):
        t = {"y": torch.ones(B, rows * cols, C, device=DEV), "ref": torch.ones(2, rows * cols, C, **f64),
             "weight": torch.ones(rows * cols, **f64), "ref_index": torch.zeros(B, dtype=torch.int32, device=DEV),
             "pose_in": torch.zeros(B, 3, device=DEV), "pose_out": torch.full((B, 3), 7.0, device=DEV),
             "score": torch.full((B,), 7.0, **f64), "offset": torch.full((B, 4), 7, dtype=torch.int32, device=DEV),
             "scores": torch.full((B, 2 * A + 1, 2 * S + 1, 2 * S + 1), 7.0, **f64)}
        return t, {k: v.data_ptr() for k, v in t.items()}

    small, p = buffers(B, rows, cols, C, A, S)

    def search(p=p, B=B, n_ref=2, rows=rows, cols=cols, C=C, A=A, step=0.1, S=S, interp=1, ws=None, ws_bytes=0, **ptr):
        q = dict(p, **ptr)
        return L.svae_pose_search(q["y"], q["ref"], q["weight"], q["ref_index"], q["pose_in"], B, n_ref, rows, cols, C, A, step, S,
                                  interp, q["pose_out"], q["score"], q["offset"], q["scores"], ws, ws_bytes, None)

    inf, nan = float("inf"), float("nan")
    for kw in (dict(B=0), dict(B=-1), dict(n_ref=0), dict(rows=1), dict(cols=1), dict(rows=1025), dict(cols=1025), dict(C=0), dict(C=5),
               dict(A=-1), dict(A=33), dict(S=-1), dict(S=9), dict(step=0.0), dict(step=-0.1), dict(step=nan), dict(step=inf),
               dict(interp=2), dict(interp=-1), dict(y=None), dict(ref=None), dict(ref_index=None), dict(pose_in=None),
               dict(pose_out=None), dict(score=None), dict(offset=None), dict(B=1 << 20, rows=1024, cols=1024),
               dict(n_ref=1 << 20, rows=1024, cols=1024)):
        _refused(search(**kw), L)
    need = L.svae_pose_search_workspace_bytes(2, 71, 72, 4, A, S)
    assert need == 2 * ((71 * 72 * 4 + 45 + 31) // 32 * 32) * 8 and L.svae_pose_search_workspace_bytes(B, rows, cols, C, A, S) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    big, bp = buffers(2, 71, 72, 4, A, S)
    for kw in (dict(ws=None, ws_bytes=0), dict(ws=ws.data_ptr(), ws_bytes=need - 1), dict(ws=None, ws_bytes=need),
               dict(ws=ws.data_ptr() + 8, ws_bytes=need)):
        _refused(search(p=bp, B=2, rows=71, cols=72, C=4, **kw), L, b"workspace")
    torch.cuda.synchronize()
    for t in (small, big):
        assert (t["pose_out"] == 7.0).all() and (t["score"] == 7.0).all() and (t["offset"] == 7).all() and (t["scores"] == 7.0).all()
        assert (t["y"] == 1.0).all() and (t["ref"] == 1.0).all() and (t["pose_in"] == 0.0).all()
    # and the calls these were variations of are accepted: a NULL weight, a NULL volume, any step where A == 0
    assert search() == 0 and search(weight=None) == 0 and search(scores=None) == 0 and search(A=0, step=nan) == 0
    assert search(p=bp, B=2, rows=71, cols=72, C=4, ws=ws.data_ptr(), ws_bytes=need) == 0
    torch.cuda.synchronize()
    for t in (small, big):
        assert not (t["pose_out"] == 7.0).any() and not (t["score"] == 7.0).any() and not (t["offset"] == 7).any()
        assert (t["offset"][:, 3] & R.SKIPPED == 0).all()
    assert not (big["scores"] == 7.0).any()


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_device_recovers_a_known_pose_on_the_analytic_image(interp):
    """tests/test_refine_cpu.py's recovery case on the device: the same 18 draws, A = 6, step 4 degrees, S = 3; within 1 step and
    0.25 pixels of the truth, no winner at an edge, and the winners are the reference's."""
    from spatial_vae_amd import ops
    from test_refine_cpu import RECOVERY_SEED
    worst = np.zeros(2)
    for i, (rows, cols) in enumerate(R.RECOVERY_BOXES):
        y, ref, true, start = R.recovery_case(rows, cols, RECOVERY_SEED + i)
        idx = torch.zeros(len(y), dtype=torch.int32, device=DEV)
        got = ops.pose_search(torch.tensor(y).to(DEV), torch.tensor(ref).to(DEV), None, idx, torch.tensor(start).to(DEV), rows, cols,
                              R.RECOVERY["A"], R.RECOVERY["step"], R.RECOVERY["S"], interp)
        e_angle, e_shift = R.recovery_errors(got.pose.cpu().numpy(), true, rows, cols)
        worst = np.maximum(worst, [e_angle.max(), e_shift.max()])
        assert (got.offset[:, 3] == 0).all()
        want = R.pose_search(y, ref, None, np.zeros(len(y), np.int32), start, rows, cols, R.RECOVERY["A"], R.RECOVERY["step"],
                             R.RECOVERY["S"], interp)
        assert want["margin"].min() > MARGIN and np.array_equal(got.offset.cpu().numpy(), want["offset"])
    print("recovery on the device (%s): %.3f steps, %.3f px" % (interp, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 0.25
