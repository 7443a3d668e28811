"""Multi-reference alignment (include/svae_classify.h: svae_pose_classify; ops.pose_classify) on the MI355X: the candidate
scores bit for bit those of M separate pose searches and within tests/test_gpu_refine.py's bound of the float64 reference
tests/classify_ref.py, the winners, the margins, shape by shape through both memory forms, both ways of sharing the work over
the waves and both interpolations; bit-equality of repeated and of split calls; every refusal of the header with the buffers
prefilled and compared; and the planted-truth case of tests/test_classify_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import classify_ref as CR
import refine_ref as R
from test_gpu_refine import MARGIN, TOL_SCORE

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 5
EMPTY = 2           # the image whose slots are all empty
# (rows, cols, C, A, step, S, M, weighted).  M = 1 and M = 3 share each candidate's shifts over the waves, the others give each
# wave whole candidates (7 and 33 are no multiples of 4).  71 x 72 x 4 with M = 2 keeps 20448 + 2 + 8 doubles, which still fit
# the 20480 of the LDS; 72 x 72 x 4 = 20736 is the smallest box of four channels beside it that does not, and goes through the
# workspace.  9 x 8 with A = 32, S = 8 is the largest search the header takes; A = S = 0 a volume of one entry.
SHAPES = [(24, 24, 1, 3, 0.05, 2, 1, True), (17, 13, 3, 2, 0.08, 3, 3, False), (9, 8, 1, 32, 0.02, 8, 7, False),
          (71, 72, 4, 2, 0.03, 1, 2, True), (72, 72, 4, 2, 0.03, 1, 2, True), (9, 8, 1, 0, 0.1, 0, 33, True)]
WORKSPACE_FORM = {(72, 72, 4)}


def candidates(M):
    """cand (B, M) over n_ref = M + 2 references of which number 2 is all zero: slot j of image b holds (b + j) mod n_ref, so no
    row repeats a reference; image EMPTY has no slot at all.  M = 3 is written out: an empty slot, the all-zero reference, a
    duplicate (of a reference that does not win: a duplicated winner has margin 0, see test_a_duplicated_winner...), and an
    index past the last reference."""
    n_ref = M + 2
    cand = (np.arange(B)[:, None] + np.arange(M)[None, :]) % n_ref
    if M == 3:
        cand = np.array([[0, -1, 1], [1, 2, 0], [0, 0, 0], [1, 1, 3], [4, 1, 9]])
    cand[EMPTY] = -1
    return cand.astype(np.int32), n_ref


@functools.lru_cache(maxsize=None)
def _case(rows, cols, C, A, step, S, M, weighted, interp):
    """The shared, read-only inputs and reference results of one shape, in the style of tests/test_gpu_refine.py's: B = 5 smooth
    random images; reference r is image r mod 5 at a pose near its own plus noise of its own (so every volume has a peak and no
    two references score alike), reference 2 all zero; the mask of elbo.refine_mask or none."""
    from spatial_vae_amd import elbo as E
    import align_ref as AR
    rs = np.random.RandomState(rows * cols + C + A + M)
    cand, n_ref = candidates(M)
    y = rs.normal(size=(B, rows, cols, C))
    y = (y + np.roll(y, 1, 1) + np.roll(y, 1, 2) + np.roll(y, (1, 1), (1, 2))).reshape(B, rows * cols, C).astype(np.float32)
    pose = np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.15, 0.15, (B, 2))], 1).astype(np.float32)
    near = pose.astype(np.float64) + np.concatenate([rs.uniform(-A, A, (B, 1)) * step, rs.uniform(-S, S, (B, 2)) / ((cols - 1) / 2.0)], 1)
    aligned, _ = AR.align_ref(y, near[:, 0], near[:, 1:], rows, cols, interp, dtype=np.float64)
    ref = np.stack([aligned[r % B] for r in range(n_ref)]) + 0.1 * rs.normal(size=(n_ref, rows * cols, C))
    ref[2] = 0.0
    weight = E.refine_mask(rows, cols, S).reshape(-1) if weighted else None
    want = CR.pose_classify(y, ref, weight, cand, pose, rows, cols, A, step, S, interp)
    for x in (y, ref, pose, cand) + tuple(want.values()):
        x.setflags(write=False)
    return {"y": y, "ref": ref, "weight": weight, "pose": pose, "cand": cand, "want": want}


def _dev(a, lo=0, hi=None):
    return None if a is None else torch.tensor(a[lo:hi]).to(DEV)


def _classify(c, rows, cols, A, step, S, interp, lo=0, hi=None, margin=True):
    from spatial_vae_amd import ops
    return ops.pose_classify(_dev(c["y"], lo, hi), _dev(c["ref"]), _dev(c["weight"]), _dev(c["cand"], lo, hi), _dev(c["pose"], lo, hi),
                             rows, cols, A, step, S, interp, return_margin=margin)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
@pytest.mark.parametrize("rows,cols,C,A,step,S,M,weighted", SHAPES)
def test_pose_classify_matches_the_searches_and_the_reference(rows, cols, C, A, step, S, M, weighted, interp):
    """cand_score is, bit for bit, the score of M separate ops.pose_search calls where those are not skipped and -inf where they
    are; within 1e-10 of the reference; choice and ref_chosen equal the reference's (its margin exceeds 1e-9 for every live image
    of every case: asserted, so nothing is left out) and the margin is within 1e-10; the image with no slot has choice -1, an
    infinite margin and -inf scores; a second run and the halves [0, 2) + [2, 5) are bit-equal to the one call; without the margin
    the other outputs are the same bits."""
    from spatial_vae_amd import _lib, ops
    c = _case(rows, cols, C, A, step, S, M, weighted, interp)
    want, cand = c["want"], c["cand"]
    n_ref = c["ref"].shape[0]
    need = _lib.lib().svae_pose_classify_workspace_bytes(B, n_ref, M, rows, cols, C)
    uses_ws = need > 8 * ((n_ref + 31) // 32 * 32)
    assert uses_ws == ((rows, cols, C) in WORKSPACE_FORM)
    got = _classify(c, rows, cols, A, step, S, interp)
    assert got.choice.shape == (B,) and got.choice.dtype == torch.int32 and got.ref_chosen.shape == (B,) and got.ref_chosen.dtype == torch.int32
    assert got.cand_score.shape == (B, M) and got.cand_score.dtype == torch.float64 and got.margin.shape == (B,) and got.margin.dtype == torch.float64
    again = _classify(c, rows, cols, A, step, S, interp)
    first, second = _classify(c, rows, cols, A, step, S, interp, 0, 2), _classify(c, rows, cols, A, step, S, interp, 2, 5)
    bare = _classify(c, rows, cols, A, step, S, interp, margin=False)
    assert bare.margin is None
    for name in ("choice", "ref_chosen", "cand_score", "margin"):
        t = getattr(got, name)
        assert _bits(t, getattr(again, name)), name
        assert _bits(t, torch.cat([getattr(first, name), getattr(second, name)])), name
        if name != "margin":
            assert _bits(t, getattr(bare, name)), name
    # M separate searches
    y, ref, weight, pose = _dev(c["y"]), _dev(c["ref"]), _dev(c["weight"]), _dev(c["pose"])
    columns = []
    for j in range(M):
        one = ops.pose_search(y, ref, weight, _dev(np.ascontiguousarray(cand[:, j])), pose, rows, cols, A, step, S, interp)
        skipped = (one.offset[:, 3] & R.SKIPPED) != 0
        columns.append(torch.where(skipped, torch.full_like(one.score, float("-inf")), one.score))
    assert _bits(got.cand_score, torch.stack(columns, 1))
    choice, ref_chosen, score, margin = (t.cpu().numpy() for t in got)
    live = np.array([b for b in range(B) if b != EMPTY])
    finite = np.isfinite(want["cand_score"])
    assert np.array_equal(np.isneginf(score), ~finite) and finite[live].any(1).all() and not finite[EMPTY].any()
    e_score = float(np.abs(score[finite] - want["cand_score"][finite]).max())
    both = np.isfinite(want["margin"])
    e_margin = float(np.abs(margin[both] - want["margin"][both]).max()) if both.any() else 0.0
    print("%dx%dx%d A=%d S=%d M=%d %s %s: cand_score %.2e, margin %.2e; least reference margin %.1e; choice %s"
          % (rows, cols, C, A, S, M, interp, "workspace" if uses_ws else "LDS", e_score, e_margin, want["margin"][live].min(), choice.tolist()))
    assert want["margin"][live].min() > MARGIN, want["margin"]
    assert e_score <= TOL_SCORE and e_margin <= TOL_SCORE and np.array_equal(np.isinf(margin), ~both) and (margin[~both] > 0).all()
    assert np.array_equal(choice, want["choice"]) and np.array_equal(ref_chosen, want["ref_chosen"])
    assert choice[EMPTY] == -1 and ref_chosen[EMPTY] == -1 and margin[EMPTY] == np.inf and (choice[live] >= 0).all()
    assert np.abs(score[finite]).max() <= 1 + 1e-12
    if M == 3:          # the all-zero reference and the index past the last are -inf; the duplicate has its twin's bits
        assert np.isneginf(score[0, 1]) and np.isneginf(score[1, 1]) and np.isneginf(score[4, 2]) and score[3, 0] == score[3, 1]
        assert choice[3] == 2


def test_a_duplicated_winner_a_nan_image_and_a_non_finite_pose():
    """The same reference in both slots: equal bits, the first wins and the margin is exactly 0.  An image that holds a NaN gives
    NaN scores only and a NaN never enters a maximum: every slot -inf, choice -1; a pose with a NaN or an infinity likewise."""
    from spatial_vae_amd import ops
    c = _case(17, 13, 3, 2, 0.08, 3, 3, False, "bicubic")
    y, pose = _dev(c["y"]), _dev(c["pose"])
    y[4, 7, 1] = float("nan")
    pose[0, 0], pose[1, 2] = float("nan"), float("inf")
    cand = torch.tensor([[0, 1], [1, 3], [3, 3], [1, 1], [0, 1]], dtype=torch.int32, device=DEV)
    got = ops.pose_classify(y, _dev(c["ref"]), None, cand, pose, 17, 13, 2, 0.08, 3)
    assert got.choice.tolist() == [-1, -1, 0, 0, -1] and got.ref_chosen.tolist() == [-1, -1, 3, 1, -1]
    assert torch.isneginf(got.cand_score[[0, 1, 4]]).all() and torch.isfinite(got.cand_score[[2, 3]]).all()
    assert (got.cand_score[2:4, 0] == got.cand_score[2:4, 1]).all() and (got.margin[2:4] == 0).all()
    assert (got.margin[[0, 1, 4]] == float("inf")).all()


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
    B, M, rows, cols, C, A, S = 3, 2, 10, 8, 2, 2, 1
    f64 = dict(dtype=torch.float64, device=DEV)

    def buffers(B, M, rows, cols, C):
        t = {"y": torch.ones(B, rows * cols, C, device=DEV), "ref": torch.ones(2, rows * cols, C, **f64),
             "weight": torch.ones(rows * cols, **f64), "cand": torch.zeros(B, M, dtype=torch.int32, device=DEV),
             "pose_in": torch.zeros(B, 3, device=DEV), "choice": torch.full((B,), 7, dtype=torch.int32, device=DEV),
             "ref_chosen": torch.full((B,), 7, dtype=torch.int32, device=DEV), "cand_score": torch.full((B, M), 7.0, **f64),
             "margin": torch.full((B,), 7.0, **f64)}
        need = L.svae_pose_classify_workspace_bytes(B, 2, M, rows, cols, C)
        t["ws"] = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
        return t, {k: v.data_ptr() for k, v in t.items()}, need

    small, p, need = buffers(B, M, rows, cols, C)
    assert need == 8 * 32
    unset = object()

    def classify(p=p, B=B, n_ref=2, M=M, rows=rows, cols=cols, C=C, A=A, step=0.1, S=S, interp=1, ws=unset, ws_bytes=None, need=need, **ptr):
        q = dict(p, **ptr)
        return L.svae_pose_classify(q["y"], q["ref"], q["weight"], q["cand"], q["pose_in"], B, n_ref, M, rows, cols, C, A, step, S, interp,
                                    q["choice"], q["ref_chosen"], q["cand_score"], q["margin"], q["ws"] if ws is unset else ws,
                                    need if ws_bytes is None else ws_bytes, None)

    inf, nan = float("inf"), float("nan")
    for kw in (dict(B=0), dict(B=-1), dict(n_ref=0), dict(M=0), dict(M=-1), dict(M=4097), dict(rows=1), dict(cols=1), dict(rows=1025),
               dict(cols=1025), dict(C=0), dict(C=5), dict(A=-1), dict(A=33), dict(S=-1), dict(S=9), dict(step=0.0), dict(step=-0.1),
               dict(step=nan), dict(step=inf), dict(interp=2), dict(interp=-1), dict(y=None), dict(ref=None), dict(cand=None),
               dict(pose_in=None), dict(choice=None), dict(ref_chosen=None), dict(cand_score=None),
               dict(B=1 << 20, rows=1024, cols=1024, ws_bytes=1 << 62), dict(n_ref=1 << 20, rows=1024, cols=1024, ws_bytes=1 << 62),
               dict(B=1 << 19, M=4096, rows=2, cols=2, C=1, ws_bytes=1 << 62)):
        _refused(classify(**kw), L)
    for kw in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=need - 1), dict(ws=p["ws"] + 8)):
        _refused(classify(**kw), L, b"workspace")
    big, bp, big_need = buffers(2, M, 72, 72, 4)
    assert big_need == 8 * (32 + 2 * ((72 * 72 * 4 + M + 31) // 32 * 32))
    for kw in (dict(ws=None), dict(ws_bytes=big_need - 1), dict(ws_bytes=8 * 32), dict(ws=bp["ws"] + 8)):
        _refused(classify(p=bp, B=2, rows=72, cols=72, C=4, need=big_need, **kw), L, b"workspace")
    torch.cuda.synchronize()
    for t in (small, big):
        assert (t["choice"] == 7).all() and (t["ref_chosen"] == 7).all() and (t["cand_score"] == 7.0).all() and (t["margin"] == 7.0).all()
        assert (t["ws"] == 7).all() and (t["y"] == 1.0).all() and (t["ref"] == 1.0).all() and (t["pose_in"] == 0.0).all() and (t["cand"] == 0).all()
    # and the calls these were variations of are accepted: a NULL weight, a NULL margin, any step where A == 0
    assert classify(margin=None) == 0
    torch.cuda.synchronize()
    assert (small["margin"] == 7.0).all() and not (small["choice"] == 7).any()
    assert classify() == 0 and classify(weight=None) == 0 and classify(A=0, step=nan) == 0
    assert classify(p=bp, B=2, rows=72, cols=72, C=4, need=big_need) == 0
    torch.cuda.synchronize()
    for t in (small, big):
        assert (t["choice"] == 0).all() and (t["ref_chosen"] == 0).all() and not (t["cand_score"] == 7.0).any() and (t["margin"] == 0.0).all()


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_device_assigns_every_planted_image_to_its_class(interp):
    """tests/test_classify_cpu.py's planted case on the device: twelve images of three analytic classes, every third with a wrong
    starting label; scored against the three canonical images every image goes to its true class, the choices are the
    reference's (its least margin is 6e-3) and elbo.classify_poses refines each pose against the chosen reference exactly as
    ops.pose_search does."""
    from spatial_vae_amd import elbo as E, ops
    y, ref, true, label, start = CR.planted_case()
    p = CR.PLANTED
    cand = np.tile(np.arange(3, dtype=np.int32), (len(y), 1))
    want = CR.pose_classify(y, ref, None, cand, start, p["rows"], p["cols"], p["A"], p["step"], p["S"], interp)
    assert want["margin"].min() > MARGIN and np.array_equal(want["choice"], true)
    yd, rd, sd = _dev(y), _dev(ref), _dev(start)
    picked, found = E.classify_poses(yd, p["rows"], p["cols"], rd, None, _dev(cand), sd, p["A"], p["step"], p["S"], interp)
    choice = picked.choice.cpu().numpy()
    assert np.array_equal(choice, true) and np.array_equal(choice, want["choice"]) and np.array_equal(picked.ref_chosen.cpu().numpy(), true)
    assert (choice != label).sum() == 4 and np.abs(picked.cand_score.cpu().numpy() - want["cand_score"]).max() <= TOL_SCORE
    assert np.abs(picked.margin.cpu().numpy() - want["margin"]).max() <= TOL_SCORE
    alone = ops.pose_search(yd, rd, None, picked.ref_chosen, sd, p["rows"], p["cols"], p["A"], p["step"], p["S"], interp)
    for name in ("pose", "score", "offset"):
        assert _bits(getattr(found, name), getattr(alone, name)), name
    assert _bits(found.score, picked.cand_score.gather(1, picked.choice.long().unsqueeze(1)).squeeze(1))
