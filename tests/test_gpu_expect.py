"""Maximum-likelihood class averages (include/svae_expect.h: svae_pose_expect, svae_expect_sums_update; ops.pose_expect,
ops.ClassSums.update_soft) on the MI355X: posterior, evidence, winner and contribution rows within 1e-10 of the float64
reference tests/expect_ref.py, shape by shape through both memory forms, both interpolations, with and without weight and
prior; bit-equality of repeated and of split calls; the soft sums against the hard ones where the posterior is one entry, and
folded against unfolded; every refusal of the header with the buffers prefilled and compared."""
import functools

import numpy as np
import pytest
import torch

import expect_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-10         # the bound of the sibling kernel tests (tests/test_gpu_refine.py's TOL_SCORE), relative to the array's largest magnitude
SKIPPED = 3         # the fixture image whose row of cand is empty
WORKSPACE_FORM = {(9, 8, 1, 32, 8, 7), (72, 72, 4, 1, 1, 2)}       # by the volume, by the plane


@functools.lru_cache(maxsize=None)
def _case(index, interp, weighted, prior):
    """The shared, read-only inputs and reference results of one configuration."""
    f = X.fixture(index, weighted, prior)
    inv = X.pick_inv_sigma2(f, interp)
    want = X.run(f, inv, interp)
    for a in list(want.values()) + [v for v in f.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return f, inv, want


def _dev(a, lo=0, hi=None):
    return None if a is None else torch.tensor(a[lo:hi]).to(DEV)


def _expect(f, inv, interp, lo=0, hi=None):
    from spatial_vae_amd import ops
    return ops.pose_expect(_dev(f["y"], lo, hi), _dev(f["ref"]), _dev(f["weight"]), _dev(f["log_prior"]), _dev(f["cand"], lo, hi),
                           _dev(f["pose"], lo, hi), f["rows"], f["cols"], f["A"], f["step"], f["S"], inv, interp)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("prior", [True, False], ids=["prior", "noprior"])
@pytest.mark.parametrize("weighted", [True, False], ids=["weight", "noweight"])
@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
@pytest.mark.parametrize("index", range(len(X.SHAPES)), ids=X.SHAPE_IDS)
def test_pose_expect_matches_the_reference(index, interp, weighted, prior):
    """class_post, contrib and cover_w within 1e-10 of the reference relative to the array's largest magnitude, log_evidence
    within 1e-10 max(1, |value|), best equal for EVERY image (tests/test_expect_cpu.py asserts a gap above 1e-9 for each); the
    image with the empty row is skipped, the repeated slot dead; a second run and the halves [0, 2) + [2, 5) are bit-equal to the
    one call.  Measured on an MI355X, the largest of the 40 configurations: class_post 8.7e-15, contrib
    8.2e-15, cover_w 1.0e-14, log_evidence 2.7e-15 (each relative as above)."""
    from spatial_vae_amd import _lib
    f, inv, want = _case(index, interp, weighted, prior)
    B, M, N, C = f["B"], f["M"], f["rows"] * f["cols"], f["C"]
    need = _lib.lib().svae_pose_expect_workspace_bytes(B, f["n_ref"], M, f["rows"], f["cols"], C, f["A"], f["S"])
    uses_ws = need > 8 * ((f["n_ref"] + 31) // 32 * 32)
    assert uses_ws == (X.SHAPES[index] in WORKSPACE_FORM)
    got = _expect(f, inv, interp)
    assert got.contrib.shape == (B, M, N, C) and got.cover_w.shape == (B, M, N) and got.class_post.shape == (B, M)
    assert got.log_evidence.shape == (B,) and got.best.shape == (B, 4) and got.best.dtype == torch.int32
    assert all(t.dtype == torch.float64 for t in got[:4])
    again = _expect(f, inv, interp)
    first, second = _expect(f, inv, interp, 0, 2), _expect(f, inv, interp, 2, 5)
    for name in got._fields:
        t = getattr(got, name)
        assert _bits(t, getattr(again, name)), name
        assert _bits(t, torch.cat([getattr(first, name), getattr(second, name)])), name
    contrib, cover_w, class_post, log_evidence, best = (t.cpu().numpy() for t in got)
    errors = {}
    for name, have in (("class_post", class_post), ("contrib", contrib), ("cover_w", cover_w)):
        errors[name] = float(np.abs(have - want[name]).max() / np.abs(want[name]).max())
    errors["log_evidence"] = float((np.abs(log_evidence - want["log_evidence"]) / np.maximum(1.0, np.abs(want["log_evidence"]))).max())
    print("%s %s w=%d p=%d %s inv_sigma2 %g: " % (X.SHAPE_IDS[index], interp, weighted, prior, "workspace" if uses_ws else "LDS", inv)
          + ", ".join("%s %.2e" % kv for kv in errors.items()) + "; largest posterior %.3f" % class_post.max())
    assert np.array_equal(best, want["best"]), (best, want["best"])
    assert all(e <= TOL for e in errors.values()), errors
    assert best[SKIPPED].tolist() == [-1, 0, 0, 0] and log_evidence[SKIPPED] == 0 and not class_post[SKIPPED].any()
    assert not contrib[SKIPPED].any() and not cover_w[SKIPPED].any()
    live = [b for b in range(B) if b != SKIPPED]
    assert (best[live, 0] >= 0).all() and np.abs(class_post[live].sum(1) - 1).max() <= 1e-12
    if M > 1:
        assert class_post[1, M - 1] == 0 and not contrib[1, M - 1].any() and not cover_w[1, M - 1].any()
    if M > 2:
        assert class_post[0, 1] == 0 and not contrib[0, 1].any()


def test_a_nan_image_a_non_finite_pose_and_a_dead_prior():
    """NaN inputs are data: an image that holds a NaN has a non-finite L and is skipped, a pose with a NaN or an infinity
    likewise; a reference whose prior is -inf is a dead slot: zero posterior and zero rows, the others as without it."""
    from spatial_vae_amd import ops
    f, inv, _ = _case(1, "bicubic", False, True)
    y, pose, prior = _dev(f["y"]), _dev(f["pose"]), _dev(f["log_prior"])
    y[4, 7, 1] = float("nan")
    pose[0, 0], pose[1, 2] = float("nan"), float("inf")
    cand = torch.tensor([[0, 1, 2], [1, 3, 2], [3, 0, 1], [1, 1, 4], [0, 1, 2]], dtype=torch.int32, device=DEV)
    prior[0] = float("-inf")
    got = ops.pose_expect(y, _dev(f["ref"]), None, prior, cand, pose, 17, 13, 2, f["step"], 3, inv)
    for b in (0, 1, 4):
        assert got.best[b].tolist() == [-1, 0, 0, 0] and got.log_evidence[b] == 0 and not got.class_post[b].any()
        assert not got.contrib[b].any() and not got.cover_w[b].any()
    assert got.class_post[2, 1] == 0 and not got.contrib[2, 1].any() and got.class_post[2, 0] > 0 and got.class_post[2, 2] > 0
    assert got.class_post[3, 1] == 0 and not got.contrib[3, 1].any() and abs(got.class_post[3].sum().item() - 1) <= 1e-12
    want = X.pose_expect(f["y"][2:4], f["ref"], None, prior.cpu().numpy(), cand[2:4].cpu().numpy(), f["pose"][2:4], 17, 13, 2, f["step"], 3, inv)
    assert np.abs(got.class_post[2:4].cpu().numpy() - want["class_post"]).max() <= TOL
    assert np.array_equal(got.best[2:4].cpu().numpy(), want["best"])


@pytest.mark.parametrize("interp", ["bicubic", "bilinear"])
def test_soft_sums_with_one_entry_are_the_hard_sums(interp):
    """M = 1, A = S = 0 on labels: the posterior is the one entry, contrib is the aligned image in double and cover_w its
    coverage, so update_soft gives ClassSums.update's sums of the float-rounded aligned images within 1e-6 relative and its
    count exactly; the unlabelled image adds nothing to either."""
    from spatial_vae_amd import ops
    f, _, _ = _case(1, interp, False, False)
    rows, cols, C, B = f["rows"], f["cols"], f["C"], f["B"]
    label = torch.tensor([2, 0, 1, -1, 2], dtype=torch.int32, device=DEV)
    y, pose, ref = _dev(f["y"]), _dev(f["pose"]), _dev(f["ref"])
    spread = ops.pose_expect(y, ref, None, None, label.view(B, 1).contiguous(), pose, rows, cols, 0, 0.0, 0, 0.7, interp)
    assert (spread.class_post[[0, 1, 2, 4]] == 1).all() and spread.class_post[3, 0] == 0
    soft = ops.ClassSums(3, rows * cols, C, DEV)
    soft.update_soft(spread, label.view(B, 1).contiguous())
    aligned, cover = ops.align_images(y, pose[:, 0].contiguous(), pose[:, 1:].contiguous(), rows, cols, interp)
    hard = ops.ClassSums(3, rows * cols, C, DEV)
    hard.update(aligned, cover, label)
    assert torch.equal(soft.count, hard.count) and 0 < hard.count.sum() < 4 * rows * cols
    err = ((soft.sum - hard.sum).abs().max() / hard.sum.abs().max()).item()
    print("soft against hard sums (%s): %.2e relative" % (interp, err))
    assert err <= 1e-6
    soft.update_soft(spread, label.view(B, 1).contiguous())             # accumulates: a second update doubles both
    assert torch.equal(soft.count, 2 * hard.count)


def test_folded_sums_are_the_sum_of_the_halves_and_match_the_reference():
    """target folding 2K -> K equals the sum of the two identity halves within 1e-12 relative; both equal the reference's walk
    (images upwards, slots upwards) within 1e-12 relative; two runs are bit-equal; a target outside the classes is skipped."""
    from spatial_vae_amd import ops
    f, inv, want = _case(1, "bicubic", True, True)
    N, C, n_ref = f["rows"] * f["cols"], f["C"], f["n_ref"]
    assert n_ref == 5
    spread = _expect(f, inv, "bicubic")
    cand = _dev(f["cand"])
    target = torch.tensor([0, 0, 1, 1, 7], dtype=torch.int32, device=DEV)
    halves, full, again = ops.ClassSums(6, N, C, DEV), ops.ClassSums(3, N, C, DEV), ops.ClassSums(3, N, C, DEV)
    halves.update_soft(spread, cand)
    full.update_soft(spread, cand, target)
    again.update_soft(spread, cand, target)
    assert _bits(full.sum, again.sum) and _bits(full.count, again.count)
    pairs = halves.sum.view(3, 2, N, C).sum(1), halves.count.view(3, 2, N).sum(1)
    pairs[0][2], pairs[1][2] = 0, 0                                     # reference 4 maps to class 7: skipped; class 2 stays empty
    assert not full.sum[2].any() and not full.count[2].any() and halves.sum[4].any()
    for a, b in ((full.sum, pairs[0]), (full.count, pairs[1])):
        assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-12
    ref_sum, ref_count = X.sums_update(np.zeros((3, N, C)), np.zeros((3, N)), want["contrib"], want["cover_w"], f["cand"],
                                       target.cpu().numpy(), n_ref)
    assert np.abs(full.sum.cpu().numpy() - ref_sum).max() <= TOL * np.abs(ref_sum).max()
    assert np.abs(full.count.cpu().numpy() - ref_count).max() <= TOL * np.abs(ref_count).max()


def _refused(rc, L, word=None):
    from spatial_vae_amd import _lib
    message = L.svae_last_error()
    assert rc == _lib.E_INVALID and message, (rc, message)
    if word is not None:
        assert word in message, message


def test_every_refusal_leaves_the_buffers_untouched():
    """Each SVAE_E_INVALID case of the header, through the raw entry points: the code, a message (naming the workspace where that
    is the reason), and every output still what it was prefilled with; the calls these were variations of are accepted."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    B, M, rows, cols, C, A, S = 3, 2, 10, 8, 2, 2, 1
    f64 = dict(dtype=torch.float64, device=DEV)
    outputs = ("contrib", "cover_w", "class_post", "log_evidence")

    def buffers(B, M, rows, cols, C, A, S):
        N = rows * cols
        t = {"y": torch.ones(B, N, C, device=DEV), "ref": torch.ones(2, N, C, **f64), "weight": torch.ones(N, **f64),
             "log_prior": torch.zeros(2, **f64), "cand": torch.zeros(B, M, dtype=torch.int32, device=DEV),
             "pose_in": torch.zeros(B, 3, device=DEV), "contrib": torch.full((B, M, N, C), 7.0, **f64),
             "cover_w": torch.full((B, M, N), 7.0, **f64), "class_post": torch.full((B, M), 7.0, **f64),
             "log_evidence": torch.full((B,), 7.0, **f64), "best": torch.full((B, 4), 7, dtype=torch.int32, device=DEV)}
        need = L.svae_pose_expect_workspace_bytes(B, 2, M, rows, cols, C, A, S)
        t["ws"] = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
        return t, {k: v.data_ptr() for k, v in t.items()}, need

    small, p, need = buffers(B, M, rows, cols, C, A, S)
    assert need == 8 * 32
    unset = object()

    def expect(p=p, B=B, n_ref=2, M=M, rows=rows, cols=cols, C=C, A=A, step=0.1, S=S, interp=1, inv_sigma2=0.5, ws=unset,
               ws_bytes=None, need=need, **ptr):
        q = dict(p, **ptr)
        return L.svae_pose_expect(q["y"], q["ref"], q["weight"], q["log_prior"], q["cand"], q["pose_in"], B, n_ref, M, rows, cols, C, A,
                                  step, S, interp, inv_sigma2, q["contrib"], q["cover_w"], q["class_post"], q["log_evidence"], q["best"],
                                  q["ws"] if ws is unset else ws, need if ws_bytes is None else ws_bytes, None)

    inf, nan = float("inf"), float("nan")
    for kw in (dict(B=0), dict(B=-1), dict(n_ref=0), dict(M=0), dict(M=-1), dict(M=65), dict(rows=1), dict(cols=1), dict(rows=1025),
               dict(cols=1025), dict(C=0), dict(C=5), dict(A=-1), dict(A=33), dict(S=-1), dict(S=9), dict(step=0.0), dict(step=-0.1),
               dict(step=nan), dict(step=inf), dict(interp=2), dict(interp=-1), dict(inv_sigma2=-1e-300), dict(inv_sigma2=inf),
               dict(inv_sigma2=nan), dict(y=None), dict(ref=None), dict(cand=None), dict(pose_in=None), dict(contrib=None),
               dict(cover_w=None), dict(class_post=None), dict(log_evidence=None), dict(best=None),
               dict(B=1 << 20, rows=1024, cols=1024, ws_bytes=1 << 62), dict(n_ref=1 << 20, rows=1024, cols=1024, ws_bytes=1 << 62),
               dict(B=1 << 10, M=64, rows=256, cols=256, C=1, ws_bytes=1 << 62)):
        _refused(expect(**kw), L)
    for kw in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=need - 1), dict(ws=p["ws"] + 8)):
        _refused(expect(**kw), L, b"workspace")
    big, bp, big_need = buffers(2, M, 72, 72, 4, 1, 1)
    assert big_need == 8 * (32 + 2 * ((72 * 72 * 5 + M * 27 + 31) // 32 * 32))
    for kw in (dict(ws=None), dict(ws_bytes=big_need - 1), dict(ws_bytes=8 * 32), dict(ws=bp["ws"] + 8)):
        _refused(expect(p=bp, B=2, rows=72, cols=72, C=4, A=1, S=1, need=big_need, **kw), L, b"workspace")
    torch.cuda.synchronize()
    for t in (small, big):
        assert all((t[k] == 7.0).all() for k in outputs) and (t["best"] == 7).all() and (t["ws"] == 7).all()
        assert (t["y"] == 1.0).all() and (t["ref"] == 1.0).all() and (t["pose_in"] == 0.0).all() and (t["cand"] == 0).all()
    # the soft sums
    total, count = torch.full((3, rows * cols, C), 7.0, **f64), torch.full((3, rows * cols), 7.0, **f64)
    target = torch.zeros(2, dtype=torch.int32, device=DEV)

    def update(B=B, M=M, N=rows * cols, C=C, n_ref=2, n_classes=3, **ptr):
        q = dict(dict(p, target=target.data_ptr(), sum=total.data_ptr(), count=count.data_ptr()), **ptr)
        return L.svae_expect_sums_update(q["contrib"], q["cover_w"], q["cand"], q["target"], B, M, N, C, n_ref, n_classes, q["sum"],
                                         q["count"], None)

    for kw in (dict(B=0), dict(M=0), dict(M=65), dict(N=0), dict(C=0), dict(C=5), dict(n_ref=0), dict(n_classes=0), dict(n_classes=4097),
               dict(B=1 << 20, N=1 << 20), dict(n_classes=4096, N=1 << 20), dict(B=1 << 10, M=64, N=1 << 16, C=1), dict(contrib=None),
               dict(cover_w=None), dict(cand=None), dict(sum=None), dict(count=None)):
        _refused(update(**kw), L)
    torch.cuda.synchronize()
    assert (total == 7.0).all() and (count == 7.0).all() and (small["contrib"] == 7.0).all()
    # and the calls these were variations of are accepted: a NULL weight, a NULL prior, any step where A == 0, inv_sigma2 = 0
    assert expect() == 0 and expect(weight=None) == 0 and expect(log_prior=None) == 0 and expect(A=0, step=nan) == 0
    assert expect(inv_sigma2=0.0) == 0
    assert expect(p=bp, B=2, rows=72, cols=72, C=4, A=1, S=1, need=big_need) == 0
    torch.cuda.synchronize()
    for t in (small, big):                      # slot 1 repeats slot 0: dead; slot 0 holds the whole posterior
        assert ((t["class_post"][:, 0] - 1).abs() <= 1e-12).all() and (t["class_post"][:, 1] == 0).all() and (t["best"][:, 0] == 0).all()
        assert not (t["contrib"] == 7.0).any() and not (t["cover_w"] == 7.0).any() and not (t["log_evidence"] == 7.0).any()
    assert update() == 0 and update(target=None) == 0
    torch.cuda.synchronize()
    assert not (total[0] == 7.0).all() and (total[1:] == 7.0).all() and (count[1:] == 7.0).all()
