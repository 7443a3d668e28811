"""The rows of tests/stream_cases.py's table for the analysis headers (include/svae_cluster.h, _frc.h, _refine.h, _classify.h,
_gmm.h, _expect.h, _pca.h, _eigen.h, _neighbours.h): one row per header (two for the eigenimage chain), at the smallest shapes
that exercise the three-chunk tail (N = 600), the odd-by-odd plane and the LDS form, and for the last two headers at the shapes
of their own GPU tests.  stream_cases.make_cases() appends analysis_cases(); import stream_cases, not this file.

Every check here takes the seed: the baselines of BOTH input sets are held to the header's float64 reference."""
import functools

import numpy as np

import classify_ref as CR
import eigen_ref as ER
import expect_ref as X
import frc_ref as F
import gmm_ref as G
import kmeans_ref as K
import neighbours_ref as NR
import pca_ref as PR
import refine_ref as R
import stream_cases as S
from spatial_vae_amd import _lib

GMM_REG, GMM_TOL = 1e-6, 1e-12
INV_SIGMA2 = 1.5


def _workspace(case):
    ws = case.scratch.get("ws")
    return (ws.ptr, ws.nbytes) if ws else (None, 0)


class KMeansCase(S.Case):
    """Seed, two update steps, one assign-only step.  N = 600 (three chunks, the last of 88 points), D = 3, k = 4.  The record
    is the calls' to advance: state, and zero in both sets."""
    name, entry_points, has_reference = "kmeans_N600_D3_k4", ("svae_kmeans_seed", "svae_kmeans_step"), True
    state, same_in_both_sets, must_differ = ("rec",), ("rec",), ("centres",)
    N, D, k = 600, 3, 4

    def inputs(self, seed):
        x, u = K.blobs(40 + seed, self.N, self.D, self.k)
        return {"x": x, "u": u, "rec": np.zeros(6, np.int64)}

    def _outputs(self):
        return {"centres": ((self.k, self.D), np.float64), "label": ((self.N,), np.int32), "members": ((self.k,), np.int64),
                "seed_index": ((self.k,), np.int32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_kmeans_workspace_bytes(self.N, self.D, self.k)}

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        seed = lambda st: self.L.svae_kmeans_seed(p("x"), self.N, self.D, self.k, p("u"), p("centres"), p("seed_index"), ws.ptr, ws.nbytes, st)
        step = lambda update: (lambda st: self.L.svae_kmeans_step(p("x"), self.N, self.D, self.k, update, p("centres"), p("label"),
                                                                  p("members"), p("rec"), ws.ptr, ws.nbytes, st))
        return [seed, step(1), step(1), step(0)]

    def check(self, out, seed=0):
        """Bit for bit tests/kmeans_ref.py, record included."""
        i = self.inputs(seed)
        want = K.fit(i["x"], self.k, i["u"], 2)
        assert np.array_equal(out["label"], want["label"]) and np.array_equal(out["members"], want["members"])
        assert np.array_equal(out["seed_index"], want["seed_index"])
        assert np.array_equal(out["centres"].view(np.uint64), want["centres"].view(np.uint64))
        rec = out["rec"]
        assert rec[:5].tolist() == [2, want["changed"], want["converged_at"], self.N, want["empty"]]
        assert rec[5:].view(np.float64)[0] == want["inertia"]


class FrcCase(S.Case):
    """svae_frc, then svae_frc_filter of the first half with weights the case holds.  13 x 10 (odd by even, oblong; LDS form, so
    there is no workspace), 3 planes, the default mask (2, 3)."""
    name, entry_points, has_reference = "frc_13x10_P3", ("svae_frc", "svae_frc_filter"), True
    must_differ = ("frc",)
    n, m, P = 13, 10, 3
    R = 6

    def inputs(self, seed):
        a, b = F.half_planes(70 + seed, self.n, self.m, self.P)
        rs = np.random.RandomState(700 + seed)
        return {"a": a.copy(), "b": b.copy(), "weight": rs.uniform(0.0, 1.0, size=(self.P, self.R))}

    def _outputs(self):
        return {"sums": ((self.P, self.R, 3), np.float64), "frc": ((self.P, self.R), np.float64), "ring_count": ((self.R,), np.int32),
                "filtered": ((self.P, self.n, self.m), np.float32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_frc_workspace_bytes(self.P, self.n, self.m)}

    def steps(self):
        p, (ws, ws_bytes) = self.ptr, _workspace(self)
        radius, edge = F.default_mask(self.n, self.m)
        return [lambda st: self.L.svae_frc(p("a"), p("b"), self.P, self.n, self.m, radius, edge, p("sums"), p("frc"), p("ring_count"),
                                           ws, ws_bytes, st),
                lambda st: self.L.svae_frc_filter(p("a"), p("weight"), self.P, self.n, self.m, p("filtered"), ws, ws_bytes, st)]

    def check(self, out, seed=0):
        """tests/frc_ref.py within tests/test_gpu_frc.py's bounds.  ring_count equals frc_ref.ring_count(n, m), which no input
        enters: held on both sets, it is the same in both."""
        from test_gpu_frc import TOL_FILTER, TOL_FRC, TOL_SUMS
        i = self.inputs(seed)
        sums, curve, counts = F.frc(i["a"], i["b"], self.n, self.m, *F.default_mask(self.n, self.m))
        assert np.array_equal(out["ring_count"], counts)
        scale = sums[..., 1:].reshape(self.P, -1).max(1)
        assert (np.abs(out["sums"] - sums).reshape(self.P, -1).max(1) / scale).max() <= TOL_SUMS
        assert np.abs(out["frc"] - curve).max() <= TOL_FRC
        want = F.filter_planes(i["a"], i["weight"], self.n, self.m)
        err = np.abs(out["filtered"] - want).reshape(self.P, -1).max(1) / np.abs(want).reshape(self.P, -1).max(1)
        assert err.max() <= TOL_FILTER


def _posed_images(rs, B, rows, cols, C):
    """(y, pose_in) of the two pose-search rows: images whose neighbouring pixels correlate, poses within the search's reach."""
    y = rs.normal(size=(B, rows, cols, C))
    y = (y + np.roll(y, 1, 1) + np.roll(y, 1, 2)).reshape(B, rows * cols, C).astype(np.float32)
    return y, np.concatenate([rs.uniform(-3, 3, (B, 1)), rs.uniform(-0.1, 0.1, (B, 2))], 1).astype(np.float32)


class RefineCase(S.Case):
    """17 x 13 x 2 (odd by odd, oblong; LDS form, so there is no workspace), 4 images of which one is in no class, two
    references, a weight, A = 2, S = 1, bicubic."""
    name, entry_points, has_reference = "pose_search_17x13x2_B4", ("svae_pose_search",), True
    same_in_both_sets, must_differ = ("weight", "ref_index"), ("scores",)
    rows, cols, C, B, n_ref, A, step, Sh = 17, 13, 2, 4, 2, 2, 0.06, 1

    def inputs(self, seed):
        from spatial_vae_amd import elbo as E
        rs = np.random.RandomState(900 + seed)
        y, pose = _posed_images(rs, self.B, self.rows, self.cols, self.C)
        return {"y": y, "ref": rs.normal(size=(self.n_ref, self.rows * self.cols, self.C)),
                "weight": E.refine_mask(self.rows, self.cols, self.Sh).reshape(-1), "ref_index": np.array([0, 1, -1, 1], np.int32),
                "pose_in": pose}

    def _outputs(self):
        nA, nS = 2 * self.A + 1, 2 * self.Sh + 1
        return {"pose_out": ((self.B, 3), np.float32), "score": ((self.B,), np.float64), "offset": ((self.B, 4), np.int32),
                "scores": ((self.B, nA, nS, nS), np.float64)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_pose_search_workspace_bytes(self.B, self.rows, self.cols, self.C, self.A, self.Sh)}

    def steps(self):
        p, (ws, ws_bytes) = self.ptr, _workspace(self)
        return [lambda st: self.L.svae_pose_search(p("y"), p("ref"), p("weight"), p("ref_index"), p("pose_in"), self.B, self.n_ref,
                                                   self.rows, self.cols, self.C, self.A, self.step, self.Sh, 1, p("pose_out"),
                                                   p("score"), p("offset"), p("scores"), ws, ws_bytes, st)]

    def check(self, out, seed=0):
        """tests/refine_ref.py within tests/test_gpu_refine.py's bounds."""
        from test_gpu_refine import MARGIN, TOL_POSE, TOL_SCORE
        i = self.inputs(seed)
        want = R.pose_search(i["y"], i["ref"], i["weight"], i["ref_index"], i["pose_in"], self.rows, self.cols, self.A, self.step,
                             self.Sh, "bicubic")
        assert want["margin"][[0, 1, 3]].min() > MARGIN
        assert np.abs(out["scores"] - want["scores"]).max() <= TOL_SCORE and np.abs(out["score"] - want["score"]).max() <= TOL_SCORE
        assert np.array_equal(out["offset"], want["offset"]) and out["offset"][2].tolist() == [0, 0, 0, R.SKIPPED]
        assert np.abs(out["pose_out"].astype(np.float64) - want["pose"].astype(np.float64)).max() <= TOL_POSE


class ClassifyCase(S.Case):
    """Both launches of the call, the norms and the search.  17 x 13 x 2 (odd by odd, oblong; LDS form, the workspace holding
    the norms alone), 4 images of which one has no slot, five slots over six references (one all zero, one slot empty), a
    weight, A = 2, S = 1, bicubic."""
    name, entry_points, has_reference = "pose_classify_17x13x2_B4_M5", ("svae_pose_classify",), True
    same_in_both_sets, must_differ = ("weight", "cand"), ("cand_score",)
    rows, cols, C, B, M, n_ref, A, step, Sh = 17, 13, 2, 4, 5, 6, 2, 0.06, 1

    def inputs(self, seed):
        from spatial_vae_amd import elbo as E
        rs = np.random.RandomState(950 + seed)
        y, pose = _posed_images(rs, self.B, self.rows, self.cols, self.C)
        ref = rs.normal(size=(self.n_ref, self.rows * self.cols, self.C))
        ref[3] = 0.0
        cand = np.array([[0, 1, 2, 3, 4], [5, -1, 0, 1, 2], [-1, -1, -1, -1, -1], [4, 3, 5, 1, 0]], np.int32)
        return {"y": y, "ref": ref, "weight": E.refine_mask(self.rows, self.cols, self.Sh).reshape(-1), "cand": cand, "pose_in": pose}

    def _outputs(self):
        return {"choice": ((self.B,), np.int32), "ref_chosen": ((self.B,), np.int32), "cand_score": ((self.B, self.M), np.float64),
                "margin": ((self.B,), np.float64)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_pose_classify_workspace_bytes(self.B, self.n_ref, self.M, self.rows, self.cols, self.C)}

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        return [lambda st: self.L.svae_pose_classify(p("y"), p("ref"), p("weight"), p("cand"), p("pose_in"), self.B, self.n_ref, self.M,
                                                     self.rows, self.cols, self.C, self.A, self.step, self.Sh, 1, p("choice"),
                                                     p("ref_chosen"), p("cand_score"), p("margin"), ws.ptr, ws.nbytes, st)]

    def check(self, out, seed=0):
        """tests/classify_ref.py within tests/test_gpu_refine.py's bounds."""
        from test_gpu_refine import MARGIN, TOL_SCORE
        i = self.inputs(seed)
        want = CR.pose_classify(i["y"], i["ref"], i["weight"], i["cand"], i["pose_in"], self.rows, self.cols, self.A, self.step,
                                self.Sh, "bicubic")
        assert want["margin"][[0, 1, 3]].min() > MARGIN and want["choice"][2] == -1
        finite = np.isfinite(want["cand_score"])
        assert np.array_equal(np.isneginf(out["cand_score"]), ~finite)
        assert np.abs(out["cand_score"][finite] - want["cand_score"][finite]).max() <= TOL_SCORE
        assert np.array_equal(out["choice"], want["choice"]) and np.array_equal(out["ref_chosen"], want["ref_chosen"])
        assert out["margin"][2] == np.inf and np.abs(out["margin"][[0, 1, 3]] - want["margin"][[0, 1, 3]]).max() <= TOL_SCORE


@functools.lru_cache(maxsize=None)
def _gmm_inputs(seed, N, D, k):
    """Overlapping blobs (planted centres randn * 0.6, noise 0.35), so that EM is still moving after a handful of steps, and
    their k-means start: three steps of kmeans_ref.fit.  Shared: treat as read-only."""
    rs = np.random.RandomState(60 + seed)
    planted = rs.randn(k, D) * 0.6
    x = (planted[rs.randint(0, k, size=N)] + 0.35 * rs.randn(N, D)).astype(np.float32)
    km = K.fit(x, k, rs.rand(k), 3)
    return x, km["label"].astype(np.int32), km["centres"]


class GmmCase(S.Case):
    """Init, two update steps, one labelling step.  N = 600 (three chunks, the last of 88 points), D = 3, k = 4.  The record is
    the calls' to advance (zero in both sets), and `mean` arrives holding the k-means centres and leaves holding the mixture's
    means: both are state."""
    name, entry_points, has_reference = "gmm_N600_D3_k4", ("svae_gmm_init", "svae_gmm_step"), True
    state, same_in_both_sets, must_differ = ("rec", "mean"), ("rec",), ("mean",)
    N, D, k = 600, 3, 4

    def inputs(self, seed):
        x, label_in, centres = _gmm_inputs(seed, self.N, self.D, self.k)
        return {"x": x, "label_in": label_in, "mean": centres.copy(), "rec": np.zeros(6, np.int64)}

    def _outputs(self):
        return {"weight": ((self.k,), np.float64), "var": ((self.k, self.D), np.float64), "resp": ((self.N, self.k), np.float64),
                "label": ((self.N,), np.int32), "loglik_point": ((self.N,), np.float64)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_gmm_workspace_bytes(self.N, self.D, self.k)}

    def step(self, update):
        p, ws = self.ptr, self.scratch["ws"]
        return lambda st: self.L.svae_gmm_step(p("x"), self.N, self.D, self.k, update, GMM_REG, GMM_TOL, p("weight"), p("mean"), p("var"),
                                               p("resp"), p("label"), p("loglik_point"), p("rec"), ws.ptr, ws.nbytes, st)

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        init = lambda st: self.L.svae_gmm_init(p("x"), self.N, self.D, self.k, p("label_in"), GMM_REG, p("weight"), p("mean"), p("var"),
                                               p("resp"), p("rec"), ws.ptr, ws.nbytes, st)
        return [init, self.step(1), self.step(1), self.step(0)]

    def check(self, out, seed=0, iters=2):
        """tests/gmm_ref.py to 1e-10 of the largest entry, the labels and the record's counts exactly."""
        i = self.inputs(seed)
        want = G.fit(i["x"], i["label_in"], i["mean"], iters, GMM_REG, GMM_TOL)
        assert want["iterations"] == iters and want["converged_at"] == 0        # still moving: a further step would advance it
        assert np.array_equal(out["label"], want["label"])
        for key in ("weight", "mean", "var", "resp", "loglik_point"):
            assert np.abs(out[key] - want[key]).max() <= 1e-10 * max(1.0, np.abs(want[key]).max()), key
        rec = out["rec"]
        assert rec[:4].tolist() == [iters, 0, self.N, 0]
        loglik, previous = rec[4:].view(np.float64)
        assert abs(loglik - want["loglik"]) <= 1e-10 * abs(want["loglik"]) and abs(previous - want["previous"]) <= 1e-10 * abs(want["previous"])


_expect_fixture = functools.lru_cache(maxsize=None)(lambda: X.fixture(1, True, True))


class ExpectCase(S.Case):
    """svae_pose_expect, then svae_expect_sums_update on what it wrote.  tests/expect_ref.py's second shape (17 x 13 x 3, A = 2,
    S = 3, M = 3: five references) with weight and prior; the soft sums fold the five references into three classes on top of
    start values.  Set B is set A's images in reverse order with other start values: other numbers of equal shapes."""
    name, entry_points, has_reference = "expect_17x13x3_M3_sums", ("svae_pose_expect", "svae_expect_sums_update"), True
    state, same_in_both_sets, must_differ = ("sum", "count"), ("ref", "weight", "log_prior", "target"), ("sum", "class_post")
    n_classes = 3
    f = property(lambda self: _expect_fixture())            # shared and built on first use: treat as read-only
    n_ref = property(lambda self: self.f["n_ref"])

    def inputs(self, seed):
        f = self.f
        rs = np.random.RandomState(7 + seed)
        order = slice(None, None, -1) if seed else slice(None)
        N = f["rows"] * f["cols"]
        return {"y": f["y"][order].copy(), "ref": f["ref"], "weight": f["weight"], "log_prior": f["log_prior"],
                "cand": f["cand"][order].copy(), "pose": f["pose"][order].copy(), "target": np.array([0, 1, 2, 2, 5], np.int32),
                "sum": rs.normal(size=(self.n_classes, N, f["C"])), "count": np.floor(rs.uniform(0, 5, size=(self.n_classes, N)))}

    def _outputs(self):
        f = self.f
        B, M, N = f["B"], f["M"], f["rows"] * f["cols"]
        return {"contrib": ((B, M, N, f["C"]), np.float64), "cover_w": ((B, M, N), np.float64), "class_post": ((B, M), np.float64),
                "log_evidence": ((B,), np.float64), "best": ((B, 4), np.int32)}

    def _scratch_bytes(self):
        f = self.f
        return {"ws": _lib.lib().svae_pose_expect_workspace_bytes(f["B"], f["n_ref"], f["M"], f["rows"], f["cols"], f["C"], f["A"], f["S"])}

    def steps(self):
        p, f, ws = self.ptr, self.f, self.scratch["ws"]
        N = f["rows"] * f["cols"]
        return [lambda st: self.L.svae_pose_expect(p("y"), p("ref"), p("weight"), p("log_prior"), p("cand"), p("pose"), f["B"], f["n_ref"],
                                                   f["M"], f["rows"], f["cols"], f["C"], f["A"], float(f["step"]), f["S"],
                                                   _lib.ALIGN_INTERP["bicubic"], INV_SIGMA2, p("contrib"), p("cover_w"), p("class_post"),
                                                   p("log_evidence"), p("best"), ws.ptr, ws.nbytes, st),
                lambda st: self.L.svae_expect_sums_update(p("contrib"), p("cover_w"), p("cand"), p("target"), f["B"], f["M"], N, f["C"],
                                                          f["n_ref"], self.n_classes, p("sum"), p("count"), st)]

    def check(self, out, seed=0):
        """tests/test_gpu_expect.py's bounds against expect_ref; the sums against its walk added to the start values."""
        i, f = self.inputs(seed), self.f
        want = X.pose_expect(i["y"], i["ref"], i["weight"], i["log_prior"], i["cand"], i["pose"], f["rows"], f["cols"], f["A"], f["step"],
                             f["S"], INV_SIGMA2)
        assert want["gap"].min() > 1e-9 and np.array_equal(out["best"], want["best"])
        for k in ("contrib", "cover_w", "class_post"):
            assert np.abs(out[k] - want[k]).max() <= 1e-10 * np.abs(want[k]).max(), k
        assert (np.abs(out["log_evidence"] - want["log_evidence"]) <= 1e-10 * np.maximum(1.0, np.abs(want["log_evidence"]))).all()
        s, c = X.sums_update(i["sum"].copy(), i["count"].copy(), want["contrib"], want["cover_w"], i["cand"], i["target"], f["n_ref"])
        assert np.abs(out["sum"] - s).max() <= 1e-10 * np.abs(s).max() and np.abs(out["count"] - c).max() <= 1e-10 * np.abs(c).max()
        assert not np.array_equal(out["sum"], i["sum"])


_pca_inputs = functools.lru_cache(maxsize=None)(PR.labelled)     # shared: treat as read-only


class PcaCase(S.Case):
    """Moments, eigen, project: a single chain on one stream, so the captured graph has no parallel branches.  N = 600 (three
    chunks, the last of 88 points), D = 3, G = 4: two live groups, one of a single member, one empty; labels outside [0, G) and
    two non-finite rows.  P = 2 of the 3 components are projected."""
    name, entry_points, has_reference = "pca_N600_D3_G4", ("svae_pca_moments", "svae_pca_eigen", "svae_pca_project"), True
    must_differ, non_finite_inputs = ("mean",), ("x",)
    N, D, G, P = 600, 3, 4, 2

    def inputs(self, seed):
        x, group = _pca_inputs(60 + seed, self.N, self.D, self.G)
        return {"x": x, "group": group}

    def _outputs(self):
        G, D = self.G, self.D
        return {"count": ((G,), np.int64), "mean": ((G, D), np.float64), "cov": ((G, D, D), np.float64),
                "eigenvalues": ((G, D), np.float64), "components": ((G, D, D), np.float64), "sweeps": ((G,), np.int32),
                "off_norm": ((G,), np.float64), "proj": ((self.N, self.P), np.float64)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_pca_workspace_bytes(self.N, self.D, self.G)}

    def steps(self):
        p, ws, L = self.ptr, self.scratch["ws"], self.L
        N, D, G, P = self.N, self.D, self.G, self.P
        return [lambda st: L.svae_pca_moments(p("x"), N, D, G, p("group"), p("count"), p("mean"), p("cov"), ws.ptr, ws.nbytes, st),
                lambda st: L.svae_pca_eigen(p("cov"), D, G, p("eigenvalues"), p("components"), p("sweeps"), p("off_norm"), st),
                lambda st: L.svae_pca_project(p("x"), N, D, G, P, p("group"), p("count"), p("mean"), p("components"), p("proj"), st)]

    def check(self, out, seed=0):
        """tests/pca_ref.py to 1e-10 of the largest entry, the counts and sweeps exactly."""
        i = self.inputs(seed)
        want = PR.fit(i["x"], i["group"], self.G, self.P)
        assert np.array_equal(out["count"], want["count"]) and np.array_equal(out["sweeps"], want["sweeps"])
        assert sorted(want["count"].tolist())[:2] == [0, 1] and (want["sweeps"] > 0).sum() == 2
        for key in ("mean", "cov", "eigenvalues", "components", "off_norm", "proj"):
            assert np.abs(out[key] - want[key]).max() <= 1e-10 * max(1.0, np.abs(want[key]).max()), key


@functools.lru_cache(maxsize=None)
def _eigen_inputs(case):
    """The inputs of one chain of tests/test_gpu_eigen.py, built as its reference() builds them.  Shared: treat as read-only."""
    seed, B, rows, cols, C, K, Rc, P, covered = case
    aligned, cover, label = ER.images(seed, B, rows, cols, C, K, covered)
    label64, D = label.astype(np.int64), rows * cols * C
    return {"aligned": aligned, "cover": cover, "class_of": label, "mean": ER.class_moments(aligned, cover, label64, K)[0].reshape(K, D),
            "members": np.array([(label64 == k).sum() for k in range(K)], np.int64), "start": ER.start_array(seed + 100, K, D, Rc),
            "Y": np.zeros((K, D, Rc)), "ssq": np.zeros((K, D))}


class EigenCase(S.Case):
    """The whole chain of tests/test_gpu_eigen.py's Run.chain at one of its CASES: orthonormalise, project, accumulate,
    orthonormalise, gram, svae_pca_eigen (one call: K is far below its group limit), rotate, coords.  Y and ssq are the calls'
    to add to: state, and zero in both sets.  The labels (with their -1 and K + 1) and the member counts depend on B and K
    alone, so they are the same in both sets; set B is the same fixture builder with another seed."""
    entry_points = ("svae_eig_orthonormalise", "svae_eig_project", "svae_eig_accumulate", "svae_eig_gram", "svae_pca_eigen",
                    "svae_eig_rotate", "svae_eig_coords")
    has_reference = True
    state, same_in_both_sets, must_differ = ("Y", "ssq"), ("Y", "ssq", "class_of", "members"), ("T", "eigenimages")

    def __init__(self, case):
        self.case = case
        _, self.B, rows, cols, self.C, self.K, self.R, self.P, _ = case
        self.N = rows * cols
        self.D = self.N * self.C
        self.name = "eigen_B%d_%dx%dx%d_K%d_R%d_P%d" % case[1:8]

    def fixture(self, seed):
        return (self.case[0] + 20 * seed,) + self.case[1:]

    def inputs(self, seed):
        return dict(_eigen_inputs(self.fixture(seed)))

    def _outputs(self):
        K, D, Rc, P, B, f8 = self.K, self.D, self.R, self.P, self.B, np.float64
        return {"Q0": ((K, D, Rc), f8), "T": ((B, Rc), f8), "Q1": ((K, D, Rc), f8), "G": ((K, Rc, Rc), f8), "lambda": ((K, Rc), f8),
                "W": ((K, Rc, Rc), f8), "sweeps": ((K,), np.int32), "off_norm": ((K,), f8), "eigenimages": ((K, P, D), f8),
                "residual": ((K, P), f8), "rot": ((K, P, Rc), f8), "coords": ((B, P), f8)}

    def steps(self):
        p, L = self.ptr, self.L
        B, N, C, K, Rc, P, D = self.B, self.N, self.C, self.K, self.R, self.P, self.D
        images = lambda: (p("aligned"), p("cover"), p("class_of"), p("mean"))
        return [lambda st: L.svae_eig_orthonormalise(p("start"), K, D, Rc, p("Q0"), st),
                lambda st: L.svae_eig_project(*images(), p("Q0"), B, N, C, K, Rc, p("T"), st),
                lambda st: L.svae_eig_accumulate(*images(), p("T"), B, N, C, K, Rc, p("Y"), p("ssq"), st),
                lambda st: L.svae_eig_orthonormalise(p("Y"), K, D, Rc, p("Q1"), st),
                lambda st: L.svae_eig_gram(p("Q0"), p("Y"), p("members"), K, D, Rc, p("G"), st),
                lambda st: L.svae_pca_eigen(p("G"), Rc, K, p("lambda"), p("W"), p("sweeps"), p("off_norm"), st),
                lambda st: L.svae_eig_rotate(p("Q0"), p("Y"), p("W"), p("lambda"), p("members"), K, D, Rc, P, p("eigenimages"),
                                             p("residual"), p("rot"), st),
                lambda st: L.svae_eig_coords(p("T"), p("class_of"), p("rot"), B, K, Rc, P, p("coords"), st)]

    def check(self, out, seed=0):
        """tests/eigen_ref.py within tests/test_gpu_eigen.py's BOUND, through that file's chain_errors: what hangs on an
        eigenvector is compared where its eigenvalue is separated."""
        from test_gpu_eigen import BOUND, chain_errors, reference
        want = reference(self.fixture(seed))[1]
        errs, _ = chain_errors(out, want, self.inputs(seed)["class_of"], self.K, self.R, self.P)
        assert not {k: e for k, e in errs.items() if not e <= BOUND}, (self.name, errs)


class NeighbourCase(S.Case):
    """svae_nbr_search on tests/test_gpu_neighbours.py's 300 x 7 latents, K = 64, the candidates offered in three chunks out of
    order, then svae_nbr_average on its 40 x 105 x 3 stack (B = 17, T = 257: repeated images, empty slots, indices that are
    skipped) with weight and support.  The lists are the search's to update: state, and (+inf, -1) in both sets."""
    name, entry_points, has_reference = "neighbours_300x7_K64_avg_40x105x3_T257", ("svae_nbr_search", "svae_nbr_average"), True
    state, same_in_both_sets, non_finite_inputs, must_differ = ("d2", "index"), ("d2", "index"), ("d2",), ("d2", "average")
    chunks = ((70, 300), (0, 64), (64, 70))
    Q, D, K = 300, 7, 64                                    # queries (all of them candidates too), coordinates, list length
    images, N, C, B, T = 40, 105, 3, 17, 257                # of the stack; a slot outside [0, images) is skipped

    def fixtures(self, seed):
        from test_gpu_neighbours import average_case, search_case
        return search_case("300x7_K64", seed), average_case("40x105x3_T257", seed)

    def inputs(self, seed):
        (z, K, _, _), (stack, cover, slots, weight, _, _, _) = self.fixtures(seed)
        d2, index = NR.empty_lists(z.shape[0], K)
        return {"z": z.copy(), "d2": d2, "index": index, "stack": stack.copy(), "cover": cover.copy(), "slots": slots.copy(),
                "weight": weight.copy()}                    # copies: the fixtures are shared and read-only

    def _outputs(self):
        return {"average": ((self.B, self.N, self.C), np.float32), "support": ((self.B, self.N), np.float64)}

    def steps(self):
        p, L = self.ptr, self.L
        Q, D, K, images, N, C, B, T = self.Q, self.D, self.K, self.images, self.N, self.C, self.B, self.T
        search = [lambda st, lo=lo, hi=hi: L.svae_nbr_search(p("z"), Q, 0, p("z") + lo * D * 8, hi - lo, lo, D, K, p("d2"), p("index"), st)
                  for lo, hi in self.chunks]
        return search + [lambda st: L.svae_nbr_average(p("stack"), p("cover"), images, N, C, p("slots"), p("weight"), B, T, p("average"),
                                                       p("support"), st)]

    def check(self, out, seed=0):
        """The lists and the support bit for bit (neighbours_ref.brute_force, neighbours_ref.average), the averages within one
        float32 of the reference's quotient: the bounds of tests/test_gpu_neighbours.py."""
        (_, _, want_d, want_i), (_, _, _, _, _, want_sup, exact) = self.fixtures(seed)
        assert out["d2"].tobytes() == want_d.tobytes() and out["index"].tobytes() == want_i.tobytes()
        assert out["support"].tobytes() == want_sup.tobytes()
        assert NR.within_one_float(out["average"], exact)[0].all()


def analysis_cases():
    """Fresh, unallocated instances in a fixed order.  Construction is cheap: the data are built, once, by inputs()."""
    from test_gpu_eigen import CASES
    return [KMeansCase(), GmmCase(), PcaCase(), FrcCase(), RefineCase(), ClassifyCase(), ExpectCase(), EigenCase(CASES[1]),
            EigenCase(CASES[7]), NeighbourCase()]
