"""float64 numpy restatement of include/svae_expect.h on top of tests/refine_ref.py (planes and shifts) and tests/align_ref.py
(coverage): the live slots, the log-weight volume, the first maximum, the posterior, the contribution rows in the header's order
of accumulation (k, then sy, then sx upwards) and the soft class sums.  Written from the header's text, not from the kernels;
the sums of D, h, Z and class_post are numpy's, so the device agrees to rounding and not bit for bit.  Also the fixtures of the
kernel tests and the rule that picks each fixture's inv_sigma2.  tests/test_expect_cpu.py holds all of it to properties of what
it restates."""
import numpy as np

import align_ref as AR
import classify_ref as CR
import refine_ref as R


def live_slots(cand_row, n_ref, log_prior):
    """The reference of each slot of one row of cand, -1 for a dead slot (out of range, a repeat of an earlier slot, or a prior
    that is not finite)."""
    out = []
    for j, r in enumerate(cand_row):
        r = int(r)
        live = 0 <= r < n_ref and r not in [int(v) for v in cand_row[:j]]
        if live and log_prior is not None:
            live = bool(np.isfinite(log_prior[r]))
        out.append(r if live else -1)
    return out


def coverage_planes(y, pose, rows, cols, A, step, interp):
    """(B, 2A+1, rows, cols) float64 of 0 / 1: svae_align.h's coverage flag of P_k."""
    B = np.asarray(y).shape[0]
    pose = np.asarray(pose).astype(np.float64).reshape(B, 3)
    step = float(step) if A > 0 else 0.0
    out = []
    for k in range(-A, A + 1):
        _, cover = AR.align_ref(y, pose[:, 0] + float(k) * step, pose[:, 1:], rows, cols, interp, dtype=np.float64)
        out.append(cover.reshape(B, rows, cols).astype(np.float64))
    return np.stack(out, 1)


def correlations(y, ref, weight, cand, pose_in, rows, cols, A, step, S, interp="bicubic"):
    """What of the log-weights depends on neither inv_sigma2 nor the prior.  Per image None (a non-finite pose) or a dict: "D"
    (M, nA, nS, nS) indexed [j, k + A, sy + S, sx + S], NaN in the rows of slots that are out of range or repeats; "h" (M); "Q"
    {(sy, sx): (nA, rows, cols, C + 1)}: every shifted image of P_k with the shifted coverage of P_k as one more channel."""
    y = np.asarray(y)
    B = y.shape[0]
    cand = np.asarray(cand, dtype=np.int32)
    M = cand.shape[1]
    pose_in = np.asarray(pose_in, dtype=np.float32).reshape(B, 3)
    ref = np.asarray(ref, dtype=np.float64)
    n_ref = ref.shape[0]
    ref = ref.reshape(n_ref, rows, cols, -1)
    C = ref.shape[3]
    w = np.ones((rows, cols)) if weight is None else np.asarray(weight, dtype=np.float64).reshape(rows, cols)
    nA, nS = 2 * A + 1, 2 * S + 1
    out = []
    for b in range(B):
        if not np.isfinite(pose_in[b].astype(np.float64)).all():
            out.append(None)
            continue
        slots = live_slots(cand[b], n_ref, None)
        P = R.candidate_planes(y[b:b + 1], pose_in[b:b + 1], rows, cols, A, step, interp)[0]
        cov = coverage_planes(y[b:b + 1], pose_in[b:b + 1], rows, cols, A, step, interp)[0]
        both = np.concatenate([P, cov[..., None]], 3)
        Q = {(sy, sx): R.shifted(both, sx, sy) for sy in range(-S, S + 1) for sx in range(-S, S + 1)}
        D = np.full((M, nA, nS, nS), np.nan)
        h = np.full(M, np.nan)
        on = [j for j, r in enumerate(slots) if r >= 0]
        if on:
            wr = np.stack([w[..., None] * ref[slots[j]] for j in on])               # (live, rows, cols, C)
            h[on] = (wr * np.stack([ref[slots[j]] for j in on])).reshape(len(on), -1).sum(1)
            with np.errstate(invalid="ignore", over="ignore"):
                for (sy, sx), q in Q.items():
                    D[on, :, sy + S, sx + S] = (wr[:, None] * q[None, ..., :C]).reshape(len(on), nA, -1).sum(2)
        out.append({"D": D, "h": h, "Q": Q})
    return out


def log_weights(corr, cand, n_ref, log_prior, inv_sigma2):
    """Per image None (no live slot or a non-finite pose) or (slots (M) with -1 = dead, L (M, nA, nS, nS) with NaN in the rows of
    dead slots), from what correlations() returned."""
    out = []
    for b, item in enumerate(corr):
        slots = live_slots(cand[b], n_ref, log_prior)
        if item is None or max(slots) < 0:
            out.append(None)
            continue
        L = np.full(item["D"].shape, np.nan)
        with np.errstate(invalid="ignore", over="ignore"):
            for j, r in enumerate(slots):
                if r >= 0:
                    lp = 0.0 if log_prior is None else float(log_prior[r])
                    L[j] = inv_sigma2 * (item["D"][j] - 0.5 * item["h"][j]) + lp
        out.append((slots, L))
    return out


def pose_expect(y, ref, weight, log_prior, cand, pose_in, rows, cols, A, step, S, inv_sigma2, interp="bicubic", corr=None):
    """{"contrib" (B, M, N, C), "cover_w" (B, M, N), "class_post" (B, M), "log_evidence" (B) float64, "best" (B, 4) int32 = slot, k,
    sx, sy, "gap" (B) float64: Lmax minus the second-largest L (inf with one entry or a skipped image), "spread" (B) float64:
    max L - min L over the live volume (nan for a skipped image)}.  corr: what correlations() gave for the same inputs."""
    y = np.asarray(y)
    B = y.shape[0]
    cand = np.asarray(cand, dtype=np.int32)
    M = cand.shape[1]
    N = rows * cols
    C = y.size // (B * N)
    nA, nS = 2 * A + 1, 2 * S + 1
    n_ref = np.asarray(ref).shape[0]
    out = {"contrib": np.zeros((B, M, N, C)), "cover_w": np.zeros((B, M, N)), "class_post": np.zeros((B, M)),
           "log_evidence": np.zeros(B), "best": np.zeros((B, 4), np.int32), "gap": np.full(B, np.inf), "spread": np.full(B, np.nan)}
    out["best"][:, 0] = -1
    if corr is None:
        corr = correlations(y, ref, weight, cand, pose_in, rows, cols, A, step, S, interp)
    for b, item in enumerate(log_weights(corr, cand, n_ref, log_prior, inv_sigma2)):
        if item is None:
            continue
        slots, L = item
        live = np.array([r >= 0 for r in slots])
        if not np.isfinite(L[live]).all():
            continue
        flat = L.reshape(-1)
        with np.errstate(invalid="ignore"):
            top = np.nanmax(flat)
            best = int(np.flatnonzero(flat == top)[0])      # the first maximum under strict `>`; dead rows are NaN
        E = np.zeros(L.shape)
        E[live] = np.exp(L[live] - top)
        Z = float(E.sum())
        p = E / Z
        out["class_post"][b] = p.reshape(M, -1).sum(1)
        out["log_evidence"][b] = top + np.log(Z)
        j, ik, iy, ix = np.unravel_index(best, L.shape)
        out["best"][b] = (j, ik - A, ix - S, iy - S)
        values = np.sort(L[live].reshape(-1))
        out["spread"][b] = values[-1] - values[0]
        if values.size > 1:
            out["gap"][b] = values[-1] - values[-2]
        both = np.zeros((M, rows, cols, C + 1))             # dead rows stay zero: their p is 0
        Q = corr[b]["Q"]
        for ik in range(nA):                                # every element's terms k upwards, then sy, then sx
            for iy in range(nS):
                for ix in range(nS):
                    both += p[:, ik, iy, ix, None, None, None] * Q[(iy - S, ix - S)][ik]
        out["contrib"][b] = both[..., :C].reshape(M, N, C)
        out["cover_w"][b] = both[..., C].reshape(M, N)
    return out


def sums_update(total, count, contrib, cover_w, cand, target, n_ref):
    """svae_expect_sums_update on the float64 accumulators total (n_classes, N, C) and count (n_classes, N), in place: images
    upwards, slots upwards."""
    n_classes = total.shape[0]
    cand = np.asarray(cand)
    for b in range(cand.shape[0]):
        for j in range(cand.shape[1]):
            r = int(cand[b, j])
            if not 0 <= r < n_ref:
                continue
            t = r if target is None else int(target[r])
            if not 0 <= t < n_classes:
                continue
            total[t] = total[t] + contrib[b, j]
            count[t] = count[t] + cover_w[b, j]
    return total, count


# ---------------------------------------------------------------- fixtures
# (rows, cols, C, A, S, M): the shapes of tests/test_gpu_expect.py, each with B = 5 images
SHAPES = ((24, 24, 1, 3, 2, 1), (17, 13, 3, 2, 3, 3), (9, 8, 1, 32, 8, 7), (72, 72, 4, 1, 1, 2), (9, 8, 1, 0, 0, 64))
SHAPE_IDS = ["%dx%dx%d_A%d_S%d_M%d" % s for s in SHAPES]
FIXTURE_B = 5
SPREAD = (5.0, 50.0)        # the band max L - min L of every fixture image is brought into
SPREAD_TARGET = 20.0


def fixture(index, weighted=True, prior=True):
    """The inputs of one shape, from a seed fixed by the index alone: smooth references (low-pass noise) of which every image is
    one, posed and with noise added; image 3 has an all-empty row of cand, image 1 a repeated slot (where M > 1).  Returns a dict
    of y (B, N, C) float32, ref (n_ref, N, C) float64, weight (N) float64 or None, log_prior (n_ref) float64 or None, cand (B, M)
    int32, pose (B, 3) float32, step, and the shape's numbers."""
    rows, cols, C, A, S, M = SHAPES[index]
    rs = np.random.RandomState(1000 + index)
    N, B = rows * cols, FIXTURE_B
    n_ref = M + 2
    raw = rs.standard_normal((n_ref, rows, cols, C))
    for _ in range(2):                          # a separable 1-2-1 blur, twice: neighbouring pixels correlate
        raw = 0.25 * (np.roll(raw, 1, 1) + np.roll(raw, -1, 1)) + 0.5 * raw
        raw = 0.25 * (np.roll(raw, 1, 2) + np.roll(raw, -1, 2)) + 0.5 * raw
    ref = raw.reshape(n_ref, N, C)
    cand = np.stack([rs.permutation(n_ref)[:M] for _ in range(B)]).astype(np.int32)
    cand[3, :] = -1
    if M > 1:
        cand[1, M - 1] = cand[1, 0]
    if M > 2:
        cand[0, 1] = n_ref + 3                  # an entry past the references is an empty slot
    y = np.stack([ref[max(int(cand[b, 0]), 0)] for b in range(B)]) + 0.5 * rs.standard_normal((B, N, C))
    pose = np.concatenate([rs.uniform(-np.pi, np.pi, (B, 1)), rs.uniform(-0.1, 0.1, (B, 2))], 1).astype(np.float32)
    jy, jx = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    rad = np.hypot(jy - (rows - 1) / 2.0, jx - (cols - 1) / 2.0) / (min(rows, cols) / 2.0)
    weight = np.clip(1.25 - rad, 0.0, 1.0).reshape(N) if weighted else None
    log_prior = np.log(rs.dirichlet(np.full(n_ref, 4.0))) if prior else None
    return dict(y=y.astype(np.float32), ref=ref, weight=weight, log_prior=log_prior, cand=cand, pose=pose, step=np.deg2rad(3.0),
                rows=rows, cols=cols, C=C, A=A, S=S, M=M, n_ref=n_ref, B=B, index=index)


_CORR = {}


def fixture_correlations(f, interp):
    """correlations() of a fixture, computed once per (shape, weighted or not, interp): neither the prior nor inv_sigma2 enters."""
    key = (f["index"], f["weight"] is not None, interp)
    if key not in _CORR:
        _CORR[key] = correlations(f["y"], f["ref"], f["weight"], f["cand"], f["pose"], f["rows"], f["cols"], f["A"], f["step"],
                                  f["S"], interp)
    return _CORR[key]


def spreads(f, inv_sigma2, interp):
    """max L - min L over the live volume of each image of the fixture that is not skipped."""
    out = []
    for item in log_weights(fixture_correlations(f, interp), f["cand"], f["n_ref"], f["log_prior"], inv_sigma2):
        if item is not None:
            slots, L = item
            v = L[np.array(slots) >= 0]
            out.append(float(v.max() - v.min()))
    return np.array(out)


def pick_inv_sigma2(f, interp="bicubic"):
    """The inv_sigma2 a fixture is run at: the spread of L at inv_sigma2 = 1 without the prior (whose part does not scale) is
    measured per image, and inv_sigma2 = SPREAD_TARGET / sqrt(min max) of those, rounded to three significant digits.  The
    posterior is then neither flat nor one-hot; tests/test_expect_cpu.py asserts the band for every fixture."""
    s = spreads(dict(f, log_prior=None), 1.0, interp)
    return float("%.3g" % (SPREAD_TARGET / float(np.sqrt(s.min() * s.max()))))


def run(f, inv_sigma2, interp="bicubic"):
    return pose_expect(f["y"], f["ref"], f["weight"], f["log_prior"], f["cand"], f["pose"], f["rows"], f["cols"], f["A"], f["step"],
                       f["S"], inv_sigma2, interp, corr=fixture_correlations(f, interp))


def planted_one_hot():
    """classify_ref's planted three-class case as an expectation problem: every image against all three references."""
    y, ref, true, label, start = CR.planted_case()
    cand = np.tile(np.arange(3, dtype=np.int32), (len(true), 1))
    return y, ref, cand, start
