"""Helper of the eigenimage tests (not collected): include/svae_eigen.h restated in numpy float64 -- the same residuals, the same
segment and lane orders of every sum, the same Gram-Schmidt with its dead-column rule, the same Rayleigh-Ritz step and sign rule
-- and the fixtures the CPU and GPU tests share.  numpy's +, -, *, / and sqrt on float64 are the IEEE operations the header
names, so the restatement follows the header operation for operation.  Where the header skips a term this file adds +0: the
running sums start at +0 and are therefore never -0, so that changes no bit."""
import functools

import numpy as np

import pca_ref

MAX_R, MAX_K, MAX_BASIS, MAX_OUT = 64, 4096, 2 ** 28, 4
DEAD = 2.0 ** -26


def limits_ok(K, D, R):
    return 1 <= K <= MAX_K and 1 <= R <= MAX_R and D >= 1 and K * D * R <= MAX_BASIS


def _seq(rows, axis=0):
    """The entries along `axis` added in order onto +0 (cumsum adds sequentially)."""
    rows = np.moveaxis(rows, axis, 0)
    zero = np.zeros((1,) + rows.shape[1:], np.float64)
    return np.cumsum(np.concatenate([zero, rows]), axis=0)[-1]


def segments(D, R):
    """(S, L): the number of segments and their length."""
    Rp = 1
    while Rp < R:
        Rp *= 2
    S = 256 // Rp
    return S, -(-D // S)


def seg_sum(terms, R):
    """The sum over axis 0 (length D) in the header's segment order for a basis of R columns."""
    D = terms.shape[0]
    S, L = segments(D, R)
    pad = np.zeros((S * L - D,) + terms.shape[1:], np.float64)          # +0 at the end of the last segments: no bit changes
    return _seq(_seq(np.concatenate([terms, pad]).reshape((S, L) + terms.shape[1:]), axis=1))


def lane_sum(terms):
    """The sum over axis 0 (length D) in the header's lane order."""
    D = terms.shape[0]
    rows = -(-D // 256)
    pad = np.zeros((rows * 256 - D,) + terms.shape[1:], np.float64)
    return _seq(_seq(np.concatenate([terms, pad]).reshape((rows, 256) + terms.shape[1:])))


def class_moments(aligned, cover, label, K):
    """svae_class_sums_update over the images in index order and the mean of them: (mean (K, N, C), count (K, N))."""
    B, N, C = aligned.shape
    total, count = np.zeros((K, N, C)), np.zeros((K, N))
    for b in range(B):
        k = int(label[b])
        if 0 <= k < K:
            cv = np.ones(N, bool) if cover is None else cover[b] != 0
            total[k] = total[k] + np.where(cv[:, None], aligned[b].astype(np.float64), 0.0)
            count[k] = count[k] + cv
    with np.errstate(all="ignore"):
        mean = np.where(count[:, :, None] > 0, total / np.where(count > 0, count, 1.0)[:, :, None], 0.0)
    return mean, count


def residuals(aligned, cover, label, mean):
    """(d (B, D) with +0 where uncovered or in no class, covered (B, D) bool, in_class (B) bool)."""
    B, N, C = aligned.shape
    K = mean.shape[0]
    live = (label >= 0) & (label < K)
    k = np.where(live, label, 0)
    cv = np.ones((B, N), bool) if cover is None else cover != 0
    cv = np.repeat(cv[:, :, None], C, 2).reshape(B, N * C) & live[:, None]
    with np.errstate(all="ignore"):
        d = aligned.astype(np.float64).reshape(B, N * C) - mean.reshape(K, N * C)[k]
    return np.where(cv, d, 0.0), cv, live


def project(aligned, cover, label, mean, Q):
    """svae_eig_project: T (B, R)."""
    B = aligned.shape[0]
    R = Q.shape[2]
    d, _, live = residuals(aligned, cover, label, mean)
    T = np.zeros((B, R))
    with np.errstate(all="ignore"):
        for b in range(B):
            if live[b]:
                T[b] = seg_sum(d[b][:, None] * Q[label[b]], R)
    return T


def accumulate(aligned, cover, label, mean, T, Y, ssq=None):
    """svae_eig_accumulate, in place on Y (K, D, R) and ssq (K, D) or None."""
    d, cv, live = residuals(aligned, cover, label, mean)
    with np.errstate(all="ignore"):
        for b in range(aligned.shape[0]):
            if live[b]:
                k = label[b]
                Y[k] = Y[k] + np.where(cv[b][:, None], d[b][:, None] * T[b][None, :], 0.0)
                if ssq is not None:
                    ssq[k] = ssq[k] + np.where(cv[b], d[b] * d[b], 0.0)


def orthonormalise(Y):
    """svae_eig_orthonormalise: Q (K, D, R)."""
    K, D, R = Y.shape
    Q = np.zeros((K, D, R))
    with np.errstate(all="ignore"):
        for k in range(K):
            live = []
            for j in range(R):
                q = Y[k, :, j].copy()
                before = np.sqrt(lane_sum(q * q))
                for _ in range(2):
                    for i in range(j):
                        if live[i]:
                            c = lane_sum(Q[k, :, i] * q)
                            q = q - c * Q[k, :, i]
                after = np.sqrt(lane_sum(q * q))
                dead = not after > 0.0 or not np.isfinite(after) or after < DEAD * before
                live.append(not dead)
                if not dead:
                    Q[k, :, j] = q / after
    return Q


def gram(Q, Y, members):
    """svae_eig_gram: G (K, R, R)."""
    K, D, R = Q.shape
    G = np.zeros((K, R, R))
    with np.errstate(all="ignore"):
        for k in range(K):
            if members[k] >= 2:
                A = np.stack([seg_sum(Q[k, :, r][:, None] * Y[k], R) for r in range(R)])
                G[k] = ((A + A.T) * 0.5) / np.float64(members[k] - 1)
    return G


def rotate(Q, Y, W, lam, members, P):
    """svae_eig_rotate: (eigenimages (K, P, D), residual (K, P), rot (K, P, R))."""
    K, D, R = Q.shape
    images, residual, rot = np.zeros((K, P, D)), np.zeros((K, P)), np.zeros((K, P, R))
    with np.errstate(all="ignore"):
        for k in range(K):
            if members[k] < 2:
                continue
            for p in range(P):
                v = _seq((Q[k] * W[k, p][None, :]).T)
                u = _seq((Y[k] * W[k, p][None, :]).T) / np.float64(members[k] - 1)
                mag = np.where(np.isnan(v), -1.0, np.abs(v))
                flip = mag.max() >= 0 and v[np.argmax(mag)] < 0      # the first of equal magnitudes
                if flip:
                    v, u = -v, -u
                images[k, p] = v
                rot[k, p] = -W[k, p] if flip else W[k, p]
                w = u - lam[k, p] * v
                residual[k, p] = np.sqrt(lane_sum(w * w))
    return images, residual, rot


def coords(T, label, rot):
    """svae_eig_coords: (B, P)."""
    K = rot.shape[0]
    live = (label >= 0) & (label < K)
    with np.errstate(all="ignore"):
        out = _seq((T[:, None, :] * rot[np.where(live, label, 0)]).transpose(2, 0, 1))
    return np.where(live[:, None], out, 0.0)


def eigen(G):
    """svae_pca_eigen on the Gram matrices: (lambda (K, R), W (K, R, R) with rows as vectors)."""
    out = pca_ref.eigen(G)
    return out["eigenvalues"], out["components"]


def fit(aligned, cover, label, K, R, P, passes, start, batch=None):
    """The whole chain as ops.EigenImages and spatial_vae_amd/eigen_images.py make it: the class averages, the start array made
    orthonormal, `passes` walks in minibatches of `batch` images, then the Rayleigh-Ritz step.  Returns a dict of every array."""
    B, N, C = aligned.shape
    D = N * C
    batch = batch or B
    label = np.asarray(label, np.int64)
    mean, count = class_moments(aligned, cover, label, K)
    members = np.array([(label == k).sum() for k in range(K)], np.int64)
    Q = orthonormalise(np.asarray(start, np.float64).reshape(K, D, R))
    ssq = np.zeros((K, D))
    for it in range(passes):
        if it:
            Q = orthonormalise(Y)
        Y = np.zeros((K, D, R))
        rows = []
        for lo in range(0, B, batch):
            sl = slice(lo, lo + batch)
            cv = None if cover is None else cover[sl]
            T = project(aligned[sl], cv, label[sl], mean, Q)
            accumulate(aligned[sl], cv, label[sl], mean, T, Y, ssq if it == 0 else None)
            rows.append(T)
    T = np.concatenate(rows)
    G = gram(Q, Y, members)
    lam, W = eigen(G)
    images, residual, rot = rotate(Q, Y, W, lam, members, P)
    return {"mean": mean, "count": count, "members": members, "ssq": ssq, "Q": Q, "Y": Y, "T": T, "G": G, "lambda": lam, "W": W,
            "eigenimages": images, "residual": residual, "rot": rot, "coords": coords(T, label, rot)}


def host_outputs(fit_, P):
    """What the command line derives on the host: variance, total_variance, eigenvalues (K, P), explained_variance_ratio."""
    K, N = fit_["count"].shape
    C = fit_["ssq"].shape[1] // N
    members = fit_["members"]
    count = np.repeat(fit_["count"][:, :, None], C, 2).reshape(K, N * C)
    with np.errstate(all="ignore"):
        variance = np.where(count >= 2, fit_["ssq"] / np.where(count >= 2, count - 1.0, 1.0), 0.0)
        total = np.where(members >= 2, fit_["ssq"].sum(1) / np.where(members >= 2, members - 1.0, 1.0), 0.0)
        lam = fit_["lambda"][:, :P] + 0.0
        ratio = np.where(total[:, None] > 0, lam / np.where(total > 0, total, 1.0)[:, None], 0.0)
    return {"variance": variance, "total_variance": total, "eigenvalues": lam, "explained_variance_ratio": ratio}


def covariance(aligned, cover, label, k, mean):
    """The explicit D x D covariance of class k about `mean` (for small fixtures only) and its member count."""
    d, _, _ = residuals(aligned, cover, np.asarray(label, np.int64), mean)
    d = d[np.asarray(label) == k]
    return d.T.dot(d) / max(d.shape[0] - 1, 1), d.shape[0]


# ---------------------------------------------------------------- fixtures
def start_array(seed, K, D, R):
    return np.random.RandomState(seed).randn(K, D, R)


def rotated_covers(seed, B, rows, cols):
    """Covers of real poses: the pixels of a rows x cols box that a rotation by a random angle and a shift of up to 15 % of the
    half-width keep inside it (svae_align.h's geometry, without its 1e-6 slack)."""
    rs = np.random.RandomState(seed)
    jy, jx = np.mgrid[0:rows, 0:cols]
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    X, Y = jx - a, bq - jy
    out = np.empty((B, rows * cols), np.uint8)
    for b in range(B):
        t, dx = rs.uniform(-np.pi, np.pi), rs.uniform(-0.15, 0.15, 2)
        c, s = np.cos(t), np.sin(t)
        U, V = X - a * dx[0], Y - bq * dx[1]
        fx, fy = c * U + s * (a / bq) * V + a, bq - (-s * (bq / a) * U + c * V)
        out[b] = ((fx >= 0) & (fx <= cols - 1) & (fy >= 0) & (fy <= rows - 1)).reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def images(seed, B, rows, cols, C, K, covered=True):
    """(aligned (B, N, C) float32, cover (B, N) uint8 or None, label (B) int32) with what the header singles out: labels -1 and
    >= K, an empty class (K - 1) and a one-member class (K - 2) where K >= 3 and, where K >= 5, class 0 with three members
    only (rank deficient for R >= 3).  Cached and shared: treat as read-only."""
    rs = np.random.RandomState(seed)
    N = rows * cols
    base = rs.randn(max(K, 1), N, C)
    aligned = (base[rs.randint(0, K, B)] * 0.5 + rs.randn(B, N, C) * np.linspace(0.2, 1.5, N * C).reshape(N, C)).astype(np.float32)
    if K == 1:
        label = np.zeros(B, np.int32)
    elif K < 3 or B < 12:
        label = (np.arange(B) % K).astype(np.int32)
    else:
        if K < 5:
            label = np.zeros(B, np.int32)
        else:
            label = (1 + np.arange(B) % (K - 3)).astype(np.int32)
            label[[2, 5, 9]] = 0
        label[7] = K - 2
        label[[3, 10]] = [-1, K + 1]
    cover = rotated_covers(seed + 1, B, rows, cols) if covered else None
    if cover is not None:
        aligned = np.where(cover[:, :, None] != 0, aligned, np.float32(0))
    return aligned, cover, label


def low_rank_images(seed, B, N, K, rank):
    """Members that lie exactly in a `rank`-dimensional affine subspace per class: small integers, exact in float32, with
    integer coefficients of well separated scales.  label = index mod K."""
    rs = np.random.RandomState(seed)
    basis = rs.randint(-3, 4, size=(K, rank, N)).astype(np.float64)
    label = (np.arange(B) % K).astype(np.int32)
    coef = rs.randint(-4, 5, size=(B, rank)) * (2 ** np.arange(rank, 0, -1))
    aligned = np.einsum("br,brn->bn", coef, basis[label]) + rs.randint(-5, 6, size=(K, N))[label]
    return aligned.astype(np.float32).reshape(B, N, 1), None, label


def planted_images(seed, B, N, spectrum):
    """One class of B members with a planted, full-rank spectrum: independent normals along a random orthonormal frame."""
    rs = np.random.RandomState(seed)
    frame = np.linalg.qr(rs.randn(N, N))[0]
    aligned = (rs.randn(B, N) * np.sqrt(spectrum)).dot(frame.T) + rs.randn(N)
    return aligned.astype(np.float32).reshape(B, N, 1), None, np.zeros(B, np.int32)
