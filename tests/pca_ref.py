"""Helper of the PCA tests (not collected): include/svae_pca.h restated in numpy float64 -- the same chunk rule and two-level
order of every sum, the same round-robin Jacobi with its three phases per step, the same stopping, sort and sign rules -- and
the fixtures the CPU and GPU tests share.  numpy's +, -, *, / and sqrt on float64 are the IEEE operations the header names, so
the restatement follows the header operation for operation."""
import functools

import numpy as np

from kmeans_ref import chunk_len

MAX_SWEEPS = 30
STOP = 2.0 ** -104


def limits_ok(N, D, G):
    return 1 <= D <= 64 and 1 <= G <= 1024 and G * (D * (D + 1) // 2) <= 32768 and 1 <= N < 2 ** 31


def workspace_bytes(N, D, G):
    if not limits_ok(N, D, G):
        return 0
    C = -(-N // chunk_len(N))
    return 8 * (C * G * (1 + D + D * (D + 1) // 2) + (N + 1) // 2)


def members(x, group, G):
    """(N) the group each point counts in, -1 = none."""
    x = np.asarray(x, np.float32)
    g = np.zeros(x.shape[0], np.int64) if group is None else np.asarray(group, np.int64).copy()
    g[(g < 0) | (g >= G)] = -1
    g[~np.isfinite(x).all(1)] = -1
    return g


def _ordered(rows):
    """The rows added in order onto +0, along axis 0."""
    zero = np.zeros((1,) + rows.shape[1:], np.float64)
    return np.cumsum(np.concatenate([zero, rows]), axis=0)[-1]        # cumsum adds sequentially


def moments(x, group=None, G=1):
    """svae_pca_moments: {"count" (G) int64, "mean" (G, D), "cov" (G, D, D)}."""
    x = np.asarray(x, np.float32)
    N, D = x.shape
    assert limits_ok(N, D, G) and (group is not None or G == 1)
    x64 = x.astype(np.float64)
    member = members(x, group, G)
    L = chunk_len(N)
    chunks = [(lo, min(N, lo + L)) for lo in range(0, N, L)]
    count = np.array([(member == g).sum() for g in range(G)], np.int64)
    mean = np.zeros((G, D))
    cov = np.zeros((G, D, D))
    for g in range(G):
        if count[g] == 0:
            continue
        sums = np.stack([_ordered(x64[lo:hi][member[lo:hi] == g]) for lo, hi in chunks])
        mean[g] = _ordered(sums) / np.float64(count[g])
        if count[g] < 2:
            continue
        parts = []
        for lo, hi in chunks:
            d = x64[lo:hi][member[lo:hi] == g] - mean[g]
            parts.append(_ordered(d[:, :, None] * d[:, None, :]))
        cov[g] = _ordered(np.stack(parts)) / np.float64(count[g] - 1)
    return {"count": count, "mean": mean, "cov": cov}


def seat(k, s, n):
    return 0 if k == 0 else 1 + (k - 1 + (n - 1) - s) % (n - 1)


def step_pairs(D, s):
    """The (p, q) pairs of step s, p < q, the bye left out, in seat order."""
    n = D + (D & 1)
    out = []
    for k in range(n // 2):
        a, b = seat(k, s, n), seat(n - 1 - k, s, n)
        p, q = min(a, b), max(a, b)
        if q < D:
            out.append((p, q))
    return out


def _norm2(A, diagonal):
    """rowsum in q order onto +0, then the rows in r order onto +0."""
    D = A.shape[0]
    sq = A * A
    if not diagonal:
        sq = sq.copy()
        sq[np.arange(D), np.arange(D)] = 0.0        # adding +0 to a sum that is +0 or positive changes no bit: the same as skipping
    return _ordered(_ordered(sq.T)[:, None])[0]


def eigen_one(C):
    """svae_pca_eigen on one matrix: (eigenvalues (D), components (D, D) with rows as axes, sweeps, off_norm)."""
    A = np.array(C, np.float64)
    D = A.shape[0]
    with np.errstate(all="ignore"):
        fro2 = _norm2(A, True)
        if not np.isfinite(fro2):
            return np.zeros(D), np.zeros((D, D)), -1, 0.0
        V = np.eye(D)
        n = D + (D & 1)
        done = 0
        while True:
            off2 = _norm2(A, False)
            if off2 <= STOP * fro2 or done >= MAX_SWEEPS:
                break
            for s in range(n - 1):
                pairs = step_pairs(D, s)
                if not pairs:
                    continue
                p, q = np.array(pairs).T
                apq = A[p, q]
                safe = np.where(apq != 0, apq, 1.0)
                theta = (A[q, q] - A[p, p]) / (2.0 * safe)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                c, sn = np.where(apq != 0, c, 1.0), np.where(apq != 0, sn, 0.0)
                ap, aq = A[p, :].copy(), A[q, :].copy()
                A[p, :] = c[:, None] * ap - sn[:, None] * aq
                A[q, :] = sn[:, None] * ap + c[:, None] * aq
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c[None, :] * mp - sn[None, :] * mq
                    M[:, q] = sn[None, :] * mp + c[None, :] * mq
                A[p, q] = 0.0
                A[q, p] = 0.0
            done += 1
        lam = np.diag(A).copy()
        order = np.argsort(-lam, kind="stable")     # descending, equal values by ascending column
        comp = np.empty((D, D))
        for r, j in enumerate(order):
            v = V[:, j]
            at = v[np.argmax(np.abs(v))]            # the first of equal magnitudes
            comp[r] = -v if at < 0 else v
        return lam[order], comp, done, float(np.sqrt(off2))


def eigen(cov):
    """svae_pca_eigen on (G, D, D): {"eigenvalues", "components", "sweeps" int32, "off_norm"}."""
    out = [eigen_one(C) for C in cov]
    return {"eigenvalues": np.stack([o[0] for o in out]), "components": np.stack([o[1] for o in out]),
            "sweeps": np.array([o[2] for o in out], np.int32), "off_norm": np.array([o[3] for o in out])}


def project(x, group, G, count, mean, components, P):
    """svae_pca_project: (N, P)."""
    x = np.asarray(x, np.float32)
    N, D = x.shape
    member = members(x, group, G)
    live = (member >= 0) & (count[np.maximum(member, 0)] >= 2)
    g = np.where(live, member, 0)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - mean[g]
        acc = np.zeros((N, P))
        for t in range(D):
            acc = acc + d[:, t:t + 1] * components[g, :P, t]
    return np.where(live[:, None], acc, 0.0)


def fit(x, group=None, G=1, P=None):
    """The three calls in a row, as ops.LatentPCA.fit makes them."""
    out = moments(x, group, G)
    out.update(eigen(out["cov"]))
    out["proj"] = project(x, group, G, out["count"], out["mean"], out["components"], x.shape[1] if P is None else P)
    return out


def min_gap(eigenvalues):
    """The smallest gap between adjacent eigenvalues over the largest eigenvalue (inf for D == 1)."""
    lam = np.asarray(eigenvalues, np.float64)
    if lam.shape[0] < 2:
        return float("inf")
    return float(np.min(-np.diff(lam)) / lam[0])


# ---------------------------------------------------------------- fixtures
def spread_points(seed, N, D):
    """N points of D coordinates: unit normals with the column scales linspace(1, 3, D), shifted off the origin."""
    rs = np.random.RandomState(seed)
    return (rs.randn(N, D) * np.linspace(1.0, 3.0, D) + rs.randn(D)).astype(np.float32)


def labelled(seed, N, D, G):
    """spread_points in G groups of distinct offsets and scales, with what the header singles out: label -1, labels outside
    [0, G), a group without a member (G - 1), a group of one member (G - 2) and rows holding NaN and inf."""
    rs = np.random.RandomState(1000 + seed)
    x = spread_points(seed, N, D)
    label = rs.randint(0, G - 2, size=N).astype(np.int32)
    x = (x * (1.0 + 0.25 * label[:, None]) + label[:, None]).astype(np.float32)
    label[rs.choice(N, 4, replace=False)] = [-1, G, G + 7, -5]
    one = int(np.flatnonzero(label == 0)[0])
    label[one] = G - 2
    bad = np.flatnonzero((label >= 0) & (label < G - 2))[[3, 11]]
    x[bad[0], 0] = np.nan
    x[bad[1], D - 1] = np.inf
    return x, label


# (seed, N, D, G): G == 1 runs with a NULL group.  The vectors of the fixtures in GAPPED are compared with the reference: the
# CPU test asserts their smallest relative eigenvalue gap.
SINGLE = [(0, 1, 3, 1), (1, 2, 2, 1), (2, 255, 5, 1), (3, 256, 1, 1), (4, 257, 8, 1), (5, 1000, 17, 1), (6, 259, 64, 1),
          (7, 262145 + 300, 2, 1)]
GROUPED = [(8, 1000, 3, 3), (9, 1000, 5, 50), (10, 257, 8, 3), (11, 262145 + 300, 2, 3)]
FIXTURES = SINGLE + GROUPED
GAP = 1e-4


def fixture_id(f):
    return "N%d_D%d_G%d" % f[1:]


@functools.lru_cache(maxsize=None)
def fixture(seed, N, D, G):
    """(x, group or None) -- cached and shared: treat as read-only."""
    if G == 1:
        x = spread_points(seed, N, D)
        if N >= 255:
            x[7, D - 1] = np.nan                    # one point out, so that skipping is exercised without labels too
        return x, None
    return labelled(seed, N, D, G)


@functools.lru_cache(maxsize=None)
def fixture_fit(seed, N, D, G):
    """The reference fit of a fixture, computed once -- treat as read-only."""
    x, group = fixture(seed, N, D, G)
    return fit(x, group, G)


def low_rank(seed, N, D, rank):
    """N points of D coordinates in a `rank`-dimensional subspace (up to float rounding)."""
    rs = np.random.RandomState(seed)
    return (rs.randn(N, rank) * np.linspace(1.0, 2.0, rank)).dot(rs.randn(rank, D)).astype(np.float32)


def diagonal_cov(D):
    """A (1, D, D) matrix that is diagonal already, its values neither sorted nor distinct."""
    d = np.array([((7 * i) % 5) + 0.5 for i in range(D)])
    return np.diag(d)[None]
