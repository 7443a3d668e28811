"""float64 numpy restatement of include/svae_cluster.h (helper of the cluster tests, not collected): the distance with its
dimension loop, the strict-< tie rule, unassigned points, and the two-level order of every sum -- np.cumsum(...)[-1] for the
in-order sum inside a chunk, then the chunk totals in chunk order.  Adding +0 for a point that does not take part is exact, so
masked values stand for skipped ones."""
import numpy as np


def chunk_len(N):
    """256, doubled until ceil(N / P) <= 1024: svae_grad_guard_norm's rule."""
    P = 256
    while -(-N // P) > 1024:
        P *= 2
    return P


def _chunked(v, N):
    """v (N, ...) padded with +0 to (chunks, P, ...)."""
    P = chunk_len(N)
    C = -(-N // P)
    pad = np.zeros((C * P,) + v.shape[1:], np.float64)
    pad[:N] = v
    return pad.reshape((C, P) + v.shape[1:])


def chunk_totals(v):
    """The in-order sum of each chunk of v (N, ...), started from +0: (chunks, ...)."""
    return np.cumsum(_chunked(v, v.shape[0]), axis=1)[:, -1] + 0.0


def ordered_sum(v):
    """The header's two-level sum of v (N, ...) over its first axis."""
    return np.cumsum(chunk_totals(v), axis=0)[-1] + 0.0


def finite_rows(x):
    return np.isfinite(x).all(1)


def d2(x, c):
    """(N, k) squared distances of float32 points x (N, D) to double centres c (k, D): the sum over t in index order, each term
    one subtraction and one multiplication in double.  Rows of non-finite points hold nothing meaningful."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    c = np.asarray(c, np.float64)
    out = np.zeros((x64.shape[0], c.shape[0]))
    rows = max(1, 65536 // c.shape[0])              # blocks of points small enough to stay in cache; the arithmetic is per element
    with np.errstate(all="ignore"):
        for lo in range(0, x64.shape[0], rows):
            acc = out[lo:lo + rows]
            for t in range(x64.shape[1]):
                d = x64[lo:lo + rows, t, None] - c[None, :, t]
                acc += d * d
    return out


def assign(x, c):
    """(label (N) with -1 for unassigned points, winning d2 (N) with 0 there): centre 0 first, then upwards under strict <."""
    dist = d2(x, c)
    best, label = dist[:, 0].copy(), np.zeros(x.shape[0], np.int64)
    with np.errstate(all="ignore"):
        for j in range(1, c.shape[0]):
            closer = dist[:, j] < best
            best[closer], label[closer] = dist[closer, j], j
    fin = finite_rows(x)
    label[~fin], best[~fin] = -1, 0.0
    return label, best


def step(x, centres, label_in, iterations, update=True):
    """One svae_kmeans_step: {label, members, inertia, changed, assigned, empty, centres, iterations}; label_in is ignored while
    iterations == 0."""
    x = np.asarray(x, np.float32)
    centres = np.asarray(centres, np.float64)
    N, k = x.shape[0], centres.shape[0]
    label, best = assign(x, centres)
    members = np.bincount(label[label >= 0], minlength=k).astype(np.int64)
    out = {"label": label, "members": members, "inertia": float(ordered_sum(best)), "assigned": int((label >= 0).sum()),
           "changed": int((label >= 0).sum()) if iterations == 0 else int((label != np.asarray(label_in)).sum()),
           "empty": int((members == 0).sum()), "centres": centres.copy(), "iterations": iterations}
    if update:
        x64, P = x.astype(np.float64), chunk_len(N)
        part = np.zeros((-(-N // P), k, x.shape[1]))
        for c in range(part.shape[0]):              # per chunk and centre, the members' coordinates added in index order onto +0
            lab = label[c * P:(c + 1) * P]
            for j in np.unique(lab[lab >= 0]):
                part[c, j] = np.cumsum(x64[c * P:(c + 1) * P][lab == j], axis=0)[-1] + 0.0
        total = np.cumsum(part, axis=0)[-1] + 0.0   # the chunks in chunk order
        filled = members > 0
        out["centres"][filled] = total[filled] / members[filled, None].astype(np.float64)
        out["iterations"] = iterations + 1
    return out


def fallback(u, N):
    return int(min(np.floor(u * N), N - 1))


def seed(x, k, u):
    """svae_kmeans_seed: (seed_index (k), centres (k, D), rounds) with rounds[j] = (m, T) of centre j >= 1 (None for j = 0)."""
    x = np.asarray(x, np.float32)
    N = x.shape[0]
    P = chunk_len(N)
    fin = finite_rows(x)
    x64 = x.astype(np.float64)
    index, rounds, m = [fallback(u[0], N)], [None], None
    for j in range(1, k):
        d = d2(x, x64[index[-1]][None])[:, 0]
        d[~fin] = 0.0
        m = d if m is None else np.where(m < d, m, d)
        totals = chunk_totals(m)
        pre = np.cumsum(totals) + 0.0                    # inclusive prefix of the chunk totals
        T = pre[-1]
        pick = fallback(u[j], N)
        if T > 0 and np.isfinite(T):
            target = u[j] * T
            over = np.nonzero(pre > target)[0]
            if over.size:
                c = int(over[0])
                before = pre[c - 1] if c else 0.0
                inside = before + (np.cumsum(m[c * P:(c + 1) * P]) + 0.0)
                pick = c * P + int(np.nonzero(inside > target)[0][0])
        index.append(pick)
        rounds.append((m.copy(), float(T)))
    index = np.array(index, np.int64)
    return index, x64[index], rounds


def fit(x, k, u, iters):
    """ops.KMeans.fit: seed, `iters` update steps, one assign-only step.  Returns the last step's dict with seed_index and
    converged_at added."""
    index, centres, _ = seed(x, k, u)
    label, it, converged = None, 0, 0
    for update in [True] * iters + [False]:
        out = step(x, centres, label, it, update)
        centres, label, it = out["centres"], out["label"], out["iterations"]
        if update and not converged and out["changed"] == 0:
            converged = it
    return dict(out, seed_index=index, converged_at=converged)


def blobs(seed_, N, D, k):
    """The fixture data of the kernel tests: min(k, 6) planted centres randn*2, noise 0.35*randn, cast to fp32; and the k
    uniforms RandomState(100 + seed).rand(k)."""
    rs = np.random.RandomState(seed_)
    planted = rs.randn(min(k, 6), D) * 2
    x = (planted[rs.randint(0, planted.shape[0], size=N)] + 0.35 * rs.randn(N, D)).astype(np.float32)
    return x, np.random.RandomState(100 + seed_).rand(k)
