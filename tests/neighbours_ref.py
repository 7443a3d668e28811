"""The float64 numpy restatement of include/svae_neighbours.h: what svae_nbr_search and svae_nbr_average are held to, bit for bit
where only subtraction, multiplication and addition are involved.  Every sum is an explicit loop in the header's order (np.sum
adds pairwise and is not the contract)."""
import numpy as np

MAX_K = 256
MAX_T = MAX_K + 1


def empty_lists(B, K):
    """(best_d2, best_index) filled with the empty slot (+inf, -1)."""
    return np.full((B, K), np.inf), np.full((B, K), -1, np.int64)


def sqdist(query, cand):
    """d2 (B, M): the sum over j in index order onto +0 of t * t, t = query[b, j] - cand[c, j]."""
    query, cand = np.asarray(query, np.float64), np.asarray(cand, np.float64)
    d2 = np.zeros((query.shape[0], cand.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(query.shape[1]):
            t = query[:, j, None] - cand[None, :, j]
            d2 = d2 + t * t
    return d2


def search(query, query_base, cand, cand_base, best_d2, best_index):
    """One svae_nbr_search call: returns the new (best_d2, best_index); the arguments are not changed."""
    B, K = best_index.shape
    d2 = sqdist(query, cand)
    out_d, out_i = empty_lists(B, K)
    for b in range(B):
        entries = [(float(d), int(i)) for d, i in zip(best_d2[b], best_index[b]) if i >= 0]
        for c in range(cand.shape[0]):
            if cand_base + c != query_base + b and np.isfinite(d2[b, c]):
                entries.append((float(d2[b, c]), cand_base + c))
        entries.sort()                      # the total order (d2, index)
        for p, (d, i) in enumerate(entries[:K]):
            out_d[b, p], out_i[b, p] = d, i
    return out_d, out_i


def search_all(latents, K, chunks=None, query_chunks=None):
    """The lists of all images against all images: the candidates offered in the (lo, hi) `chunks`, in that order, to the
    queries of each of `query_chunks`."""
    images = latents.shape[0]
    chunks = chunks or [(0, images)]
    query_chunks = query_chunks or [(0, images)]
    best_d2, best_index = empty_lists(images, K)
    for qlo, qhi in query_chunks:
        for lo, hi in chunks:
            best_d2[qlo:qhi], best_index[qlo:qhi] = search(latents[qlo:qhi], qlo, latents[lo:hi], lo, best_d2[qlo:qhi], best_index[qlo:qhi])
    return best_d2, best_index


def brute_force(latents, K):
    """A full sort of the (d2, index) tuples of every row: what the running lists must end as."""
    images = latents.shape[0]
    d2 = sqdist(latents, latents)
    out_d, out_i = empty_lists(images, K)
    for b in range(images):
        row = sorted((float(d2[b, c]), c) for c in range(images) if c != b and np.isfinite(d2[b, c]))
        for p, (d, i) in enumerate(row[:K]):
            out_d[b, p], out_i[b, p] = d, i
    return out_d, out_i


def ties_at_cut(latents, K):
    """Per row: (has tied distances, the cut after K entries falls inside a tie)."""
    images = latents.shape[0]
    d2 = sqdist(latents, latents)
    tied, cut = np.zeros(images, bool), np.zeros(images, bool)
    for b in range(images):
        row = sorted(float(d2[b, c]) for c in range(images) if c != b)
        tied[b] = len(set(row)) < len(row)
        cut[b] = len(row) > K and row[K - 1] == row[K]
    return tied, cut


def average(stack, cover, index, weight=None):
    """svae_nbr_average: (average (B, N, C) float32, support (B, N) float64, exact (B, N, C) float64 the unrounded quotient,
    +0 where den is not positive)."""
    stack = np.asarray(stack, np.float32)
    images, N, C = stack.shape
    B, T = index.shape
    wide = stack.astype(np.float64)
    num, den = np.zeros((B, N, C)), np.zeros((B, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for t in range(T):
                i = int(index[b, t])
                if i < 0 or i >= images:
                    continue
                w = 1.0 if weight is None else float(weight[b, t])
                on = np.ones(N, bool) if cover is None else cover[i] != 0
                num[b, on] = num[b, on] + w * wide[i, on]
                den[b, on] = den[b, on] + w
        positive = den > 0
        exact = np.where(positive[:, :, None], num / np.where(positive, den, 1.0)[:, :, None], 0.0)
        return exact.astype(np.float32), den, exact


def within_one_float(got, exact):
    """Per value: `got` (float32) is the float32 nearest to `exact` or one of that float's two float32 neighbours (NaN matches
    NaN).  Returns (ok, identical)."""
    with np.errstate(invalid="ignore", over="ignore"):
        want = exact.astype(np.float32)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    near = (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))
    return same | near, same


def gaussian_weights(sqd, index, exclude_self=False):
    """The weights neighbours.py stores under --weights gaussian: slot 0 (the image itself) 1, a listed neighbour
    exp(-d2 / (2 s2)) with s2 the row's largest listed d2, and 1 wherever the slot is empty or s2 is 0."""
    images, K = index.shape
    w = np.ones((images, K + 1))
    for b in range(images):
        valid = index[b] >= 0
        if valid.any():
            s2 = sqd[b][valid].max()
            if s2 > 0:
                w[b, 1:][valid] = np.exp(-sqd[b][valid] / (2.0 * s2))
    return w


def lattice(seed=0, images=150, D=2, span=3):
    """Integer-lattice latents in -span..span: every row has tied distances."""
    return np.random.RandomState(seed).randint(-span, span + 1, size=(images, D)).astype(np.float64)
