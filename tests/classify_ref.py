"""float64 numpy restatement of include/svae_classify.h on top of tests/refine_ref.py: the candidate scores are the winning
scores of refine_ref.pose_search slot by slot (-infinity where that search skips), the winner is the first maximum under strict
`>`, the margin its lead over the best other live slot.  Written from the header's text, not from the kernel.  Also the
planted-truth case of the classification tests: three analytic classes built on refine_ref's blobs.
tests/test_classify_cpu.py holds it to properties of what it restates."""
import numpy as np

import refine_ref as R


def pose_classify(y, ref, weight, cand, pose_in, rows, cols, A, step, S, interp="bicubic"):
    """{"choice" (B) int32, "ref_chosen" (B) int32, "cand_score" (B, M) float64, "margin" (B) float64}."""
    cand = np.asarray(cand, dtype=np.int32)
    B, M = cand.shape
    score = np.full((B, M), -np.inf)
    for j in range(M):
        found = R.pose_search(y, ref, weight, cand[:, j], pose_in, rows, cols, A, step, S, interp)
        live = found["offset"][:, 3] & R.SKIPPED == 0
        score[live, j] = found["score"][live]
    out = {"choice": np.full(B, -1, np.int32), "ref_chosen": np.full(B, -1, np.int32), "cand_score": score, "margin": np.full(B, np.inf)}
    for b in range(B):
        best, top = -1, -np.inf
        for j in range(M):
            if score[b, j] > top:
                best, top = j, score[b, j]
        if best < 0:
            continue
        out["choice"][b], out["ref_chosen"][b] = best, cand[b, best]
        others = np.delete(score[b], best)
        others = others[others > -np.inf]
        if others.size:
            out["margin"][b] = top - others.max()
    return out


# ---------------------------------------------------------------- the planted-truth case
# Three distinct classes: refine_ref.BLOBS, its mirror in x (every centre's x negated: the ring of five has no mirror symmetry,
# so no rotation undoes it), and BLOBS with the amplitudes of blobs 1 and 3 set to 0.
def class_tables():
    mirror = R.BLOBS.copy()
    mirror[:, 0] = -mirror[:, 0]
    fewer = R.BLOBS.copy()
    fewer[[1, 3], 3] = 0.0
    return [R.BLOBS, mirror, fewer]


def class_image(table, px, py):
    """refine_ref.blobs for another table of blobs."""
    out = np.zeros(np.broadcast(px, py).shape)
    for x0, y0, sigma, amp in table:
        out = out + amp * np.exp(-((px - x0) ** 2 + (py - y0) ** 2) / (2.0 * sigma * sigma))
    return out


PLANTED = dict(rows=24, cols=24, A=R.RECOVERY["A"], step=R.RECOVERY["step"], S=R.RECOVERY["S"], seed=300,
               true=np.array([0, 1, 2, 1, 2, 0, 2, 0, 1, 0, 1, 2], np.int32))


def planted_case():
    """Twelve images, four of each class, posed as refine_ref.posed_blobs poses its image (evaluated exactly, no resampling, no
    noise) with the start poses perturbed as refine_ref.recovery_case perturbs them (within 2.8 steps and 2 pixels); every third
    image carries a wrong starting label (the next class).  Returns (y (12, N, 1) float32, ref (3, N, 1) float64: the canonical
    image of each class, true (12) int32, start_label (12) int32, pose_start (12, 3) float32)."""
    rows, cols, step = PLANTED["rows"], PLANTED["cols"], PLANTED["step"]
    true = PLANTED["true"]
    n = len(true)
    rs = np.random.RandomState(PLANTED["seed"])
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    theta = rs.uniform(-np.pi, np.pi, n)
    dx = rs.uniform(-0.12, 0.12, (n, 2))
    pose = np.concatenate([theta[:, None], dx], 1).astype(np.float32)
    start = pose.astype(np.float64)
    start[:, 0] += rs.uniform(-2.8, 2.8, n) * step
    start[:, 1] += rs.uniform(-2.0, 2.0, n) / a
    start[:, 2] += rs.uniform(-2.0, 2.0, n) / bq
    tables = class_tables()
    gx, gy = R.grid(rows, cols)
    y = []
    for i in range(n):
        t, d = float(pose[i, 0]), pose[i, 1:].astype(np.float64)
        c, s = np.cos(t), np.sin(t)
        y.append(class_image(tables[true[i]], c * gx - s * gy + d[0], s * gx + c * gy + d[1]))
    y = np.stack(y).reshape(n, rows * cols, 1).astype(np.float32)
    ref = np.stack([class_image(t, gx, gy) for t in tables]).reshape(3, rows * cols, 1)
    label = true.copy()
    label[::3] = (label[::3] + 1) % 3
    return y, ref, true, label, start.astype(np.float32)
