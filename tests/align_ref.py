"""float64 numpy restatement of include/svae_align.h: the source position of every output pixel, coverage, the bilinear and
Catmull-Rom resamplers in the header's stated order of operations, and the class sums in index order.  Written from the header's
text, not from the kernels; tests/test_align_cpu.py holds it to properties of the geometry it restates."""
import numpy as np

SLACK = 1e-6


def source_positions(theta, dx, B, rows, cols):
    """(fx, fy), each (B, rows, cols): the continuous source column / row of every output pixel, before coverage and clamping.
    theta (B) or None, dx (B, 2) or None; both are taken as given and widened to float64."""
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    jy, jx = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    X, Y = (jx - a)[None], (bq - jy)[None]
    if theta is None:
        c, s = np.ones((B, 1, 1)), np.zeros((B, 1, 1))
    else:
        th = np.asarray(theta).astype(np.float64).reshape(B, 1, 1)
        c, s = np.cos(th), np.sin(th)
    d = np.zeros((B, 2)) if dx is None else np.asarray(dx).astype(np.float64).reshape(B, 2)
    dx0, dx1 = d[:, 0].reshape(B, 1, 1), d[:, 1].reshape(B, 1, 1)
    U = X - a * dx0
    V = Y - bq * dx1
    SX = c * U + s * (a / bq) * V
    SY = -s * (bq / a) * U + c * V
    return SX + a, bq - SY


def covered(fx, fy, rows, cols):
    with np.errstate(invalid="ignore"):
        return (fx >= -SLACK) & (fx <= cols - 1 + SLACK) & (fy >= -SLACK) & (fy <= rows - 1 + SLACK)


def near_threshold(fx, fy, rows, cols, eps=1e-9):
    """Pixels whose source position lies within eps of a coverage threshold (where the device's sin / cos may decide otherwise)."""
    out = np.zeros(fx.shape, bool)
    for f, hi in ((fx, cols - 1 + SLACK), (fy, rows - 1 + SLACK)):
        out |= (np.abs(f + SLACK) <= eps) | (np.abs(f - hi) <= eps)
    return out


def cubic_weights(t):
    t2 = t * t
    t3 = t2 * t
    return [(-t3 + 2.0 * t2 - t) / 2.0, (3.0 * t3 - 5.0 * t2 + 2.0) / 2.0, (-3.0 * t3 + 4.0 * t2 + t) / 2.0, (t3 - t2) / 2.0]


def align_ref(y, theta, dx, rows, cols, interp="bicubic", dtype=np.float32):
    """y (B, rows*cols[, C]) -> (aligned (B, rows*cols, C) rounded once to `dtype`, cover (B, rows*cols) uint8)."""
    y = np.asarray(y)
    B = y.shape[0]
    img = y.astype(np.float64).reshape(B, rows, cols, -1)
    C = img.shape[3]
    fx, fy = source_positions(theta, dx, B, rows, cols)
    cov = covered(fx, fy, rows, cols)
    fx = np.where(cov, np.minimum(np.maximum(fx, 0.0), cols - 1.0), 0.0)
    fy = np.where(cov, np.minimum(np.maximum(fy, 0.0), rows - 1.0), 0.0)
    i0 = np.minimum(np.floor(fx).astype(np.int64), cols - 2)
    j0 = np.minimum(np.floor(fy).astype(np.int64), rows - 2)
    tx, ty = (fx - i0)[..., None], (fy - j0)[..., None]
    bi = np.arange(B).reshape(B, 1, 1)

    def sample(jj, ii):
        return img[bi, jj, ii]                                       # (B, rows, cols, C)

    if interp == "bilinear":
        r0 = (1.0 - tx) * sample(j0, i0) + tx * sample(j0, i0 + 1)
        r1 = (1.0 - tx) * sample(j0 + 1, i0) + tx * sample(j0 + 1, i0 + 1)
        v = (1.0 - ty) * r0 + ty * r1
    elif interp == "bicubic":
        wx, wy = cubic_weights(tx), cubic_weights(ty)
        xc = [np.clip(i0 - 1 + k, 0, cols - 1) for k in range(4)]
        v = None
        for r in range(4):
            yy = np.clip(j0 - 1 + r, 0, rows - 1)
            row = wx[0] * sample(yy, xc[0]) + wx[1] * sample(yy, xc[1]) + wx[2] * sample(yy, xc[2]) + wx[3] * sample(yy, xc[3])
            v = wy[0] * row if r == 0 else v + wy[r] * row
    else:
        raise ValueError(interp)
    v = np.where(cov[..., None], v, 0.0)
    return v.astype(dtype).reshape(B, rows * cols, C), cov.astype(np.uint8).reshape(B, rows * cols)


def class_sums_ref(calls, n_classes, N, C):
    """calls: [(aligned (B, N, C), cover (B, N) or None, label (B))], in the order of the update calls -> (sum (n_classes, N, C),
    count (n_classes, N)), float64, every image added in index order."""
    total = np.zeros((n_classes, N, C), np.float64)
    count = np.zeros((n_classes, N), np.float64)
    for aligned, cover, label in calls:
        aligned = np.asarray(aligned).reshape(len(label), N, C)
        for b, k in enumerate(np.asarray(label)):
            if not 0 <= k < n_classes:
                continue
            on = np.ones(N, bool) if cover is None else np.asarray(cover).reshape(len(label), N)[b] != 0
            total[k][on] = total[k][on] + aligned[b][on].astype(np.float64)
            count[k][on] = count[k][on] + 1.0
    return total, count
