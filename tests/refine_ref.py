"""float64 numpy restatement of include/svae_refine.h on top of tests/align_ref.py (dtype=np.float64: the candidates are not
rounded to float): the candidate planes, their shifted images, the normalised scores, the first-maximum winner, the three
parabolas and the skip rules.  Written from the header's text, not from the kernel; every sum here is numpy's, so the device
agrees to rounding and not bit for bit.  tests/test_refine_cpu.py holds it to properties of what it restates."""
import numpy as np

import align_ref as AR

EDGE_ANGLE, EDGE_SHIFT, SKIPPED = 1, 2, 4


def candidate_planes(y, pose, rows, cols, A, step, interp):
    """P (B, 2A+1, rows, cols, C) float64: image b in the canonical frame at (theta + k step, dx0, dx1), k = -A..A."""
    y = np.asarray(y)
    B = y.shape[0]
    pose = np.asarray(pose).astype(np.float64).reshape(B, 3)
    step = float(step) if A > 0 else 0.0
    out = []
    for k in range(-A, A + 1):
        theta_k = pose[:, 0] + float(k) * step
        plane, _ = AR.align_ref(y, theta_k, pose[:, 1:], rows, cols, interp, dtype=np.float64)
        out.append(plane.reshape(B, rows, cols, -1))
    return np.stack(out, 1)


def shifted(P, sx, sy):
    """Q[..., jy, jx, :] = P[..., jy + sy, jx - sx, :] inside the box, 0 outside; P (..., rows, cols, C)."""
    rows, cols = P.shape[-3], P.shape[-2]
    Q = np.zeros_like(P)
    y0, y1 = max(0, -sy), min(rows, rows - sy)
    x0, x1 = max(0, sx), min(cols, cols + sx)
    if y0 < y1 and x0 < x1:
        Q[..., y0:y1, x0:x1, :] = P[..., y0 + sy:y1 + sy, x0 - sx:x1 - sx, :]
    return Q


def parabola(l, c, r):
    d = l - 2.0 * c + r
    if not d < 0.0:
        return 0.0
    return float(min(max(0.5 * (l - r) / d, -0.5), 0.5))


def pose_search(y, ref, weight, ref_index, pose_in, rows, cols, A, step, S, interp="bicubic"):
    """{"pose" (B, 3) float32, "score" (B) float64, "offset" (B, 4) int32 = k, sx, sy, flags, "scores" (B, 2A+1, 2S+1, 2S+1)
    float64 indexed [k + A, sy + S, sx + S], "margin" (B) float64: the winner's score minus the largest of the others (inf for
    a volume of one entry or a skipped image)}."""
    y = np.asarray(y)
    B = y.shape[0]
    pose_in = np.asarray(pose_in, dtype=np.float32).reshape(B, 3)
    ref = np.asarray(ref, dtype=np.float64)
    n_ref = ref.shape[0]
    ref = ref.reshape(n_ref, rows, cols, -1)
    w = np.ones((rows, cols)) if weight is None else np.asarray(weight, dtype=np.float64).reshape(rows, cols)
    nA, nS = 2 * A + 1, 2 * S + 1
    step = float(step) if A > 0 else 0.0
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    out = {"pose": pose_in.copy(), "score": np.zeros(B), "offset": np.zeros((B, 4), np.int32),
           "scores": np.zeros((B, nA, nS, nS)), "margin": np.full(B, np.inf)}
    for b in range(B):
        r = int(ref_index[b])
        p = pose_in[b].astype(np.float64)
        skip = not 0 <= r < n_ref or not np.isfinite(p).all()
        if not skip:
            wr = w[..., None] * ref[r]
            ref_sq = float((wr * wr).sum())
            skip = ref_sq == 0.0
        if not skip:
            P = candidate_planes(y[b:b + 1], pose_in[b:b + 1], rows, cols, A, step, interp)[0]
            vol = out["scores"][b]
            for ik in range(nA):
                p_sq = float((P[ik] * P[ik]).sum())
                denom = np.sqrt(ref_sq) * np.sqrt(p_sq)
                for iy in range(nS):
                    for ix in range(nS):
                        num = float((wr * shifted(P[ik], ix - S, iy - S)).sum())
                        vol[ik, iy, ix] = 0.0 if p_sq == 0.0 else num / denom
            best, top = -1, -np.inf
            flat = vol.reshape(-1)
            for i in range(flat.shape[0]):
                if flat[i] > top:
                    best, top = i, flat[i]
            skip = best < 0
        if skip:
            out["offset"][b, 3] = SKIPPED
            continue
        ik, iy, ix = np.unravel_index(best, vol.shape)
        flags, fk, fx, fy = 0, 0.0, 0.0, 0.0
        if 0 < ik < nA - 1:
            fk = parabola(vol[ik - 1, iy, ix], top, vol[ik + 1, iy, ix])
        elif nA > 1:
            flags |= EDGE_ANGLE
        if 0 < ix < nS - 1:
            fx = parabola(vol[ik, iy, ix - 1], top, vol[ik, iy, ix + 1])
        elif nS > 1:
            flags |= EDGE_SHIFT
        if 0 < iy < nS - 1:
            fy = parabola(vol[ik, iy - 1, ix], top, vol[ik, iy + 1, ix])
        elif nS > 1:
            flags |= EDGE_SHIFT
        k, sx, sy = int(ik) - A, int(ix) - S, int(iy) - S
        out["pose"][b] = np.array([p[0] + (k + fk) * step, p[1] + (sx + fx) / a, p[2] + (sy + fy) / bq]).astype(np.float32)
        out["score"][b] = top
        out["offset"][b] = (k, sx, sy, flags)
        others = np.delete(flat, best)
        if others.size:
            with np.errstate(invalid="ignore"):
                out["margin"][b] = top - np.nanmax(others) if not np.isnan(others).all() else np.inf
    return out


# ---------------------------------------------------------------- the analytic image of the recovery tests
# x, y, sigma, amplitude: five off-centre Gaussians on the [-1, 1] grid, spread around the centre at radii 0.40 .. 0.50 and at
# irregular angles (10, 85, 150, 220, 300 degrees) with comparable amplitudes.  Spread matters: a rotation moves each blob
# tangentially and a shift moves all of them alike, so the half-pixel residue of the integer shifts cannot pass for a rotation
# (with one dominant blob at radius 5 pixels it can, for up to 0.5 / 5 rad = 1.4 steps of 4 degrees).
BLOBS = np.array([
    [0.4432, 0.0781, 0.16, 1.0],
    [0.0349, 0.3985, 0.18, 0.9],
    [-0.433, 0.25, 0.15, 1.1],
    [-0.3217, -0.27, 0.2, 0.8],
    [0.24, -0.4157, 0.17, 1.0],
])


def blobs(px, py):
    out = np.zeros(np.broadcast(px, py).shape)
    for x0, y0, sigma, amp in BLOBS:
        out = out + amp * np.exp(-((px - x0) ** 2 + (py - y0) ** 2) / (2.0 * sigma * sigma))
    return out


def grid(rows, cols):
    """(gx, gy), each (rows, cols): column jx -> -1 + 2 jx/(cols-1), row jy -> 1 - 2 jy/(rows-1), y up (svae_align.h)."""
    jy, jx = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    return -1.0 + 2.0 * jx / (cols - 1), 1.0 - 2.0 * jy / (rows - 1)


def posed_blobs(theta, dx, rows, cols):
    """The observed images (B, rows*cols, 1) float32 of the blobs at the poses (theta (B), dx (B, 2)): the analytic image
    evaluated exactly at grid @ [[cos t, sin t], [-sin t, cos t]] + dx -- no resampling, no noise."""
    gx, gy = grid(rows, cols)
    out = []
    for t, d in zip(np.asarray(theta, dtype=np.float64), np.asarray(dx, dtype=np.float64)):
        c, s = np.cos(t), np.sin(t)
        out.append(blobs(c * gx - s * gy + d[0], s * gx + c * gy + d[1]))
    return np.stack(out).reshape(len(out), rows * cols, 1).astype(np.float32)


def canonical_blobs(rows, cols):
    return blobs(*grid(rows, cols)).reshape(1, rows * cols, 1)


RECOVERY_BOXES = ((24, 24), (17, 17), (17, 13))
RECOVERY = dict(A=6, step=np.deg2rad(4.0), S=3, draws=6)


def recovery_case(rows, cols, seed):
    """`draws` poses for one box: the truth, and a start within 2.8 steps and 2 pixels of it.  Returns (y, ref, pose_true,
    pose_start), the poses (draws, 3) float32."""
    rs = np.random.RandomState(seed)
    n, step = RECOVERY["draws"], RECOVERY["step"]
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    theta = rs.uniform(-np.pi, np.pi, n)
    dx = rs.uniform(-0.12, 0.12, (n, 2))
    true = np.concatenate([theta[:, None], dx], 1).astype(np.float32)
    start = true.astype(np.float64)
    start[:, 0] += rs.uniform(-2.8, 2.8, n) * step
    start[:, 1] += rs.uniform(-2.0, 2.0, n) / a
    start[:, 2] += rs.uniform(-2.0, 2.0, n) / bq
    y = posed_blobs(true[:, 0].astype(np.float64), true[:, 1:].astype(np.float64), rows, cols)
    return y, canonical_blobs(rows, cols), true, start.astype(np.float32)


def recovery_errors(pose, true, rows, cols):
    """(angle errors in steps, shift errors in pixels: the larger of the two axes), each (draws)."""
    a, bq = (cols - 1) / 2.0, (rows - 1) / 2.0
    d = pose.astype(np.float64) - true.astype(np.float64)
    return np.abs(d[:, 0]) / RECOVERY["step"], np.maximum(np.abs(d[:, 1]) * a, np.abs(d[:, 2]) * bq)
