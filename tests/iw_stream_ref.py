"""Plain, unchunked evaluation of the streaming K-sample scorer's definitions (include/svae_stream.h) in numpy, from all
samples of an image at once: shared by tests/test_gpu_iw_stream.py and tests/test_infer_cpu.py.  dtype=np.float64 is the
reference, dtype=np.float32 the same definitions in single precision (the tests' error bounds come from the gap between the
two).  Nothing here merges chunks or rescales anything."""
import numpy as np


def wrap(d):
    """An angle difference brought into [-pi, pi)."""
    return (np.asarray(d, np.float64) + np.pi) % (2 * np.pi) - np.pi


def coords(theta, dx, zc, B, K):
    """(B, K, inf_dim) latent coordinates in latent order (rotation, dx0, dx1, content) from the per-sample arrays."""
    parts = []
    if theta is not None:
        parts.append(np.asarray(theta).reshape(B, K, 1))
    if dx is not None:
        parts.append(np.asarray(dx).reshape(B, K, 2))
    if zc is not None and np.asarray(zc).size:
        parts.append(np.asarray(zc).reshape(B, K, -1))
    return np.concatenate(parts, 2)


def iw_stream_ref(loglik, log_ratio, v, rotate, dtype=np.float64):
    """loglik, log_ratio (B, K); v (B, K, inf_dim) = coords(...).  Returns (per_image (B, 6 + 2 inf_dim), out3, weights (B, K))
    in `dtype`: the columns of svae_iw_stream_finish."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ll, lr, v = np.asarray(loglik, dtype), np.asarray(log_ratio, dtype), np.asarray(v, dtype)
        B, K = ll.shape
        inf = v.shape[2]
        a = ll + lr
        M = a.max(1)
        Ms = np.where(np.isfinite(M), M, dtype(0))
        w = np.exp(a - Ms[:, None])
        s, s2 = w.sum(1), (w * w).sum(1)
        dead = s == 0
        safe = np.where(dead, dtype(1), s)
        out = np.zeros((B, 6 + 2 * inf), dtype)
        out[:, 0] = Ms + np.log(s) - dtype(np.log(dtype(K)))
        out[:, 1] = ll.mean(1)
        out[:, 2] = -(lr.mean(1))
        out[:, 3] = np.where(dead, dtype(0), s * s / np.where(dead, dtype(1), s2))
        out[:, 4] = M
        mean = (w[:, :, None] * v).sum(1) / safe[:, None]
        out[:, 5] = 1
        if rotate:
            C, S = (w * np.cos(v[:, :, 0])).sum(1), (w * np.sin(v[:, :, 0])).sum(1)
            out[:, 5] = np.where(dead, dtype(0), np.sqrt(C * C + S * S) / safe)
            mean[:, 0] = np.arctan2(S, C)
        out[:, 6:6 + inf] = np.where(dead[:, None], dtype(0), mean)
        best = np.argmax(a, 1)                      # the first index at the max; 0 when every a is -inf
        out[:, 6 + inf:] = v[np.arange(B), best]
        out3 = np.array([out[:, 0].mean(), ll.mean(), -(lr.mean())], dtype)
        return out, out3, w / safe[:, None]
