"""Helper (not collected): the float64 restatement of include/svae_frc.h with np.fft -- the integer ring rule, the soft mask,
the per-ring sums and the FRC, the weight, the filter by per-ring weights and the resolution -- and the test planes the GPU
tests share.  Nothing here imports the package: the kernels, elbo.py's helpers and infer.py's arrays are all held to it."""
import functools
from fractions import Fraction

import numpy as np


def layout(n, m):
    """(L, R): the shorter side and the number of rings."""
    L = min(n, m)
    return L, L // 2 + 1


def signed(length):
    """fftfreq order as integers: a <= (len-1)/2 ? a : a - len."""
    a = np.arange(length, dtype=np.int64)
    return np.where(a <= (length - 1) // 2, a, a - length)


@functools.lru_cache(maxsize=None)
def ring_index(n, m):
    """(n, m) int64: the largest r >= 1 with (2r-1)^2 (n m)^2 <= 4 ((ku L m)^2 + (kv L n)^2), 0 where there is none, in 64-bit
    integers; entries >= R are in no ring."""
    L, _ = layout(n, m)
    S = 4 * ((signed(n)[:, None] * L * m) ** 2 + (signed(m)[None, :] * L * n) ** 2)
    T = np.int64(n * m) ** 2
    ring = np.zeros((n, m), np.int64)
    r = 1
    while True:
        inside = (2 * r - 1) ** 2 * T <= S
        if not inside.any():
            break
        ring[inside] = r
        r += 1
    ring.setflags(write=False)
    return ring


def ring_index_rational(n, m):
    """The same by brute force on exact rationals: floor(L sqrt((ku/n)^2 + (kv/m)^2) + 1/2) as the largest r with
    (r - 1/2)^2 <= L^2 ((ku/n)^2 + (kv/m)^2)."""
    L, _ = layout(n, m)
    out = np.zeros((n, m), np.int64)
    for u, ku in enumerate(signed(n).tolist()):
        for v, kv in enumerate(signed(m).tolist()):
            rho2 = L * L * (Fraction(ku, n) ** 2 + Fraction(kv, m) ** 2)
            r = 0
            while (Fraction(2 * (r + 1) - 1, 2)) ** 2 <= rho2:
                r += 1
            out[u, v] = r
    return out


def ring_count(n, m):
    _, R = layout(n, m)
    return np.bincount(ring_index(n, m).ravel(), minlength=R)[:R].astype(np.int32)


def mask(n, m, radius, edge):
    """w = 1 for d <= radius, 0.5 (1 + cos(pi (d - radius) / edge)) inside the edge, 0 beyond; d from ((n-1)/2, (m-1)/2);
    radius 0 = no mask."""
    if radius == 0:
        return np.ones((n, m))
    dy = np.arange(n, dtype=np.float64)[:, None] - 0.5 * (n - 1)
    dx = np.arange(m, dtype=np.float64)[None, :] - 0.5 * (m - 1)
    d = np.sqrt(dx * dx + dy * dy)
    w = 0.5 * (1.0 + np.cos(np.pi * ((d - radius) / edge)))
    return np.where(d <= radius, 1.0, np.where(d >= radius + edge, 0.0, w))


def frc(a, b, n, m, radius=0.0, edge=0.0):
    """(sums (P, R, 3) = [num, pa, pb], frc (P, R), ring_count (R) int32) of the planes a, b (P, n, m)."""
    _, R = layout(n, m)
    a = np.asarray(a, np.float64).reshape(-1, n, m)
    b = np.asarray(b, np.float64).reshape(-1, n, m)
    w = mask(n, m, radius, edge)
    FA, FB = np.fft.fft2(w * a), np.fft.fft2(w * b)
    ring = ring_index(n, m).ravel()
    keep = ring < R
    terms = np.stack([(FA * FB.conj()).real, np.abs(FA) ** 2, np.abs(FB) ** 2], -1).reshape(len(a), n * m, 3)
    sums = np.zeros((len(a), R, 3))
    for p in range(len(a)):
        for j in range(3):
            sums[p, :, j] = np.bincount(ring[keep], weights=terms[p, keep, j], minlength=R)
    power = sums[..., 1] * sums[..., 2]
    curve = np.divide(sums[..., 0], np.sqrt(power), out=np.zeros_like(power), where=power != 0)
    return sums, curve, ring_count(n, m)


def weight(curve):
    """sqrt(2 f / (1 + f)) where f > 0, else 0."""
    f = np.asarray(curve, np.float64)
    pos = np.where(f > 0, f, 0.0)
    return np.where(f > 0, np.sqrt(2.0 * pos / (1.0 + pos)), 0.0)


def filter_planes(x, weights, n, m):
    """Re IDFT( weights[p, ring] DFT(x[p]) ), float64; a frequency in no ring contributes 0."""
    _, R = layout(n, m)
    x = np.asarray(x, np.float64).reshape(-1, n, m)
    ring = ring_index(n, m)
    table = np.concatenate([np.asarray(weights, np.float64).reshape(len(x), R), np.zeros((len(x), ring.max() + 1))], 1)
    return np.fft.ifft2(table[:, ring] * np.fft.fft2(x)).real


def resolution(curve, threshold, L):
    """(pixels, never_below): NaN when ring 0 is below the threshold; the linearly interpolated crossing before the first ring
    r >= 1 below it; else L / (R - 1) and True."""
    f = np.asarray(curve, np.float64)
    if not f[0] >= threshold:
        return float("nan"), False
    for r in range(1, len(f)):
        if f[r] < threshold:
            with np.errstate(divide="ignore"):
                return float(np.float64(L) / np.float64((r - 1) + (f[r - 1] - threshold) / (f[r - 1] - f[r]))), False
    return float(L) / (len(f) - 1), True


def default_mask(n, m):
    """The mask the GPU tests and infer.py's defaults use: (max(L/2 - 3, 1), 3)."""
    return max(min(n, m) / 2.0 - 3.0, 1.0), 3.0


def half_planes(seed, n, m, planes):
    """Two half-set planes per plane (read-only, float64): a normal field low-passed by exp(-(f / 0.15)^2 / 2) (f in cycles per
    pixel) and scaled to unit variance, plus independent white noise of 0.35 in each half: every ring keeps noise power."""
    rs = np.random.RandomState(seed)
    f2 = (signed(n)[:, None] / n) ** 2 + (signed(m)[None, :] / m) ** 2
    signal = np.fft.ifft2(np.fft.fft2(rs.normal(size=(planes, n, m))) * np.exp(-0.5 * f2 / 0.15 ** 2)).real
    signal /= signal.std(axis=(1, 2), keepdims=True)
    a = signal + 0.35 * rs.normal(size=(planes, n, m))
    b = signal + 0.35 * rs.normal(size=(planes, n, m))
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def rings_keep_power(sums, counts):
    """The smallest over planes and rings of sqrt(pa pb) / ring_count relative to the plane's largest ring: a condition on the
    reference (no FRC may be a quotient of rounding noise)."""
    per = np.sqrt(sums[..., 1] * sums[..., 2]) / np.maximum(counts, 1)[None]
    return float((per / per.max(1, keepdims=True)).min())
