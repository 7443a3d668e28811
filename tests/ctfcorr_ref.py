"""float64 numpy restatement of include/svae_ctfcorr.h: the transfer function of each particle on the image's own frequency grid
(built on oracle.ctf_oracle.ctf_2d, the closed form the reference's ctf.py:7-24 states), phase flipping / multiplication in
Fourier space, the per-class sums of H^2 and the Wiener quotient, all with np.fft.  Written from the header's text, not from the
kernels."""
import numpy as np

from oracle import ctf_oracle as C

COLUMN = {name: i for i, name in enumerate(C.COLUMNS)}


def random_table(P, seed):
    """tests/test_gpu_ctf.py's generator: RandomState(seed), defocus 0.8-3.5, voltage 200 or 300, apix 1.0-2.5, B-factor 0-200,
    amplitude contrast 5-15."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(0.8, 3.5, P), np.full(P, 2.7), rs.choice([200.0, 300.0], P), rs.uniform(1.0, 2.5, P),
                     rs.uniform(0, 200, P), rs.uniform(5, 15, P), np.zeros(P), rs.uniform(0, 180, P)], 1)


def transfer(table, n, m, scale=1.0):
    """(H, u), each (P, n, m) float64 in fftfreq order: H_i = -c_i with the B-factor envelope, u_i the oscillating part of c_i
    without it.  Both defoci are defocus*10000 and dfdiff is unused, as in the reference."""
    table = np.asarray(table, np.float64).reshape(-1, 8)
    ty, tx = np.meshgrid(np.fft.fftfreq(n), np.fft.fftfreq(m), indexing="ij")
    freqs = np.stack([ty.ravel(), tx.ravel()], 1)
    H = np.zeros((len(table), n, m))
    u = np.zeros((len(table), n, m))
    for i, row in enumerate(table):
        f = freqs / (row[COLUMN["apix"]] * scale)
        args = (f, row[COLUMN["defocus"]] * 10000, row[COLUMN["defocus"]] * 10000, 2 * np.pi * row[COLUMN["dfang"]] / 360,
                row[COLUMN["voltage"]], row[COLUMN["cs"]], row[COLUMN["ampcont"]] / 100)
        H[i] = -C.ctf_2d(*args, row[COLUMN["bfactor"]]).reshape(n, m)
        u[i] = C.ctf_2d(*args, None).reshape(n, m)
    return H, u


def flip_sign(u):
    """s = (u <= 0) ? +1 : -1: the sign of H = -c taken from the oscillating part."""
    return np.where(u <= 0, 1.0, -1.0)


def apply_ref(y, table, n, m, scale=1.0, mode="flip", dtype=np.float32):
    """y (B, n*m) or (B, n, m) -> Re IDFT(filter_i * DFT(y_i)), (B, n, m), rounded once to `dtype`."""
    y = np.asarray(y).astype(np.float64).reshape(-1, n, m)
    H, u = transfer(table, n, m, scale)
    filt = {"flip": flip_sign(u), "multiply": H}[mode]
    return np.fft.ifft2(filt * np.fft.fft2(y)).real.astype(dtype)


def power_ref(calls, n_classes, n, m, scale=1.0):
    """calls: [(table (B, 8), label (B))] in the order of the update calls -> den (n_classes, n, m) float64, every image added in
    index order; labels outside [0, n_classes) are skipped."""
    den = np.zeros((n_classes, n, m))
    for table, label in calls:
        H, _ = transfer(table, n, m, scale)
        for b, k in enumerate(np.asarray(label)):
            if 0 <= k < n_classes:
                den[k] = den[k] + H[b] * H[b]
    return den


def finish_ref(total, den, lam, n, m, dtype=np.float32):
    """average[k] = Re IDFT( DFT(sum[k]) / (den[k] + lam) ), a frequency whose den + lam is 0 contributing 0; (n_classes, n, m)."""
    total = np.asarray(total, np.float64).reshape(-1, n, m)
    d = np.asarray(den, np.float64).reshape(-1, n, m) + lam
    F = np.fft.fft2(total)
    G = np.divide(F, d, out=np.zeros_like(F), where=d != 0)
    return np.fft.ifft2(G).real.astype(dtype)


def example_image():
    """The 40 x 40 image of the recovery example: two Gaussian blobs plus 0.05 N(0, 1) from default_rng(0), mean removed."""
    y, x = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij")
    A = np.exp(-((y - 20) ** 2 + (x - 17) ** 2) / 18) - 0.7 * np.exp(-((y - 24) ** 2 + (x - 22) ** 2) / 8)
    A = A + 0.05 * np.random.default_rng(0).standard_normal((40, 40))
    return A - A.mean()

