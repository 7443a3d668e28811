"""Float64 CPU restatements of the operations behind the decoder -- the likelihoods, the latent head, the minibatch means --
and the seeded inputs tests/test_gpu_loss_head.py and its child process tests/loss_head_child.py share.  Plain numpy / torch
double: these state the OPERATION (zero-padded cross-correlation as a sum of shifted images, its adjoint as the transposed
scatter, the formulas of train_particles.py:102-139 and train_mnist.py:33-86), not how a kernel walks it."""
import numpy as np
import torch

import cases

U = 2.0 ** -24          # unit roundoff of fp32

# (n, k) of the CTF likelihood cases and what each one reaches in gaussian_ctf_lds_kernel / svae_gaussian_loglik
CTF_PAIRS = [(1, 1), (1, 3), (7, 1), (5, 5), (9, 9), (10, 9), (13, 3), (6, 11), (8, 7), (41, 41), (56, 55), (80, 79), (88, 87)]
CTF_BOTH_FORMS = [(5, 5), (10, 9), (41, 41), (56, 55)]
CTF_B = 2


def ctf_lds_bytes(n, k):
    """Dynamic LDS svae_gaussian_loglik asks for at (n, k): CtfLds::make's padded image plus the padded filter."""
    pad = k // 2
    W = n + 2 * pad
    kp = (k + 3) & ~3
    M = 3 + ((4 - ((2 * pad) & 3)) & 3)
    Wp = ((W + M + 3) & ~3) + 8
    return (W * Wp + k * kp) * 4


def ctf_form(n, k):
    """Which launch svae_gaussian_loglik picks with SVAE_CTF_LDS unset: 'lds', 'lds_attr' (above the 48 KB a kernel gets
    without hipFuncSetAttribute) or 'global' (above the 150 KB cut)."""
    b = ctf_lds_bytes(n, k)
    return "global" if b > 150 * 1024 else ("lds_attr" if b > 48 * 1024 else "lds")


def xcorr(img, f):
    """out[b, r, c] = sum_{u, v} img0[b, r + u - pad, c + v - pad] f[b, u, v] with img0 = img zero-extended (F.conv2d with
    padding k // 2 and groups = B, train_particles.py:112-119).  img (B, n, n), f (B, k, k), in their own dtype."""
    B, n, _ = img.shape
    k = f.shape[-1]
    pad = k // 2
    P = np.zeros((B, n + 2 * pad, n + 2 * pad), img.dtype)
    P[:, pad:pad + n, pad:pad + n] = img
    out = np.zeros_like(img)
    for u in range(k):
        for v in range(k):
            out += P[:, u:u + n, v:v + n] * f[:, u, v][:, None, None]
    return out


def xcorr_adjoint(d, f):
    """The transpose of xcorr in its first argument: every output pixel's gradient is scattered back over the window it read."""
    B, n, _ = d.shape
    k = f.shape[-1]
    pad = k // 2
    P = np.zeros((B, n + 2 * pad, n + 2 * pad), d.dtype)
    for u in range(k):
        for v in range(k):
            P[:, u:u + n, v:v + n] += d * f[:, u, v][:, None, None]
    return P[:, pad:pad + n, pad:pad + n].copy()


def gaussian64(y_params, target, mask=None, ctf=None):
    """Per-image Gaussian log-likelihood and d(loglik_b)/d(y_params) in float64 (train_particles.py:102-139): the first N
    entries of a row are the mean, the last N (when there are 2 N) the log-variance; ctf (B, k, k) filters the mean image;
    the sum runs over the pixels of `mask`.  Also returns the intermediates the exactness argument needs."""
    y = np.asarray(y_params, np.float64)
    t = np.asarray(target, np.float64)
    B, N = t.shape
    on = np.ones(N, bool) if mask is None else np.asarray(mask, bool)
    mu = y[:, :N]
    n = int(round(np.sqrt(N)))
    f = None if ctf is None else np.asarray(ctf, np.float64).reshape(B, ctf.shape[-1], ctf.shape[-1])
    if f is not None:
        mu = xcorr(mu.reshape(B, n, n), f).reshape(B, N)
    diff = (mu - t) * on
    dll = np.zeros_like(y)
    if y.shape[1] > N:
        lv = y[:, N:]
        ll = -0.5 * ((diff * diff / np.exp(lv) + lv) * on).sum(1)
        dmu = -diff / np.exp(lv)
        dll[:, N:] = -0.5 * (1.0 - diff * diff * np.exp(-lv)) * on
    else:
        ll = -0.5 * (diff * diff).sum(1)
        dmu = -diff
    dll[:, :N] = dmu if f is None else xcorr_adjoint(dmu.reshape(B, n, n), f).reshape(B, N)
    return dict(loglik=ll, dll=dll, filt=mu, diff=diff, dmu=dmu)


def ctf_mask(n, masked):
    return cases.circular_mask(n, n) if masked else None


def ctf_inputs_random(n, k, B=CTF_B):
    """Normal image and target, filter normal / k plus a unit centre tap (cases.build_inputs)."""
    rs = np.random.RandomState(7000 + 97 * n + k)
    img = rs.normal(size=(B, n * n)).astype(np.float32)
    tgt = rs.normal(size=(B, n * n)).astype(np.float32)
    f = rs.normal(size=(B, k, k)) / k
    f[:, k // 2, k // 2] += 1.0
    return img, tgt, f.astype(np.float32)


def ctf_inputs_integer(n, k, B=CTF_B):
    """Image and target in {-1, 0, 1}; filter taps in {-1, 0, 1}: every tap drawn for k <= 13, above that the border rows and
    columns (where a misplaced margin shows) drawn in full and the interior at a density of 200 / k^2, so that the sums stay
    far inside fp32's exact integers.  The four corner taps are fixed to (1, -1; 1, -1): unequal under a transpose and under
    a half turn, so a mirrored or transposed filter cannot reproduce the result."""
    rs = np.random.RandomState(8000 + 97 * n + k)
    img = rs.randint(-1, 2, size=(B, n * n)).astype(np.float32)
    tgt = rs.randint(-1, 2, size=(B, n * n)).astype(np.float32)
    f = rs.randint(-1, 2, size=(B, k, k)).astype(np.float32)
    if k > 13:
        keep = rs.uniform(size=(B, k, k)) < 200.0 / (k * k)
        keep[:, [0, -1], :] = True
        keep[:, :, [0, -1]] = True
        f *= keep
    if k > 1:
        f[:, 0, 0], f[:, 0, -1], f[:, -1, 0], f[:, -1, -1] = 1.0, -1.0, 1.0, -1.0
    return img, tgt, f


def ctf_inputs_one_hot(n, k):
    """Five images, a single 1 at each corner and at the centre; every tap of the filter a different small integer."""
    img = np.zeros((5, n, n), np.float32)
    for b, (r, c) in enumerate([(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, n // 2)]):
        img[b, r, c] = 1.0
    f = np.broadcast_to(np.arange(1, k * k + 1, dtype=np.float32).reshape(1, k, k), (5, k, k)).copy()
    return img.reshape(5, n * n), np.zeros((5, n * n), np.float32), f


def assert_fp32_exact(ref, ctf):
    """Every number an fp32 evaluation of `ref`'s case forms, in ANY summation order, is exact: inputs and taps are integers,
    so products and partial sums are integers (half-integers in the log-likelihood) bounded by the sums of absolute values
    checked here -- integers below 2^24 and multiples of 1/2 below 2^23 are fp32 numbers."""
    B, N = ref["diff"].shape
    n = int(round(np.sqrt(N)))
    f = np.abs(np.asarray(ctf, np.float64)).reshape(B, ctf.shape[-1], ctf.shape[-1])
    for name in ("filt", "diff", "dmu", "dll"):
        assert np.array_equal(ref[name], np.round(ref[name])), name
    assert np.array_equal(2 * ref["loglik"], np.round(2 * ref["loglik"]))
    assert f.sum((1, 2)).max() < 2.0 ** 24                                   # |any partial sum of the forward filter| (|image| <= 1)
    assert (np.abs(ref["diff"]) ** 2).max() < 2.0 ** 24
    assert 0.5 * (ref["diff"] ** 2).sum(1).max() < 2.0 ** 23                 # same-sign terms: no partial sum exceeds the total
    assert xcorr_adjoint(np.abs(ref["dmu"]).reshape(B, n, n), f).max() < 2.0 ** 24


def bce64(y_hat, target):
    """Per-image Bernoulli log-likelihood of fp32 values, in float64, with F.binary_cross_entropy's clamps at -100."""
    s = np.asarray(y_hat, np.float64).reshape(len(y_hat), -1)
    t = np.asarray(target, np.float64).reshape(len(y_hat), -1)
    with np.errstate(divide="ignore"):
        return (t * np.maximum(np.log(s), -100.0) + (1.0 - t) * np.maximum(np.log1p(-s), -100.0)).sum(1)


def bce_dll64(y_hat, target):
    """-(s - t) / max((1 - s) s, 1e-12): the denominator formed in fp32 (two roundings, as the kernels form it: whether it
    falls below the 1e-12 floor is decided there), everything else in float64."""
    s = np.asarray(y_hat, np.float32)
    t = np.asarray(target, np.float32)
    den = np.maximum((np.float32(1) - s) * s, np.float32(1e-12)).astype(np.float64)
    return -(s.astype(np.float64) - t.astype(np.float64)) / den


def latent_formulas(q_out, r, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
    """train_mnist.py:33-86 (mu_penalty: the mu^2 term of :63; z_scale as train_galaxy.py) in the dtype of q_out, torch ops
    only, so that autograd gives d/d(q_out).  Returns (theta | None, dx | None, z_content, kl_per_image)."""
    inf = r.shape[1]
    z_mu, z_logstd = q_out[:, :inf], q_out[:, inf:]
    z_std = torch.exp(z_logstd)
    z = z_std * r + z_mu
    kl = torch.zeros(r.shape[0], dtype=q_out.dtype)
    off = 0
    theta = dx = None
    if rotate:
        theta = z[:, 0]
        sigma = theta_prior
        kl = -z_logstd[:, 0] + float(np.log(sigma)) + z_std[:, 0] ** 2 / 2 / sigma ** 2 - 0.5
        if mu_penalty:
            kl = kl + z_mu[:, 0] ** 2 / 2 / sigma ** 2
        off = 1
    c0 = off
    if translate:
        dx = z[:, off:off + 2] * dx_scale
        c0 = off + 2
    zc = z[:, c0:] * z_scale
    kl = kl + (-z_logstd[:, off:] + 0.5 * z_std[:, off:] ** 2 + 0.5 * z_mu[:, off:] ** 2 - 0.5).sum(1)
    return theta, dx, zc, kl
