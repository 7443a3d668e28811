"""Float64-capable restatement of the K-sample latent head in torch ops (autograd gives its backward): shared by
tests/test_gpu_iw_kernels.py and tests/test_gpu_iw_step.py.  Row b*K + k is sample k of image b."""
import math

import torch


def iw_latent_formulas(q_out, r, K, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
    """The reparameterised samples and log p(z) - log q(z|x) per sample in the dtype of q_out, torch ops only.
    q(z|x) = N(mu, std^2); p = N(0, 1) per coordinate, except the rotation: N(0, theta_prior^2) with mu_penalty, else
    N(mu, theta_prior^2).  The log(2 pi)/2 terms cancel."""
    inf = r.shape[1]
    mu, ls = q_out[:, :inf].repeat_interleave(K, 0), q_out[:, inf:].repeat_interleave(K, 0)
    std = torch.exp(ls)
    z = std * r + mu
    log_q = (-ls - r ** 2 / 2).sum(1)
    log_p = torch.zeros(r.shape[0], dtype=q_out.dtype)
    off = 0
    theta = dx = None
    if rotate:
        theta = z[:, 0]
        d = z[:, 0] if mu_penalty else std[:, 0] * r[:, 0]
        log_p = -math.log(theta_prior) - d ** 2 / (2 * theta_prior ** 2)
        off = 1
    c0 = off
    if translate:
        dx = z[:, off:off + 2] * dx_scale
        c0 = off + 2
    log_p = log_p + (-z[:, off:] ** 2 / 2).sum(1)
    return theta, dx, z[:, c0:] * z_scale, log_p - log_q
