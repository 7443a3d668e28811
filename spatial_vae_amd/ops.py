"""torch.autograd plumbing around the C-ABI (include/svae.h).

PyTorch is used here for device memory, the current HIP stream and the autograd graph only; all
arithmetic of the decoder path happens in the HIP library.  There is deliberately NO fallback:
CPU tensors or a missing library raise.
"""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

DecoderSpec = namedtuple("DecoderSpec", "latent_dim hidden_dim n_out num_layers act softplus resid expand_coords bilinear")

_ws_cache = {}


def _require_hip(t, what):
    if not t.is_cuda:
        raise RuntimeError("spatial_vae_amd: %s must live on a HIP device (got %s); the MI355X path has no CPU "
                           "fallback" % (what, t.device))


def _buf(device, nbytes, key):
    """Grow-only scratch buffer per (device, stream, key); 256-byte aligned by the caching allocator.  Keyed by the current
    stream: the library's scratch may be reused as soon as the call's work has completed ON ITS STREAM, so two streams must
    not share one."""
    k = (device, torch.cuda.current_stream(device).cuda_stream, key)
    t = _ws_cache.get(k)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[k] = t
    return t


def _workspace(entry, key, device, *geometry, required=False):
    """(ws, ws_bytes) for the entry point `entry`: what its <entry>_workspace_bytes asks for that geometry, in the grow-only
    buffer `key`.  Where it asks for nothing ws is None; with `required` there is a buffer all the same, and a `required` that is
    a message is raised instead (0 then means a geometry the library refuses)."""
    ws_bytes = getattr(_lib.lib(), entry + "_workspace_bytes")(*geometry)
    if not ws_bytes and isinstance(required, str):
        raise RuntimeError(required)
    return (_buf(device, ws_bytes, key) if ws_bytes or required else None), ws_bytes


def _hip_device(who, device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("spatial_vae_amd: %s must live on a HIP device (got %s); the MI355X path has no CPU "
                           "fallback" % (who, device))
    return device


def _points(who, points, D):
    _require_hip(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2 or points.size(1) != D or not points.is_contiguous():
        raise RuntimeError("%s: points must be a contiguous (N, %d) float32 tensor, got %s %s"
                           % (who, D, tuple(points.shape), points.dtype))


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


# per entry point, the positions of its device-pointer arguments (the trailing stream aside): what _call takes tensors for
_POINTER_ARGS = {name: tuple(i for i, t in enumerate(argtypes[:-1]) if t is _lib.vp)
                 for name, (_, argtypes) in _lib.ALL_SIGNATURES.items()}


def _call(name, device, *args):
    """Run the status-returning entry point `name` of include/svae.h on `device` and its current stream (the header's last
    argument, appended here).  Where the header takes a device pointer the argument is a tensor, handed over as its data_ptr(),
    or None for NULL; numbers and ctypes.byref(...) pass as they are.  Nothing is converted or copied: a tensor must already
    have the dtype and the contiguous layout the header asks for."""
    argv = list(args)
    for i in _POINTER_ARGS[name]:
        t = argv[i]
        if t is not None:
            if not t.is_contiguous():
                raise RuntimeError("spatial_vae_amd: %s was handed a non-contiguous tensor of shape %s, strides %s"
                                   % (name, tuple(t.shape), t.stride()))
            argv[i] = t.data_ptr()
    fn = getattr(_lib.lib(), name)
    with torch.cuda.device(device):
        _lib.check(fn(*argv, torch.cuda.current_stream(device).cuda_stream))


def make_desc(spec, B, N):
    d = _lib.Desc()
    d.B, d.N, d.H, d.L = int(B), int(N), int(spec.hidden_dim), int(spec.num_layers)
    d.Zd, d.C = int(spec.latent_dim), int(spec.n_out)
    d.in_dim = 5 if spec.expand_coords else 2
    d.act = _lib.ACT[spec.act]
    bil = bool(spec.bilinear) and spec.latent_dim > 0
    d.flags = (_lib.FLAG_RESID if spec.resid else 0) | (_lib.FLAG_BILINEAR if bil else 0) | \
              (_lib.FLAG_SOFTPLUS if spec.softplus else 0)
    return d


def _fill_params(struct, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, hidden):
    struct.coord_w, struct.coord_b = _p(coord_w), _p(coord_b)
    struct.latent_w, struct.bilinear_w = _p(latent_w), _p(bilinear_w)
    struct.out_w, struct.out_b = _p(out_w), _p(out_b)
    for l in range(len(hidden) // 2):
        struct.hidden_w[l] = _p(hidden[2 * l])
        struct.hidden_b[l] = _p(hidden[2 * l + 1])
    return struct


class _Decoder(torch.autograd.Function):
    """y, logits[, loglik] = decoder(coords | grid+theta+dx, z; parameters)   (svae_decoder_forward[_bce] / _backward).

    With `target` (a Bernoulli observation, same shape as y) the per-image log-likelihood of train_mnist.py:78-81 comes out
    of the same call (svae_decoder_forward_bce): no bce kernel, and the backward pass hands the kept d(loglik)/d(y) plus
    the upstream gradient of loglik to svae_decoder_backward as (dy, dy_scale) -- no elementwise multiply in between."""

    # positions of the tensor arguments in forward(): spec, B, sinks, target come first
    _ARG0 = 4

    @staticmethod
    def forward(ctx, spec, B, sinks, target, coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, *hidden):
        L = _lib.lib()
        ref = coords if coords is not None else grid
        _require_hip(ref, "coordinates")
        device = ref.device
        coords, grid, theta, dx, z = _f32(coords), _f32(grid), _f32(theta), _f32(dx), _f32(z)
        coord_w, coord_b, latent_w, bilinear_w = _f32(coord_w), _f32(coord_b), _f32(latent_w), _f32(bilinear_w)
        out_w, out_b = _f32(out_w), _f32(out_b)
        hidden = tuple(_f32(h) for h in hidden)
        for t in (z, coord_w, out_w) + hidden:
            if t is not None:
                _require_hip(t, "decoder inputs and parameters")
        N = coords.shape[1] if coords is not None else grid.shape[0]
        if len(hidden) != 2 * (spec.num_layers - 1):
            raise RuntimeError("expected %d hidden tensors, got %d" % (2 * (spec.num_layers - 1), len(hidden)))
        if spec.latent_dim > 0 and (z is None or tuple(z.shape) != (B, spec.latent_dim)):
            raise RuntimeError("z must be (%d, %d), got %s" % (B, spec.latent_dim, None if z is None else tuple(z.shape)))
        desc = make_desc(spec, B, N)
        params = _fill_params(_lib.Params(), coord_w, coord_b, latent_w if spec.latent_dim > 0 else None,
                              bilinear_w if (desc.flags & _lib.FLAG_BILINEAR) else None, out_w, out_b, hidden)
        pose = _lib.Pose()
        pose.coords, pose.grid, pose.theta, pose.dx = _p(coords), _p(grid), _p(theta), _p(dx)
        need_grad = any(ctx.needs_input_grad)
        ws_bytes = L.svae_workspace_bytes(ctypes.byref(desc))
        ws = _buf(device, ws_bytes, "ws")
        saved = None
        if need_grad:
            saved = torch.empty(max(L.svae_saved_bytes(ctypes.byref(desc)), 256), dtype=torch.uint8, device=device)
        y = torch.empty((B, N, spec.n_out), dtype=torch.float32, device=device)
        logits = torch.empty_like(y)
        loglik = dll = None
        if target is None:
            _call("svae_decoder_forward", device, ctypes.byref(desc), ctypes.byref(params), ctypes.byref(pose), z, y, logits,
                  saved, ws, ws.numel())
        else:
            target = _f32(target)
            _require_hip(target, "target")
            if target.numel() != y.numel():
                raise RuntimeError("target shape %s does not match the decoder output %s" % (tuple(target.shape), tuple(y.shape)))
            loglik = torch.empty(B, dtype=torch.float32, device=device)
            dll = torch.empty_like(y) if need_grad else None
            _call("svae_decoder_forward_bce", device, ctypes.byref(desc), ctypes.byref(params), ctypes.byref(pose), z, target,
                  y, logits, loglik, dll, saved, ws, ws.numel())
        ctx.spec, ctx.B, ctx.N = spec, B, N
        ctx.sinks = sinks
        # everything the backward call reads goes through save_for_backward, so the buffers have the lifetime the reference's
        # autograd graph gives its activations (spatial_vae/models.py:90-132 is plain autograd): released after the first
        # backward(), kept under retain_graph=True (any number of backward passes), and a second backward() without it raises
        # torch's own "backward through the graph a second time" error
        ctx.save_for_backward(coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, logits, saved,
                              dll, *hidden)
        ctx.mark_non_differentiable(logits)
        ctx.set_materialize_grads(False)      # an unused output (y when only loglik feeds the loss) arrives as None
        if loglik is None:
            return y, logits
        return y, logits, loglik

    @staticmethod
    def backward(ctx, dy, _dlogits, g_loglik=None):
        L = _lib.lib()
        spec, B, N = ctx.spec, ctx.B, ctx.N
        (coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, logits, saved_buf, dll,
         *hidden) = ctx.saved_tensors
        hidden = tuple(hidden)
        device = logits.device
        # what reaches the kernels: dy (B, N, C) and an optional per-image factor dy_scale (B)
        dy_scale = None
        if dll is not None and g_loglik is not None:
            if dy is None:
                dy, dy_scale = dll, _f32(g_loglik).reshape(-1)          # the fused loss: d(loglik_b)/dy times its upstream gradient
            else:
                dy = _f32(dy) + dll * g_loglik.reshape(-1, 1, 1)        # y_hat is ALSO used downstream: add the two paths
        elif dy is None:
            dy = torch.zeros((B, N, spec.n_out), dtype=torch.float32, device=device)
        dy = _f32(dy)
        desc = make_desc(spec, B, N)
        bil = bool(desc.flags & _lib.FLAG_BILINEAR)
        params = _fill_params(_lib.Params(), coord_w, coord_b, latent_w if spec.latent_dim > 0 else None,
                              bilinear_w if bil else None, out_w, out_b, hidden)
        pose = _lib.Pose()
        pose.coords, pose.grid, pose.theta, pose.dx = _p(coords), _p(grid), _p(theta), _p(dx)
        # (spec, B, sinks, target, coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, *hidden)
        ng = ctx.needs_input_grad[_Decoder._ARG0:]
        sinks = ctx.sinks or {}

        def new(t, want, key=None):
            """Gradient buffer: the caller's sink (a view of a flat gradient buffer the kernels write
            into directly, see dp.FlatGrads) when one is registered for this parameter, else fresh."""
            if t is None or not want:
                return None
            sk = sinks.get(key) if key is not None else None
            if sk is not None and sk.shape == t.shape and sk.dtype == torch.float32 and sk.is_contiguous():
                return sk
            return torch.empty_like(t)

        g_coords, g_theta, g_dx, g_z = new(coords, ng[0]), new(theta, ng[2]), new(dx, ng[3]), new(z, ng[4] and spec.latent_dim > 0)
        g_cw, g_cb = new(coord_w, ng[5], "coord_w"), new(coord_b, ng[6], "coord_b")
        g_lw = new(latent_w, ng[7] and spec.latent_dim > 0, "latent_w")
        g_bw = new(bilinear_w, ng[8] and bil, "bilinear_w")
        g_ow, g_ob = new(out_w, ng[9], "out_w"), new(out_b, ng[10], "out_b")
        g_hidden = tuple(new(h, ng[11 + i], "hidden%d" % i) for i, h in enumerate(hidden))
        grads = _fill_params(_lib.Grads(), g_cw, g_cb, g_lw, g_bw, g_ow, g_ob, g_hidden)
        pg = _lib.PoseGrads()
        pg.dcoords, pg.dtheta, pg.ddx = _p(g_coords), _p(g_theta), _p(g_dx)
        ws_bytes = L.svae_workspace_bytes(ctypes.byref(desc))
        ws = _buf(device, ws_bytes, "ws")
        _call("svae_decoder_backward", device, ctypes.byref(desc), ctypes.byref(params), ctypes.byref(pose), z, logits, dy,
              dy_scale, saved_buf, ctypes.byref(grads), g_z, ctypes.byref(pg), ws, ws.numel())
        ready = sinks.get("__ready__")   # dp.TrainStep: every decoder gradient is now enqueued -> start its all-reduce
        if ready is not None:
            ready()

        def ret(t, key):
            """A gradient the kernels wrote straight into the caller's sink is not handed to autograd again
            (it would clone the view and, were .grad the same view, add it to itself)."""
            return None if (t is not None and sinks.get(key) is t) else t

        return (None, None, None, None, g_coords, None, g_theta, g_dx, g_z, ret(g_cw, "coord_w"), ret(g_cb, "coord_b"),
                ret(g_lw, "latent_w"), ret(g_bw, "bilinear_w"), ret(g_ow, "out_w"), ret(g_ob, "out_b")) + \
            tuple(ret(h, "hidden%d" % i) for i, h in enumerate(g_hidden))


def decoder(spec, B, coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w, out_b, hidden, sinks=None,
            bce_target=None):
    """Returns (y, logits), each (B, N, n_out) -- and, with bce_target (B, N, n_out), also the per-image Bernoulli
    log-likelihood (B) computed inside the same call.  Exactly one of coords / grid is given.
    sinks: optional {name: tensor} of preallocated parameter-gradient buffers (names coord_w, coord_b,
    latent_w, bilinear_w, out_w, out_b, hidden0, hidden1, ...) the backward kernels write into; the entry
    "__ready__", if present, is a callable invoked once the backward launch sequence has been enqueued."""
    return _Decoder.apply(spec, B, sinks, bce_target, coords, grid, theta, dx, z, coord_w, coord_b, latent_w, bilinear_w, out_w,
                          out_b, *hidden)


class _Latent(torch.autograd.Function):
    """theta, dx, z_content, kl = latent_head(q_out, r)   (svae_latent_forward/backward)."""

    @staticmethod
    def forward(ctx, q_out, r, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
        _require_hip(q_out, "encoder output")
        q_out, r = _f32(q_out), _f32(r)
        B, inf = r.shape
        if q_out.shape != (B, 2 * inf):
            raise RuntimeError("q_out must be (%d, %d), got %s" % (B, 2 * inf, tuple(q_out.shape)))
        d = _lib.LatentDesc(B, inf, int(bool(rotate)), int(bool(translate)), int(bool(mu_penalty)), float(dx_scale),
                            float(z_scale), float(theta_prior))
        dev = q_out.device
        zd = inf - (1 if rotate else 0) - (2 if translate else 0)
        theta = torch.empty(B, dtype=torch.float32, device=dev) if rotate else None
        dx = torch.empty(B, 2, dtype=torch.float32, device=dev) if translate else None
        zc = torch.empty(B, zd, dtype=torch.float32, device=dev)
        kl = torch.empty(B, dtype=torch.float32, device=dev)
        _call("svae_latent_forward", dev, ctypes.byref(d), q_out, r, theta, dx, zc if zd > 0 else None, kl)
        ctx.desc, ctx.q_out, ctx.r = d, q_out, r
        return theta, dx, zc, kl

    @staticmethod
    def backward(ctx, g_theta, g_dx, g_zc, g_kl):
        q_out, r = ctx.q_out, ctx.r
        g_theta, g_dx, g_zc, g_kl = _f32(g_theta), _f32(g_dx), _f32(g_zc), _f32(g_kl)
        if g_zc is not None and g_zc.numel() == 0:
            g_zc = None
        gq = torch.empty_like(q_out)
        _call("svae_latent_backward", q_out.device, ctypes.byref(ctx.desc), q_out, r, g_theta, g_dx, g_zc, g_kl, gq)
        return gq, None, None, None, None, None, None, None


def latent_head(q_out, r, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
    """(theta | None, dx | None, z_content, kl_per_image) from the encoder output [z_mu | z_logstd] and the noise r."""
    return _Latent.apply(q_out, r, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior)


class _ElboHead(torch.autograd.Function):
    """elbo, log_p, kl = mean(loglik) - mean(kl_b), mean(loglik), mean(kl_b)  (svae_elbo_head_forward/backward)."""

    @staticmethod
    def forward(ctx, loglik, kl_b):
        _require_hip(loglik, "loglik")
        loglik, kl_b = _f32(loglik), _f32(kl_b)
        B = loglik.numel()
        if kl_b.numel() != B:
            raise RuntimeError("loglik has %d entries, kl %d" % (B, kl_b.numel()))
        ctx.set_materialize_grads(False)     # unused outputs (log_p, kl) arrive as None, not as zero tensors autograd fills
        out = torch.empty(3, dtype=torch.float32, device=loglik.device)
        _call("svae_elbo_head_forward", loglik.device, loglik, kl_b, B, out)
        ctx.B, ctx.shapes = B, (loglik.shape, kl_b.shape)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_elbo, g_logp, g_kl):
        ref = next(g for g in (g_elbo, g_logp, g_kl) if g is not None)
        g_elbo, g_logp, g_kl = _f32(g_elbo), _f32(g_logp), _f32(g_kl)
        dl = torch.empty(ctx.B, dtype=torch.float32, device=ref.device)
        dk = torch.empty(ctx.B, dtype=torch.float32, device=ref.device)
        _call("svae_elbo_head_backward", ref.device, g_elbo, g_logp, g_kl, ctx.B, dl, dk)
        return dl.view(ctx.shapes[0]), dk.view(ctx.shapes[1])


def elbo_head(loglik, kl_b):
    """(elbo, log_p_x_g_z, kl_div) of a minibatch from its per-image log-likelihoods and KL terms."""
    return _ElboHead.apply(loglik, kl_b)


def _check_samples(K):
    K = int(K)
    if not 1 <= K <= _lib.IW_MAX_SAMPLES:
        raise RuntimeError("num_samples must be in [1, %d], got %d" % (_lib.IW_MAX_SAMPLES, K))
    return K


class _LatentIW(torch.autograd.Function):
    """theta, dx, z_content, log_ratio = latent_head_iw(q_out, r, K): K draws per image from one encoder output, row b*K + k
    is sample k of image b (svae_latent_iw_forward/backward)."""

    @staticmethod
    def forward(ctx, q_out, r, K, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
        _require_hip(q_out, "encoder output")
        _require_hip(r, "noise")
        K = _check_samples(K)
        q_out, r = _f32(q_out), _f32(r)
        rows, inf = r.shape
        B = q_out.shape[0]
        if rows != B * K or q_out.shape != (B, 2 * inf):
            raise RuntimeError("latent_head_iw: q_out %s and r %s do not describe %d samples per image"
                               % (tuple(q_out.shape), tuple(r.shape), K))
        d = _lib.LatentDesc(B, inf, int(bool(rotate)), int(bool(translate)), int(bool(mu_penalty)), float(dx_scale),
                            float(z_scale), float(theta_prior))
        dev = q_out.device
        zd = inf - (1 if rotate else 0) - (2 if translate else 0)
        theta = torch.empty(rows, dtype=torch.float32, device=dev) if rotate else None
        dx = torch.empty(rows, 2, dtype=torch.float32, device=dev) if translate else None
        zc = torch.empty(rows, zd, dtype=torch.float32, device=dev)
        log_ratio = torch.empty(rows, dtype=torch.float32, device=dev)
        _call("svae_latent_iw_forward", dev, ctypes.byref(d), K, q_out, r, theta, dx, zc if zd > 0 else None, log_ratio)
        ctx.desc, ctx.K, ctx.q_out, ctx.r = d, K, q_out, r
        ctx.set_materialize_grads(False)
        return theta, dx, zc, log_ratio

    @staticmethod
    def backward(ctx, g_theta, g_dx, g_zc, g_lr):
        q_out, r = ctx.q_out, ctx.r
        g_theta, g_dx, g_zc, g_lr = _f32(g_theta), _f32(g_dx), _f32(g_zc), _f32(g_lr)
        if g_zc is not None and g_zc.numel() == 0:
            g_zc = None
        gq = torch.empty_like(q_out)
        _call("svae_latent_iw_backward", q_out.device, ctypes.byref(ctx.desc), ctx.K, q_out, r, g_theta, g_dx, g_zc, g_lr, gq)
        return gq, None, None, None, None, None, None, None, None


def latent_head_iw(q_out, r, K, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior):
    """(theta | None, dx | None, z_content, log p(z) - log q(z|x)) for K samples per image: q_out (B, 2*inf_dim) is the encoder
    output [z_mu | z_logstd], r (B*K, inf_dim) the noise; every output has B*K rows, sample k of image b in row b*K + k."""
    return _LatentIW.apply(q_out, r, K, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior)


class _IWHead(torch.autograd.Function):
    """bound, log_p, kl = mean_b log mean_k exp(loglik + log_ratio), mean(loglik), mean(-log_ratio)
    (svae_iw_head_forward/backward)."""

    @staticmethod
    def forward(ctx, loglik, log_ratio, K):
        _require_hip(loglik, "loglik")
        _require_hip(log_ratio, "log_ratio")
        K = _check_samples(K)
        loglik, log_ratio = _f32(loglik), _f32(log_ratio)
        rows = loglik.numel()
        if log_ratio.numel() != rows or rows % K or rows == 0:
            raise RuntimeError("iw_head: loglik has %d entries, log_ratio %d, for %d samples per image"
                               % (rows, log_ratio.numel(), K))
        ctx.set_materialize_grads(False)
        out = torch.empty(3, dtype=torch.float32, device=loglik.device)
        weights = torch.empty(rows, dtype=torch.float32, device=loglik.device)
        _call("svae_iw_head_forward", loglik.device, loglik, log_ratio, rows // K, K, out, weights)
        ctx.B, ctx.K, ctx.shapes = rows // K, K, (loglik.shape, log_ratio.shape)
        ctx.save_for_backward(weights)
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, g_bound, g_logp, g_kl):
        weights, = ctx.saved_tensors
        g_bound, g_logp, g_kl = _f32(g_bound), _f32(g_logp), _f32(g_kl)
        dl = torch.empty_like(weights)
        dr = torch.empty_like(weights)
        _call("svae_iw_head_backward", weights.device, g_bound, g_logp, g_kl, weights, ctx.B, ctx.K, dl, dr)
        return dl.view(ctx.shapes[0]), dr.view(ctx.shapes[1]), None


def iw_head(loglik, log_ratio, K):
    """(bound, log_p_x_g_z, kl_div) of a minibatch from the per-sample log-likelihoods and log p(z) - log q(z|x), each (B*K):
    three views of one vector, like elbo_head.  For K >= 2 the bound is not log_p - kl."""
    return _IWHead.apply(loglik, log_ratio, K)


class IWStream:
    """The streaming K-sample scorer (include/svae_stream.h) for B images of inf_dim latents: update() merges one chunk of
    at most IW_MAX_SAMPLES samples per image, finish() gives (per_image (B, 6 + 2*inf_dim), out3) for everything merged so
    far.  Any number of chunks; the record it keeps on the device is a few doubles per image.  Forward only."""

    def __init__(self, B, inf_dim, device):
        device = _hip_device("IWStream", device)
        self.B, self.inf_dim, self.device = int(B), int(inf_dim), device
        nbytes = _lib.lib().svae_iw_stream_state_bytes(self.B, self.inf_dim)
        if nbytes == 0:
            raise RuntimeError("IWStream: bad B = %d or inf_dim = %d" % (self.B, self.inf_dim))
        self.state = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        self.reset()

    def reset(self):
        _call("svae_iw_stream_reset", self.device, self.state, self.B, self.inf_dim)
        self._pose = None

    def update(self, rotate, translate, mu_penalty, dx_scale, z_scale, theta_prior, K, loglik, log_ratio, theta, dx, zc):
        """One chunk: loglik, log_ratio (B*K) and the theta / dx / zc that ops.latent_head_iw gave for it (the descriptor
        arguments are latent_head_iw's); row b*K + k is sample k of image b."""
        K = _check_samples(K)
        for name, t in (("loglik", loglik), ("log_ratio", log_ratio), ("theta", theta), ("dx", dx), ("zc", zc)):
            if t is not None:
                _require_hip(t, name)
        loglik, log_ratio, theta, dx, zc = (_f32(t) for t in (loglik, log_ratio, theta, dx, zc))
        zd = self.inf_dim - (1 if rotate else 0) - (2 if translate else 0)
        rows = self.B * K
        theta, dx, zc = theta if rotate else None, dx if translate else None, zc if zd > 0 else None
        for name, t, n in (("loglik", loglik, rows), ("log_ratio", log_ratio, rows), ("theta", theta, rows if rotate else None),
                           ("dx", dx, 2 * rows if translate else None), ("zc", zc, zd * rows if zd > 0 else None)):
            if (None if t is None else t.numel()) != n:
                raise RuntimeError("IWStream.update: %s has %s elements, %s expected for %d samples of %d images"
                                   % (name, None if t is None else t.numel(), n, K, self.B))
        d = _lib.LatentDesc(self.B, self.inf_dim, int(bool(rotate)), int(bool(translate)), int(bool(mu_penalty)),
                            float(dx_scale), float(z_scale), float(theta_prior))
        _call("svae_iw_stream_update", self.device, self.state, ctypes.byref(d), K, loglik, log_ratio, theta, dx, zc)
        self._pose = (int(bool(rotate)), int(bool(translate)))

    def finish(self):
        """(per_image, out3) of everything merged since the last reset; may be called again after further updates."""
        if getattr(self, "_pose", None) is None:
            raise RuntimeError("IWStream.finish: no chunk has been merged")
        d = _lib.LatentDesc(self.B, self.inf_dim, self._pose[0], self._pose[1], 0, 1.0, 1.0, 1.0)
        per_image = torch.empty(self.B, _lib.iw_stream_cols(self.inf_dim), dtype=torch.float32, device=self.device)
        out3 = torch.empty(3, dtype=torch.float32, device=self.device)
        _call("svae_iw_stream_finish", self.device, self.state, ctypes.byref(d), per_image, out3)
        return per_image, out3


ENC_ACT = {None: _lib.LINEAR_ACT_NONE, **_lib.ACT}
ENC_LINEAR_MAX_WEIGHT = 4 * 1024 * 1024     # elements: the hand-written layer is for weights of a few MB (see svae.h)


def enc_linear_applies(x, weight):
    """The small-batch Linear kernels take fp32 CUDA operands whose weight matrix has at most 4 M elements."""
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 2 and
            weight.numel() <= ENC_LINEAR_MAX_WEIGHT)


class _EncLinear(torch.autograd.Function):
    """out = act(x W^T + b) in ONE launch (svae_linear_forward); the backward pass is ONE launch too (svae_linear_backward):
    dW, db and dx with act' applied to the upstream gradient as it is loaded.  Replaces an nn.Linear + activation pair of
    InferenceNetwork.layers (models.py:31-43) -- addmm, tanh, tanh_backward, two mm and a column sum otherwise.  With sinks
    (views of dp.FlatGrads' flat buffer) dW / db are written in place and not handed to autograd."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, sink_w, sink_b):
        x, weight, bias = _f32(x), _f32(weight), _f32(bias)
        rows, k = x.shape
        n = weight.shape[0]
        out = torch.empty(rows, n, dtype=torch.float32, device=x.device)
        _call("svae_linear_forward", x.device, x, weight, bias, out, rows, k, n, ENC_ACT[act])
        ctx.act = act
        ctx.sinks = (sink_w, sink_b)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        sink_w, sink_b = ctx.sinks
        dout = _f32(dout)
        rows, k = x.shape
        n = weight.shape[0]
        want_x, want_w, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if want_x else None
        dw = (sink_w if sink_w is not None else torch.empty_like(weight)) if want_w else None
        db = (sink_b if sink_b is not None else torch.empty(n, dtype=torch.float32, device=x.device)) if want_b else None
        _call("svae_linear_backward", x.device, x, weight, out, dout, rows, k, n, ENC_ACT[ctx.act], dw, db, dx)
        return (dx, None if (dw is None or dw is sink_w) else dw, None if (db is None or db is sink_b) else db, None, None, None)


def enc_linear(x, weight, bias, act=None, sink_w=None, sink_b=None):
    """act(x W^T + b), act in (None, "tanh", "leakyrelu", "relu", "sigmoid") -- see _EncLinear."""
    return _EncLinear.apply(x, weight, bias, act, sink_w, sink_b)


class _SinkLinear(torch.autograd.Function):
    """y = x W^T + b; the backward pass writes dW and db straight into caller-owned gradient views (slices of the flat
    buffer of dp.FlatGrads) with torch.mm(out=) / torch.sum(out=) instead of returning tensors that autograd would then
    ADD into those views: one kernel less per parameter per step.  The arithmetic is torch's (hipBLASLt).

    With a `collector` (data-parallel runs: dp.LowRankExchange) the backward pass does not form dW at all: it hands its two
    factors (x, dy) to the collector, and the step all-gathers the factors of every rank and forms the GLOBAL dW = dy_all^T
    x_all locally -- rank <= global batch, a few MB on the wire instead of the weight's size."""

    @staticmethod
    def forward(ctx, x, weight, bias, sink_w, sink_b, collector=None, key=None):
        ctx.save_for_backward(x, weight)
        ctx.sinks = (sink_w, sink_b)
        ctx.collector, ctx.key = collector, key
        return torch.addmm(bias, x, weight.t())

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        sink_w, sink_b = ctx.sinks
        dx = dy.mm(weight) if ctx.needs_input_grad[0] else None
        if ctx.collector is not None:
            ctx.collector.add(ctx.key, x, dy)
            return dx, None, None, None, None, None, None
        torch.mm(dy.t(), x, out=sink_w)
        if dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and sink_b.is_contiguous():
            # column sums in ~3 us (ATen's reduce kernel takes 13 us for 256 x 500)
            _call("svae_colsum", dy.device, dy, dy.size(0), dy.size(1), sink_b)
        else:
            torch.sum(dy, 0, out=sink_b)
        return dx, None, None, None, None, None, None


def sink_linear(x, weight, bias, sink_w, sink_b, collector=None, key=None):
    return _SinkLinear.apply(x, weight, bias, sink_w, sink_b, collector, key)


class _BceLoglik(torch.autograd.Function):
    """loglik[b] = -sum_j bce(y_hat[b, j], target[b, j])  (svae_bce_loglik)."""

    @staticmethod
    def forward(ctx, y_hat, target):
        _require_hip(y_hat, "y_hat")
        y_hat, target = _f32(y_hat), _f32(target)
        B = y_hat.shape[0]
        n = y_hat.numel() // B
        if target.numel() != y_hat.numel():
            raise RuntimeError("target shape %s does not match y_hat %s" % (tuple(target.shape), tuple(y_hat.shape)))
        loglik = torch.empty(B, dtype=torch.float32, device=y_hat.device)
        dll = torch.empty_like(y_hat) if ctx.needs_input_grad[0] else None
        _call("svae_bce_loglik", y_hat.device, B, n, y_hat, target, loglik, dll)
        ctx.save_for_backward(dll)
        return loglik

    @staticmethod
    def backward(ctx, g):
        dll, = ctx.saved_tensors
        return dll * g.reshape((-1,) + (1,) * (dll.dim() - 1)), None


def bce_loglik(y_hat, target):
    return _BceLoglik.apply(y_hat, target)


class _GaussianLoglik(torch.autograd.Function):
    """Per-image Gaussian log-likelihood of train_particles.py:102-139 (svae_gaussian_loglik)."""

    @staticmethod
    def forward(ctx, y_params, target, mask, ctf):
        L = _lib.lib()
        _require_hip(y_params, "y_params")
        y_params, target, ctf = _f32(y_params), _f32(target), _f32(ctf)
        B, N = target.shape
        C = y_params.shape[1] // N
        if mask is not None:
            mask = mask.to(device=y_params.device, dtype=torch.uint8).contiguous()
        k = 0 if ctf is None else int(ctf.shape[-1])
        ws_bytes = L.svae_gaussian_workspace_bytes(B, N) if ctf is not None else 0
        ws = _buf(y_params.device, ws_bytes, "gauss") if ws_bytes else None
        loglik = torch.empty(B, dtype=torch.float32, device=y_params.device)
        dll = torch.zeros_like(y_params) if ctx.needs_input_grad[0] else None
        _call("svae_gaussian_loglik", y_params.device, B, N, C, y_params, target, mask, ctf, k, loglik, dll, ws, ws_bytes)
        ctx.save_for_backward(dll)
        return loglik

    @staticmethod
    def backward(ctx, g):
        dll, = ctx.saved_tensors
        return dll * g[:, None], None, None, None


def gaussian_loglik(y_params, target, mask=None, ctf=None):
    return _GaussianLoglik.apply(y_params, target, mask, ctf)


def rotation_matrices(offset, rows, cols):
    """Host part of Image.rotate for a batch: per image the six inverse-affine coefficients PIL/Image.py derives
    from the angle (cos/sin of -radians(angle) rounded to 15 decimals about the centre (cols/2, rows/2)), and the
    quarter-turn code of Pillow's exact fast paths (-1 = general angle).  offset: radians, as drawn by
    train_galaxy.py:44; the reference passes 360*offset/2/pi degrees (train_galaxy.py:51)."""
    B = len(offset)
    mat = np.zeros((B, 6), np.float64)
    quarter = np.full(B, -1, np.int32)
    cx, cy = cols / 2, rows / 2
    for i in range(B):
        angle = (360 * float(offset[i]) / 2 / np.pi) % 360.0
        if angle in (0.0, 180.0) or (angle in (90.0, 270.0) and rows == cols):
            quarter[i] = int(angle // 90)
            continue
        a = -math.radians(angle)
        c, s = round(math.cos(a), 15), round(math.sin(a), 15)
        ms, mc = round(-math.sin(a), 15), round(math.cos(a), 15)
        tx = c * (-cx) + s * (-cy) + 0.0
        ty = ms * (-cx) + mc * (-cy) + 0.0
        mat[i] = (c, s, tx + cx, ms, mc, ty + cy)
    return mat, quarter


def rotate_augment(y, offset, rows, cols, quantize_u8):
    """Rotate image i of the batch by offset[i] radians the way the reference does with Pillow
    (train_galaxy.py:41-54 quantize_u8=True; train_particles.py:31-43 quantize_u8=False), on the device
    (svae_rotate_bicubic).  y: (B, rows*cols[, C]) fp32 CUDA tensor; returns a new tensor of the same shape."""
    _require_hip(y, "y")
    B = y.size(0)
    yc = y.contiguous().float()
    C = yc.numel() // (B * rows * cols)
    if C * B * rows * cols != yc.numel() or len(offset) != B:
        raise RuntimeError("rotate_augment: y %s does not match %d images of %dx%d" % (tuple(y.shape), len(offset), rows, cols))
    mat, quarter = rotation_matrices(offset, rows, cols)
    mat_d = torch.from_numpy(mat).to(y.device, non_blocking=True)
    q_d = torch.from_numpy(quarter).to(y.device, non_blocking=True)
    out = torch.empty_like(yc)
    _call("svae_rotate_bicubic", y.device, yc, out, mat_d, q_d, B, rows, cols, C, 1 if quantize_u8 else 0)
    return out.view_as(y)


def align_images(y, theta, dx, rows, cols, interp="bicubic"):
    """Bring each observed image into the model's canonical frame (svae_align_images, include/svae_align.h): the image
    resampled where the decoder's pose (theta (B) radians or None, dx (B, 2) in the decoder's units or None) maps its grid.
    y: (B, rows*cols[, C]) fp32 on the device, the poses device tensors too (nothing is read back).  Returns (aligned, a new
    tensor shaped like y; cover (B, rows*cols) uint8, 1 where the observed image covers the pixel, whose value is 0 otherwise)."""
    _require_hip(y, "y")
    if interp not in _lib.ALIGN_INTERP:
        raise RuntimeError("align_images: interp must be one of %s, got %r" % (sorted(_lib.ALIGN_INTERP), interp))
    B = y.size(0)
    yc = _f32(y)
    C = yc.numel() // (B * rows * cols) if B * rows * cols else 0
    if C * B * rows * cols != yc.numel() or C < 1:
        raise RuntimeError("align_images: y %s does not hold %d images of %dx%d" % (tuple(y.shape), B, rows, cols))
    for name, t, n in (("theta", theta, B), ("dx", dx, 2 * B)):
        if t is not None:
            _require_hip(t, name)
            if t.numel() != n:
                raise RuntimeError("align_images: %s has %d elements, %d expected for %d images" % (name, t.numel(), n, B))
    theta, dx = _f32(theta), _f32(dx)
    out = torch.empty_like(yc)
    cover = torch.empty(B, rows * cols, dtype=torch.uint8, device=y.device)
    _call("svae_align_images", y.device, yc, theta, dx, B, rows, cols, C, _lib.ALIGN_INTERP[interp], out, cover)
    return out.view_as(y), cover


class ClassSums:
    """Per-class sums of aligned images (svae_class_sums_update): update() adds one minibatch -- aligned (B, N[, C]) and cover
    (B, N) or None as align_images returns them, label (B) int32 on the device, -1 = in no class --, result() gives (sum
    (n_classes, N, C), count (n_classes, N)), float64 on the device.  Images are added in the order they are handed over, without
    atomics: the same sequence of updates gives the same bits.  update_soft() adds posterior-weighted rows to the same
    accumulators, which are fractional from then on."""

    def __init__(self, n_classes, N, C, device):
        device = _hip_device("ClassSums", device)
        self.n_classes, self.N, self.C, self.device = int(n_classes), int(N), int(C), device
        if self.n_classes < 1 or self.N < 1 or self.C < 1:
            raise RuntimeError("ClassSums: bad n_classes = %d, N = %d or C = %d" % (self.n_classes, self.N, self.C))
        self.sum = torch.zeros(self.n_classes, self.N, self.C, dtype=torch.float64, device=device)
        self.count = torch.zeros(self.n_classes, self.N, dtype=torch.float64, device=device)

    def update(self, aligned, cover, label):
        for name, t in (("aligned", aligned), ("cover", cover), ("label", label)):
            if t is not None:
                _require_hip(t, name)
        B = label.numel()
        aligned = _f32(aligned)
        if label.dtype != torch.int32 or (cover is not None and cover.dtype != torch.uint8):
            raise RuntimeError("ClassSums.update: label must be int32 and cover uint8")
        if aligned.numel() != B * self.N * self.C or (cover is not None and cover.numel() != B * self.N):
            raise RuntimeError("ClassSums.update: aligned %s / cover %s do not hold %d images of %d pixels, %d channels"
                               % (tuple(aligned.shape), None if cover is None else tuple(cover.shape), B, self.N, self.C))
        _call("svae_class_sums_update", self.device, aligned, cover, label, B, self.N, self.C, self.n_classes, self.sum, self.count)

    def update_soft(self, expect, cand, target=None):
        """The soft counterpart of update() (svae_expect_sums_update, include/svae_expect.h): adds the contribution rows of
        `expect` (a PoseExpect made for cand (B, M) int32) into the classes its references map to -- target (n_ref) int32 names
        the class of each reference, None = the reference's own index -- in image order, then slot order, without atomics."""
        for name, t in (("contrib", expect.contrib), ("cover_w", expect.cover_w), ("cand", cand), ("target", target)):
            if t is not None:
                _require_hip(t, name)
        if cand.dtype != torch.int32 or cand.dim() != 2 or (target is not None and target.dtype != torch.int32):
            raise RuntimeError("ClassSums.update_soft: cand must be (B, M) int32 and target int32")
        B, M = cand.shape
        if expect.contrib.dtype != torch.float64 or expect.cover_w.dtype != torch.float64 or \
                expect.contrib.numel() != B * M * self.N * self.C or expect.cover_w.numel() != B * M * self.N:
            raise RuntimeError("ClassSums.update_soft: contrib %s / cover_w %s do not hold %d x %d float64 rows of %d pixels, %d channels"
                               % (tuple(expect.contrib.shape), tuple(expect.cover_w.shape), B, M, self.N, self.C))
        n_ref = self.n_classes if target is None else target.numel()
        _call("svae_expect_sums_update", self.device, expect.contrib, expect.cover_w, cand.contiguous(),
              None if target is None else target.contiguous(), B, M, self.N, self.C, n_ref, self.n_classes, self.sum, self.count)

    def result(self):
        return self.sum, self.count


def _ctf_rows(table, device, who):
    """The (P, 8) float64 parameter table of spatial_vae/ctf.py:26-30 on `device`: a host array is uploaded, a device tensor
    is taken as it is."""
    tab = table if torch.is_tensor(table) else torch.from_numpy(np.array(table, dtype=np.float64, order="C"))
    if tab.dim() != 2 or tab.size(1) != 8:
        raise RuntimeError("%s: expected a (P, 8) parameter table, got %s" % (who, tuple(tab.shape)))
    tab = tab.to(device=device, dtype=torch.float64).contiguous()
    _require_hip(tab, "CTF table")
    return tab


def ctf_apply(y, table, n, m, scale=1.0, mode="flip"):
    """Each observed image through its own transfer function in Fourier space (svae_ctf_apply, include/svae_ctfcorr.h):
    mode "flip" multiplies every Fourier coefficient by the sign of H_i (phase flipping), "multiply" by H_i itself.  y: (B,
    n*m) or (B, n, m) fp32 on the device, one channel; table: the (B, 8) parameters of the same images, a host array or a
    float64 device tensor (nothing is read back).  Returns a new tensor shaped like y."""
    _require_hip(y, "y")
    if mode not in _lib.CTF_MODE:
        raise RuntimeError("ctf_apply: mode must be one of %s, got %r" % (sorted(_lib.CTF_MODE), mode))
    B = y.size(0)
    yc = _f32(y)
    if yc.numel() != B * n * m:
        raise RuntimeError("ctf_apply: y %s does not hold %d one-channel images of %dx%d" % (tuple(y.shape), B, n, m))
    tab = _ctf_rows(table, y.device, "ctf_apply")
    if tab.size(0) != B:
        raise RuntimeError("ctf_apply: %d rows of CTF parameters for %d images" % (tab.size(0), B))
    out = torch.empty_like(yc)
    ws, ws_bytes = _workspace("svae_ctf_apply", "ctfcorr", y.device, B, n, m)    # none while the planes fit the LDS (up to 71 x 71)
    _call("svae_ctf_apply", y.device, yc, tab, B, n, m, float(scale), _lib.CTF_MODE[mode], out, ws, ws_bytes)
    return out.view_as(y)


class CtfPower:
    """Per-class sums of the squared transfer functions (svae_ctf_power_update), the denominator of a Wiener class average:
    update() adds one minibatch -- table (B, 8) as for ctf_apply, label (B) int32 on the device, -1 = in no class --, result()
    gives den (n_classes, n, m), float64 on the device, in fftfreq order.  Images are added in the order they are handed over,
    without atomics: the same sequence of updates gives the same bits."""

    def __init__(self, n_classes, n, m, device, scale=1.0):
        device = _hip_device("CtfPower", device)
        self.n_classes, self.n, self.m, self.scale, self.device = int(n_classes), int(n), int(m), float(scale), device
        if self.n_classes < 1 or self.n < 2 or self.m < 2:
            raise RuntimeError("CtfPower: bad n_classes = %d, n = %d or m = %d" % (self.n_classes, self.n, self.m))
        self.den = torch.zeros(self.n_classes, self.n, self.m, dtype=torch.float64, device=device)

    def update(self, table, label):
        _require_hip(label, "label")
        if label.dtype != torch.int32:
            raise RuntimeError("CtfPower.update: label must be int32")
        tab = _ctf_rows(table, self.device, "CtfPower.update")
        B = label.numel()
        if tab.size(0) != B:
            raise RuntimeError("CtfPower.update: %d rows of CTF parameters for %d labels" % (tab.size(0), B))
        _call("svae_ctf_power_update", self.device, tab, label.contiguous(), B, self.n, self.m, self.scale, self.n_classes, self.den)

    def result(self):
        return self.den


def wiener_finish(sum, den, lam, n, m):
    """The Wiener class averages Re IDFT( DFT(sum[k]) / (den[k] + lam) ) (svae_wiener_finish): sum (n_classes, n*m[, 1]) float64
    on the device, the real-space sums of aligned CTF-multiplied images (ClassSums.result()[0] at C == 1), den (n_classes, n, m)
    from CtfPower.  Returns (n_classes, n, m) float32."""
    _require_hip(sum, "sum")
    _require_hip(den, "den")
    n_classes = den.size(0) if den.dim() == 3 else den.numel() // (n * m)
    if sum.dtype != torch.float64 or den.dtype != torch.float64:
        raise RuntimeError("wiener_finish: sum and den must be float64")
    if sum.numel() != n_classes * n * m or den.numel() != n_classes * n * m:
        raise RuntimeError("wiener_finish: sum %s / den %s do not hold %d one-channel planes of %dx%d"
                           % (tuple(sum.shape), tuple(den.shape), n_classes, n, m))
    out = torch.empty(n_classes, n, m, dtype=torch.float32, device=sum.device)
    ws, ws_bytes = _workspace("svae_wiener_finish", "ctfcorr", sum.device, n_classes, n, m)
    _call("svae_wiener_finish", sum.device, sum.contiguous(), den.contiguous(), float(lam), n_classes, n, m, out, ws, ws_bytes)
    return out


def frc(a, b, n, m, mask_radius=0.0, mask_edge=0.0):
    """The Fourier ring correlation of each pair of planes (svae_frc, include/svae_frc.h): a, b (planes, n*m) or (planes, n, m)
    float64 on the device, under the soft circular mask (mask_radius 0 = none).  Returns (sums (planes, R, 3) = [num, pa, pb],
    frc (planes, R), both float64, ring_count (R) int32) with R = min(n, m) // 2 + 1, on the device; nothing is read back."""
    _require_hip(a, "a")
    _require_hip(b, "b")
    if a.dtype != torch.float64 or b.dtype != torch.float64:
        raise RuntimeError("frc: a and b must be float64")
    planes = a.size(0)
    if a.numel() != planes * n * m or b.numel() != planes * n * m:
        raise RuntimeError("frc: a %s / b %s do not hold %d planes of %dx%d each" % (tuple(a.shape), tuple(b.shape), planes, n, m))
    R = min(n, m) // 2 + 1
    sums = torch.empty(planes, R, 3, dtype=torch.float64, device=a.device)
    out = torch.empty(planes, R, dtype=torch.float64, device=a.device)
    ring_count = torch.empty(R, dtype=torch.int32, device=a.device)
    ws, ws_bytes = _workspace("svae_frc", "frc", a.device, planes, n, m)     # none while the planes fit the LDS (up to 71 x 71)
    _call("svae_frc", a.device, a.contiguous(), b.contiguous(), planes, n, m, float(mask_radius), float(mask_edge), sums, out,
          ring_count, ws, ws_bytes)
    return sums, out, ring_count


def frc_filter(x, weight, n, m):
    """Each plane filtered by its per-ring weights, Re IDFT( weight[p, ring] DFT(x[p]) ) (svae_frc_filter): x (planes, n*m) or
    (planes, n, m) and weight (planes, R) float64 on the device.  Returns (planes, n, m) float32."""
    _require_hip(x, "x")
    _require_hip(weight, "weight")
    if x.dtype != torch.float64 or weight.dtype != torch.float64:
        raise RuntimeError("frc_filter: x and weight must be float64")
    planes, R = x.size(0), min(n, m) // 2 + 1
    if x.numel() != planes * n * m or weight.numel() != planes * R:
        raise RuntimeError("frc_filter: x %s / weight %s do not hold %d planes of %dx%d and their %d rings"
                           % (tuple(x.shape), tuple(weight.shape), planes, n, m, R))
    out = torch.empty(planes, n, m, dtype=torch.float32, device=x.device)
    ws, ws_bytes = _workspace("svae_frc_filter", "frc", x.device, planes, n, m)
    _call("svae_frc_filter", x.device, x.contiguous(), weight.contiguous(), planes, n, m, out, ws, ws_bytes)
    return out


def _pose_inputs(who, y, ref, weight, pose, rows, cols, interp, cand=None):
    """The checks pose_search, pose_classify and pose_expect share on y, ref, weight, cand (where there is one), pose and interp.
    Returns (y as contiguous fp32, B, N, C, n_ref, weight contiguous or None)."""
    for name, t in (("y", y), ("ref", ref), ("cand", cand), ("pose", pose)):
        if t is not None:
            _require_hip(t, name)
    if interp not in _lib.ALIGN_INTERP:
        raise RuntimeError("%s: interp must be one of %s, got %r" % (who, sorted(_lib.ALIGN_INTERP), interp))
    B, N = y.size(0), rows * cols
    yc = _f32(y)
    C = yc.numel() // (B * N) if B * N else 0
    if C < 1 or C * B * N != yc.numel():
        raise RuntimeError("%s: y %s does not hold %d images of %dx%d" % (who, tuple(y.shape), B, rows, cols))
    if ref.dtype != torch.float64 or ref.numel() % (N * C) or not ref.numel():
        raise RuntimeError("%s: ref %s (%s) must be float64 planes of %dx%dx%d" % (who, tuple(ref.shape), ref.dtype, rows, cols, C))
    if weight is not None:
        _require_hip(weight, "weight")
        if weight.dtype != torch.float64 or weight.numel() != N:
            raise RuntimeError("%s: weight must be %d float64 values, got %s (%s)" % (who, N, tuple(weight.shape), weight.dtype))
        weight = weight.contiguous()
    if cand is not None and (cand.dtype != torch.int32 or cand.dim() != 2 or cand.size(0) != B or cand.size(1) < 1):
        raise RuntimeError("%s: cand must be (%d, M >= 1) int32, got %s (%s)" % (who, B, tuple(cand.shape), cand.dtype))
    if pose.dtype != torch.float32 or tuple(pose.shape) != (B, 3):
        raise RuntimeError("%s: pose must be (%d, 3) float32, got %s (%s)" % (who, B, tuple(pose.shape), pose.dtype))
    return yc, B, N, C, ref.numel() // (N * C), weight


PoseSearch = namedtuple("PoseSearch", "pose score offset scores")


def pose_search(y, ref, weight, ref_index, pose, rows, cols, angles, step, shift, interp="bicubic", return_scores=False):
    """The pose of each image refined against its reference (svae_pose_search, include/svae_refine.h): 2 * angles + 1 rotations
    `step` radians apart and the integer shifts of at most `shift` pixels around `pose` (B, 3) fp32 = theta, dx0, dx1 in the
    decoder's units; the winner is the candidate whose canonical-frame image correlates best with ref[ref_index[b]] under
    `weight`, moved by a parabola through its neighbours on each axis.  y (B, rows*cols[, C]) fp32, ref (n_ref, rows*cols[, C])
    float64, weight (rows*cols) float64 or None, ref_index (B) int32, all on the device.  Returns PoseSearch(pose (B, 3) fp32,
    score (B) float64, offset (B, 4) int32 = k, sx, sy, flags, scores (B, 2 angles + 1, 2 shift + 1, 2 shift + 1) float64 or
    None) on the device; nothing is read back."""
    _require_hip(ref_index, "ref_index")
    yc, B, N, C, n_ref, weight = _pose_inputs("pose_search", y, ref, weight, pose, rows, cols, interp)
    if ref_index.dtype != torch.int32 or ref_index.numel() != B:
        raise RuntimeError("pose_search: ref_index must be (%d) int32" % B)
    A, S = int(angles), int(shift)
    dev = y.device
    out = torch.empty(B, 3, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    offset = torch.empty(B, 4, dtype=torch.int32, device=dev)
    scores = torch.empty(B, 2 * A + 1, 2 * S + 1, 2 * S + 1, dtype=torch.float64, device=dev) if return_scores and A >= 0 and S >= 0 else None
    ws, ws_bytes = _workspace("svae_pose_search", "refine", dev, B, rows, cols, C, A, S)     # none while plane and volume fit the LDS
    _call("svae_pose_search", dev, yc, ref.contiguous(), weight, ref_index.contiguous(), pose.contiguous(), B, n_ref, rows, cols, C,
          A, float(step), S, _lib.ALIGN_INTERP[interp], out, score, offset, scores, ws, ws_bytes)
    return PoseSearch(out, score, offset, scores)


PoseClassify = namedtuple("PoseClassify", "choice ref_chosen cand_score margin")


def pose_classify(y, ref, weight, cand, pose, rows, cols, angles, step, shift, interp="bicubic", return_margin=True):
    """Each image scored against several references over pose_search's neighbourhood (svae_pose_classify,
    include/svae_classify.h): cand (B, M) int32 names the references of image b slot by slot, an entry outside [0, n_ref) being
    an empty slot; every other argument is pose_search's.  cand_score[b, j] is the best score of the search against ref[cand[b, j]],
    bit for bit what pose_search returns for it, or -inf where that search skips; choice is the first slot of the highest score
    (-1: none), ref_chosen its reference, margin the winner's lead over the best other live slot (+inf with fewer than two).
    Returns PoseClassify(choice (B) int32, ref_chosen (B) int32, cand_score (B, M) float64, margin (B) float64 or None) on the
    device; the pose is not refined (pose_search with ref_index = ref_chosen does that) and nothing is read back."""
    yc, B, N, C, n_ref, weight = _pose_inputs("pose_classify", y, ref, weight, pose, rows, cols, interp, cand)
    A, S, M = int(angles), int(shift), cand.size(1)
    dev = y.device
    choice = torch.empty(B, dtype=torch.int32, device=dev)
    ref_chosen = torch.empty(B, dtype=torch.int32, device=dev)
    cand_score = torch.empty(B, M, dtype=torch.float64, device=dev)
    margin = torch.empty(B, dtype=torch.float64, device=dev) if return_margin else None
    # the norms, + plane slices above the LDS limit
    ws, ws_bytes = _workspace("svae_pose_classify", "classify", dev, B, n_ref, M, rows, cols, C, required=True)
    _call("svae_pose_classify", dev, yc, ref.contiguous(), weight, cand.contiguous(), pose.contiguous(), B, n_ref, M, rows, cols, C,
          A, float(step), S, _lib.ALIGN_INTERP[interp], choice, ref_chosen, cand_score, margin, ws, ws_bytes)
    return PoseClassify(choice, ref_chosen, cand_score, margin)


PoseExpect = namedtuple("PoseExpect", "contrib cover_w class_post log_evidence best")


def pose_expect(y, ref, weight, log_prior, cand, pose, rows, cols, angles, step, shift, inv_sigma2, interp="bicubic"):
    """Each image spread over its candidate references and pose_search's neighbourhood by its posterior under Gaussian noise of
    variance 1 / inv_sigma2 (svae_pose_expect, include/svae_expect.h): cand (B, M <= 64) int32 as pose_classify takes it (a
    repeated reference is dead in its later slots), log_prior (n_ref) float64 or None (= 0), every other argument pose_classify's.
    Returns PoseExpect(contrib (B, M, rows*cols, C) float64: the posterior-weighted sum of the image's shifted candidate planes
    per slot; cover_w (B, M, rows*cols) float64: the same sum of their coverage; class_post (B, M) float64: the posterior of each
    slot; log_evidence (B) float64; best (B, 4) int32 = slot, k, sx, sy of the largest log-weight, slot -1 for a skipped image)
    on the device; nothing is read back."""
    yc, B, N, C, n_ref, weight = _pose_inputs("pose_expect", y, ref, weight, pose, rows, cols, interp, cand)
    if log_prior is not None:
        _require_hip(log_prior, "log_prior")
        if log_prior.dtype != torch.float64 or log_prior.numel() != n_ref:
            raise RuntimeError("pose_expect: log_prior must be %d float64 values, got %s (%s)"
                               % (n_ref, tuple(log_prior.shape), log_prior.dtype))
        log_prior = log_prior.contiguous()
    A, S, M = int(angles), int(shift), cand.size(1)
    dev = y.device
    contrib = torch.empty(B, M, N, C, dtype=torch.float64, device=dev)
    cover_w = torch.empty(B, M, N, dtype=torch.float64, device=dev)
    class_post = torch.empty(B, M, dtype=torch.float64, device=dev)
    log_evidence = torch.empty(B, dtype=torch.float64, device=dev)
    best = torch.empty(B, 4, dtype=torch.int32, device=dev)
    # h, + slices above the LDS limit
    ws, ws_bytes = _workspace("svae_pose_expect", "expect", dev, B, n_ref, M, rows, cols, C, A, S, required=True)
    _call("svae_pose_expect", dev, yc, ref.contiguous(), weight, log_prior, cand.contiguous(), pose.contiguous(), B, n_ref, M, rows,
          cols, C, A, float(step), S, _lib.ALIGN_INTERP[interp], float(inv_sigma2), contrib, cover_w, class_post, log_evidence, best,
          ws, ws_bytes)
    return PoseExpect(contrib, cover_w, class_post, log_evidence, best)


KMeansFit = namedtuple("KMeansFit", "label centres members record seed_index")


class KMeans:
    """k-means of (N, D) fp32 points into k classes on the device (include/svae_cluster.h): k-means++ seeding from host-drawn
    uniforms, then Lloyd steps.  Every sum has a fixed order and nothing is atomic, so the same points and uniforms give the
    same bits; nothing is read back.  A point with a non-finite coordinate gets the label -1 and enters nothing."""

    RECORD_WORDS = ctypes.sizeof(_lib.KMeansRecord) // 8
    MAX_K = 1024                # include/svae_cluster.h's limits on k and D
    MAX_D = 64

    def __init__(self, k, D, device):
        device = _hip_device("KMeans", device)
        self.k, self.D, self.device = int(k), int(D), device
        if not (1 <= self.k <= self.MAX_K and 1 <= self.D <= self.MAX_D):
            raise RuntimeError("KMeans: k = %d must be in 1..%d and D = %d in 1..%d" % (self.k, self.MAX_K, self.D, self.MAX_D))

    def fit(self, points, iters, uniforms):
        """Seed, `iters` update steps and one final assign-only step, all enqueued on the current stream.  points: (N, D) fp32
        contiguous on the device, N >= k; uniforms: k numbers in [0, 1), a host array or a float64 device tensor.  Returns
        KMeansFit of device tensors: label (N) int32, centres (k, D) float64, members (k) int64, record (the svae_kmeans_record
        as 6 int64 words, see read_record; its last word holds the inertia's bits) and seed_index (k) int32."""
        _points("KMeans.fit", points, self.D)
        N, iters = points.size(0), int(iters)
        if N < self.k or iters < 0:
            raise RuntimeError("KMeans.fit: %d points for k = %d, iters = %d" % (N, self.k, iters))
        u = uniforms if torch.is_tensor(uniforms) else torch.from_numpy(np.array(uniforms, dtype=np.float64, order="C"))
        if u.dtype != torch.float64 or u.numel() != self.k:
            raise RuntimeError("KMeans.fit: uniforms must be %d float64 numbers, got %s %s" % (self.k, tuple(u.shape), u.dtype))
        u = u.reshape(-1).to(self.device).contiguous()
        dev, k, D = self.device, self.k, self.D
        ws, _ = _workspace("svae_kmeans", "kmeans", dev, N, D, k,
                           required="KMeans.fit: bad geometry N = %d, D = %d, k = %d" % (N, D, k))
        out = KMeansFit(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(k, D, dtype=torch.float64, device=dev),
                        torch.empty(k, dtype=torch.int64, device=dev), torch.zeros(self.RECORD_WORDS, dtype=torch.int64, device=dev),
                        torch.empty(k, dtype=torch.int32, device=dev))
        _call("svae_kmeans_seed", dev, points, N, D, k, u, out.centres, out.seed_index, ws, ws.numel())
        for update in [1] * iters + [0]:
            _call("svae_kmeans_step", dev, points, N, D, k, update, out.centres, out.label, out.members, out.record, ws, ws.numel())
        return out

    @staticmethod
    def inertia(record):
        """The record's inertia as a one-element float64 device tensor (a view: no synchronisation)."""
        return record[_lib.KMeansRecord.inertia.offset // 8:][:1].view(torch.float64)

    @staticmethod
    def read_record(record):
        """{iterations, changed, converged_at, assigned, empty, inertia} of a record tensor: synchronises."""
        rec = _lib.KMeansRecord()
        ctypes.memmove(ctypes.byref(rec), record.cpu().numpy().tobytes(), ctypes.sizeof(rec))
        out = {name: int(getattr(rec, name)) for name, _ in _lib.KMeansRecord._fields_[:-1]}
        out["inertia"] = float(rec.inertia)
        return out


GmmFit = namedtuple("GmmFit", "weight mean var resp label loglik_point record trace")


class GaussianMixture:
    """A diagonal-covariance Gaussian mixture of (N, D) fp32 points with k components, fitted by EM on the device from a k-means
    result (include/svae_gmm.h).  Every sum has a fixed order and nothing is atomic, so the same inputs give the same bits;
    nothing is read back.  A point with a non-finite coordinate gets the label -1 and an all-zero row of responsibilities."""

    RECORD_WORDS = ctypes.sizeof(_lib.GmmRecord) // 8
    MAX_K = 1024                # include/svae_gmm.h's limits on k and D
    MAX_D = 64

    def __init__(self, k, D, device):
        device = _hip_device("GaussianMixture", device)
        self.k, self.D, self.device = int(k), int(D), device
        if not (1 <= self.k <= self.MAX_K and 1 <= self.D <= self.MAX_D):
            raise RuntimeError("GaussianMixture: k = %d must be in 1..%d and D = %d in 1..%d" % (self.k, self.MAX_K, self.D, self.MAX_D))

    def fit(self, points, label, centres, iters, reg=1e-6, tol=1e-8):
        """svae_gmm_init from the k-means `label` (N) int32 and `centres` (k, D) float64, `iters` update steps and one labelling
        step, all enqueued on the current stream; after each step the record's loglik is copied device-to-device into trace.
        points: (N, D) fp32 contiguous on the device, N >= k.  Returns GmmFit of device tensors: weight (k), mean (k, D),
        var (k, D) and resp (N, k) float64, label (N) int32, loglik_point (N) float64, record (the svae_gmm_record as 6 int64
        words, see read_record) and trace (iters + 1) float64.  The inputs are left as they were."""
        _points("GaussianMixture.fit", points, self.D)
        N, iters, reg, tol = points.size(0), int(iters), float(reg), float(tol)
        dev, k, D = self.device, self.k, self.D
        if N < k or iters < 0:
            raise RuntimeError("GaussianMixture.fit: %d points for k = %d, iters = %d" % (N, k, iters))
        if not (math.isfinite(reg) and reg > 0 and math.isfinite(tol) and tol >= 0):
            raise RuntimeError("GaussianMixture.fit: reg = %r must be finite and > 0, tol = %r finite and >= 0" % (reg, tol))
        if not torch.is_tensor(label) or label.dtype != torch.int32 or tuple(label.shape) != (N,) or not label.is_cuda:
            raise RuntimeError("GaussianMixture.fit: label must be %d int32 numbers on the device" % N)
        if not torch.is_tensor(centres) or centres.dtype != torch.float64 or tuple(centres.shape) != (k, D) or not centres.is_cuda:
            raise RuntimeError("GaussianMixture.fit: centres must be a (%d, %d) float64 tensor on the device" % (k, D))
        ws, _ = _workspace("svae_gmm", "gmm", dev, N, D, k,
                           required="GaussianMixture.fit: bad geometry N = %d, D = %d, k = %d" % (N, D, k))
        f64 = dict(dtype=torch.float64, device=dev)
        out = GmmFit(torch.empty(k, **f64), centres.contiguous().clone(), torch.empty(k, D, **f64), torch.empty(N, k, **f64),
                     torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, **f64),
                     torch.zeros(self.RECORD_WORDS, dtype=torch.int64, device=dev), torch.empty(iters + 1, **f64))
        _call("svae_gmm_init", dev, points, N, D, k, label.contiguous(), reg, out.weight, out.mean, out.var, out.resp, out.record, ws,
              ws.numel())
        loglik = self.loglik(out.record)
        for i, update in enumerate([1] * iters + [0]):
            _call("svae_gmm_step", dev, points, N, D, k, update, reg, tol, out.weight, out.mean, out.var, out.resp, out.label,
                  out.loglik_point, out.record, ws, ws.numel())
            out.trace[i:i + 1].copy_(loglik)
        return out

    @staticmethod
    def loglik(record):
        """The record's loglik as a one-element float64 device tensor (a view: no synchronisation)."""
        return record[_lib.GmmRecord.loglik.offset // 8:][:1].view(torch.float64)

    @staticmethod
    def read_record(record):
        """{iterations, converged_at, assigned, dead, loglik, previous} of a record tensor: synchronises."""
        rec = _lib.GmmRecord()
        ctypes.memmove(ctypes.byref(rec), record.cpu().numpy().tobytes(), ctypes.sizeof(rec))
        out = {name: int(getattr(rec, name)) for name, _ in _lib.GmmRecord._fields_[:4]}
        out.update(loglik=float(rec.loglik), previous=float(rec.previous))
        return out


PcaFit = namedtuple("PcaFit", "count mean cov eigenvalues components sweeps off_norm proj")


class LatentPCA:
    """The principal axes of (N, D) fp32 points on the device, globally or per group (include/svae_pca.h): mean and covariance
    in two ordered passes, cyclic Jacobi per covariance, every point's coordinates along its group's axes.  Every sum and
    rotation has a fixed order and nothing is atomic, so the same inputs give the same bits; nothing is read back."""

    MAX_GROUPS = 1024
    MAX_PARTIALS = 32768        # G * D (D + 1) / 2

    def __init__(self, D, device):
        device = _hip_device("LatentPCA", device)
        self.D, self.device = int(D), device
        if not 1 <= self.D <= 64:
            raise RuntimeError("LatentPCA: D = %d must be in 1..64" % self.D)

    @classmethod
    def max_groups(cls, D):
        """The most groups one call takes for points of D coordinates."""
        return min(cls.MAX_GROUPS, cls.MAX_PARTIALS // (D * (D + 1) // 2))

    def fit(self, points, group=None, G=1, P=None):
        """svae_pca_moments, svae_pca_eigen and svae_pca_project, enqueued on the current stream.  points: (N, D) fp32 contiguous
        on the device; group: (N) int32 on the device with entries in [0, G) (any other entry: in no group), or None with G == 1;
        P: the columns of proj, 1..D (default D).  Returns PcaFit of device tensors: count (G) int64, mean (G, D), cov (G, D, D),
        eigenvalues (G, D) descending, components (G, D, D) with rows as axes, sweeps (G) int32, off_norm (G) and proj (N, P)."""
        _points("LatentPCA.fit", points, self.D)
        N, D, G, dev = points.size(0), self.D, int(G), self.device
        P = D if P is None else int(P)
        if not 1 <= P <= D:
            raise RuntimeError("LatentPCA.fit: P = %d must be in 1..%d" % (P, D))
        if group is None:
            if G != 1:
                raise RuntimeError("LatentPCA.fit: without a group tensor G must be 1 (got %d)" % G)
        elif not torch.is_tensor(group) or group.dtype != torch.int32 or tuple(group.shape) != (N,) or not group.is_cuda:
            raise RuntimeError("LatentPCA.fit: group must be %d int32 numbers on the device" % N)
        ws, _ = _workspace("svae_pca", "pca", dev, N, D, G, required="LatentPCA.fit: bad geometry N = %d, D = %d, G = %d (G D (D + 1) / 2 "
                           "<= %d)" % (N, D, G, self.MAX_PARTIALS))
        group = None if group is None else group.contiguous()
        f64 = dict(dtype=torch.float64, device=dev)
        out = PcaFit(torch.empty(G, dtype=torch.int64, device=dev), torch.empty(G, D, **f64), torch.empty(G, D, D, **f64),
                     torch.empty(G, D, **f64), torch.empty(G, D, D, **f64), torch.empty(G, dtype=torch.int32, device=dev),
                     torch.empty(G, **f64), torch.empty(N, P, **f64))
        _call("svae_pca_moments", dev, points, N, D, G, group, out.count, out.mean, out.cov, ws, ws.numel())
        _call("svae_pca_eigen", dev, out.cov, D, G, out.eigenvalues, out.components, out.sweeps, out.off_norm)
        _call("svae_pca_project", dev, points, N, D, G, P, group, out.count, out.mean, out.components, out.proj)
        return out


EigenFit = namedtuple("EigenFit", "members ssq eigenvalues eigenimages residual coords sweeps off_norm")


class EigenImages:
    """The leading eigenimages of every class's aligned members about their class average (include/svae_eigen.h): block subspace
    iteration with R columns per class, the covariance never formed.  start() takes the (K, D, R) start array; a pass is
    begin_pass(), update() per minibatch in dataset order (svae_eig_project, svae_eig_accumulate) and end_pass() (the basis made
    orthonormal again) -- or, after the last pass, finish() (svae_eig_gram, svae_pca_eigen, svae_eig_rotate, svae_eig_coords).
    Every sum has a fixed order and nothing is atomic, so the same sequence of calls gives the same bits; nothing is read back."""

    MAX_R = _lib.EIGEN_LIMITS["max_r"]
    MAX_CLASSES = 4096
    MAX_BASIS = 1 << 28         # K * D * R

    def __init__(self, n_classes, N, C, R, device):
        device = _hip_device("EigenImages", device)
        self.K, self.N, self.C, self.R, self.device = int(n_classes), int(N), int(C), int(R), device
        self.D = self.N * self.C
        if not (1 <= self.K <= self.MAX_CLASSES and self.N >= 1 and 1 <= self.C <= _lib.MAX_OUT and 1 <= self.R <= self.MAX_R
                and self.K * self.D * self.R <= self.MAX_BASIS):
            raise RuntimeError("EigenImages: bad n_classes = %d, N = %d, C = %d or R = %d (n_classes <= %d, R <= %d, "
                               "n_classes * N * C * R <= 2^28)" % (self.K, self.N, self.C, self.R, self.MAX_CLASSES, self.MAX_R))
        f64 = dict(dtype=torch.float64, device=device)
        self.Q = torch.empty(self.K, self.D, self.R, **f64)
        self.Y = torch.zeros(self.K, self.D, self.R, **f64)
        self.ssq = torch.zeros(self.K, self.D, **f64)
        self.members = torch.zeros(self.K, dtype=torch.int64, device=device)
        self._classes = torch.arange(self.K, dtype=torch.int32, device=device).unsqueeze(0)
        self.passes, self._rows, self._labels = 0, [], []

    def start(self, array):
        """The basis of the first pass: `array` (K, D, R) float64 on the device, made orthonormal per class."""
        _require_hip(array, "array")
        if array.dtype != torch.float64 or tuple(array.shape) != (self.K, self.D, self.R) or not array.is_contiguous():
            raise RuntimeError("EigenImages.start: the start array must be a contiguous (%d, %d, %d) float64 tensor, got %s %s"
                               % (self.K, self.D, self.R, tuple(array.shape), array.dtype))
        _call("svae_eig_orthonormalise", self.device, array, self.K, self.D, self.R, self.Q)

    def begin_pass(self):
        self.Y.zero_()
        self._rows, self._labels = [], []

    def update(self, aligned, cover, label, mean):
        """One minibatch: aligned (B, N[, C]) fp32 and cover (B, N) uint8 or None as align_images returns them, label (B) int32,
        -1 = in no class, mean (K, N, C) float64 the class averages.  The first pass also counts the members and sums the squares."""
        for name, t in (("aligned", aligned), ("cover", cover), ("label", label), ("mean", mean)):
            if t is not None:
                _require_hip(t, name)
        B = label.numel()
        aligned = _f32(aligned)
        if label.dtype != torch.int32 or (cover is not None and cover.dtype != torch.uint8) or mean.dtype != torch.float64:
            raise RuntimeError("EigenImages.update: label must be int32, cover uint8 and mean float64")
        if aligned.numel() != B * self.D or (cover is not None and cover.numel() != B * self.N) or mean.numel() != self.K * self.D:
            raise RuntimeError("EigenImages.update: aligned %s / cover %s / mean %s do not fit %d images of %d pixels, %d channels in "
                               "%d classes" % (tuple(aligned.shape), None if cover is None else tuple(cover.shape), tuple(mean.shape),
                                               B, self.N, self.C, self.K))
        first = self.passes == 0
        T = torch.empty(B, self.R, dtype=torch.float64, device=self.device)
        _call("svae_eig_project", self.device, aligned, cover, label, mean, self.Q, B, self.N, self.C, self.K, self.R, T)
        _call("svae_eig_accumulate", self.device, aligned, cover, label, mean, T, B, self.N, self.C, self.K, self.R, self.Y,
              self.ssq if first else None)
        if first:
            self.members += (label.unsqueeze(1) == self._classes).sum(0)
        self._rows.append(T)
        self._labels.append(label)

    def end_pass(self):
        """Between two passes: Q <- the orthonormalised Y."""
        _call("svae_eig_orthonormalise", self.device, self.Y, self.K, self.D, self.R, self.Q)
        self.passes += 1

    def finish(self, P):
        """After the last pass's updates (no end_pass): the Rayleigh-Ritz step.  Returns EigenFit of device tensors: members (K)
        int64, ssq (K, D), eigenvalues (K, R) descending, eigenimages (K, P, D), residual (K, P), coords (images, P) in the order
        of the last pass's updates, sweeps (K) int32 and off_norm (K) of svae_pca_eigen."""
        K, D, R, P, dev = self.K, self.D, self.R, int(P), self.device
        if not 1 <= P <= R:
            raise RuntimeError("EigenImages.finish: P = %d must be in 1..%d" % (P, R))
        if not self._rows:
            raise RuntimeError("EigenImages.finish: no pass has been walked")
        f64 = dict(dtype=torch.float64, device=dev)
        G, W, lam = torch.empty(K, R, R, **f64), torch.empty(K, R, R, **f64), torch.empty(K, R, **f64)
        sweeps, off_norm = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, **f64)
        _call("svae_eig_gram", dev, self.Q, self.Y, self.members, K, D, R, G)
        step = LatentPCA.max_groups(R)
        for lo in range(0, K, step):
            g = min(step, K - lo)
            _call("svae_pca_eigen", dev, G[lo:lo + g], R, g, lam[lo:lo + g], W[lo:lo + g], sweeps[lo:lo + g], off_norm[lo:lo + g])
        images, residual, rot = torch.empty(K, P, D, **f64), torch.empty(K, P, **f64), torch.empty(K, P, R, **f64)
        _call("svae_eig_rotate", dev, self.Q, self.Y, W, lam, self.members, K, D, R, P, images, residual, rot)
        T, label = torch.cat(self._rows), torch.cat(self._labels)
        coords = torch.empty(T.size(0), P, **f64)
        _call("svae_eig_coords", dev, T, label, rot, T.size(0), K, R, P, coords)
        self.passes += 1
        return EigenFit(self.members, self.ssq, lam, images, residual, coords, sweeps, off_norm)


class NeighbourSearch:
    """The running lists of every image's K nearest neighbours under the order (squared distance, image index)
    (svae_nbr_search, include/svae_neighbours.h): d2 (images, K) float64 and index (images, K) int64 on the device, filled with
    the empty slot (+inf, -1).  update() offers the images cand_base.. to the images query_base..; the lists are a property of
    the set offered, whatever the split into calls.  Nothing is read back."""

    MAX_K = _lib.NEIGHBOUR_LIMITS["max_k"]
    MAX_D = 512

    def __init__(self, images, K, device):
        device = _hip_device("NeighbourSearch", device)
        self.images, self.K, self.device = int(images), int(K), device
        if self.images < 1 or not 1 <= self.K <= self.MAX_K:
            raise RuntimeError("NeighbourSearch: bad images = %d or K = %d (K in 1..%d)" % (self.images, self.K, self.MAX_K))
        self.d2 = torch.full((self.images, self.K), float("inf"), dtype=torch.float64, device=device)
        self.index = torch.full((self.images, self.K), -1, dtype=torch.int64, device=device)

    def update(self, query, query_base, cand, cand_base):
        """One call: query (B, D) and cand (M, D) float64 contiguous on the device, the latents of the images query_base .. and
        cand_base ..; the rows query_base .. query_base + B - 1 of the lists are updated."""
        _require_hip(query, "query")
        _require_hip(cand, "cand")
        q0, c0 = int(query_base), int(cand_base)
        if (query.dtype != torch.float64 or cand.dtype != torch.float64 or query.dim() != 2 or cand.dim() != 2
                or query.size(1) != cand.size(1) or not 1 <= query.size(1) <= self.MAX_D or query.size(0) < 1 or cand.size(0) < 1):
            raise RuntimeError("NeighbourSearch.update: query %s %s and cand %s %s must be float64 (B, D) and (M, D) with D in 1..%d"
                               % (tuple(query.shape), query.dtype, tuple(cand.shape), cand.dtype, self.MAX_D))
        B = query.size(0)
        if q0 < 0 or c0 < 0 or q0 + B > self.images:
            raise RuntimeError("NeighbourSearch.update: the queries %d .. %d are not among the %d images" % (q0, q0 + B - 1, self.images))
        _call("svae_nbr_search", self.device, query, B, q0, cand, cand.size(0), c0, query.size(1), self.K, self.d2[q0:q0 + B],
              self.index[q0:q0 + B])

    def lists(self):
        """(d2, index): the device tensors."""
        return self.d2, self.index


def neighbour_average(stack, cover, index, weight=None, support=False):
    """svae_nbr_average: stack (images, N[, C]) fp32 and cover (images, N) uint8 or None as align_images returns them, index
    (B, T) int64 with -1 for an empty slot, weight (B, T) float64 or None for all 1.  Returns average (B, N, C) fp32, and with
    support=True (average, support (B, N) float64): device tensors."""
    for name, t in (("stack", stack), ("cover", cover), ("index", index), ("weight", weight)):
        if t is not None:
            _require_hip(t, name)
    if stack.dim() == 2:
        stack = stack.unsqueeze(2)
    if stack.dtype != torch.float32 or stack.dim() != 3 or index.dtype != torch.int64 or index.dim() != 2:
        raise RuntimeError("neighbour_average: stack must be float32 (images, N, C) and index int64 (B, T), got %s %s and %s %s"
                           % (tuple(stack.shape), stack.dtype, tuple(index.shape), index.dtype))
    images, N, C = stack.shape
    B, T = index.shape
    if cover is not None and (cover.dtype != torch.uint8 or tuple(cover.shape) != (images, N)):
        raise RuntimeError("neighbour_average: cover must be uint8 (%d, %d), got %s %s" % (images, N, tuple(cover.shape), cover.dtype))
    if weight is not None and (weight.dtype != torch.float64 or tuple(weight.shape) != (B, T)):
        raise RuntimeError("neighbour_average: weight must be float64 (%d, %d), got %s %s" % (B, T, tuple(weight.shape), weight.dtype))
    average = torch.empty(B, N, C, dtype=torch.float32, device=stack.device)
    sup = torch.empty(B, N, dtype=torch.float64, device=stack.device) if support else None
    _call("svae_nbr_average", stack.device, stack, cover, images, N, C, index, weight, B, T, average, sup)
    return (average, sup) if support else average


def ctf_filter(table, n, m, scale=1.0, device=None):
    """(P, n, m) real-space CTF filters on the device from the (P, 8) parameter table of spatial_vae/ctf.py:26-30
    (svae_ctf_filter; the reference builds them one particle at a time with numpy, ctf.py:33-56)."""
    tab = torch.as_tensor(np.ascontiguousarray(table, dtype=np.float64))
    if tab.dim() != 2 or tab.size(1) != 8:
        raise RuntimeError("ctf_filter: expected a (P, 8) parameter table, got %s" % (tuple(tab.shape),))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    tab = tab.to(dev)
    _require_hip(tab, "CTF table")
    out = torch.empty(tab.size(0), n, m, dtype=torch.float32, device=dev)
    L = _lib.lib()
    ws_bytes = L.svae_ctf_filter_workspace_bytes(tab.size(0), n, m)    # 0 while a filter's transform fits the LDS (~80 x 80)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    _call("svae_ctf_filter", dev, tab, out, tab.size(0), n, m, float(scale), ws, ws_bytes)
    return out


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam's update (amsgrad off, no weight decay) for ONE flat fp32 CUDA parameter, executed by
    svae_adam_step.  Same defaults and state names (step, exp_avg, exp_avg_sq) as torch.optim.Adam.

    max_grad_norm / skip_nonfinite switch step() to the guarded pair of calls (svae_grad_guard_norm +
    svae_adam_step_guarded): torch.nn.utils.clip_grad_norm_(p, max_grad_norm) and "leave parameters and moments alone when
    the gradient's norm is not finite", decided on the device -- step() reads nothing back.  skip_nonfinite alone clips at
    +inf, i.e. never.  In that mode state["step"] is a one-element int64 CUDA tensor (torch.optim.Adam's own convention for
    a device-resident count) aliasing the control record's `t`: it counts the updates APPLIED."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, zero_grad=False, max_grad_norm=None,
                 skip_nonfinite=False):
        """zero_grad=True: step() also clears each parameter's .grad buffer in the same kernel (the loop's
        optim.zero_grad(), train_mnist.py:150, without a second pass)."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.zero_grad_in_step = bool(zero_grad)
        self.guarded = max_grad_norm is not None or bool(skip_nonfinite)
        self.max_grad_norm = math.inf if max_grad_norm is None else float(max_grad_norm)
        if not self.max_grad_norm > 0:
            raise ValueError("FlatAdam: max_grad_norm must be > 0, got %r" % (max_grad_norm,))
        if self.guarded and sum(len(g["params"]) for g in self.param_groups) != 1:
            raise RuntimeError("FlatAdam: the gradient guard takes the GLOBAL norm of one flat parameter; got several")

    def init_state(self, p):
        """The state the first step() would create (zero moments, step 0); guarded: plus the zeroed control record."""
        st = self.state[p]
        if not st:
            if self.guarded:
                _require_hip(p, "FlatAdam parameter")
                words = (ctypes.sizeof(_lib.GuardControl) + 7) // 8
                st["guard"] = torch.zeros(words, dtype=torch.int64, device=p.device)     # all zero bytes = a fresh record
                st["step"] = st["guard"][:1]                                             # svae_guard_control.t
            else:
                st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        return st

    def guard_stats(self, reset=False):
        """{steps, clipped, skipped, mean_norm, max_norm, last_norm} since the last reset, read from the control record: the
        ONE place of the guard that synchronises.  reset=True clears the statistics (not the step count) behind the read."""
        if not self.guarded:
            raise RuntimeError("FlatAdam.guard_stats: built without max_grad_norm / skip_nonfinite")
        p = self.param_groups[0]["params"][0]
        rec = _lib.GuardControl()
        st = self.state.get(p)
        if st:
            raw = st["guard"].cpu().numpy().tobytes()
            ctypes.memmove(ctypes.byref(rec), raw, ctypes.sizeof(rec))
            if reset:
                st["guard"][_lib.GuardControl.steps.offset // 8:].zero_()
        applied = rec.steps - rec.skipped
        return {"steps": int(rec.steps), "clipped": int(rec.clipped), "skipped": int(rec.skipped),
                "mean_norm": rec.norm_sum / applied if applied else float("nan"), "max_norm": float(rec.norm_max),
                "last_norm": float(rec.total)}

    @torch.no_grad()
    def step(self, closure=None):
        L = _lib.lib()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                _require_hip(p, "FlatAdam parameter")
                if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous():
                    raise RuntimeError("FlatAdam needs contiguous fp32 parameters and gradients")
                st = self.init_state(p)
                zero = 1 if self.zero_grad_in_step else 0
                if self.guarded:
                    ws_bytes = L.svae_grad_guard_workspace_bytes(p.numel())
                    ws = _buf(p.device, ws_bytes, "guard")
                    _call("svae_grad_guard_norm", p.device, p.grad, p.numel(), self.max_grad_norm, group["lr"], b1, b2,
                          st["guard"], ws, ws.numel())
                    _call("svae_adam_step_guarded", p.device, p, p.grad, st["exp_avg"], st["exp_avg_sq"], p.numel(), b1, b2,
                          group["eps"], zero, st["guard"])
                    continue
                st["step"] += 1
                _call("svae_adam_step", p.device, p, p.grad, st["exp_avg"], st["exp_avg_sq"], p.numel(), group["lr"], b1, b2,
                      group["eps"], st["step"], zero)
