"""ELBO of one minibatch -- the three eval_minibatch functions of the reference, host side.

  eval_minibatch_mnist      <- /root/reference/train_mnist.py:24-90
  eval_minibatch_galaxy     <- /root/reference/train_galaxy.py:27-128
  eval_minibatch_particles  <- /root/reference/train_particles.py:22-148

Same positional arguments and return tuples.  The encoder is the caller's torch module; from its output
onward everything -- reparameterisation, pose split and KL terms (one small kernel), pose, decoder and
log-likelihood (everything that touches B*N rows) -- goes through the HIP library (ops.py).  Differences from the
reference, all additive: `noise=` lets a caller supply the N(0,1) draw (parity tests; data-parallel
runs that slice one global draw), `return_logits=` also returns the pre-Sigmoid output, `offset=` supplies the
augmentation angles (radians) instead of the np.random draw.
`augment_rotation` (train_galaxy.py:41-54, train_particles.py:31-43) rotates the observed images before inference
with the device restatement of Pillow's bicubic Image.rotate (ops.rotate_augment) instead of a per-image PIL loop on
the host; the angles come from np.random exactly as in the reference.
"""
import collections
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops


_ENC_ACT_NAMES = {nn.Tanh: "tanh", nn.LeakyReLU: "leakyrelu", nn.ReLU: "relu", nn.Sigmoid: "sigmoid"}


def _fusable_act(m):
    """Name of an activation module the small-batch Linear kernel can fold into its epilogue, else None."""
    name = _ENC_ACT_NAMES.get(type(m))
    if name == "leakyrelu" and m.negative_slope != 0.01:
        return None
    return name


def _encode(q_net, y2d):
    """Raw encoder output [z_mu | z_logstd] (B, 2*inf_dim): InferenceNetwork.forward is layers(x) split in two
    (models.py:46-54); any other encoder's two outputs are concatenated back.

    On the device the plain Linear layers of InferenceNetwork.layers run through ops.enc_linear -- one launch per layer
    forward (bias + activation in the epilogue) and one backward (dW, db, dx) -- with the gradient sinks of dp.TrainStep when
    they are set (views into its flat buffer: no AccumulateGrad adds).  Layers the kernel does not cover (ResidLinear, weights
    above 4 M elements such as the galaxy encoder's 49 152 x 5 000 first layer) stay torch ops (ops.sink_linear / the module)."""
    if hasattr(q_net, "layers") and hasattr(q_net, "latent_dim"):
        sinks = getattr(q_net, "_grad_sinks", None) or {}
        sinks = sinks if torch.is_grad_enabled() else {}
        if not y2d.is_cuda:
            return q_net.layers(y2d)
        mods = list(q_net.layers)
        h = y2d
        idx = 0
        while idx < len(mods):
            m = mods[idx]
            if isinstance(m, nn.Linear) and m.bias is not None:
                sw, sb = sinks.get("layers.%d.weight" % idx), sinks.get("layers.%d.bias" % idx)
                if ops.enc_linear_applies(h, m.weight):
                    act = _fusable_act(mods[idx + 1]) if idx + 1 < len(mods) else None
                    h = ops.enc_linear(h, m.weight, m.bias, act, sw, sb)
                    idx += 2 if act is not None else 1
                    continue
                if sw is not None:
                    # data parallel: a layer this large exchanges the two factors of its weight gradient, not the gradient
                    coll = sinks.get("__lowrank__")
                    key = "layers.%d" % idx
                    h = ops.sink_linear(h, m.weight, m.bias, sw, sb, coll if (coll is not None and coll.has(key)) else None, key)
                    idx += 1
                    continue
            h = m(h)
            idx += 1
        return h
    z_mu, z_logstd = q_net(y2d)
    return torch.cat([z_mu, z_logstd], 1)


def draw_offsets(rotate, B):
    """The augmentation angles of train_galaxy.py:43-46 / train_particles.py:33-36 from np.random, in the reference's
    draw order."""
    offset = np.random.uniform(0, 2 * np.pi, size=B)
    if rotate < 1:
        offset = offset * np.random.binomial(1, p=rotate, size=B)
    return offset


def _augment(script, y, rotate, offset):
    """The reference's augmentation block: offset ~ U(0, 2 pi) per image from np.random (times a Bernoulli(rotate) when
    rotate is a probability < 1), image i rotated by offset[i] -- through uint8 for galaxy images
    (train_galaxy.py:44-54), as float32 for particles (train_particles.py:35-43)."""
    B = y.size(0)
    if offset is None:
        offset = draw_offsets(rotate, B)
    offset = np.asarray(offset, np.float64)
    side = int(np.sqrt(y.size(1)))
    return ops.rotate_augment(y, offset, side, side, quantize_u8=(script == "galaxy")), offset


def _decode_score(script, x, y, p_net, B, theta, dx, zc, mask, ctf):
    """Pose -> decoder -> per-row log-likelihood for B rows (images, or samples of images): (y_hat, logits, loglik)."""
    loglik = None
    if hasattr(p_net, "forward_posed"):
        if script == "particles" or getattr(p_net, "softplus", False):
            y_hat, logits = p_net.forward_posed(x, B, theta=theta, dx=dx, z=zc, return_logits=True)
        else:   # Bernoulli likelihood: scored inside the decoder call (no second pass over y_hat, no scaling pass backward)
            y_hat, logits, loglik = p_net.forward_posed(x, B, theta=theta, dx=dx, z=zc, bce_target=y)
    else:                                           # --vanilla baseline: ignores coordinates
        y_hat, logits = p_net(x, zc), None

    if script == "particles":
        loglik = ops.gaussian_loglik(y_hat.reshape(B, -1), y.view(B, -1), mask=mask, ctf=ctf)
    elif loglik is None:
        loglik = ops.bce_loglik(y_hat.reshape(B, -1), y.reshape(B, -1))
    return y_hat, logits, loglik


def _core(script, x, y, p_net, q_net, rotate, translate, dx_scale, theta_prior, z_scale, mask, ctf, noise, use_cuda,
          augment_rotation=False, offset=None, num_samples=1):
    B = y.size(0)
    K = int(num_samples)
    if K < 1:
        raise RuntimeError("num_samples must be >= 1, got %d" % K)
    if use_cuda:
        y = y.cuda()
    y_in = y
    if rotate and augment_rotation:
        y_in, offset = _augment(script, y, rotate, offset)
    else:
        offset = None
    q_out = _encode(q_net, y_in.view(B, -1))
    inf_dim = q_out.size(1) // 2
    # E_q[log p(x|z)] by one reparameterised sample (train_mnist.py:36-39); the draw itself stays a torch call
    r = noise if noise is not None else torch.empty(B * K, inf_dim, device=x.device, dtype=q_out.dtype).normal_()
    if K > 1:
        # the K-sample importance-weighted bound: one encoder output per image, K draws from it; from here to the head the
        # B * K samples are B * K images to the unchanged decoder and likelihood kernels (row b * K + k = sample k of image b)
        if tuple(r.shape) != (B * K, inf_dim):
            raise RuntimeError("noise must be (%d, %d) for %d samples of %d images, got %s"
                               % (B * K, inf_dim, K, B, tuple(r.shape)))
        theta, dx, zc, kl_b = ops.latent_head_iw(q_out, r, K, rotate, translate, script == "mnist", dx_scale, z_scale,
                                                 theta_prior)       # kl_b: log p(z) - log q(z|x) per sample
        y = y.repeat_interleave(K, 0)
        if ctf is not None:
            ctf = ctf.repeat_interleave(K, 0)
        B = B * K
    else:
        # reparameterise + pose split + KL terms in one kernel (train_mnist.py:33-39, 42-72, 61-63, 83-85)
        theta, dx, zc, kl_b = ops.latent_head(q_out, r, rotate, translate, script == "mnist", dx_scale, z_scale, theta_prior)
    if offset is not None and np.any(offset > 0):
        # invert the random rotation: reconstruct the original with the offset added (train_galaxy.py:84-87)
        turn = torch.from_numpy(offset).float().to(theta.device)
        theta = theta + (turn.repeat_interleave(K) if K > 1 else turn)

    y_hat, logits, loglik = _decode_score(script, x, y, p_net, B, theta, dx, zc, mask, ctf)
    if K > 1:
        elbo, log_p_x_g_z, kl_div = ops.iw_head(loglik, kl_b, K)    # log-mean-exp over each image's samples, then the batch means
    else:
        elbo, log_p_x_g_z, kl_div = ops.elbo_head(loglik, kl_b)     # the two batch means and their difference, one kernel
    return elbo, log_p_x_g_z, kl_div, y_hat, logits


def eval_minibatch_mnist(x, y, p_net, q_net, rotate=True, translate=True, dx_scale=0.1, theta_prior=math.pi,
                         use_cuda=False, noise=None, return_logits=False, num_samples=1):
    elbo, log_p, kl, y_hat, logits = _core("mnist", x, y, p_net, q_net, rotate, translate, dx_scale, theta_prior, 1,
                                           None, None, noise, use_cuda, num_samples=num_samples)
    out = (elbo, log_p, kl, y_hat.view(y.size(0) * num_samples, -1))
    return out + (logits,) if return_logits else out


def eval_minibatch_galaxy(x, y, p_net, q_net, rotate=True, translate=True, dx_scale=0.1, theta_prior=math.pi,
                          augment_rotation=False, z_scale=1, use_cuda=False, noise=None, return_logits=False, offset=None,
                          num_samples=1):
    channels = y.size(2)
    elbo, log_p, kl, y_hat, logits = _core("galaxy", x, y, p_net, q_net, rotate, translate, dx_scale, theta_prior,
                                           z_scale, None, None, noise, use_cuda, augment_rotation, offset, num_samples)
    out = (elbo, log_p, kl, y_hat.view(y.size(0) * num_samples, -1, channels))
    return out + (logits,) if return_logits else out


def eval_minibatch_particles(x, y, mask, ctf, p_net, q_net, rotate=True, translate=True, dx_scale=0.1,
                             theta_prior=math.pi, augment_rotation=False, z_scale=1, use_cuda=False, noise=None,
                             return_logits=False, offset=None, num_samples=1):
    elbo, log_p, kl, y_hat, logits = _core("particles", x, y, p_net, q_net, rotate, translate, dx_scale, theta_prior,
                                           z_scale, mask, ctf, noise, use_cuda, augment_rotation, offset, num_samples)
    out = (elbo, log_p, kl)
    return out + (logits,) if return_logits else out


# ---------------------------------------------------------------- per-image scoring (infer.py)
RowLayout = collections.namedtuple("RowLayout", "theta dx content z_dim inf_dim iw best width")


def row_layout(rotate, translate, inf_dim):
    """Where things are in what score_minibatch returns, the one statement of it.  theta, dx, content: the column slices of a
    latent row (inf_dim wide: "q_mu", "q_std", the noise), theta and dx empty when the model has no such coordinate; z_dim: the
    width of content.  iw, best: the slices of a "per_image" row (as svae_iw_stream_finish lays it out, `width` = 6 + 2 * inf_dim
    columns) that hold the importance-weighted mean and the best sample, each one latent row."""
    off = 1 if rotate else 0
    c0 = off + (2 if translate else 0)
    return RowLayout(slice(0, off), slice(off, c0), slice(c0, inf_dim), inf_dim - c0, inf_dim,
                     slice(6, 6 + inf_dim), slice(6 + inf_dim, 6 + 2 * inf_dim), 6 + 2 * inf_dim)


@torch.no_grad()
def score_minibatch(script, x, y, p_net, q_net, *, num_samples, chunk, rotate, translate, dx_scale, theta_prior, z_scale=1,
                    mask=None, ctf=None, noise=None, return_best=False):
    """Per-image K-sample scores of one minibatch with K unbounded: the encoder runs ONCE, then each chunk of at most `chunk`
    samples per image goes through ops.latent_head_iw on the same q_out, the unchanged decoder and log-likelihood calls on
    B * chunk rows, and ops.IWStream.update; peak memory is that of a B * chunk minibatch.  No counterpart in the reference.
    noise: (B * num_samples, inf_dim), row b * num_samples + k = sample k of image b; chunk c of image b takes its rows
    [c0, c1).  Returns {"per_image": (B, 6 + 2 * inf_dim) as svae_iw_stream_finish lays it out, "out3": {bound, log p(x|z),
    Monte-Carlo KL} means, "q_mu", "q_std": the encoder's posterior per coordinate, translation and content in the decoder's
    units (times dx_scale / z_scale)}, and with return_best "y_best": the posed reconstruction at each image's best sample."""
    K, C = int(num_samples), int(chunk)
    if K < 1:
        raise RuntimeError("num_samples must be >= 1, got %d" % K)
    if not 1 <= C <= ops._lib.IW_MAX_SAMPLES:
        raise RuntimeError("chunk must be in [1, %d], got %d" % (ops._lib.IW_MAX_SAMPLES, C))
    B = y.size(0)
    q_out = _encode(q_net, y.view(B, -1))
    inf_dim = q_out.size(1) // 2
    if noise is not None:
        if tuple(noise.shape) != (B * K, inf_dim):
            raise RuntimeError("noise must be (%d, %d) for %d samples of %d images, got %s"
                               % (B * K, inf_dim, K, B, tuple(noise.shape)))
        noise = noise.view(B, K, inf_dim)
    stream = ops.IWStream(B, inf_dim, q_out.device)
    rep = {}                                        # the observed images (and filters) repeated per sample, by chunk size
    for c0 in range(0, K, C):
        kc = min(C, K - c0)
        if noise is not None:
            r = noise[:, c0:c0 + kc].reshape(B * kc, inf_dim)
        else:
            r = torch.empty(B * kc, inf_dim, device=q_out.device, dtype=torch.float32).normal_()
        theta, dx, zc, log_ratio = ops.latent_head_iw(q_out, r, kc, rotate, translate, script == "mnist", dx_scale, z_scale,
                                                      theta_prior)
        if kc not in rep:
            rep = {kc: (y.repeat_interleave(kc, 0), None if ctf is None else ctf.repeat_interleave(kc, 0))}
        y_k, ctf_k = rep[kc]
        _, _, loglik = _decode_score(script, x, y_k, p_net, B * kc, theta, dx, zc, mask, ctf_k)
        stream.update(rotate, translate, script == "mnist", dx_scale, z_scale, theta_prior, kc, loglik, log_ratio, theta, dx, zc)
    per_image, out3 = stream.finish()
    lay = row_layout(rotate, translate, inf_dim)
    unit = torch.ones(inf_dim, device=q_out.device)
    unit[lay.dx] = float(dx_scale)
    unit[lay.content] = float(z_scale)
    out = {"per_image": per_image, "out3": out3, "q_mu": q_out[:, :inf_dim] * unit, "q_std": torch.exp(q_out[:, inf_dim:]) * unit}
    if return_best:
        best = per_image[:, lay.best]
        theta = best[:, 0].contiguous() if rotate else None
        dx = best[:, lay.dx].contiguous() if translate else None
        zc = best[:, lay.content].contiguous()
        out["y_best"] = _decode_score(script, x, y, p_net, B, theta, dx, zc, mask, ctf)[0]
    return out


POSES = ("iw", "best", "q")     # which estimate of an image's pose and content: the importance-weighted mean, the best sample, q's mean


def _pose_rows(per_image, q_mu, pose, lay):
    """The (B, inf_dim) latent rows of one estimate out of what score_minibatch returned, in the decoder's units."""
    if pose not in POSES:
        raise RuntimeError("pose must be one of %s, got %r" % (POSES, pose))
    return {"iw": per_image[:, lay.iw], "best": per_image[:, lay.best], "q": q_mu}[pose]


@torch.no_grad()
def align_minibatch(y, rows, cols, per_image, q_mu, rotate, translate, pose="iw", interp="bicubic"):
    """The minibatch's observed images brought into the model's canonical frame (ops.align_images) at the pose estimate
    `pose` (POSES) taken from score_minibatch's "per_image" and "q_mu": device slices, nothing is read back.  Returns (aligned,
    shaped like y; cover (B, rows*cols) uint8).  A model with neither rotation nor translation gets its images back."""
    return align_at(y, rows, cols, initial_pose(per_image, q_mu, rotate, translate, pose), rotate, translate, interp)


def initial_pose(per_image, q_mu, rotate, translate, pose="iw"):
    """The (B, 3) fp32 tensor theta, dx0, dx1 of the estimate `pose` (POSES), in the decoder's units, out of score_minibatch's
    "per_image" and "q_mu": a coordinate the model does not infer is 0.  The one statement of what aligns an image before any
    refinement; device slices, nothing is read back."""
    lay = row_layout(rotate, translate, q_mu.size(1))
    lat = _pose_rows(per_image, q_mu, pose, lay)
    out = torch.zeros(lat.size(0), 3, dtype=torch.float32, device=lat.device)
    if rotate:
        out[:, 0] = lat[:, 0]
    if translate:
        out[:, 1:] = lat[:, lay.dx]
    return out


@torch.no_grad()
def align_at(y, rows, cols, pose3, rotate=True, translate=True, interp="bicubic"):
    """ops.align_images at the (B, 3) poses of initial_pose / refine_poses; a coordinate the model does not infer is not handed
    over (NULL: the exact identity).  Returns (aligned, cover)."""
    theta = pose3[:, 0].contiguous() if rotate else None
    dx = pose3[:, 1:].contiguous() if translate else None
    return ops.align_images(y, theta, dx, rows, cols, interp)


def refine_mask(n, m, S):
    """The weight the pose search puts on the reference of an n x m box searched over shifts of at most S pixels, (n, m) float64
    on the host: frc_mask_weights with edge = 3 and radius = max(min(n, m)/2 - 3 - S, 1), so that no shift of the search moves
    a weighted pixel across the border.  A convention, not a tuned value."""
    return frc_mask_weights(n, m, max(min(n, m) / 2.0 - 3.0 - S, 1.0), 3.0)


@torch.no_grad()
def refine_poses(y, rows, cols, ref, weight, ref_index, pose3, angles, step, shift, interp="bicubic"):
    """One round of reference-based refinement for one minibatch (ops.pose_search): around each image's pose3 row, 2 * angles
    + 1 rotations `step` radians apart and the integer shifts up to `shift` pixels, scored by the weighted correlation of the
    re-aligned image with ref[ref_index[b]].  Returns ops.PoseSearch(pose (B, 3), score (B), offset (B, 4), None) on the device;
    an image with ref_index -1 or an all-zero reference keeps its pose."""
    return ops.pose_search(y, ref, weight, ref_index, pose3, rows, cols, angles, step, shift, interp)


@torch.no_grad()
def classify_poses(y, rows, cols, ref, weight, cand, pose3, angles, step, shift, interp="bicubic"):
    """One round of multi-reference alignment for one minibatch: ops.pose_classify scores each image against the references its
    row of cand (B, M) int32 names (-1 = an empty slot) over refine_poses' neighbourhood, and ops.pose_search then refines the
    pose against the chosen reference alone: the winner and the parabolas stay the work of one kernel.  Returns
    (ops.PoseClassify, ops.PoseSearch) on the device; an image with no live slot has choice and ref_chosen -1 and keeps its
    pose."""
    picked = ops.pose_classify(y, ref, weight, cand, pose3, rows, cols, angles, step, shift, interp)
    return picked, ops.pose_search(y, ref, weight, picked.ref_chosen, pose3, rows, cols, angles, step, shift, interp)


@torch.no_grad()
def expect_poses(y, rows, cols, ref, weight, cand, pose3, angles, step, shift, inv_sigma2, interp="bicubic", log_prior=None):
    """The expectation step of maximum-likelihood class averaging for one minibatch (ops.pose_expect): each image spread over
    the references its row of cand (B, M <= 64) int32 names and over classify_poses' neighbourhood of poses by its posterior under
    Gaussian noise of variance 1 / inv_sigma2.  Returns ops.PoseExpect on the device, what ops.ClassSums.update_soft adds."""
    return ops.pose_expect(y, ref, weight, log_prior, cand, pose3, rows, cols, angles, step, shift, inv_sigma2, interp)


@torch.no_grad()
def noise_sums(y, rows, cols, ref, weight, ref_index, pose3, rotate=True, translate=True, interp="bicubic"):
    """What one minibatch adds to the noise estimate of a soft round, a (2) float64 device tensor: (sum over its labelled images,
    pixels and channels of weight * cover * (aligned - ref[ref_index])^2 at the poses pose3, the same sum of weight * cover).
    An image with ref_index < 0 adds nothing.  The round's sigma^2 is the ratio of the two, summed over the minibatches."""
    aligned, cover = align_at(y, rows, cols, pose3, rotate, translate, interp)
    B = y.size(0)
    C = ref.numel() // (ref.size(0) * rows * cols)
    on = ref_index >= 0
    picked = ref.view(ref.size(0), rows * cols, C)[ref_index.clamp(min=0).long()]
    w = weight.view(1, -1) * cover.double() * on.double().view(B, 1)
    diff = aligned.view(B, rows * cols, C).double() - picked
    return torch.stack([(w.unsqueeze(2) * diff * diff).sum(), w.sum() * C])


def content_latents(per_image, q_mu, rotate, translate, pose="iw"):
    """The content part (B, z_dim) of the same estimate: what reconstruct_unposed decodes."""
    lay = row_layout(rotate, translate, q_mu.size(1))
    return _pose_rows(per_image, q_mu, pose, lay)[:, lay.content].contiguous()


@torch.no_grad()
def cluster_latents(points, k, iters, restarts=1, generator=None):
    """k-means of the content latents `points` (N, D) fp32 on the device into k classes (ops.KMeans: k-means++ seeding, `iters`
    Lloyd steps, a final labelling), `restarts` times from uniforms drawn (restarts, k) from the HOST generator; the run of
    lowest inertia is picked on the device (torch.argmin: the first of equals) without synchronising.  Returns device tensors:
    {"label" (N) int32, -1 = a point with a non-finite coordinate; "centres" (k, D) float64; "members" (k) int64; "record" (the
    svae_kmeans_record, ops.KMeans.read_record); "seed_index" (k) int32; "restart_inertia" (restarts) float64;
    "chosen_restart" (1) int64}."""
    restarts = int(restarts)
    if restarts < 1:
        raise RuntimeError("cluster_latents: restarts must be >= 1, got %d" % restarts)
    points = points.float().contiguous()
    uniforms = torch.rand(restarts, int(k), dtype=torch.float64, generator=generator)
    km = ops.KMeans(k, points.size(1), points.device)
    fits = [km.fit(points, iters, uniforms[r]) for r in range(restarts)]
    inertia = torch.cat([ops.KMeans.inertia(f.record) for f in fits])
    chosen = torch.argmin(inertia, 0, keepdim=True)
    out = {name: torch.stack([getattr(f, name) for f in fits]).index_select(0, chosen)[0] for name in ops.KMeansFit._fields}
    out.update(restart_inertia=inertia, chosen_restart=chosen)
    return out


def mixture_latents(points, kmeans_fit, iters, reg=1e-6, tol=1e-8, min_resp=0.0):
    """A diagonal-covariance Gaussian mixture of the content latents `points` (N, D) on the device (ops.GaussianMixture), started
    from `kmeans_fit`, the dict of cluster_latents: one component per k-means class.  Returns the GmmFit's device tensors by name
    with "max_resp" (N) float64, the largest responsibility of each point, and "label_used" (N) int32 = the mixture's label
    where max_resp >= min_resp and -1 elsewhere (and wherever the label already is -1).  Nothing is read back."""
    points = points.float().contiguous()
    k = kmeans_fit["centres"].size(0)
    fit = ops.GaussianMixture(k, points.size(1), points.device).fit(points, kmeans_fit["label"], kmeans_fit["centres"], iters, reg, tol)
    out = dict(fit._asdict())
    out["max_resp"] = fit.resp.max(1).values
    out["label_used"] = torch.where(out["max_resp"] >= float(min_resp), fit.label, torch.full_like(fit.label, -1)).contiguous()
    return out


def principal_axes(points, label=None, n_classes=None, components=None):
    """The principal axes of the content latents `points` (N, D) on the device (ops.LatentPCA): of all of them (label None: one
    group), or of each of the n_classes classes of `label` (N) int32, -1 or any entry outside [0, n_classes) = in no class.
    components: the columns of "projections" (default D).  Returns the PcaFit's device tensors by name, each with a leading
    group axis -- "count", "mean", "cov", "eigenvalues", "components" (rows are axes), "sweeps", "off_norm" -- with "projections"
    (N, components): each point along the axes of its own group, and "explained_variance_ratio" = eigenvalues / their sum, 0
    where the sum is 0.  Nothing is read back."""
    points = points.float().contiguous()
    G = 1 if label is None else int(n_classes)
    fit = ops.LatentPCA(points.size(1), points.device).fit(points, None if label is None else label.to(torch.int32).contiguous(), G,
                                                           components)
    out = dict(fit._asdict())
    out["projections"] = out.pop("proj")
    total = fit.eigenvalues.sum(1, keepdim=True)
    out["explained_variance_ratio"] = torch.where(total != 0, fit.eigenvalues / total, torch.zeros_like(fit.eigenvalues))
    return out


def traverse_latents(mean, eigenvalues, components, axes, steps, span):
    """Walks along the first `axes` principal axes: z[..., p, s + steps, :] = mean + (s / steps) * span * sqrt(max(lambda_p, 0))
    * v_p for s = -steps..steps, with mean (..., D), eigenvalues (..., D) and components (..., D, D) as principal_axes returns
    them (any leading axes).  Formed in double where the inputs live, rounded to float once: (..., axes, 2 steps + 1, D) fp32."""
    axes, steps = int(axes), int(steps)
    mean, lam, v = mean.double(), eigenvalues.double()[..., :axes], components.double()[..., :axes, :]
    frac = torch.arange(-steps, steps + 1, dtype=torch.float64, device=mean.device) / steps
    reach = (frac * float(span)).unsqueeze(0) * torch.sqrt(torch.clamp(lam, min=0.0)).unsqueeze(-1)     # (..., axes, frames)
    z = mean[..., None, None, :] + reach.unsqueeze(-1) * v.unsqueeze(-2)
    return z.float()


def ring_layout(n, m):
    """The rings of an n x m plane (include/svae_frc.h): (L, R, ring_frequency) with L = min(n, m), R = L // 2 + 1 rings and
    ring r standing for ring_frequency[r] = r / L cycles per pixel."""
    L = min(int(n), int(m))
    R = L // 2 + 1
    return L, R, np.arange(R, dtype=np.float64) / L


def frc_weight(frc):
    """The per-ring weight sqrt(2 f / (1 + f)) that takes a half-set FRC f to the full average's correlation with the signal;
    0 where f <= 0.  A torch expression: on the device nothing is read back."""
    f = torch.clamp(frc, min=0.0)
    return torch.where(frc > 0, torch.sqrt(2.0 * f / (1.0 + f)), torch.zeros_like(frc))


def frc_resolution(frc_row, threshold, L):
    """(resolution in pixels, never_below) of one FRC curve (R) on the host: NaN where ring 0 is already below the threshold;
    else at the first ring r >= 1 below it, L over the ring position interpolated linearly between r - 1 and r; else L / (R - 1),
    the last ring, with never_below = True: the curve says no more than that."""
    f = np.asarray(frc_row, dtype=np.float64)
    t = float(threshold)
    if not f[0] >= t:
        return float("nan"), False
    for r in range(1, f.shape[0]):
        if f[r] < t:
            with np.errstate(divide="ignore"):
                return float(np.float64(L) / np.float64((r - 1) + (f[r - 1] - t) / (f[r - 1] - f[r]))), False
    return float(L) / (f.shape[0] - 1), True


def frc_mask_weights(n, m, radius, edge):
    """The soft circular mask of svae_frc as its rule gives it, (n, m) float64 on the host; radius 0 = all ones."""
    if radius == 0:
        return np.ones((n, m), np.float64)
    dy = np.arange(n, dtype=np.float64)[:, None] - 0.5 * (n - 1)
    dx = np.arange(m, dtype=np.float64)[None, :] - 0.5 * (m - 1)
    d = np.sqrt(dx * dx + dy * dy)
    w = 0.5 * (1.0 + np.cos(np.pi * ((d - radius) / edge)))
    return np.where(d <= radius, 1.0, np.where(d >= radius + edge, 0.0, w))


def _decode_on_grid(x, p_net, B, zc):
    """The decoder on the un-posed grid at the content latents zc."""
    if hasattr(p_net, "forward_posed"):
        return p_net.forward_posed(x, B, z=zc)
    return p_net(x, zc)


@torch.no_grad()
def reconstruct_unposed(x, p_net, B, zc, gaussian_mean=False):
    """The pose-free reconstruction at the content latents zc (B, z_dim) -> (B, N, C).  gaussian_mean (the particle scripts):
    a decoder that also fits the noise (n_out == 2) keeps its mean only, which is the first N entries of each row (the layout
    quirk of svae_gaussian_loglik)."""
    out = _decode_on_grid(x, p_net, B, zc)
    N = x.size(0)
    if gaussian_mean and out.numel() == B * N * 2:
        return out.reshape(B, -1)[:, :N].reshape(B, N, 1)
    return out.reshape(B, N, -1)


# ---------------------------------------------------------------- forward-only paths (image dumps of the training scripts)
def _decode_unposed(x, y, p_net, q_net, rotate, translate, z_scale, use_cuda, noise):
    B = y.size(0)
    if use_cuda:
        y = y.cuda()
    q_out = _encode(q_net, y.view(B, -1))
    inf_dim = q_out.size(1) // 2
    r = noise if noise is not None else torch.empty(B, inf_dim, device=x.device, dtype=q_out.dtype).normal_()
    # sample z, then drop the rotation and translation slots: the image is drawn on the UNposed grid
    _, _, zc, _ = ops.latent_head(q_out, r, rotate, translate, False, 1.0, z_scale, math.pi)
    return _decode_on_grid(x, p_net, B, zc)


@torch.no_grad()
def minibatch_for_display(x, y, p_net, q_net, rotate=True, translate=True, z_scale=1, use_cuda=False, noise=None):
    """train_mnist.py:93-124: reconstruct from the content latents only (pose removed) -> (B, N)."""
    return _decode_unposed(x, y, p_net, q_net, rotate, translate, z_scale, use_cuda, noise).view(y.size(0), -1)


@torch.no_grad()
def minibatch_for_display_galaxy(x, y, q_net, p_net, rotate=True, translate=True, z_scale=1, use_cuda=False, noise=None):
    """train_galaxy.py:131-163 (note the reference's argument order: q_net before p_net) -> (B, N, C)."""
    return _decode_unposed(x, y, p_net, q_net, rotate, translate, z_scale, use_cuda, noise).view(y.size(0), -1, y.size(2))


@torch.no_grad()
def random_minibatch_generator(x, y, p_net, z_dim, z_scale=1, use_cuda=False, noise=None):
    """train_galaxy.py:166-183: decode z ~ N(0, 1) * z_scale on the unposed grid -> (B, N, C)."""
    B = y.size(0)
    z = noise if noise is not None else torch.empty(B, z_dim, device=x.device, dtype=torch.float32).normal_()
    z = z * z_scale
    out = p_net.forward_posed(x, B, z=z) if hasattr(p_net, "forward_posed") else p_net(x, z)
    return out.view(B, -1, y.size(2))
