"""infer.py: apply a trained model to a dataset, one row per image (the root script infer.py is the entry point).

The command line, the rules between its options, the rules against the model and the `meta` record are declared once, as
tables, in infer_request.py (infer_arguments, check_request, run_meta: every refusal that needs no device, made before the
kernel library is loaded); their names are importable from here as they always were.  This module holds the file writers and
infer_main: a short sequence of stages -- load the model, check the request against the split, allocate the accumulators, walk
the minibatches scoring (and aligning) them, cluster, take the principal axes of the content latents (--pca), refine the poses
against the class averages (--refine; with --reassign also the classes), finish the half-set correlation (--frc), collect and
write.  The device work is elbo.py's (score_minibatch, align_minibatch, reconstruct_unposed, cluster_latents, principal_axes,
traverse_latents, refine_poses, classify_poses, frc_weight) and ops.py's.
"""
import collections
import json
import math
import os

import numpy as np
import torch

from . import elbo as E
from . import infer_request
from . import ops
from .cli import (SCRIPTS, RESUME_ARG_DEFAULTS, CheckpointError, check_resume_fingerprint, coord_grid, dataset_fingerprint,
                  pick_device, read_checkpoint)
from .infer_request import (INFER_FRC_MAX_BOX, INFER_FRC_MAX_CLASSES, INFER_MAX_CHUNK, INFER_MAX_CLASSES,  # noqa: F401
                            INFER_MAX_CLUSTERS, INFER_MAX_GMM_ITERS, INFER_MAX_GMM_RESP, INFER_MAX_PCA_PARTIALS,
                            INFER_MAX_PCA_STEPS, INFER_MAX_REASSIGN_CLASSES, INFER_MAX_REFINE_ANGLES, INFER_MAX_REFINE_ROUNDS,
                            INFER_MAX_REFINE_SHIFT, INFER_MAX_RESTARTS, INFER_MAX_SOFT_CLASSES, INFER_PATH_OVERRIDES,
                            INFER_STACK_FORMATS, SplitFacts, _refuse, check_request, frc_mask_radius, read_labels, run_meta)

FRC_THRESHOLDS = (("resolution_0143", 0.143), ("resolution_05", 0.5))
PCA_KEYS = ("count", "mean", "cov", "eigenvalues", "components", "explained_variance_ratio", "projections", "sweeps", "off_norm")


def infer_arguments(argv=None):
    """infer_request.infer_arguments, under this module's INFER_MAX_REASSIGN_CLASSES: the one limit that no command line can
    reach (--labels and --cluster stop below it) and that is therefore seen only when lowered here."""
    return infer_request.infer_arguments(argv, INFER_MAX_REASSIGN_CLASSES)


def stored_namespace(ck, defaults, script):
    """The training run's argument namespace from a state file: the stored arguments over RESUME_ARG_DEFAULTS over the
    script's own defaults.  A file another script wrote names arguments this script's parser does not have (and lacks some it
    has): refused, exit code 2."""
    import argparse
    stored = dict(ck["args"])
    unknown = sorted(set(stored) - set(defaults))
    missing = sorted(set(defaults) - set(stored) - set(RESUME_ARG_DEFAULTS))
    if unknown or missing:
        _refuse("the state file was not written by train_{}.py: it has the arguments {} which that script lacks, and lacks {}"
                .format(script, unknown, missing))
    return argparse.Namespace(**dict(defaults, **dict(RESUME_ARG_DEFAULTS, **stored)))


def write_atomically(path, save):
    """save(f) writes the open binary file f; the file is written under a temporary name beside `path` and renamed over it: an
    interrupted write leaves no file under the final name."""
    tmp = "{}.tmp{}".format(path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            save(f)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def write_npz(path, arrays):
    """One .npz of plain arrays, written under a temporary name beside `path` and renamed over it."""
    return write_atomically(path, lambda f: np.savez(f, **arrays))


def write_stack(path, stack):
    """An image stack (images, rows, cols, C) float32 as .npy, or as an MRC stack (C == 1), by the path's extension."""
    if path.endswith(".mrcs"):
        from . import mrc
        return write_atomically(path, lambda f: mrc.write(f, stack[..., 0]))
    return write_atomically(path, lambda f: np.save(f, stack))


def read_npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def split_rows(rows, lay):
    """(per_image, q_mu, q_std) out of the stored rows [per_image | q_mu | q_std] of one or more minibatches."""
    return rows[:, :lay.width], rows[:, lay.width:lay.width + lay.inf_dim], rows[:, lay.width + lay.inf_dim:]


def score_arrays(per_image, q_mu, q_std, rotate, translate):
    """The named arrays of infer.py's output from the rows of elbo.score_minibatch (host arrays): theta_* iff the model rotates,
    dx_* iff it translates."""
    lay = E.row_layout(rotate, translate, q_mu.shape[1])
    iw, best = per_image[:, lay.iw], per_image[:, lay.best]
    out = {"bound": per_image[:, 0], "loglik": per_image[:, 1], "kl": per_image[:, 2], "ess": per_image[:, 3]}
    if rotate:
        out.update(theta_q=q_mu[:, 0], theta_q_std=q_std[:, 0], theta_iw=iw[:, 0], theta_R=per_image[:, 5], theta_best=best[:, 0])
    if translate:
        out.update(dx_q=q_mu[:, lay.dx], dx_q_std=q_std[:, lay.dx], dx_iw=iw[:, lay.dx], dx_best=best[:, lay.dx])
    out.update(z_q=q_mu[:, lay.content], z_q_std=q_std[:, lay.content], z_iw=iw[:, lay.content], z_best=best[:, lay.content])
    out["index"] = np.arange(per_image.shape[0], dtype=np.int64)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


# ---- the stages of infer_main ------------------------------------------------------------------------------------------------
Model = collections.namedtuple("Model", "targs cfg p_net q_net z_scale device completed")


def load_model(args, parser_fn, build, positional):
    """The training arguments (from the state file, or parsed from what followed `--`), what build() makes of them and both
    networks on the device in eval mode.  A state file that cannot be read, is another script's, is of another dataset or does
    not fit the networks is refused."""
    script = args.script
    ck = None
    overridden = [n for n in INFER_PATH_OVERRIDES if vars(args)[n] is not None]
    if args.state is not None:
        try:
            ck = read_checkpoint(args.state)
        except CheckpointError as e:
            _refuse(str(e).replace("--resume: ", ""))
        targs = stored_namespace(ck, vars(parser_fn(list(positional))), script)
        for n in overridden:
            if not hasattr(targs, n):
                _refuse("train_{}.py has no --{} to override".format(script, n))
            setattr(targs, n, vars(args)[n])
        completed = int(ck["completed"])
    else:
        targs = parser_fn(args.train_argv)
        completed = targs.num_epochs
    device = pick_device(args.device)
    if targs.seed is not None:                      # build() must make the split the run trained on (galaxy shuffles in it)
        torch.manual_seed(targs.seed)
        np.random.seed(targs.seed % (2 ** 32))
    if targs.gemm:
        from . import _lib
        _lib.set_gemm_mode(targs.gemm)
    cfg = build(targs, device)
    if ck is not None:
        if not overridden:
            try:
                check_resume_fingerprint(ck, dataset_fingerprint(cfg["y_train"], cfg["y_test"]))
            except CheckpointError as e:
                _refuse(str(e).replace("--resume: ", ""))
        try:
            cfg["p_net"].load_state_dict(ck["train_step"]["p_net"])
            cfg["q_net"].load_state_dict(ck["train_step"]["q_net"])
        except (RuntimeError, KeyError) as e:
            _refuse("the state file's networks do not fit what train_{}.py builds from its arguments: {}".format(
                script, str(e).splitlines()[0]))
        p_net, q_net = cfg["p_net"], cfg["q_net"]
    else:
        p_net = torch.load(args.generator, map_location="cpu", weights_only=False)
        q_net = torch.load(args.inference, map_location="cpu", weights_only=False)
    z_scale = (0 if completed < getattr(targs, "z_delay", 0) else 1) if SCRIPTS[script].z_schedule else 1
    return Model(targs, cfg, p_net.to(device).eval(), q_net.to(device).eval(), z_scale, device, completed)


def split_facts(args, model):
    cfg = model.cfg
    data, n, m = cfg["y_" + args.split], cfg["n"], cfg["m"]
    table = cfg.get("ctf_params_" + args.split)
    return SplitFacts(data.size(0), n, m, data[0].numel() // (n * m) if data.size(0) else 1, cfg["rotate"], cfg["translate"],
                      model.q_net.latent_dim, model.z_scale, args.split, None if table is None else table.shape[0])


Split = collections.namedtuple("Split", "data ctf mask x")


def upload_split(cfg, split, device):
    """The split's images, its CTF filters and the mask (None where the script has none) and the coordinate grid, on the device."""
    data = cfg["y_" + split].to(device)
    ctf = cfg.get("ctf_" + split)
    ctf = ctf.to(device) if ctf is not None else None
    mask = cfg.get("mask")
    mask = mask.to(device) if mask is not None else None
    return Split(data, ctf, mask, coord_grid(cfg["n"], cfg["m"]).to(device))


class Accumulators(object):
    """What the image outputs accumulate over the minibatches: the pinned host stacks of --aligned / --recon (filled by
    non-blocking copies), the class sums of --class_averages with their labels on the device, and under --ctf_correct the
    uploaded table rows of the split and, for wiener, the pair (class sums of the aligned H*y, class sums of H^2).  Under --frc
    also the half-set sums: class k's images of even dataset index in row 2k, of odd index in row 2k + 1."""

    def __init__(self, args, facts, cfg, device):
        images, n, m, channels = facts.images, facts.n, facts.m, facts.channels
        self.device, self.n, self.m, self.rotate, self.translate = device, n, m, facts.rotate, facts.translate
        self.pose, self.interp, self.correct = args.pose, args.interp, args.ctf_correct
        self.stacks = {k: torch.empty(images, n * m * channels, dtype=torch.float32, pin_memory=True)
                       for k in ("aligned", "recon") if vars(args)[k] is not None}
        self.labels = args.label_array              # host; under --cluster both arrive after the scoring walk
        self.sums = self.label_d = self.table_d = self.wiener = self.ctf_scale = self.halves = self.frc = None
        self.refined = None                         # refine_walk's record, when --refine ran
        if args.class_averages is not None:
            if args.cluster is not None:
                n_classes = args.cluster
            else:
                if self.labels is None:
                    self.labels = np.zeros(images, np.int64)    # one class holding every image
                n_classes = max(int(self.labels.max()) + 1, 1) if images else 1
                self.label_d = torch.from_numpy(self.labels.astype(np.int32)).to(device)
            self.sums = ops.ClassSums(n_classes, n * m, channels, device)
            if args.frc:
                self.halves = ops.ClassSums(2 * n_classes, n * m, channels, device)
        if self.correct is not None:                # each image through its own transfer function before it is aligned
            table = cfg["ctf_params_" + facts.split]
            self.table_d = torch.from_numpy(np.ascontiguousarray(table[:images], dtype=np.float64)).to(device)
            self.ctf_scale = cfg["ctf_scale"]
            if self.correct == "wiener":
                self.wiener = (ops.ClassSums(self.sums.n_classes, n * m, 1, device),
                               ops.CtfPower(self.sums.n_classes, n, m, device, scale=self.ctf_scale))

    def _align(self, y, per_image, q_mu):
        return E.align_minibatch(y, self.n, self.m, per_image, q_mu, self.rotate, self.translate, self.pose, self.interp)

    def _half_labels(self, lo, hi, label=None):
        """label_d[lo:hi] (or `label`, the labels of those images) with class k split by the parity of the dataset index:
        2k + (i & 1); -1 stays -1."""
        label = self.label_d[lo:hi] if label is None else label
        parity = torch.arange(lo, hi, dtype=torch.int32, device=label.device) & 1
        return torch.where(label >= 0, 2 * label + parity, label).contiguous()

    def align_and_update(self, lo, y, per_image, q_mu, labelled):
        """The minibatch y = images [lo, lo + B) brought into the canonical frame, copied into the aligned stack when there is
        one; with `labelled` also its class-sum and Wiener updates under label_d.  The scoring walk and --cluster's second walk
        both make exactly these calls, in this order."""
        hi = lo + y.size(0)
        seen = self.seen(lo, y)
        aligned, cover = self._align(seen, per_image, q_mu)
        if labelled and self.wiener is not None:
            g = ops.ctf_apply(y, self.table_d[lo:hi], self.n, self.m, self.ctf_scale, "multiply")
            g, g_cover = self._align(g, per_image, q_mu)
            self.wiener[0].update(g, g_cover, self.label_d[lo:hi])
            self.wiener[1].update(self.table_d[lo:hi], self.label_d[lo:hi])
            if self.halves is not None:             # the halves of what the Wiener average divides: the aligned H y
                self.halves.update(g, g_cover, self._half_labels(lo, hi))
        if labelled:
            self.sums.update(aligned, cover, self.label_d[lo:hi])
            if self.halves is not None and self.wiener is None:
                self.halves.update(aligned, cover, self._half_labels(lo, hi))
        return aligned

    def seen(self, lo, y):
        """What is aligned of the minibatch y = images [lo, lo + B): the raw images, or under --ctf_correct flip the phase-flipped."""
        if self.correct != "flip":
            return y
        return ops.ctf_apply(y, self.table_d[lo:lo + y.size(0)], self.n, self.m, self.ctf_scale, "flip")

    def update_at(self, lo, seen, pose3, label=None):
        """refine_walk's half of align_and_update: `seen` aligned at the poses pose3 (B, 3) and added to the class sums (and the
        half-set sums) under label_d, or under `label` (B) int32 where --reassign has moved the images.  --refine excludes the
        Wiener sums."""
        hi = lo + seen.size(0)
        aligned, cover = E.align_at(seen, self.n, self.m, pose3, self.rotate, self.translate, self.interp)
        self.sums.update(aligned, cover, self.label_d[lo:hi] if label is None else label)
        if self.halves is not None:
            self.halves.update(aligned, cover, self._half_labels(lo, hi, label))
        return aligned

    def keep(self, name, lo, images):
        """images (B, ...) on the device into rows [lo, lo + B) of the pinned stack `name`; nothing waits for the copy."""
        self.stacks[name][lo:lo + images.size(0)].copy_(images.reshape(images.size(0), -1), non_blocking=True)


def score_walk(args, model, split, acc):
    """Every minibatch in dataset order through elbo.score_minibatch, its noise one (B * K, inf_dim) draw from the host generator
    seeded with --seed; the image outputs that need no --cluster labels are accumulated on the way.  Returns the per-minibatch
    rows [per_image | q_mu | q_std] on the device: nothing is read back inside the loop."""
    cfg, targs, script = model.cfg, model.targs, args.script
    rotate, translate = cfg["rotate"], cfg["translate"]
    K, bs, inf_dim = args.num_samples, args.minibatch_size, model.q_net.latent_dim
    gen = torch.Generator()
    gen.manual_seed(args.seed)
    labelled = acc.sums is not None and args.cluster is None    # --cluster: the labels do not exist yet, the updates wait
    rows = []
    for lo in range(0, split.data.size(0), bs):
        y = split.data[lo:lo + bs]
        noise = torch.empty(y.size(0) * K, inf_dim).normal_(generator=gen).to(model.device, non_blocking=True)
        out = E.score_minibatch(script, split.x, y, model.p_net, model.q_net, num_samples=K, chunk=min(args.chunk, K),
                                rotate=rotate, translate=translate, dx_scale=targs.dx_scale, theta_prior=targs.theta_prior,
                                z_scale=model.z_scale, mask=split.mask, ctf=None if split.ctf is None else split.ctf[lo:lo + bs],
                                noise=noise)
        rows.append(torch.cat([out["per_image"], out["q_mu"], out["q_std"]], 1))
        if "aligned" in acc.stacks or labelled:
            aligned = acc.align_and_update(lo, y, out["per_image"], out["q_mu"], labelled)
            if "aligned" in acc.stacks:
                acc.keep("aligned", lo, aligned)
        if "recon" in acc.stacks:
            zc = E.content_latents(out["per_image"], out["q_mu"], rotate, translate, args.pose)
            acc.keep("recon", lo, E.reconstruct_unposed(split.x, model.p_net, y.size(0), zc, gaussian_mean=(script == "particles")))
    return rows


def cluster_walk(args, model, split, acc, rows, lay):
    """--cluster: k-means of every image's content latents (the k-means++ uniforms from a fresh host generator seeded with
    --cluster_seed), then for --class_averages a second walk over the minibatches that re-aligns from the stored rows and makes
    the update calls the scoring walk would have made, in its order; no host read in between.  Under --cluster_gmm the mixture
    of elbo.mixture_latents is fitted on the chosen restart's k-means fit and ITS labels (-1 below --cluster_min_resp) are what
    every later stage sees.  Returns (the fit of elbo.cluster_latents, with the mixture's tensors under "gmm" and the decoder's
    un-posed reconstruction of its means under "gmm_mean_recon"; the decoder's un-posed reconstruction of the centres)."""
    per_image, q_mu, _ = split_rows(torch.cat(rows), lay)
    zc = E.content_latents(per_image, q_mu, model.cfg["rotate"], model.cfg["translate"], args.pose)
    kgen = torch.Generator()
    kgen.manual_seed(args.cluster_seed)
    fit = E.cluster_latents(zc, args.cluster, args.cluster_iters, args.cluster_restarts, kgen)
    acc.label_d = fit["label"]
    if args.cluster_gmm is not None:
        fit["gmm"] = E.mixture_latents(zc, fit, args.cluster_gmm, args.cluster_gmm_reg, args.cluster_gmm_tol, args.cluster_min_resp)
        acc.label_d = fit["gmm"]["label_used"]
    if acc.sums is not None:
        for i, lo in enumerate(range(0, split.data.size(0), args.minibatch_size)):
            per_image, q_mu, _ = split_rows(rows[i], lay)
            acc.align_and_update(lo, split.data[lo:lo + args.minibatch_size], per_image, q_mu, True)
    centres = E.reconstruct_unposed(split.x, model.p_net, args.cluster, fit["centres"].float(),
                                    gaussian_mean=(args.script == "particles"))
    if args.cluster_gmm is not None:
        fit["gmm_mean_recon"] = E.reconstruct_unposed(split.x, model.p_net, args.cluster, fit["gmm"]["mean"].float(),
                                                      gaussian_mean=(args.script == "particles"))
    return fit, centres


def pca_walk(args, model, split, acc, rows, lay):
    """--pca: the principal axes of every image's content latents (elbo.principal_axes on what cluster_walk clusters), under
    --pca_per_class also those of every class under acc.label_d, the labels the later stages see.  With --pca_traverse the walks
    of elbo.traverse_latents -- from the global mean along the global axes, and from each class's mean along that class's own --
    go through the decoder's un-posed reconstruction in one call.  Returns {"global": ..., "class": ... or None,
    "traverse_latents", "traverse_images", "class_traverse_latents", "class_traverse_images" where asked for}, all on the
    device: nothing is read back."""
    per_image, q_mu, _ = split_rows(torch.cat(rows), lay)
    zc = E.content_latents(per_image, q_mu, model.cfg["rotate"], model.cfg["translate"], args.pose)
    found = {"global": E.principal_axes(zc, components=args.pca_components), "class": None}
    if args.pca_per_class:
        found["class"] = E.principal_axes(zc, acc.label_d, args.cluster, args.pca_components)
    if args.pca_traverse > 0:
        walks = [(name, E.traverse_latents(fit["mean"], fit["eigenvalues"], fit["components"], args.pca_traverse, args.pca_steps,
                                           args.pca_span))
                 for name, fit in (("", found["global"]), ("class_", found["class"])) if fit is not None]
        z = torch.cat([w.reshape(-1, zc.size(1)) for _, w in walks])
        images = E.reconstruct_unposed(split.x, model.p_net, z.size(0), z, gaussian_mean=(args.script == "particles"))
        lo = 0
        for name, w in walks:
            n = w.numel() // zc.size(1)
            found[name + "traverse_latents"], found[name + "traverse_images"] = w, images[lo:lo + n]
            lo += n
    return found


def pca_arrays(args, facts, found, meta):
    """The arrays of the --pca file, transferred once: the global fit without its group axis, the walks, under --pca_per_class
    the same arrays prefixed class_ with a leading class axis (class_projections: each image in its own class's basis)."""
    out = {}
    for prefix, fit in (("", found["global"]), ("class_", found["class"])):
        if fit is None:
            continue
        for key in PCA_KEYS:
            a = fit[key].cpu().numpy()
            out[prefix + key] = a[0] if not prefix and key != "projections" else a
        for key in ("traverse_latents", "traverse_images"):
            if prefix + key in found:
                a = found[prefix + key].cpu().numpy()
                lead = (args.cluster,) if prefix else ()    # the walks of the global fit carry its group axis of 1: dropped
                frames = (args.pca_traverse, 2 * args.pca_steps + 1)
                out[prefix + key] = a.reshape(lead + frames + ((facts.n, facts.m, -1) if key == "traverse_images" else (-1,)))
    out["meta"] = np.array(json.dumps(meta))
    return out


def class_means(sums):
    """sum / count of a ClassSums where the count is positive and 0 elsewhere, (n_classes, N, C) float64 on the device."""
    total, count = sums.result()
    count = count.unsqueeze(2)
    return torch.where(count > 0, total / count, torch.zeros_like(total))


def refine_walk(args, facts, split, acc, rows, lay):
    """--refine: R rounds of reference-based alignment on the device.  A round snapshots the references from the accumulators as
    they stand -- sum / count per class, under --frc half_sum / half_count per (class, half), so that no image is ever compared
    with an average that holds images of the other half --, zeroes the accumulators, and walks the minibatches in dataset order:
    the image align_and_update would align is searched around its stored pose (elbo.refine_poses under elbo.refine_mask), the
    new pose stored, the image aligned at it and the update calls made.  The last round fills --aligned again.  A coordinate
    the model does not infer is not searched.  Nothing is read back between or inside rounds; acc.refined keeps what the files
    report, the accumulators and (under --frc) the curves from before the first round among it.

    --reassign: the round scores each labelled image against all K references (under --frc the K of its own half: slot k holds
    2k + (i & 1)) with elbo.classify_poses, takes the winning slot as its label for this round's updates and the next round's
    search, and the pose refined against that winner.  An image with no live slot keeps label and pose.  The round's labels go
    into a new tensor, swapped in at its end as the poses are.

    --refine_soft: labels, poses and the aligned stack are made exactly as under --reassign, but the round's accumulators are
    filled softly.  The image's T best slots by cand_score (a stable descending sort: ties keep slot order; a slot the search
    skipped stays out) go through elbo.expect_poses, and ClassSums.update_soft adds the posterior-weighted rows: under --frc the
    references are the 2K half averages, added as they are into the halves and folded reference r -> class r >> 1 into the full
    sums.  The round's noise variance is --refine_soft_sigma2 or soft_sigma2's estimate; where its reciprocal is not positive and
    finite the round runs hard and records nan."""
    n, m, bs, device = facts.n, facts.m, args.minibatch_size, acc.device
    A = args.refine_angles if facts.rotate else 0
    S = args.refine_shift if facts.translate else 0
    step = math.radians(args.refine_step)
    per_image, q_mu, _ = split_rows(torch.cat(rows), lay)
    pose = E.initial_pose(per_image, q_mu, facts.rotate, facts.translate, args.pose)
    before = {"sum": acc.sums.sum.clone(), "count": acc.sums.count.clone()}
    if args.frc:
        frc_finish(args, facts, acc)
        before["frc"] = acc.frc["frc"]
    weight = torch.from_numpy(E.refine_mask(n, m, S).reshape(-1)).to(device)
    source = acc.halves if args.frc else acc.sums
    score = torch.zeros(facts.images, args.refine, dtype=torch.float64, device=device)
    offset = torch.zeros(facts.images, args.refine, 4, dtype=torch.int32, device=device)
    moves = None
    if args.reassign:
        K, label = acc.sums.n_classes, acc.label_d
        slots = torch.arange(K, dtype=torch.int32, device=device).unsqueeze(0)
        moves = {"labels": torch.zeros(facts.images, args.refine, dtype=torch.int32, device=device),
                 "moved": torch.zeros(args.refine, dtype=torch.int64, device=device),
                 "class_score": torch.zeros(facts.images, K, dtype=torch.float64, device=device),
                 "margin": torch.zeros(facts.images, args.refine, dtype=torch.float64, device=device)}
    soft = None
    if args.refine_soft:
        soft = {"sigma2": torch.full((args.refine,), float("nan"), dtype=torch.float64),
                "log_evidence": torch.zeros(facts.images, args.refine, dtype=torch.float64, device=device),
                "post_max": torch.zeros(facts.images, args.refine, dtype=torch.float64, device=device),
                "class_post": torch.zeros(facts.images, K, dtype=torch.float64, device=device)}
        T = min(K, args.refine_soft_classes)
        fold = (torch.arange(2 * K, dtype=torch.int32, device=device) >> 1).contiguous() if args.frc else None
    for r in range(args.refine):
        ref = class_means(source)                   # a new tensor: the accumulators can be zeroed
        inv_sigma2 = None
        if soft is not None:
            sigma2 = args.refine_soft_sigma2
            if sigma2 is None:
                sigma2 = soft_sigma2(args, facts, split, acc, ref, weight, label, pose)
            if 0 < sigma2 < float("inf") and 0 < 1.0 / sigma2 < float("inf"):
                inv_sigma2 = 1.0 / sigma2
                soft["sigma2"][r] = sigma2
        for t in (acc.sums, acc.halves):
            if t is not None:
                t.sum.zero_()
                t.count.zero_()
        new_pose = torch.empty_like(pose)
        new_label = torch.empty_like(label) if args.reassign else None
        for lo in range(0, facts.images, bs):
            hi = min(lo + bs, facts.images)
            seen = acc.seen(lo, split.data[lo:hi])
            moved_to = None
            if args.reassign:
                old = label[lo:hi]
                parity = torch.arange(lo, hi, dtype=torch.int32, device=device).unsqueeze(1) & 1
                cand = torch.where(old.unsqueeze(1) >= 0, 2 * slots + parity if args.frc else slots.expand(hi - lo, K), -1)
                picked, found = E.classify_poses(seen, n, m, ref, weight, cand.to(torch.int32).contiguous(), pose[lo:hi].contiguous(),
                                                 A, step, S, acc.interp)
                moved_to = torch.where(picked.choice >= 0, picked.choice, old).contiguous()
                new_label[lo:hi] = moved_to
                moves["margin"][lo:hi, r] = picked.margin
                if r == args.refine - 1:
                    moves["class_score"][lo:hi] = picked.cand_score
            else:
                ref_index = acc._half_labels(lo, hi) if args.frc else acc.label_d[lo:hi].contiguous()
                found = E.refine_poses(seen, n, m, ref, weight, ref_index, pose[lo:hi].contiguous(), A, step, S, acc.interp)
            new_pose[lo:hi] = found.pose
            score[lo:hi, r] = found.score
            offset[lo:hi, r] = found.offset
            last = r == args.refine - 1
            if inv_sigma2 is None:
                aligned = acc.update_at(lo, seen, found.pose, moved_to)
            else:
                # the T best slots of the round, ties in slot order; a slot the search skipped (an emptied class) stays out
                order = torch.sort(picked.cand_score, dim=1, descending=True, stable=True).indices[:, :T]
                best_of = torch.where(picked.cand_score.gather(1, order) > float("-inf"), cand.gather(1, order), -1)
                best_of = best_of.to(torch.int32).contiguous()
                spread = E.expect_poses(seen, n, m, ref, weight, best_of, pose[lo:hi].contiguous(), A, step, S, inv_sigma2, acc.interp)
                acc.sums.update_soft(spread, best_of, fold)
                if acc.halves is not None:
                    acc.halves.update_soft(spread, best_of)
                soft["log_evidence"][lo:hi, r] = spread.log_evidence
                soft["post_max"][lo:hi, r] = spread.class_post.max(1).values
                if last:
                    soft["class_post"][lo:hi] = torch.zeros_like(picked.cand_score).scatter_(1, order, spread.class_post)
                if last and "aligned" in acc.stacks:
                    aligned = E.align_at(seen, n, m, found.pose, acc.rotate, acc.translate, acc.interp)[0]
            if last and "aligned" in acc.stacks:
                acc.keep("aligned", lo, aligned)
        pose = new_pose
        if args.reassign:
            moves["labels"][:, r] = new_label
            moves["moved"][r] = (new_label != label).sum()
            label = new_label
    acc.refined = dict(before, pose=pose, score=score, offset=offset)
    if args.reassign:
        acc.refined.update(moves, label=label)
    if soft is not None:
        acc.refined["soft"] = soft


def soft_sigma2(args, facts, split, acc, ref, weight, label, pose):
    """--refine_soft's noise variance for the round about to start: over every labelled image at its current pose,
    sum weight * cover * (aligned - ref[label])^2 over pixels and channels divided by sum weight * cover * C, the reference being
    the one the image will be searched against (under --frc its own half's).  The two sums are accumulated in float64 on the
    device over the minibatches in dataset order (elbo.noise_sums); the ratio is the one number read back, once per round,
    because svae_pose_expect takes inv_sigma2 by value.  nan where nothing is labelled."""
    bs = args.minibatch_size
    sums = torch.zeros(2, dtype=torch.float64, device=acc.device)
    for lo in range(0, facts.images, bs):
        hi = min(lo + bs, facts.images)
        ref_index = acc._half_labels(lo, hi, label[lo:hi]) if args.frc else label[lo:hi].contiguous()
        sums += E.noise_sums(acc.seen(lo, split.data[lo:hi]), facts.n, facts.m, ref, weight, ref_index, pose[lo:hi].contiguous(),
                             acc.rotate, acc.translate, acc.interp)
    return float((sums[0] / sums[1]).item())


def frc_finish(args, facts, acc):
    """--frc, once after the walks and on the device: the two half planes of every (class, channel) -- half_sum / half_count
    where the count is positive and 0 elsewhere, under --ctf_correct wiener half_sum itself (a positive weight shared by both
    halves leaves a ring correlation nearly unchanged, and the numerators are the phase-corrected quantity) -- through ops.frc
    under the mask, and the full average (sum / count, or the Wiener average) through ops.frc_filter with elbo.frc_weight.
    Nothing is read back; class_arrays takes acc.frc from here."""
    n, m, channels, K = facts.n, facts.m, facts.channels, acc.sums.n_classes
    h_sum, h_count = acc.halves.result()
    h_sum, h_count = h_sum.view(K, 2, n * m, channels), h_count.view(K, 2, n * m, 1)
    total, count = acc.sums.result()
    count = count.view(K, n * m, 1)
    if acc.wiener is not None:
        planes = h_sum
        full = ops.wiener_finish(acc.wiener[0].result()[0], acc.wiener[1].result(), args.wiener_lambda, n, m).double()
        full = full.view(K, 1, n * m)
    else:
        planes = torch.where(h_count > 0, h_sum / h_count, torch.zeros_like(h_sum))
        full = torch.where(count > 0, total / count, torch.zeros_like(total)).permute(0, 2, 1)
    halves = planes.permute(1, 0, 3, 2).reshape(2, K * channels, n, m)     # (half, class * channel, n, m)
    sums, frc, ring_count = ops.frc(halves[0], halves[1], n, m, frc_mask_radius(args, n, m), args.frc_mask_edge)
    weight = E.frc_weight(frc)
    filtered = ops.frc_filter(full.reshape(K * channels, n, m), weight, n, m)
    acc.frc = {"frc_sums": sums.view(K, channels, -1, 3), "frc": frc.view(K, channels, -1), "ring_count": ring_count,
               "frc_weight": weight.view(K, channels, -1), "average_filtered": filtered.view(K, channels, n, m).permute(0, 2, 3, 1)}


def collect(args, facts, lay, rows, acc, fit, centres, axes=None):
    """The one transfer of the scores (and the one synchronisation, when stacks were filled) and what the files will hold:
    (the score file's arrays, the --cluster_out arrays or None, the host labels of the classes, the summary line, the --pca
    arrays or None)."""
    host = torch.cat(rows).cpu().numpy()
    if acc.stacks:
        torch.cuda.synchronize(acc.device)          # every minibatch's copy has landed
    arrays = score_arrays(*split_rows(host, lay), facts.rotate, facts.translate)
    means = [float(np.mean(arrays[k], dtype=np.float64)) for k in ("bound", "loglik", "kl")]
    figures = {"images": int(host.shape[0]), "mean_bound": means[0], "mean_loglik": means[1], "mean_kl": means[2]}
    if acc.refined is not None:
        arrays.update(pose_refined=acc.refined["pose"].cpu().numpy(), refine_score=acc.refined["score"].cpu().numpy(),
                      refine_offset=acc.refined["offset"].cpu().numpy())
        if args.reassign:
            arrays.update(label_refined=acc.refined["label"].cpu().numpy().astype(np.int64),
                          refine_label=acc.refined["labels"].cpu().numpy(), refine_moved=acc.refined["moved"].cpu().numpy(),
                          refine_class_score=acc.refined["class_score"].cpu().numpy(),
                          refine_class_margin=acc.refined["margin"].cpu().numpy())
        if args.refine_soft:
            soft = acc.refined["soft"]
            arrays.update(refine_soft_sigma2=soft["sigma2"].numpy(), refine_log_evidence=soft["log_evidence"].cpu().numpy(),
                          refine_post_max=soft["post_max"].cpu().numpy(), refine_class_post=soft["class_post"].cpu().numpy())
    found, labels = None, acc.labels
    if fit is not None:
        labels = fit["label"].cpu().numpy().astype(np.int64)
        record = ops.KMeans.read_record(fit["record"])
        found = {"label": labels, "centres": fit["centres"].cpu().numpy(), "members": fit["members"].cpu().numpy(),
                 "inertia": np.float64(record["inertia"]), "iterations": np.int64(record["iterations"]),
                 "converged_at": np.int64(record["converged_at"]), "seed_index": fit["seed_index"].cpu().numpy().astype(np.int64),
                 "restart_inertia": fit["restart_inertia"].cpu().numpy(), "chosen_restart": np.int64(fit["chosen_restart"].item()),
                 "centre_recon": centres.cpu().numpy().reshape(args.cluster, facts.n, facts.m, -1)}
        if args.cluster_gmm is not None:
            found.update(mixture_arrays(args, facts, fit))
            labels = found["gmm_label_used"]
        found["meta"] = np.array(json.dumps(run_meta(args, facts, figures, without=("pca",))))  # that file stays what it was
    meta = run_meta(args, facts, figures)
    pca = pca_arrays(args, facts, axes, meta) if axes is not None else None
    arrays["meta"] = np.array(json.dumps(meta))
    summary = "images {}\tbound {!r}\tlog p(x|z) {!r}\tKL {!r}\tmedian ESS {:.3f}".format(
        host.shape[0], means[0], means[1], means[2], float(np.median(arrays["ess"])))
    return arrays, found, labels, summary, pca


def mixture_arrays(args, facts, fit):
    """The arrays --cluster_gmm adds to --cluster_out, transferred once; BIC and AIC are formed here on the host from the final
    log-likelihood L: p = (live - 1) + 2 live D free parameters, BIC = -2 L + p ln(assigned), AIC = -2 L + 2 p."""
    gmm = {k: v.cpu().numpy() for k, v in fit["gmm"].items()}
    record = ops.GaussianMixture.read_record(fit["gmm"]["record"])
    K, D = gmm["mean"].shape
    used = gmm["label_used"].astype(np.int64)
    live = K - record["dead"]
    p = (live - 1) + 2 * live * D
    L = record["loglik"]
    return {"gmm_weight": gmm["weight"], "gmm_mean": gmm["mean"], "gmm_var": gmm["var"], "gmm_resp": gmm["resp"],
            "gmm_max_resp": gmm["max_resp"], "gmm_label": gmm["label"].astype(np.int64), "gmm_label_used": used,
            "gmm_members": np.bincount(used[used >= 0], minlength=K).astype(np.int64), "gmm_loglik_point": gmm["loglik_point"],
            "gmm_loglik": np.float64(L), "gmm_loglik_trace": gmm["trace"], "gmm_iterations": np.int64(record["iterations"]),
            "gmm_converged_at": np.int64(record["converged_at"]), "gmm_dead": np.int64(record["dead"]),
            "gmm_bic": np.float64(-2.0 * L + p * math.log(record["assigned"]) if record["assigned"] > 0 else np.nan),
            "gmm_aic": np.float64(-2.0 * L + 2.0 * p),
            "gmm_mean_recon": fit["gmm_mean_recon"].cpu().numpy().reshape(K, facts.n, facts.m, -1)}


def _host_average(total, count, shape):
    """(sum, count, average) on the host from the device accumulators: the average is sum / count in float64 where the count is
    positive, 0 elsewhere, rounded to float32."""
    total, count = total.cpu().numpy().reshape(shape), count.cpu().numpy().reshape(shape[:3])
    average = np.divide(total, count[..., None], out=np.zeros_like(total), where=count[..., None] > 0).astype(np.float32)
    return total, count, average


def class_arrays(args, facts, acc, labels):
    """The arrays of --class_averages: sums, counts, averages and members per class; under --ctf_correct wiener also the Wiener
    averages with their numerator and denominator (another lambda needs no second run); under --refine those of the last round,
    and average_unrefined from before the first; under --reassign members (and half_members) are those of the final labels, and
    members_unrefined those of `labels`.  Under --refine_soft sum and count (and half_sum, half_count) are fractional: the
    posterior-weighted sums of the images over classes and poses, and of their coverage; members stays the count of the hard
    labels."""
    n, m, sums = facts.n, facts.m, acc.sums
    shape = (sums.n_classes, n, m, facts.channels)
    total, count, average = _host_average(*sums.result(), shape)
    members = np.bincount(labels[labels >= 0], minlength=sums.n_classes).astype(np.int64)
    classes = {"sum": total, "count": count, "average": average, "members": members}
    if args.reassign:
        labels = acc.refined["label"].cpu().numpy().astype(np.int64)
        classes.update(members=np.bincount(labels[labels >= 0], minlength=sums.n_classes).astype(np.int64), members_unrefined=members)
    if acc.refined is not None:
        classes["average_unrefined"] = _host_average(acc.refined["sum"], acc.refined["count"], shape)[2]
    if acc.wiener is not None:
        w_sum, w_den = acc.wiener[0].result()[0], acc.wiener[1].result()
        w_avg = ops.wiener_finish(w_sum, w_den, args.wiener_lambda, n, m)
        classes.update(wiener_sum=w_sum.cpu().numpy().reshape(sums.n_classes, n, m, 1), wiener_den=w_den.cpu().numpy(),
                       wiener_average=w_avg.cpu().numpy().reshape(sums.n_classes, n, m, 1),
                       wiener_lambda=np.float64(args.wiener_lambda))
    if acc.frc is not None:
        classes.update(frc_arrays(args, facts, acc, labels))
    return classes


def frc_arrays(args, facts, acc, labels):
    """The arrays --frc adds to the --class_averages file: the half-set sums, counts and members, what frc_finish left on the
    device, and from the FRC curves on the host the resolution in pixels at both thresholds."""
    n, m, K = facts.n, facts.m, acc.sums.n_classes
    h_sum, h_count = (t.cpu().numpy() for t in acc.halves.result())
    out = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in acc.frc.items()}
    L, R, ring_frequency = E.ring_layout(n, m)
    in_class = labels >= 0
    members = np.bincount(2 * labels[in_class] + (np.arange(labels.shape[0])[in_class] & 1), minlength=2 * K)
    out.update(half_sum=h_sum.reshape(K, 2, n, m, facts.channels), half_count=h_count.reshape(K, 2, n, m),
               half_members=members.astype(np.int64).reshape(K, 2), ring_frequency=ring_frequency,
               frc_mask=E.frc_mask_weights(n, m, frc_mask_radius(args, n, m), args.frc_mask_edge))
    never = np.zeros((K, facts.channels, len(FRC_THRESHOLDS)), bool)
    for j, (name, threshold) in enumerate(FRC_THRESHOLDS):
        out[name] = np.empty((K, facts.channels), np.float64)
        for k in range(K):
            for c in range(facts.channels):
                out[name][k, c], never[k, c, j] = E.frc_resolution(out["frc"][k, c], threshold, L)
    out["frc_never_below"] = never
    if acc.refined is not None:                     # what the file would have held without --refine
        out["frc_unrefined"] = np.ascontiguousarray(acc.refined["frc"].cpu().numpy())
        for name, threshold in FRC_THRESHOLDS:
            out[name + "_unrefined"] = np.array([[E.frc_resolution(out["frc_unrefined"][k, c], threshold, L)[0]
                                                  for c in range(facts.channels)] for k in range(K)], np.float64).reshape(K, facts.channels)
    return out


def write_outputs(args, facts, acc, arrays, found, labels, pca=None):
    """The files, each written atomically: the stacks, the class averages, the cluster file and its labels, the --pca file, the
    score file last."""
    for k, stack in acc.stacks.items():
        write_stack(vars(args)[k], stack.numpy().reshape(facts.images, facts.n, facts.m, facts.channels))
    if acc.sums is not None:
        write_npz(args.class_averages, class_arrays(args, facts, acc, labels))
    if found is not None:
        write_npz(args.cluster_out, found)
        if args.cluster_labels is not None:
            write_atomically(args.cluster_labels, lambda f: np.save(f, labels))
    if args.reassign_labels is not None:
        write_atomically(args.reassign_labels, lambda f: np.save(f, arrays["label_refined"]))
    if pca is not None:
        write_npz(args.pca, pca)
    write_npz(args.out, arrays)


def infer_main(args, parser_fn, build, positional=()):
    """infer.py after its own parsing.  parser_fn(argv) is the training script's parser, build(args, device) its dataset and
    network builder, `positional` stand-ins for its positional arguments when only its defaults are wanted."""
    model = load_model(args, parser_fn, build, positional)
    facts = split_facts(args, model)
    check_request(args, facts)
    lay = E.row_layout(facts.rotate, facts.translate, facts.inf_dim)
    split = upload_split(model.cfg, args.split, model.device)
    acc = Accumulators(args, facts, model.cfg, model.device)
    rows = score_walk(args, model, split, acc)
    fit, centres = cluster_walk(args, model, split, acc, rows, lay) if args.cluster is not None else (None, None)
    axes = pca_walk(args, model, split, acc, rows, lay) if args.pca is not None else None
    if args.refine is not None:
        refine_walk(args, facts, split, acc, rows, lay)
    if args.frc:
        frc_finish(args, facts, acc)
    arrays, found, labels, summary, pca = collect(args, facts, lay, rows, acc, fit, centres, axes)
    write_outputs(args, facts, acc, arrays, found, labels, pca)
    print(summary)
    return 0
