"""What infer.py is asked to do, stated once: its options, the rules between them, the rules against the model, and the record
of the run.

OPTIONS has one row per option: its flags and what argparse needs, its group (the option that makes it meaningful), its value
inside that group when it is not given, and its check.  GROUPS and OUTPUT_GROUPS list the groups in the order their rules are
applied, each with the rules of the group's own option and the keys it adds to a file's `meta`.  infer_arguments builds the
parser from the rows, parses, walks the groups (_walk) and ends with the few rules that are no row's; REQUEST_RULES is the same
for check_request, the rules that need the split and the model (SplitFacts); run_meta makes `meta` from the groups.  A new option
of a regular kind is one row.  Nothing here touches a device or loads the kernel library: every refusal (exit code 2) is made
before that.  spatial_vae_amd.infer re-exports every name; the scripts and the tests use them through it.
"""
import argparse
import collections
import os
import sys

import numpy as np

from . import elbo as E
from . import ops
from .cli import SCRIPTS

INFER_MAX_CHUNK = 1024      # samples per image in one decoder call (the kernels' SVAE_IW_MAX_SAMPLES)
INFER_PATH_OVERRIDES = ("train_path", "test_path", "ctf_train", "ctf_test")
INFER_MAX_CLASSES = 4096    # classes of --labels (svae_class_sums_update's limit)
INFER_STACK_FORMATS = (".npy", ".mrcs")
INFER_MAX_CLUSTERS = min(INFER_MAX_CLASSES, ops.KMeans.MAX_K, ops.GaussianMixture.MAX_K)    # classes of --cluster
INFER_MAX_RESTARTS = 16
INFER_MAX_GMM_ITERS = 1000
INFER_MAX_GMM_RESP = 2 ** 28        # images * K of --cluster_gmm: the (images, K) float64 responsibilities stay within 2 GiB
INFER_FRC_MAX_CLASSES = INFER_MAX_CLASSES // 2      # --frc keeps two half-set sums per class
INFER_FRC_MAX_BOX = 1024    # include/svae_frc.h's limit on n and m
INFER_MAX_REFINE_ROUNDS = 10
INFER_MAX_REFINE_ANGLES = 32    # include/svae_refine.h's limits on A and S
INFER_MAX_REFINE_SHIFT = 8
INFER_MAX_REASSIGN_CLASSES = 4096   # include/svae_classify.h's limit on M (2K slots never arise: a half sees its own K averages)
INFER_MAX_SOFT_CLASSES = 64         # include/svae_expect.h's limit on M
INFER_MAX_PCA_STEPS = 50
INFER_MAX_PCA_PARTIALS = ops.LatentPCA.MAX_PARTIALS     # G D (D + 1) / 2
INF = float("inf")


# ---- the kinds of check on one option's value: each gives what follows "--name must " in the refusal, or None ----------------
def between(lo, hi, tail, open=""):
    """lo <= v <= hi, with a bound named in `open` excluded (nan lies in no interval).  `tail` is what follows "must be", with
    %(lo)s, %(hi)s and %(v)s: the messages differ in what they quote, and stay as they are."""
    def check(v):
        inside = (lo < v if "lo" in open else lo <= v) and (v < hi if "hi" in open else v <= hi)
        return None if inside else "be " + tail % {"lo": lo, "hi": hi, "v": v}
    return check


def whole(lo, hi, got=" (got %(v)d)"):
    return between(lo, hi, "in [%(lo)d, %(hi)d]" + got)


def at_least(lo, got=" (got %(v)d)"):
    return between(lo, INF, ">= %(lo)d" + got)


def finite(above):
    """A finite number `above` (">" or ">=") 0."""
    return between(0, INF, "a finite number " + above + " 0 (got %(v)r)", open="hi" if above == ">=" else "lo hi")


def suffix(*endings):
    def check(path):
        return None if os.path.splitext(path)[1] in endings else "end in %s (got %s)" % (" or ".join(endings), path)
    return check


# ---- the options -------------------------------------------------------------------------------------------------------------
# group: the GROUPS entry whose option must be there for this one to mean anything (given without it: "--dest needs --group");
# inside: its value inside that group when it is not given (a function takes the arguments), outside it stays None;
# check: applied to a value that is there, where its group's turn comes; kw: add_argument's.
Option = collections.namedtuple("Option", "flags dest group inside check kw")


def _opt(*flags, group=None, inside=None, check=None, **kw):
    return Option(flags, flags[-1].lstrip("-"), group, inside, check, kw)


OPTIONS = (
    _opt("script", choices=sorted(SCRIPTS), help="which training script made the model"),
    _opt("--state", metavar="PATH.ckpt", help="training state file (--checkpoint_interval): model, arguments, dataset"),
    _opt("--generator", metavar="G.sav", help="whole-module generator file; with --inference and, after `--`, the training "
         "script's own flags"),
    _opt("--inference", metavar="Q.sav"),
    _opt("--out", required=True, metavar="scores.npz"),
    _opt("--split", choices=["test", "train"], default="test"),
    _opt("--num_samples", check=at_least(1, ""), type=int, default=64, metavar="K",
         help="samples per image (any K >= 1; default 64)"),
    _opt("--chunk", check=whole(1, INFER_MAX_CHUNK, ""), type=int, default=64, metavar="C", help="samples per image decoded at "
         "once, 1..%d (default 64): memory is that of a B*C minibatch" % INFER_MAX_CHUNK),
    _opt("--minibatch_size", check=at_least(1, ""), type=int, default=100, metavar="B"),
    _opt("--seed", type=int, default=0, help="seed of the generator the N(0,1) draws come from"),
    _opt("-d", "--device", type=int, default=-2),
) + tuple(_opt("--" + name, help="instead of the path stored in the state file") for name in INFER_PATH_OVERRIDES) + (
    _opt("--aligned", check=suffix(*INFER_STACK_FORMATS), metavar="PATH", help="also write every image brought into the model's "
         "canonical frame (its pose removed), in dataset order: .npy = (images, rows, cols, C) float32, .mrcs = an MRC stack (one "
         "channel only).  The observed images resampled, nothing else: not masked, and CTF-corrected only under "
         "--ctf_correct flip"),
    _opt("--recon", check=suffix(*INFER_STACK_FORMATS), metavar="PATH", help="also write every image's pose-free reconstruction "
         "(the decoder on the un-posed grid at the image's content latents), same formats"),
    _opt("--class_averages", check=suffix(".npz"), metavar="PATH.npz", help="also write the sums, counts and averages of the "
         "aligned images over the pixels each image covers: per class of --labels, else one class of all images"),
    _opt("--labels", group="class_averages", metavar="PATH.npy", help="integer class per image of the split, -1 = in no class "
         "(with --class_averages; at most %d classes)" % INFER_MAX_CLASSES),
    _opt("--pose", choices=list(E.POSES), help="which estimate aligns, and whose content latents --recon decodes: "
         "the importance-weighted mean (iw, the default), the best sample, or q's mean"),
    _opt("--interp", choices=["bicubic", "bilinear"], help="resampling of --aligned / --class_averages (default "
         "bicubic: Catmull-Rom)"),
    _opt("--ctf_correct", choices=["flip", "wiener"], help="particles with a CTF table only: correct each observed "
         "image by its own transfer function H before it is aligned.  flip: multiply its Fourier coefficients by the sign of H; "
         "--aligned and the class averages then hold phase-flipped particles.  wiener: leave those as they are and add to "
         "--class_averages the Wiener averages sum(H y) / (sum(H^2) + lambda) per class, with their numerator and denominator.  "
         "Scoring is untouched either way"),
    _opt("--wiener_lambda", group="wiener", inside=1.0, check=finite(">="), type=float, metavar="X",
         help="with --ctf_correct wiener: the regulariser, X >= 0, the reciprocal of the per-particle spectral signal-to-noise "
         "ratio assumed (default 1.0: a convention, not a tuned value; the .npz keeps numerator and denominator, so another X "
         "needs no second run)"),
    _opt("--cluster", check=whole(2, INFER_MAX_CLUSTERS), type=int, metavar="K", help="k-means of the content "
         "latents into K classes on the device (2..%d, at most the number of images), seeded by k-means++; the classes take the "
         "place of --labels for --class_averages, and --pose selects whose content latents are clustered "
         "(z_iw, z_best or z_q)" % INFER_MAX_CLUSTERS),
    _opt("--cluster_out", group="cluster", check=suffix(".npz"), metavar="PATH.npz", help="with --cluster (required): labels, "
         "centres, members, inertia, the seeds, every restart's inertia and the decoder's un-posed reconstruction of each centre"),
    _opt("--cluster_labels", group="cluster", check=suffix(".npy"), metavar="PATH.npy", help="with --cluster: also write the "
         "labels in the format --labels reads"),
    _opt("--cluster_iters", group="cluster", inside=100, check=at_least(1, ""), type=int, metavar="I",
         help="Lloyd iterations per restart, I >= 1 (default 100; iterations after convergence change nothing)"),
    _opt("--cluster_restarts", group="cluster", inside=1, check=whole(1, INFER_MAX_RESTARTS, ""), type=int, metavar="R",
         help="independent seedings, 1..%d (default 1); the one of lowest inertia is kept, the first "
         "of equals" % INFER_MAX_RESTARTS),
    _opt("--cluster_seed", group="cluster", inside=lambda args: args.seed, type=int, metavar="S",
         help="seed of the generator the k-means++ uniforms come from (default --seed)"),
    _opt("--cluster_gmm", group="cluster", check=whole(1, INFER_MAX_GMM_ITERS), type=int, metavar="I",
         help="with --cluster: fit a diagonal-covariance Gaussian mixture to the content latents by I EM iterations (1..%d) on the "
         "device, started from the k-means result.  Its labels take the place of the k-means labels for everything downstream; "
         "--cluster_out keeps the k-means arrays and gains the mixture's (gmm_*): responsibilities, log-likelihood, BIC and AIC "
         "among them" % INFER_MAX_GMM_ITERS),
    _opt("--cluster_gmm_reg", group="cluster_gmm", inside=1e-6, check=finite(">"), type=float, metavar="X",
         help="with --cluster_gmm: added to every variance, X > 0 (default 1e-6: a convention, not a tuned value)"),
    _opt("--cluster_gmm_tol", group="cluster_gmm", inside=1e-8, check=finite(">="), type=float, metavar="X",
         help="with --cluster_gmm: the fit is frozen once an iteration gains no more than X |log-likelihood|, X >= 0 (default "
         "1e-8, a convention too)"),
    _opt("--cluster_min_resp", group="cluster_gmm", inside=0.0, check=between(0, 1, "in [0, 1) (got %(v)r)", open="hi"),
         type=float, metavar="P",
         help="with --cluster_gmm: an image whose largest responsibility is below P, 0 <= P < 1, is in no class (label -1; default "
         "0, a convention too: every image stays)"),
    _opt("--pca", check=suffix(".npz"), metavar="PATH.npz", help="also write the principal axes of the split's content latents "
         "(--pose selects whose: z_iw, z_best or z_q), found on the device: mean, covariance, eigenvalues, components (rows are "
         "axes), explained variance ratio and every image's projections"),
    _opt("--pca_components", group="pca", check=at_least(1), type=int, metavar="P", help="with --pca: the columns of "
         "projections, 1..z_dim (default z_dim)"),
    _opt("--pca_traverse", group="pca", inside=0, check=at_least(0), type=int, metavar="Q",
         help="with --pca: also decode a walk along each of the first Q axes, 0..z_dim (default 0): traverse_latents and "
         "traverse_images"),
    _opt("--pca_steps", group="pca", inside=5, check=whole(1, INFER_MAX_PCA_STEPS), type=int, metavar="T",
         help="with --pca_traverse: steps on each side of the mean, 1..%d (default 5: 2 T + 1 frames)" % INFER_MAX_PCA_STEPS),
    _opt("--pca_span", group="pca", inside=2.0, check=finite(">"), type=float, metavar="X",
         help="with --pca_traverse: how far the walk reaches on each side, in standard deviations along the axis, a finite X > 0 "
         "(default 2.0)"),
    _opt("--pca_per_class", group="pca", action="store_true", help="with --pca and --cluster: also the principal axes of every "
         "class (the arrays prefixed class_), under the labels the class averages are built from; a walk starts from the class's "
         "mean along the class's own axes"),
    _opt("--frc", action="store_true", help="with --class_averages: also accumulate each class over two disjoint halves (image i "
         "of the split in half i & 1) and add their sums, the Fourier ring correlation of the two half averages, the resolution at "
         "the 0.143 and 0.5 thresholds and the full average filtered by sqrt(2 FRC / (1 + FRC)).  One model aligns both halves, so "
         "the figure is optimistic"),
    _opt("--frc_mask_radius", group="frc", check=finite(">="), type=float, metavar="PX",
         help="with --frc: radius of the soft circular mask put on both half averages before the transform (default max(min(rows, "
         "cols)/2 - edge, 1): a convention, not a tuned value); 0 = no mask"),
    _opt("--frc_mask_edge", group="frc", inside=3.0, check=finite(">"), type=float, metavar="PX",
         help="with --frc: width of the mask's raised-cosine edge, PX > 0 (default 3, a convention too)"),
    _opt("--refine", check=whole(1, INFER_MAX_REFINE_ROUNDS), type=int, metavar="R", help="with --class_averages: R "
         "rounds (1..%d) of reference-based alignment.  Each round takes the class averages as they stand as references, searches "
         "a small neighbourhood of rotations and shifts around every image's pose for the best weighted correlation with the "
         "average of its class, and accumulates the averages again at the new poses.  With --frc each half is refined against its "
         "own half average only.  The file keeps the first averages as average_unrefined" % INFER_MAX_REFINE_ROUNDS),
    _opt("--refine_angles", group="refine", inside=5, check=whole(0, INFER_MAX_REFINE_ANGLES), type=int, metavar="A",
         help="with --refine: rotations searched on each side of the current one, 0..%d (default 5)" % INFER_MAX_REFINE_ANGLES),
    _opt("--refine_step", group="refine", inside=2.0, check=finite(">"), type=float, metavar="DEG",
         help="with --refine: their spacing in degrees, DEG > 0 (default 2.0)"),
    _opt("--refine_shift", group="refine", inside=2, check=whole(0, INFER_MAX_REFINE_SHIFT), type=int, metavar="S",
         help="with --refine: shifts searched, whole pixels up to S on both axes, 0..%d (default 2)" % INFER_MAX_REFINE_SHIFT),
    _opt("--reassign", action="store_true", help="with --refine: multi-reference alignment.  Each round scores every labelled "
         "image against the average of EVERY class over the same neighbourhood of poses and moves it to the class it fits best, "
         "then refines its pose against that class; with --frc against the averages of its own half only.  A class that loses "
         "every member has an all-zero average from then on, which the search skips: it stays empty"),
    _opt("--reassign_labels", group="reassign", check=suffix(".npy"), metavar="PATH.npy", help="with --reassign: also write the "
         "final labels in the format --labels reads"),
    _opt("--refine_soft", action="store_true", help="with --refine --reassign: maximum-likelihood class averages.  Each round "
         "still names every image's best class and pose as --reassign does (labels, poses and --aligned keep their meaning), but "
         "the averages are accumulated softly: the image is spread over its best classes and over every rotation and shift of the "
         "search by its posterior probability under Gaussian noise, and added so weighted.  The class file's sum and count are "
         "then fractional"),
    _opt("--refine_soft_classes", group="refine_soft", inside=8, check=whole(1, INFER_MAX_SOFT_CLASSES), type=int, metavar="T",
         help="with --refine_soft: the classes an image is spread over, its T best of the round, 1..%d "
         "(default 8)" % INFER_MAX_SOFT_CLASSES),
    _opt("--refine_soft_sigma2", group="refine_soft", check=finite(">"), type=float, metavar="X",
         help="with --refine_soft: the noise variance per pixel, a finite X > 0 (default: estimated each round from the residuals "
         "of the images against the averages of their classes at their current poses)"),
)
OPTION = {o.dest: o for o in OPTIONS}


def _given(value):
    """An option is there: a value was given, or a switch is on."""
    return value is not None and value is not False


# ---- the groups and the kinds of rule on a group's own option: each gives the refusal, or None -------------------------------
def needs(other, by=None):
    """The group's option -- or `by`, where that one is given -- needs `other`."""
    def rule(args, group):
        if (by is None or _given(vars(args)[by])) and not _given(vars(args)[other]):
            return "--%s needs --%s" % (by or group.label, other)
    return rule


def excludes(other, message, value=None):
    """The group's option does not go with `other` (being `value`, where one is named)."""
    def rule(args, group):
        if _given(vars(args)[other]) and value in (None, vars(args)[other]):
            return message
    return rule


def refused_if(bad, message):
    """What is no kind of its own: `message` (%-formatted with the arguments) where bad(args)."""
    def rule(args, group):
        if bad(args):
            return message % vars(args)
    return rule


def check(dest):
    """The check of the row `dest`, on a value that is there."""
    def rule(args, group):
        tail = OPTION[dest].check(vars(args)[dest]) if vars(args)[dest] is not None else None
        return tail and "--%s must %s" % (dest, tail)
    return rule


class Group(object):
    """name: the option the group hangs on (None: no option, its rules always hold); rules: what its own option must satisfy,
    in order; label: how the refusals name it; active(args); meta: the keys it adds to a file's `meta` where it is active, each
    an argument's name, or (key, argument's name), or (key, function of (args, facts))."""

    def __init__(self, name, *rules, label=None, active=None, meta=()):
        self.name, self.rules, self.label, self.meta = name, rules, label or name, meta
        self.active = active or ((lambda args: True) if name is None else (lambda args: _given(vars(args)[name])))


def frc_mask_radius(args, n, m):
    """--frc_mask_radius, or its default for an n x m box: max(min(n, m)/2 - edge, 1)."""
    return max(min(n, m) / 2.0 - args.frc_mask_edge, 1.0) if args.frc_mask_radius is None else float(args.frc_mask_radius)


# in the order the rules are applied, which decides what an argv that breaks several of them is told
GROUPS = (
    Group(None, needs("refine", by="reassign")),
    Group("refine_soft", needs("refine"), needs("reassign"), meta=("refine_soft", "refine_soft_classes", "refine_soft_sigma2")),
    Group("reassign", meta=("reassign", "reassign_labels")),
    Group("refine", check("refine"), needs("class_averages"),
          excludes("ctf_correct", "--refine does not take --ctf_correct wiener: the half references would need half denominators",
                   value="wiener"),
          meta=("refine", "refine_angles", "refine_step", "refine_shift")),
    Group("frc", needs("class_averages"),
          meta=("frc", ("frc_mask_radius", lambda args, facts: frc_mask_radius(args, facts.n, facts.m)), "frc_mask_edge")),
    Group("cluster", check("cluster"), excludes("labels", "--cluster makes the classes itself: it excludes --labels"),
          needs("cluster_out"),
          meta=("pose", "cluster", "cluster_out", "cluster_labels", "cluster_iters", "cluster_restarts", "cluster_seed")),
    Group("cluster_gmm", meta=("cluster_gmm", "cluster_gmm_reg", "cluster_gmm_tol", "cluster_min_resp")),
    Group("pca", check("pca"), needs("cluster", by="pca_per_class"),
          meta=("pca", ("pca_pose", "pose"), "pca_components", "pca_traverse", "pca_steps", "pca_span", "pca_per_class")),
    Group("ctf_correct",
          refused_if(lambda a: a.script != "particles",
                     "--ctf_correct is for particles (the script whose images have a CTF), not %(script)s"),
          refused_if(lambda a: a.ctf_correct == "flip" and a.aligned is None and a.class_averages is None,
                     "--ctf_correct flip needs one of --aligned, --class_averages"),
          meta=("ctf_correct", "wiener_lambda")),
    Group("wiener", needs("class_averages"), label="ctf_correct wiener", active=lambda args: args.ctf_correct == "wiener"),
    Group(None, check("num_samples"), check("chunk"), check("minibatch_size")),
)
# these come after the model's files have been looked for
OUTPUT_GROUPS = (
    Group(None, check("aligned"), check("recon")),
    Group("class_averages", check("class_averages")),
)
# the image outputs as one group, for `meta` alone: pose, interp and labels are recorded only with one of them
OUTPUTS = Group("outputs", active=lambda args: any(vars(args)[k] is not None for k in ("aligned", "recon", "class_averages")),
                meta=("pose", "interp", "labels", "aligned", "recon", "class_averages"))
GROUP = {g.name: g for g in GROUPS + OUTPUT_GROUPS + (OUTPUTS,) if g.name is not None}
# the order of a file's `meta`; the --cluster_out file is written `without` "pca": it stays what it was before --pca existed
META_GROUPS = ("outputs", "ctf_correct", "frc", "refine", "reassign", "refine_soft", "cluster", "cluster_gmm", "pca")


def _walk(p, args, groups):
    """Every group in turn.  One that is not active refuses the options that hang on it; an active one fills in their values,
    then applies its own rules and their checks, in the rows' order."""
    values = vars(args)
    for group in groups:
        rows = [o for o in OPTIONS if o.group == group.name] if group.name is not None else []
        if not group.active(args):
            given = [o.dest for o in rows if _given(values[o.dest])]
            if given:
                p.error("--%s needs --%s" % (given[0], group.label))
            continue
        for o in rows:
            if values[o.dest] is None and o.inside is not None:
                values[o.dest] = o.inside(args) if callable(o.inside) else o.inside
        for rule in group.rules + tuple(check(o.dest) for o in rows if o.check is not None):
            message = rule(args, group)
            if message:
                p.error(message)


def infer_arguments(argv=None, max_reassign_classes=None):
    """infer.py's command line.  Everything after a bare `--` is kept aside (args.train_argv): with --generator/--inference
    it is the training script's own flags, parsed later by that script's parser.  Refusals (exit code 2) are made here, before
    anything touches a GPU or loads the kernel library.  max_reassign_classes: instead of INFER_MAX_REASSIGN_CLASSES."""
    argv = list(sys.argv[1:] if argv is None else argv)
    train_argv = None
    if "--" in argv:
        cut = argv.index("--")
        argv, train_argv = argv[:cut], argv[cut + 1:]
    p = argparse.ArgumentParser("infer.py", description="Per-image pose, latents and K-sample importance-weighted likelihood "
                                "of a trained spatial-VAE")
    for o in OPTIONS:
        p.add_argument(*o.flags, **o.kw)
    args = p.parse_args(argv)
    args.train_argv = train_argv
    _walk(p, args, GROUPS)
    sav = args.generator is not None or args.inference is not None
    if (args.state is None) == (not sav):
        p.error("give either --state or --generator with --inference")
    if sav and (args.generator is None or args.inference is None):
        p.error("--generator and --inference go together")
    if sav and train_argv is None:
        p.error("--generator/--inference need the training script's flags after `--`")
    if not sav and train_argv:
        p.error("--state carries the training arguments: nothing may follow `--`")
    for path in (args.state, args.generator, args.inference):
        if path is not None and not os.path.isfile(path):
            p.error("no such file: %s" % path)
    _walk(p, args, OUTPUT_GROUPS)
    if not OUTPUTS.active(args):
        for name in ("pose", "interp"):
            if vars(args)[name] is not None and not (name == "pose" and (args.cluster is not None or args.pca is not None)):
                p.error("--%s needs one of --aligned, --recon, --class_averages" % name)
    args.pose, args.interp = args.pose or "iw", args.interp or "bicubic"
    args.label_array = None
    if args.labels is not None:
        try:
            args.label_array = read_labels(args.labels)
        except ValueError as e:
            p.error(str(e))
        if args.frc and args.label_array.size and args.label_array.max() + 1 > INFER_FRC_MAX_CLASSES:
            p.error("--frc keeps two sums per class: at most %d classes (--labels has %d)"
                    % (INFER_FRC_MAX_CLASSES, args.label_array.max() + 1))
    classes = args.cluster if args.cluster is not None else 1 if args.label_array is None or not args.label_array.size \
        else int(args.label_array.max()) + 1
    limit = INFER_MAX_REASSIGN_CLASSES if max_reassign_classes is None else max_reassign_classes
    if args.reassign and classes > limit:
        p.error("--reassign scores every image against every class: at most %d classes (got %d)" % (limit, classes))
    return args


def read_labels(path):
    """The int64 class labels of a --labels file; ValueError with the reason when it is no 1-D integer .npy with values >= -1
    and at most INFER_MAX_CLASSES classes."""
    if not os.path.isfile(path):
        raise ValueError("no such file: %s" % path)
    try:
        labels = np.load(path, allow_pickle=False)
    except Exception as e:
        raise ValueError("--labels %s is not a .npy array: %s" % (path, e))
    if not isinstance(labels, np.ndarray) or labels.dtype.kind not in "iu":
        raise ValueError("--labels %s must be an integer array (got %s)" % (path, getattr(labels, "dtype", type(labels).__name__)))
    if labels.ndim != 1:
        raise ValueError("--labels %s must be 1-D, one entry per image (got shape %s)" % (path, labels.shape))
    labels = labels.astype(np.int64)
    if labels.size and labels.min() < -1:
        raise ValueError("--labels %s has a value below -1 (%d)" % (path, labels.min()))
    if labels.size and labels.max() + 1 > INFER_MAX_CLASSES:
        raise ValueError("--labels %s has %d classes, at most %d are supported" % (path, labels.max() + 1, INFER_MAX_CLASSES))
    return labels


def _refuse(message):
    print("infer.py: " + message, file=sys.stderr)
    raise SystemExit(2)


# ---- the request against the split and the model -----------------------------------------------------------------------------
# What check_request needs to know of the split and the model, as plain Python values.  ctf_rows: the rows of the split's CTF
# parameter table, None = it has none.
SplitFacts = collections.namedtuple("SplitFacts", "images n m channels rotate translate inf_dim z_scale split ctf_rows")
Figures = collections.namedtuple("Figures", "z_dim pairs labels")    # what the rules and their messages derive from both


def _figures(args, facts):
    z_dim = E.row_layout(facts.rotate, facts.translate, facts.inf_dim).z_dim
    return Figures(z_dim, z_dim * (z_dim + 1) // 2, None if args.label_array is None else args.label_array.shape[0])


_BOX = "--%s takes boxes of at most {0}x{0} pixels, these images are {{f.n}}x{{f.m}}".format(INFER_FRC_MAX_BOX)
_MRCS = "--{0} {{a.{0}}}: an MRC stack holds one channel, these images have {{f.channels}}"
# (the argument the rules hang on: they apply where it is given, ((a further argument that must be given, or None; refused
# where this holds of a = the arguments, f = the facts and x = their figures; the message, formatted with the three), ...)), in
# the order they are applied: the first that fails is the one reported
REQUEST_RULES = (
    ("cluster", (
        (None, lambda a, f, x: x.z_dim < 1, "--cluster groups the content latents, and this model has none (z_dim = 0)"),
        (None, lambda a, f, x: f.z_scale == 0,
         "--cluster: this state is from before the run's z_delay ended (z_scale = 0): every content latent is 0"),
        (None, lambda a, f, x: a.cluster > f.images, "--cluster {a.cluster} exceeds the {f.images} images of the {f.split} split"),
        ("cluster_gmm", lambda a, f, x: f.images * a.cluster > INFER_MAX_GMM_RESP,
         "--cluster_gmm keeps a responsibility per image and class: {f.images} images x {a.cluster} classes exceed 2^28"))),
    ("pca", (
        (None, lambda a, f, x: x.z_dim < 1, "--pca takes the axes of the content latents, and this model has none (z_dim = 0)"),
        (None, lambda a, f, x: f.images < 1, "--pca: the {f.split} split has no image"),
        ("pca_components", lambda a, f, x: a.pca_components > x.z_dim,
         "--pca_components must be in [1, {x.z_dim}], this model's z_dim (got {a.pca_components})"),
        (None, lambda a, f, x: a.pca_traverse > x.z_dim,
         "--pca_traverse must be in [0, {x.z_dim}], this model's z_dim (got {a.pca_traverse})"),
        ("pca_per_class", lambda a, f, x: a.cluster * x.pairs > INFER_MAX_PCA_PARTIALS,
         "--pca_per_class keeps z_dim (z_dim + 1) / 2 products per class: {a.cluster} classes x {x.pairs} exceed %d"
         % INFER_MAX_PCA_PARTIALS))),
    ("refine", (
        (None, lambda a, f, x: not f.rotate and not f.translate,
         "--refine searches rotations and shifts, and this model infers neither"),
        (None, lambda a, f, x: max(f.n, f.m) > INFER_FRC_MAX_BOX, _BOX % "refine"))),
    ("frc", (
        (None, lambda a, f, x: max(f.n, f.m) > INFER_FRC_MAX_BOX, _BOX % "frc"),)),
    ("label_array", (
        (None, lambda a, f, x: x.labels != f.images,
         "--labels has {x.labels} entries, the {f.split} split has {f.images} images"),)),
    ("aligned", (
        (None, lambda a, f, x: a.aligned.endswith(".mrcs") and f.channels != 1, _MRCS.format("aligned")),)),
    ("recon", (
        (None, lambda a, f, x: a.recon.endswith(".mrcs") and f.channels != 1, _MRCS.format("recon")),)),
    ("ctf_correct", (
        (None, lambda a, f, x: f.ctf_rows is None,
         "--ctf_correct needs the CTF parameters of the {f.split} split: the run has no --ctf-{f.split} table"),
        (None, lambda a, f, x: f.ctf_rows < f.images,
         "the CTF table of the {f.split} split has {f.ctf_rows} rows, the split has {f.images} images"),
        (None, lambda a, f, x: f.channels != 1, "--ctf_correct takes one-channel images, these have {f.channels}"),
        (None, lambda a, f, x: f.rotate and f.n != f.m,
         "--ctf_correct on a model that rotates needs a square box (the transfer function commutes with the rotation "
         "only there); these images are {f.n}x{f.m}"))),
)


def check_request(args, facts):
    """Every refusal (exit code 2) that depends on the data or the model: a function of the arguments and the facts alone, made
    before anything is allocated for the run."""
    figures = _figures(args, facts)
    for group, rules in REQUEST_RULES:
        if not _given(vars(args)[group]):
            continue
        for also, bad, message in rules:
            if (also is None or _given(vars(args)[also])) and bad(args, facts, figures):
                _refuse(message.format(a=args, f=facts, x=figures))


# ---- the record of the run ---------------------------------------------------------------------------------------------------
def run_meta(args, facts, figures, without=()):
    """The `meta` of the files: what was asked and, as `figures`, what was found ({"images", "mean_bound", "mean_loglik",
    "mean_kl"}), then the keys of every active group of META_GROUPS that is not in `without`, in that order.  A key two groups
    name (pose) keeps its first place.  json.dumps writes this order, and runs are compared byte for byte."""
    meta = {k: vars(args)[k] for k in ("script", "state", "generator", "inference", "num_samples", "chunk", "seed", "split")}
    meta.update(figures)
    for name in META_GROUPS:
        if name in without or not GROUP[name].active(args):
            continue
        for key in GROUP[name].meta:
            key, source = key if isinstance(key, tuple) else (key, key)
            meta[key] = source(args, facts) if callable(source) else vars(args)[source]
    return meta
