"""eigenimages.py: how the members of a class differ from their average (the root script eigenimages.py is the entry point).

Reads what infer.py wrote -- the score file of the same model and split, for the poses, and optionally a label file -- and walks
the split on the device, in dataset order: one walk for the class sums (the calls infer.py --class_averages makes, so `mean` is
its `average`), then --passes walks of block subspace iteration (ops.EigenImages, include/svae_eigen.h): each re-aligns every
minibatch from the stored poses, projects its residuals on the per-class basis and accumulates the next one.  The covariance is
never formed and nothing is read back inside a loop; the file holds the variance map, the leading eigenimages with their
eigenvalues and residuals, and every image's coordinates along the eigenimages of its class.
"""
import argparse
import json
import os
import sys

import numpy as np

POSES = ("iw", "best", "q", "refined")
MAX_COLUMNS = 64            # --components + --oversample: include/svae_eigen.h's limit on R
MAX_PASSES = 1000
MAX_BASIS = 2 ** 28         # classes * values per image * columns: one basis stays within 2 GiB
PATH_OVERRIDES = ("train_path", "test_path", "ctf_train", "ctf_test")    # what infer.load_model may override: never here


def _refuse(message):
    print("eigenimages.py: " + message, file=sys.stderr)
    raise SystemExit(2)


def eigen_arguments(argv=None):
    """eigenimages.py's command line.  Everything after a bare `--` is kept aside (args.train_argv) as in infer.py.  Every refusal
    the arguments and the two input files alone decide is made here (exit code 2), before anything touches a GPU or loads the
    kernel library."""
    from .cli import SCRIPTS
    from .infer_request import read_labels
    argv = list(sys.argv[1:] if argv is None else argv)
    train_argv = None
    if "--" in argv:
        cut = argv.index("--")
        argv, train_argv = argv[:cut], argv[cut + 1:]
    p = argparse.ArgumentParser("eigenimages.py", description="Per-class variance map and leading eigenimages of the aligned "
                                "images of a trained spatial-VAE, from the poses infer.py stored")
    p.add_argument("script", choices=sorted(SCRIPTS), help="which training script made the model")
    p.add_argument("--state", metavar="PATH.ckpt", help="training state file, as for infer.py")
    p.add_argument("--generator", metavar="G.sav", help="whole-module generator file; with --inference and, after `--`, the "
                   "training script's own flags")
    p.add_argument("--inference", metavar="Q.sav")
    p.add_argument("--scores", required=True, metavar="scores.npz", help="what infer.py --out wrote for this model and split: "
                   "the poses come from it")
    p.add_argument("--out", required=True, metavar="eigen.npz")
    p.add_argument("--split", choices=["test", "train"], default="test")
    p.add_argument("--labels", metavar="PATH.npy", help="integer class per image of the split, -1 = in no class, as "
                   "infer.py --cluster_labels and --reassign_labels write it (default: one class of all images)")
    p.add_argument("--pose", choices=list(POSES), default="iw", help="which stored estimate aligns: theta_* / dx_* of the "
                   "score file, or its pose_refined (infer.py --refine); default iw")
    p.add_argument("--interp", choices=["bicubic", "bilinear"], default="bicubic")
    p.add_argument("--components", type=int, default=8, metavar="P", help="eigenimages per class (default 8)")
    p.add_argument("--oversample", type=int, default=8, metavar="S", help="further columns the iteration carries; "
                   "P + S <= %d (default 8)" % MAX_COLUMNS)
    p.add_argument("--passes", type=int, default=8, metavar="I", help="walks over the split (default 8).  The three defaults "
                   "are conventions, not tuned values: `residual` in the output tells whether they sufficed")
    p.add_argument("--seed", type=int, default=0, help="seed of the generator the start basis is drawn from")
    p.add_argument("--minibatch_size", type=int, default=100, metavar="B")
    p.add_argument("-d", "--device", type=int, default=-2)
    args = p.parse_args(argv)
    args.train_argv = train_argv
    for name, ending in (("scores", ".npz"), ("out", ".npz"), ("labels", ".npy")):
        path = vars(args)[name]
        if path is not None and os.path.splitext(path)[1] != ending:
            p.error("--%s must end in %s (got %s)" % (name, ending, path))
    for name, lo, hi in (("components", 1, MAX_COLUMNS), ("oversample", 0, MAX_COLUMNS - 1), ("passes", 1, MAX_PASSES),
                         ("minibatch_size", 1, 2 ** 31 - 1)):
        if not lo <= vars(args)[name] <= hi:
            p.error("--%s must be in [%d, %d] (got %d)" % (name, lo, hi, vars(args)[name]))
    if args.components + args.oversample > MAX_COLUMNS:
        p.error("--components + --oversample must not exceed %d (got %d + %d)" % (MAX_COLUMNS, args.components, args.oversample))
    sav = args.generator is not None or args.inference is not None
    if (args.state is None) == (not sav):
        p.error("give either --state or --generator with --inference")
    if sav and (args.generator is None or args.inference is None):
        p.error("--generator and --inference go together")
    if sav and train_argv is None:
        p.error("--generator/--inference need the training script's flags after `--`")
    if not sav and train_argv:
        p.error("--state carries the training arguments: nothing may follow `--`")
    for path in (args.state, args.generator, args.inference, args.scores):
        if path is not None and not os.path.isfile(path):
            p.error("no such file: %s" % path)
    for name in PATH_OVERRIDES:
        setattr(args, name, None)
    args.label_array = None
    if args.labels is not None:
        try:
            args.label_array = read_labels(args.labels)
        except ValueError as e:
            p.error(str(e))
    try:
        with np.load(args.scores, allow_pickle=False) as f:
            args.score_arrays = {k: f[k] for k in f.files if k == "meta" or k == "pose_refined" or
                                 k in ("theta_" + args.pose, "dx_" + args.pose)}
        args.score_meta = json.loads(str(args.score_arrays.pop("meta")))
    except Exception as e:
        p.error("--scores %s is not a score file of infer.py: %s" % (args.scores, e))
    for key in ("script", "split"):
        if args.score_meta.get(key) != vars(args)[key]:
            p.error("--scores %s was written for the %s %r, not %r" % (args.scores, key, args.score_meta.get(key), vars(args)[key]))
    if args.pose == "refined" and "pose_refined" not in args.score_arrays:
        p.error("--pose refined needs the pose_refined of infer.py --refine, and --scores %s has none" % args.scores)
    return args


def stored_poses(args, facts, _refuse=_refuse):
    """The (images, 3) float32 poses theta, dx0, dx1 of the chosen estimate out of the score file, in the decoder's units: a
    coordinate the model does not infer is 0.  Refuses a file whose image count or pose arrays do not fit the split (through
    `_refuse`: another script that reads the same files refuses under its own name)."""
    arrays, images = args.score_arrays, facts.images
    if args.score_meta.get("images") != images:
        _refuse("--scores {} holds {} images, the {} split has {}".format(args.scores, args.score_meta.get("images"), facts.split, images))
    if args.pose == "refined":
        pose = np.asarray(arrays["pose_refined"], np.float32)
        if pose.shape != (images, 3):
            _refuse("--scores {}: pose_refined has shape {}, expected {}".format(args.scores, pose.shape, (images, 3)))
        return np.ascontiguousarray(pose)
    pose = np.zeros((images, 3), np.float32)
    for wanted, key, cols, shape in ((facts.rotate, "theta_" + args.pose, slice(0, 1), (images,)),
                                     (facts.translate, "dx_" + args.pose, slice(1, 3), (images, 2))):
        if not wanted:
            continue
        if key not in arrays or arrays[key].shape != shape:
            _refuse("--scores {} has no {} of shape {} for this model".format(args.scores, key, shape))
        pose[:, cols] = arrays[key].reshape(images, -1)
    return pose


def check_request(args, facts):
    """The refusals (exit code 2) that need the split: made after the model is loaded, before anything is allocated."""
    if facts.images < 1:
        _refuse("the {} split has no image".format(facts.split))
    if args.label_array is not None and args.label_array.shape[0] != facts.images:
        _refuse("--labels has {} entries, the {} split has {} images".format(args.label_array.shape[0], facts.split, facts.images))
    labels = np.zeros(facts.images, np.int64) if args.label_array is None else args.label_array
    classes = max(int(labels.max()) + 1, 1)         # at most 4096: read_labels refuses more
    values, columns = facts.n * facts.m * facts.channels, args.components + args.oversample
    if classes * values * columns > MAX_BASIS:
        _refuse("the basis holds classes x values per image x columns doubles: {} x {} x {} exceed 2^28".format(classes, values, columns))
    return labels, classes


def eigen_walks(args, model, facts, split, pose, labels, classes):
    """The walks on the device.  Returns (class sums, ops.EigenFit): device tensors, nothing read back."""
    import torch
    from . import elbo as E
    from . import ops
    from .infer import class_means
    n, m, bs, device = facts.n, facts.m, args.minibatch_size, model.device
    pose_d = torch.from_numpy(pose).to(device)
    label_d = torch.from_numpy(labels.astype(np.int32)).to(device)

    def minibatches():
        for lo in range(0, facts.images, bs):
            aligned, cover = E.align_at(split.data[lo:lo + bs], n, m, pose_d[lo:lo + bs], facts.rotate, facts.translate, args.interp)
            yield aligned, cover, label_d[lo:lo + bs]

    sums = ops.ClassSums(classes, n * m, facts.channels, device)
    for aligned, cover, label in minibatches():
        sums.update(aligned, cover, label)
    mean = class_means(sums).contiguous()
    columns = args.components + args.oversample
    eig = ops.EigenImages(classes, n * m, facts.channels, columns, device)
    gen = torch.Generator()
    gen.manual_seed(args.seed)
    eig.start(torch.empty(classes, n * m * facts.channels, columns, dtype=torch.float64).normal_(generator=gen).to(device))
    for it in range(args.passes):
        if it:
            eig.end_pass()
        eig.begin_pass()
        for aligned, cover, label in minibatches():
            eig.update(aligned, cover, label, mean)
    return sums, mean, eig.finish(args.components)


def eigen_arrays(args, facts, pose, labels, count, mean, fit):
    """The arrays of the output file from the host copies of what the walks left."""
    K, P, n, m, C = mean.shape[0], args.components, facts.n, facts.m, facts.channels
    members = fit.members.astype(np.int64)
    per_value = np.repeat(count[:, :, None], C, 2).reshape(K, n * m * C)
    live = members >= 2
    scale = np.where(live, members - 1.0, 1.0)
    variance = np.where(per_value >= 2, fit.ssq / np.where(per_value >= 2, per_value - 1.0, 1.0), 0.0)
    total = np.where(live, fit.ssq.sum(1) / scale, 0.0)
    eigenvalues = fit.eigenvalues[:, :P] + 0.0
    ratio = np.where(total[:, None] > 0, eigenvalues / np.where(total > 0, total, 1.0)[:, None], 0.0)
    meta = {k: vars(args)[k] for k in ("script", "state", "generator", "inference", "scores", "split", "labels", "pose", "interp",
                                       "components", "oversample", "passes", "seed")}
    meta.update(scores_state=args.score_meta.get("state"), images=facts.images, classes=K)
    return {"mean": mean.astype(np.float32).reshape(K, n, m, C), "count": count.reshape(K, n, m), "members": members,
            "variance": variance.reshape(K, n, m, C), "total_variance": total, "eigenvalues": eigenvalues,
            "eigenimages": fit.eigenimages.reshape(K, P, n, m, C), "explained_variance_ratio": ratio, "residual": fit.residual,
            "coords": fit.coords, "label": labels.astype(np.int64), "pose": pose, "meta": np.array(json.dumps(meta))}


def eigen_main(args, parser_fn, build, positional=()):
    """eigenimages.py after its own parsing; parser_fn, build and positional as for infer.infer_main."""
    from . import infer
    model = infer.load_model(args, parser_fn, build, positional)
    facts = infer.split_facts(args, model)
    pose = stored_poses(args, facts)
    labels, classes = check_request(args, facts)
    split = infer.upload_split(model.cfg, args.split, model.device)
    sums, mean, fit = eigen_walks(args, model, facts, split, pose, labels, classes)
    count, mean = sums.count.cpu().numpy(), mean.cpu().numpy()          # the one transfer, after the last launch
    fit = type(fit)(*(t.cpu().numpy() for t in fit))
    arrays = eigen_arrays(args, facts, pose, labels, count, mean, fit)
    infer.write_npz(args.out, arrays)
    live = arrays["members"] >= 2
    print("eigenimages.py: %d images, %d classes (%d with two members or more), %d components from %d columns in %d passes; "
          "largest residual / eigenvalue %.3g" % (facts.images, classes, int(live.sum()), args.components,
                                                  args.components + args.oversample, args.passes,
                                                  float(np.max(arrays["residual"][live] / np.maximum(arrays["eigenvalues"][live][:, :1], 1e-300),
                                                               initial=0.0))))
    return 0
