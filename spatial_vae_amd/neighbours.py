"""neighbours.py: one denoised image per image, without classes (the root script neighbours.py is the entry point).

Reads what infer.py wrote -- the score file of the same model and split, for the content latents and the poses -- and works on
the device: the exact K nearest neighbours of every image among the latents of the whole split (ops.NeighbourSearch,
include/svae_neighbours.h), the graph's statistics, and with --averages the aligned stack of the split (the walk eigenimages.py
makes, at the stored poses) and every image's average over itself and its neighbours (ops.neighbour_average).  Nothing is read
back inside a loop; the file holds the lists, the slots and weights the averages were formed from, and the poses.
"""
import argparse
import json
import os
import sys

import numpy as np

from .eigen_images import PATH_OVERRIDES, POSES, stored_poses

LATENTS = ("iw", "q", "best")
MAX_NEIGHBOURS = 256        # include/svae_neighbours.h's limit on K
QUERY_BLOCK = 4096          # queries of one svae_nbr_search call: a convention, the lists do not depend on it


def _refuse(message):
    print("neighbours.py: " + message, file=sys.stderr)
    raise SystemExit(2)


def neighbour_arguments(argv=None):
    """neighbours.py's command line.  Everything after a bare `--` is kept aside (args.train_argv) as in infer.py.  Every refusal
    the arguments and the score file alone decide is made here (exit code 2), before anything touches a GPU or loads the kernel
    library."""
    from .cli import SCRIPTS
    argv = list(sys.argv[1:] if argv is None else argv)
    train_argv = None
    if "--" in argv:
        cut = argv.index("--")
        argv, train_argv = argv[:cut], argv[cut + 1:]
    p = argparse.ArgumentParser("neighbours.py", description="Every image's nearest neighbours among the content latents of a "
                                "trained spatial-VAE, and the average of their aligned images, from what infer.py stored")
    p.add_argument("script", choices=sorted(SCRIPTS), help="which training script made the model")
    p.add_argument("--state", metavar="PATH.ckpt", help="training state file, as for infer.py")
    p.add_argument("--generator", metavar="G.sav", help="whole-module generator file; with --inference and, after `--`, the "
                   "training script's own flags")
    p.add_argument("--inference", metavar="Q.sav")
    p.add_argument("--scores", required=True, metavar="scores.npz", help="what infer.py --out wrote for this model and split: "
                   "the latents and the poses come from it")
    p.add_argument("--out", required=True, metavar="nbr.npz")
    p.add_argument("--averages", metavar="avg.npy|.mrcs", help="write every image's neighbour average, (images, rows, cols, C) "
                   "float32; without it only the graph is made")
    p.add_argument("--support", metavar="support.npy", help="with --averages: the summed weight behind every pixel, (images, "
                   "rows, cols) float64")
    p.add_argument("--neighbours", type=int, default=32, metavar="K", help="neighbours per image, 1..%d (default 32)" % MAX_NEIGHBOURS)
    p.add_argument("--latent", choices=list(LATENTS), default="iw", help="which stored content latent is compared: z_* of the "
                   "score file; default iw")
    p.add_argument("--pose", choices=list(POSES), default="iw", help="which stored estimate aligns: theta_* / dx_* of the "
                   "score file, or its pose_refined (infer.py --refine); default iw")
    p.add_argument("--interp", choices=["bicubic", "bilinear"], default="bicubic")
    p.add_argument("--weights", choices=["uniform", "gaussian"], default="uniform", help="gaussian: exp(-d2 / (2 s^2)) with s^2 "
                   "the squared distance to the image's farthest listed neighbour; the image itself has weight 1")
    p.add_argument("--exclude_self", action="store_true", help="leave the image itself out of its average")
    p.add_argument("--stack_gib", type=float, default=32.0, metavar="G", help="refuse an aligned stack of more than G GiB of "
                   "device memory (default 32: a convention, not a tuned value)")
    p.add_argument("--split", choices=["test", "train"], default="test")
    p.add_argument("--minibatch_size", type=int, default=100, metavar="B")
    p.add_argument("-d", "--device", type=int, default=-2)
    args = p.parse_args(argv)
    args.train_argv = train_argv
    for name, endings in (("scores", (".npz",)), ("out", (".npz",)), ("averages", (".npy", ".mrcs")), ("support", (".npy",))):
        path = vars(args)[name]
        if path is not None and os.path.splitext(path)[1] not in endings:
            p.error("--%s must end in %s (got %s)" % (name, " or ".join(endings), path))
    for name, lo, hi in (("neighbours", 1, MAX_NEIGHBOURS), ("minibatch_size", 1, 2 ** 31 - 1)):
        if not lo <= vars(args)[name] <= hi:
            p.error("--%s must be in [%d, %d] (got %d)" % (name, lo, hi, vars(args)[name]))
    if not args.stack_gib > 0:
        p.error("--stack_gib must be positive (got %r)" % args.stack_gib)
    if args.support is not None and args.averages is None:
        p.error("--support needs --averages")
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
    try:
        with np.load(args.scores, allow_pickle=False) as f:
            args.score_arrays = {k: f[k] for k in f.files if k == "meta" or k == "pose_refined" or
                                 k in ("theta_" + args.pose, "dx_" + args.pose, "z_" + args.latent)}
        args.score_meta = json.loads(str(args.score_arrays.pop("meta")))
    except Exception as e:
        p.error("--scores %s is not a score file of infer.py: %s" % (args.scores, e))
    for key in ("script", "split"):
        if args.score_meta.get(key) != vars(args)[key]:
            p.error("--scores %s was written for the %s %r, not %r" % (args.scores, key, args.score_meta.get(key), vars(args)[key]))
    if args.pose == "refined" and "pose_refined" not in args.score_arrays:
        p.error("--pose refined needs the pose_refined of infer.py --refine, and --scores %s has none" % args.scores)
    z = args.score_arrays.get("z_" + args.latent)
    if z is None or z.ndim != 2:
        p.error("--scores %s has no z_%s of shape (images, z_dim)" % (args.scores, args.latent))
    if z.shape[1] == 0:
        p.error("the model has z_dim = 0: there are no content latents to compare")
    return args


def check_request(args, facts):
    """The refusals (exit code 2) that need the split: made after the model is loaded, before anything is allocated.  Returns the
    (images, z_dim) latents of the score file."""
    z = args.score_arrays["z_" + args.latent]
    z_dim = facts.inf_dim - (1 if facts.rotate else 0) - (2 if facts.translate else 0)
    if z_dim == 0:
        _refuse("the model has z_dim = 0: there are no content latents to compare")
    if facts.images < 2:
        _refuse("the {} split has {} image: nothing can be a neighbour".format(facts.split, facts.images))
    if z.shape != (facts.images, z_dim):
        _refuse("--scores {}: z_{} has shape {}, the {} split and the model need {}".format(args.scores, args.latent, z.shape, facts.split,
                                                                                         (facts.images, z_dim)))
    if z_dim > 512:
        _refuse("z_dim = {} exceeds the 512 coordinates the search compares".format(z_dim))
    if args.averages is not None:
        if args.averages.endswith(".mrcs") and facts.channels != 1:
            _refuse("--averages {}: an MRC stack holds one channel, the images have {}".format(args.averages, facts.channels))
        need = facts.images * facts.n * facts.m * (4 * facts.channels + 1)
        if need > args.stack_gib * 2 ** 30:
            _refuse("the aligned stack of {} images needs {:.3f} GiB, --stack_gib allows {:g}".format(facts.images, need / 2.0 ** 30,
                                                                                                   args.stack_gib))
    return z


def search_lists(z, K, device):
    """The lists of all images: queries in blocks of QUERY_BLOCK against all candidates.  Returns the ops.NeighbourSearch."""
    import torch
    from . import ops
    latents = torch.from_numpy(np.ascontiguousarray(z)).to(device).to(torch.float64).contiguous()    # widened exactly
    images = latents.size(0)
    search = ops.NeighbourSearch(images, K, device)
    for lo in range(0, images, QUERY_BLOCK):
        search.update(latents[lo:lo + QUERY_BLOCK], lo, latents, 0)
    return search


def graph_arrays(args, d2, index):
    """found, in_degree, average_index and weight from the lists: torch on the device, plumbing rather than kernels."""
    import torch
    images, K = index.shape
    valid = index >= 0
    found = valid.sum(1)
    in_degree = torch.bincount(index[valid], minlength=images)
    own = torch.arange(images, dtype=torch.int64, device=index.device).unsqueeze(1)
    if args.exclude_self:
        own = torch.full_like(own, -1)
    average_index = torch.cat([own, index], 1).contiguous()
    weight = torch.ones(images, K + 1, dtype=torch.float64, device=index.device)
    if args.weights == "gaussian":
        finite = torch.where(valid, d2, torch.zeros_like(d2))
        s2 = finite.max(1, keepdim=True).values
        live = valid & (s2 > 0)
        weight[:, 1:] = torch.where(live, torch.exp(-finite / (2.0 * torch.where(s2 > 0, s2, torch.ones_like(s2)))),
                                    torch.ones_like(d2))
    return found, in_degree, average_index, weight


def neighbour_averages(args, facts, split, pose, average_index, weight):
    """The aligned stack of the whole split at the stored poses, then the gather over query minibatches.  Returns (average
    (images, N, C) float32, support (images, N) float64 or None): device tensors."""
    import torch
    from . import elbo as E
    from . import ops
    n, m, bs, device = facts.n, facts.m, args.minibatch_size, split.data.device
    images, N, C = facts.images, facts.n * facts.m, facts.channels
    pose_d = torch.from_numpy(pose).to(device)
    stack = torch.empty(images, N, C, dtype=torch.float32, device=device)
    cover = torch.empty(images, N, dtype=torch.uint8, device=device)
    for lo in range(0, images, bs):
        aligned, cv = E.align_at(split.data[lo:lo + bs], n, m, pose_d[lo:lo + bs], facts.rotate, facts.translate, args.interp)
        stack[lo:lo + bs] = aligned.reshape(-1, N, C)
        cover[lo:lo + bs] = 1 if cv is None else cv.reshape(-1, N)
    average = torch.empty(images, N, C, dtype=torch.float32, device=device)
    support = torch.empty(images, N, dtype=torch.float64, device=device) if args.support is not None else None
    for lo in range(0, images, bs):
        out = ops.neighbour_average(stack, cover, average_index[lo:lo + bs], weight[lo:lo + bs], support=support is not None)
        if support is not None:
            average[lo:lo + bs], support[lo:lo + bs] = out
        else:
            average[lo:lo + bs] = out
    return average, support


def neighbour_main(args, parser_fn, build, positional=()):
    """neighbours.py after its own parsing; parser_fn, build and positional as for infer.infer_main."""
    from . import infer
    model = infer.load_model(args, parser_fn, build, positional)
    facts = infer.split_facts(args, model)
    pose = stored_poses(args, facts, _refuse)
    z = check_request(args, facts)
    search = search_lists(z, args.neighbours, model.device)
    d2, index = search.lists()
    found, in_degree, average_index, weight = graph_arrays(args, d2, index)
    average = support = None
    if args.averages is not None:
        split = infer.upload_split(model.cfg, args.split, model.device)
        average, support = neighbour_averages(args, facts, split, pose, average_index, weight)
    meta = {k: vars(args)[k] for k in ("script", "state", "generator", "inference", "scores", "split", "averages", "support",
                                       "neighbours", "latent", "pose", "interp", "weights", "exclude_self", "stack_gib")}
    meta.update(scores_state=args.score_meta.get("state"), images=facts.images, z_dim=int(z.shape[1]))
    arrays = {"index": index, "sqdist": d2, "found": found, "in_degree": in_degree, "average_index": average_index, "weight": weight}
    arrays = {k: v.cpu().numpy() for k, v in arrays.items()}            # the one transfer, after the last launch
    arrays.update(pose=pose, meta=np.array(json.dumps(meta)))
    if average is not None:
        infer.write_stack(args.averages, average.cpu().numpy().reshape(facts.images, facts.n, facts.m, facts.channels))
    if support is not None:
        host = support.cpu().numpy().reshape(facts.images, facts.n, facts.m)
        infer.write_atomically(args.support, lambda f: np.save(f, host))
    infer.write_npz(args.out, arrays)
    print("neighbours.py: %d images, %d neighbours each (%d lists not full), z_dim %d; in-degree 0 for %d images, at most %d; "
          "median distance to the last neighbour %.4g" % (facts.images, args.neighbours, int((arrays["found"] < args.neighbours).sum()),
                                                          z.shape[1], int((arrays["in_degree"] == 0).sum()), int(arrays["in_degree"].max()),
                                                          _median_last(arrays)))
    return 0


def _median_last(arrays):
    """The median, over the images with a neighbour, of the distance to the last listed one."""
    d2, found = arrays["sqdist"], arrays["found"]
    has = found > 0
    if not has.any():
        return float("nan")
    return float(np.median(np.sqrt(d2[has, found[has] - 1])))
