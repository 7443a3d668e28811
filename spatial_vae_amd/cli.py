"""Shared machinery of the three training command lines (train_mnist.py, train_galaxy.py,
train_particles.py at the repository root).

The reference triplicates its loop per script (train_mnist.py:127-226 and 268-469, train_galaxy.py:186-294
and 346-575, train_particles.py:151-245 and 272-547); here ONE loop serves all three.  Each script declares
only the reference's flag surface (underscores for mnist/galaxy, hyphens for particles); the options this build adds are
declared once, in add_shared_options, and what the loop does differently per script is one record in SCRIPTS.  Kept:
flag names and defaults, the step order (loss = -elbo; backward; step; zero_grad), the running-mean metric
arithmetic, the stdout tables, train.txt / val.txt / command.txt / models.txt, and the whole-module
`.sav` checkpoints with the reference's file names.  Dropped (out of scope): the
interactive "clear outputs?" prompt (the run directory is created, never wiped), the loss-curve SVG, the zip
archive and dataset download.  `--augment_rotation` runs on the device
(ops.rotate_augment, bit-identical to the reference's per-image Pillow loop).  Added: `--synthetic N`
(train on N synthetic images when no data files exist), data-parallel execution under torchrun, and
`--progress_every` (the reference pays three .item() syncs per step for its progress line), and `--num_samples K` /
`--eval_num_samples K` (the K-sample importance-weighted bound for the training / validation passes; 1 = the reference).
"""
import collections
import copy
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

from . import dp
from . import elbo as E
from . import ops


class RunningMean(object):
    """acc += b * (v - acc) / count  (train_mnist.py:156-164) in Python doubles, exactly as the reference does it -- but
    LAZILY: update() only keeps the minibatch's (elbo, log_p, kl) device vector, and values() fetches everything collected so far
    in one transfer and replays the arithmetic on the host.  No kernel and no synchronisation per step (the reference pays
    three .item() calls per step; a device-side accumulator paid five tiny kernels).  The reference logs -log_p ("gen_loss");
    negation commutes with this arithmetic bit for bit, so the sign is applied when the values are read."""

    def __init__(self, device=None, n=3):
        self.acc = [0.0] * n
        self.count = 0          # images whose metrics have been folded into acc
        self.seen = 0           # images handed to update() so far
        self.pending = []

    def update(self, batch_size, vec, volatile=False):
        """vec: the minibatch's 3-vector on the device.  volatile=True: the tensor will be overwritten by the next step (the
        data-parallel metric tail), so a copy is kept."""
        self.seen += batch_size
        self.pending.append((batch_size, vec.detach().clone() if volatile else vec.detach()))

    def _flush(self):
        if not self.pending:
            return
        host = torch.stack([v.reshape(-1) for _, v in self.pending]).cpu().double().tolist()   # the one synchronisation
        for (b, _), row in zip(self.pending, host):
            self.count += b
            self.acc = [a + b * (v - a) / self.count for a, v in zip(self.acc, row)]
        self.pending = []

    def values(self):
        self._flush()
        e, lp, k = self.acc
        return [e, -lp, k]


def coord_grid(n_rows, n_cols):
    """(N, 2) grid of train_mnist.py:315-320."""
    x0, x1 = np.meshgrid(np.linspace(-1, 1, n_cols), np.linspace(1, -1, n_rows))
    return torch.from_numpy(np.stack([x0.ravel(), x1.ravel()], 1)).float()


def loader_order(n, shuffle):
    """Index order of one pass over torch.utils.data.DataLoader(dataset, batch_size, shuffle=shuffle) as the reference makes it
    (train_mnist.py:395-396, :138, :196), consuming torch's global CPU generator the way iter(DataLoader) does: the iterator
    draws one int64 (its worker base seed) whether or not the loader shuffles; RandomSampler then draws a second int64, seeds a
    private generator with it and takes torch.randperm(n) from that one."""
    torch.empty((), dtype=torch.int64).random_()
    if not shuffle:
        return torch.arange(n)
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


def pass_noise(sizes, inf_dim, device, after_first=(), num_samples=1):
    """The N(0,1) draws of one pass over minibatches of `sizes` images, from torch's global CPU generator in the reference's
    order and shapes: one x.data.new(B, inf_dim).normal_() per minibatch (train_mnist.py:38; CPU tensors in the CPU reference),
    and -- on a pass that dumps images -- the display helpers' draws right after the first minibatch's (`after_first`: their
    shapes; train_mnist.py:107, train_galaxy.py:146, :177).  The shapes matter: the CPU normal_ kernel fills in blocks of 16 and
    re-draws the tail, so one big draw is not the concatenation of the small ones.  Returns (per-minibatch device tensors,
    display draws on the device); everything is uploaded in ONE transfer, nothing is drawn or copied inside the step loop.
    num_samples=K: ONE (b*K, inf_dim) draw per minibatch (row i*K + k = sample k of image i), so K = 1 consumes the generator
    exactly as before; the display helpers stay single-sample."""
    draws, extra = [], []
    for i, b in enumerate(sizes):
        draws.append(torch.empty(b * num_samples, inf_dim).normal_())
        if i == 0:
            extra = [torch.empty(*shape).normal_() for shape in after_first]
    flat = torch.cat([t.reshape(-1) for t in draws + extra]) if draws else torch.empty(0)
    flat = flat.to(device, non_blocking=True)
    out, off = [], 0
    for t in draws + extra:
        out.append(flat[off:off + t.numel()].view(t.shape))
        off += t.numel()
    return out[:len(draws)], out[len(draws):]


def train_pass_plan(N, bs, inf_dim, device, home=None, num_samples=1):
    """(index minibatches, their noise) of one training pass: iter(DataLoader(shuffle=True)) then one draw per minibatch
    (train_mnist.py:138-143 via :38).  The last minibatch is ragged, as the reference's loader keeps it (no drop_last)."""
    perm = loader_order(N, True)
    batches = [perm[i:i + bs].to(home if home is not None else device) for i in range(0, N, bs)]
    noise, _ = pass_noise([b.numel() for b in batches], inf_dim, device, num_samples=num_samples)
    return batches, noise


def eval_pass_plan(ntest, bs, inf_dim, device, home=None, display_shapes=(), num_samples=1):
    """(index minibatches, their noise, the display helpers' noise) of one evaluation pass over the un-shuffled validation
    loader (train_mnist.py:196-201); on a dump epoch eval_model decodes the first minibatch again for the PNG files
    (train_mnist.py:214-224, train_galaxy.py:275-292) -- `display_shapes` maps a minibatch size to those draws' shapes."""
    order = loader_order(ntest, False)
    tb = [order[i:i + bs].to(home if home is not None else device) for i in range(0, ntest, bs)]
    shapes = display_shapes(tb[0].numel()) if (display_shapes and tb) else ()
    noise, shown = pass_noise([b.numel() for b in tb], inf_dim, device, after_first=shapes, num_samples=num_samples)
    return tb, noise, shown


# What the one loop does differently for each of the three scripts; train_main(script, ...) looks its record up by name.
Script = collections.namedtuple("Script", [
    "eval_fn",              # name of the elbo.eval_minibatch_* function (looked up on the module when train_main runs)
    "mask_ctf",             # minibatches are (y, mask, ctf), not (y,)
    "z_schedule",           # z_scale = 0 for the first --z_delay epochs, 1 after them
    "augment",              # --augment_rotation applies (to training steps)
    "run_dir",              # owns outputs_<prefix>/: command.txt, models.txt, train.txt / val.txt, the sample PNG (and the
                            # loader draw in front of it), the final .sav files under trained/
    "dumps",                # PNGs of a save-interval epoch besides the reconstruction: "dis" draws (B, inf_dim), "rnd" (B, z_dim)
    "split_rows",           # table: two 1-based `Epoch / Split` rows per epoch, not a 0-based training and a validation line
    "prefix_required",      # --save_prefix is mandatory
    "save_interval_free",   # a resumed run may change --save_interval (it draws nothing: no image dump)
    "activations",          # (--activation names -> module class, the class of every other name)
])
SCRIPTS = {
    # 'relu' means LeakyReLU in mnist/particles (train_mnist.py:344-348, train_particles.py:433-436) but nn.ReLU in galaxy,
    # where 'leakyrelu' is mis-spelt in the reference and silently gives Tanh (train_galaxy.py:426-434)
    "mnist": Script(eval_fn="eval_minibatch_mnist", mask_ctf=False, z_schedule=False, augment=False, run_dir=True,
                    dumps=("dis",), split_rows=False, prefix_required=True, save_interval_free=False,
                    activations=({"tanh": nn.Tanh}, nn.LeakyReLU)),
    "galaxy": Script(eval_fn="eval_minibatch_galaxy", mask_ctf=False, z_schedule=True, augment=True, run_dir=True,
                     dumps=("dis", "rnd"), split_rows=False, prefix_required=True, save_interval_free=False,
                     activations=({"tanh": nn.Tanh, "relu": nn.ReLU, "sigmoid": nn.Sigmoid}, nn.Tanh)),
    "particles": Script(eval_fn="eval_minibatch_particles", mask_ctf=True, z_schedule=True, augment=True, run_dir=False,
                        dumps=(), split_rows=True, prefix_required=False, save_interval_free=True,
                        activations=({"tanh": nn.Tanh}, nn.LeakyReLU)),
}


def activation_class(script, name):
    """The scripts' (inconsistent) flag-to-module maps."""
    named, other = SCRIPTS[script].activations
    return named.get(name, other)


def add_shared_options(p, sep, synthetic_help):
    """The options this build adds to the reference's flag surfaces, the same for the three scripts up to the separator inside
    their names (`sep`: "_" for mnist and galaxy, "-" for particles) and the --synthetic help text."""
    def o(name):
        return "--" + name.replace("_", sep)

    p.add_argument("--synthetic", type=int, default=0, help=synthetic_help)
    p.add_argument(o("progress_every"), type=int, default=50, help="stderr progress line every N steps (0 = never)")
    p.add_argument("--seed", type=int, default=None,
                   help="seed torch and numpy before the networks are built (the reference has no such flag: unseeded by default)")
    p.add_argument("--gemm", choices=["fp32", "fp16x3"], default=None,
                   help="hidden-layer GEMM path (default: SVAE_GEMM or fp32 MFMA; fp16x3 = fp32-accurate split-operand f16 MFMA)")
    p.add_argument("--resume", default=None, metavar="PATH",
                   help="continue from this training state file (written by {}) with the same arguments; only {} "
                        "may grow.  Under the world size that wrote it the run continues bit for bit; another world size is "
                        "accepted but changes the summation order, as it does for a fresh run".format(
                            o("checkpoint_interval"), o("num_epochs")))
    p.add_argument(o("checkpoint_interval"), type=int, default=0, metavar="N",
                   help="write <prefix>_state_epoch<NN>.ckpt (parameters, Adam moments, step count, generator states, table rows) "
                        "beside the .sav files after every N-th epoch and after the last one (0 = never)")
    p.add_argument(o("clip_grad_norm"), type=float, default=None, metavar="X",
                   help="clip the global L2 norm of the gradient at X before every Adam update (the arithmetic of "
                        "torch.nn.utils.clip_grad_norm_, on the device; default: off -- the reference does not clip)")
    p.add_argument(o("skip_nonfinite"), action="store_true",
                   help="skip the Adam update of a step whose gradient norm is NaN or inf: parameters, moments and the step count "
                        "stay as they are (default: off -- the reference applies it)")
    p.add_argument(o("num_samples"), type=int, default=1, metavar="K",
                   help="train on the K-sample importance-weighted bound log((1/K) sum_k p(x|z_k) p(z_k) / q(z_k|x)) instead of "
                        "the one-sample ELBO (1 <= K <= 1024; default 1 = the reference's objective).  For K >= 2 the table's "
                        "columns are the bound, the mean log p(x|z) and a Monte-Carlo estimate of the KL: the first is no "
                        "longer the second minus the third")
    p.add_argument(o("eval_num_samples"), type=int, default=None, metavar="K",
                   help="samples per image in the validation passes (default: the value of {}); train with a small K, "
                        "compare models with a large one".format(o("num_samples")))


def finish_options(p, args):
    """--eval_num_samples defaults to --num_samples; both are sample counts the kernels take."""
    if args.eval_num_samples is None:
        args.eval_num_samples = args.num_samples
    for name in ("num_samples", "eval_num_samples"):
        if not 1 <= getattr(args, name) <= 1024:
            p.error("%s must be in [1, 1024]" % name)
    return args


def pick_device(d, world=1, local=0):
    """-d/--device: -1 = CPU, >= 0 = that GPU, -2 (default) = GPU if there is one (train_mnist.py:323-327).
    The MI355X decoder has no CPU path, so a CPU request is refused up front.  Under data-parallel execution the
    device is the rank's local one (dp.init_process_group: LOCAL_RANK, or 0 for every rank in the shared-GPU rehearsal)."""
    if d == -1 or not torch.cuda.is_available():
        raise SystemExit("spatial_vae_amd: the decoder runs on an MI355X only (-d -1 / no GPU is not supported)")
    idx = d if d >= 0 else local
    if world > 1:
        idx = local
    torch.cuda.set_device(idx)
    return torch.device("cuda", idx)


def make_run_dir(prefix, args):
    out = "outputs_{}".format(prefix)
    trained = os.path.join(out, "trained")
    os.makedirs(trained, exist_ok=True)
    os.makedirs(os.path.join(out, "images"), exist_ok=True)
    with open(os.path.join(out, "command.txt"), "w") as f:
        for k, v in sorted(vars(args).items()):
            print("{}: {}".format(k, v), file=f)
    return out, trained


def save_label(args):
    """src/misc_tools.py:15-28: '<prefix>_' + z<z_dim>pnl<p_num_layers>qnl<q_num_layers>nl<num_layers>ep<num_epochs> in
    the order the flags were declared."""
    names = {"z_dim": "z", "p_num_layers": "pnl", "q_num_layers": "qnl", "num_layers": "nl", "num_epochs": "ep"}
    label = args.save_prefix + "_"
    for k, v in vars(args).items():
        if k in names:
            label += names[k] + str(v)
    return label


def image_grid(images, nrow, padding=3, pad_value=0.5):
    """torchvision.utils.make_grid + the uint8 conversion of save_image (torchvision 0.8.2 is what the reference pins;
    it is not installed here, so this follows its published algorithm -- parity unpinned): images (B, C, h, w) in [0, 1]
    -> (H, W, 3) uint8.  Single-channel batches are replicated to RGB; cells are h+padding x w+padding on a
    pad_value canvas; value*255 + 0.5, clamped, truncated."""
    t = np.asarray(images, np.float32)
    if t.shape[1] == 1:
        t = np.repeat(t, 3, axis=1)
    B, C, h, w = t.shape
    if B == 1:
        grid = t[0]
    else:
        xmaps = min(nrow, B)
        ymaps = int(math.ceil(float(B) / xmaps))
        H, W = h + padding, w + padding
        grid = np.full((C, H * ymaps + padding, W * xmaps + padding), pad_value, np.float32)
        for k in range(B):
            r, c = divmod(k, xmaps)
            grid[:, r * H + padding:r * H + padding + h, c * W + padding:c * W + padding + w] = t[k]
    arr = np.clip(grid * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)
    return np.transpose(arr, (1, 2, 0))


def export_batch_as_image(data, output, image_dims):
    """src/misc_tools.py:30-39: a (B, N[, C]) batch as one PNG, int(sqrt(B)) images per row."""
    from PIL import Image
    B = data.size(0)
    images = data.detach().float().reshape(B, image_dims[0], image_dims[1], -1).permute(0, 3, 1, 2).cpu().numpy()
    Image.fromarray(image_grid(images, int(B ** 0.5))).save(output)


def save_models(path_prefix, epoch_str, p_net, q_net, device=None):
    """torch.save(<whole module>) under the reference's names (src/misc_tools.py:88-104).  The reference moves the live
    module (net.eval().cpu(), save, net.cuda()); here a detached CPU COPY is saved instead: the live parameters are
    views into dp.TrainStep's flat buffers, and a Module._apply round trip would re-allocate them -- the optimiser
    would keep stepping the orphaned flat buffer while the forward pass read stale module tensors."""
    for tag, net in (("generator", p_net), ("inference", q_net)):
        snapshot = copy.deepcopy(net).eval().cpu()      # the classes' __getstate__ leaves the gradient sinks out of the copy
        torch.save(snapshot, "{}_{}_epoch{}.sav".format(path_prefix, tag, epoch_str))


# ---- full training checkpoints (--checkpoint_interval / --resume) ---------------------------------------------------------
CHECKPOINT_VERSION = 1

# Arguments a resumed run may change: where it writes, where it runs, how long it goes on and what it reports.  Every other
# stored argument shapes the model, the data or the order in which random numbers are consumed (--save_interval too, for mnist
# and galaxy: a dump epoch draws the display helpers' noise) and must equal the stored value.
RESUME_FREE_ARGS = {"num_epochs", "save_prefix", "device", "progress_every", "resume", "checkpoint_interval", "no_preload",
                    "train_path", "test_path", "logging_level"}
# Arguments added after state files were first written, with the value that reproduces the run of a file that lacks them.
RESUME_ARG_DEFAULTS = {"clip_grad_norm": None, "skip_nonfinite": False, "num_samples": 1, "eval_num_samples": 1}


class CheckpointError(SystemExit):
    """A state file that cannot be read or does not belong to this run: the command line ends with the message."""


def rng_state():
    """The two host generators all randomness of a run is consumed from, as tensors and numbers (np.random.get_state() is a
    tuple holding an ndarray: stored as such it would need a full unpickler)."""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"torch": torch.get_rng_state().clone(), "numpy_kind": str(kind),
            "numpy_keys": torch.from_numpy(np.asarray(keys, np.uint32).astype(np.int64)), "numpy_pos": int(pos),
            "numpy_has_gauss": int(has_gauss), "numpy_cached_gaussian": float(cached)}


def set_rng_state(state):
    torch.set_rng_state(state["torch"])
    np.random.set_state((state["numpy_kind"], state["numpy_keys"].numpy().astype(np.uint32), int(state["numpy_pos"]),
                         int(state["numpy_has_gauss"]), float(state["numpy_cached_gaussian"])))


def plain_args(args):
    """vars(args) with values a weights-only load gives back unchanged."""
    out = {}
    for k, v in vars(args).items():
        out[k] = v if isinstance(v, (bool, int, float, str, type(None))) else str(v)
    return out


def dataset_sums(y_train, y_test):
    """The float64 sums by which data-parallel ranks check that they hold one dataset, and a resumed run that it holds the
    stored run's."""
    return torch.stack([y_train.double().sum(), y_test.double().sum()])


def dataset_fingerprint(y_train, y_test, sums=None):
    """dataset_sums (`sums`, where the caller has formed them already) plus the shapes."""
    sums = dataset_sums(y_train, y_test) if sums is None else sums
    return {"sums": sums.cpu(), "train_shape": [int(d) for d in y_train.shape], "test_shape": [int(d) for d in y_test.shape]}


def checkpoint_path(path_prefix, epoch_str):
    return "{}_state_epoch{}.ckpt".format(path_prefix, epoch_str)


def write_checkpoint(path, train_state, completed, args, world, fingerprint, lines):
    """One torch.save of a dict that torch.load(weights_only=True) reads.  Written under a temporary name in the same
    directory and renamed over `path`, so an interrupted write never leaves a file with the final name (and never damages the
    previous one).  Draws no random number: the generator states stored are the caller's states at this moment."""
    payload = {"version": CHECKPOINT_VERSION, "completed": int(completed), "train_step": train_state, "rng": rng_state(),
               "args": plain_args(args) if not isinstance(args, dict) else dict(args), "world": int(world),
               "fingerprint": fingerprint, "lines": {k: list(v) for k, v in lines.items()}}
    tmp = "{}.tmp{}".format(path, os.getpid())
    try:
        torch.save(payload, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


def read_checkpoint(path):
    """The dict of write_checkpoint, read with the weights-only unpickler on the CPU.  Anything that is not such a file --
    missing, truncated, another format -- ends in one CheckpointError naming the path."""
    try:
        ck = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise CheckpointError("--resume: cannot read the state file {}: {}: {}".format(
            path, type(e).__name__, str(e).splitlines()[0] if str(e) else "")) from None
    if not isinstance(ck, dict) or "version" not in ck:
        raise CheckpointError("--resume: {} is not a training state file (no version field)".format(path))
    if ck["version"] != CHECKPOINT_VERSION:
        raise CheckpointError("--resume: {}: format version {} (this build reads version {})".format(
            path, ck["version"], CHECKPOINT_VERSION))
    missing = [k for k in ("completed", "train_step", "rng", "args", "world", "fingerprint", "lines") if k not in ck]
    if missing:
        raise CheckpointError("--resume: {}: fields missing: {}".format(path, ", ".join(missing)))
    return ck


def check_resume_args(ck, args, script):
    """Refuse a state file whose run differs from this command line in anything that changes the model or the trajectory, and
    one that has nothing left to do.  Every rank reads the same file and the same arguments, so all refuse alike."""
    now = plain_args(args)
    free = set(RESUME_FREE_ARGS)
    if SCRIPTS[script].save_interval_free:
        free.add("save_interval")           # no images are dumped: the interval only decides when .sav files are written
    # a file written before the gradient guard / the sample counts existed: both guard options off, one sample per image
    stored = dict(RESUME_ARG_DEFAULTS, **ck["args"])
    now = dict(RESUME_ARG_DEFAULTS, **now)
    for k in sorted(set(stored) | set(now)):
        if k in free:
            continue
        if k not in stored or k not in now or stored[k] != now[k]:
            raise CheckpointError("--resume: argument {} is {!r} now but the state file was written with {!r}".format(
                k, now.get(k, "<absent>"), stored.get(k, "<absent>")))
    if ck["completed"] >= args.num_epochs:
        raise CheckpointError("--resume: completed epochs {} >= num_epochs {}: nothing left to run (give a larger "
                              "num_epochs to extend the run)".format(ck["completed"], args.num_epochs))


def check_resume_fingerprint(ck, fingerprint):
    """The sums are float64 sums of fp32 values: two evaluations over the same data agree to ~1e-16 times sqrt(count) whatever
    the summation order (host or device, any thread count), two datasets do not.  1e-12 relative separates them."""
    have = ck["fingerprint"]
    for k in ("train_shape", "test_shape"):
        if list(have[k]) != list(fingerprint[k]):
            raise CheckpointError("--resume: dataset fingerprint differs: {} is {} now, {} in the state file".format(
                k, fingerprint[k], list(have[k])))
    a, b = have["sums"].double(), fingerprint["sums"].double()
    if not bool(((a - b).abs() <= 1e-12 * b.abs().clamp_min(1.0)).all()):
        raise CheckpointError("--resume: dataset fingerprint differs: sums are {} now, {} in the state file".format(
            b.tolist(), a.tolist()))


def _take(t, sel, device):
    """Rows `sel` of a dataset tensor on `device`: a gather in HBM when the dataset is resident there (the default, as the
    reference preloads: train_mnist.py:329-332), a host gather + one asynchronous upload under --no-preload."""
    if t.device == device:
        return t[sel.to(device)]
    rows = t[sel.cpu()]
    return (rows.pin_memory() if device.type == "cuda" else rows).to(device, non_blocking=True)


def run_epoch(script, step, x, batches, train, *, data, inf_dim, noise=None, mask=None, kw=None, train_kw=None, dump=None,
              num_samples=1, epoch=0, num_epochs=1, rank=0, world=1, progress_every=0):
    """One pass over `batches` (a list of index tensors into the resident data; every rank holds the same list).
    Training uses dp.TrainStep (forward, backward, all-reduce, Adam); evaluation only the forward (it is stochastic in
    the reference too: eval_model draws noise, train_mnist.py:174-226).

    data: {"y": images, "ctf": filters or None}, indexed by `batches`; mask: the particles' pixel mask.  noise: one prepared
    (gb*K, inf_dim) draw per minibatch (pass_noise), else each is drawn here.  kw: keywords of every eval_minibatch call of
    the pass (z_scale); train_kw: those of training steps only (augment_rotation).  dump(y, y_hat): called on rank 0 with the
    first minibatch (the image files of a save-interval epoch).  epoch, num_epochs, progress_every: the progress line only.

    Data parallel: rank g works on rows [lo, hi) of each GLOBAL minibatch.  The N(0,1) draw is made for the whole
    global minibatch from the generator every rank seeded identically and sliced like the data, and
    so are the augmentation angles, so a G-rank step computes what the 1-rank step computes (up to fp32 summation
    order).  Training metrics come back inside the gradient all-reduce (step.metrics); evaluation metrics are
    collected per batch and all-reduced ONCE per epoch.  A rank with an empty slice (ragged last batch smaller than the
    world) contributes zeros.

    num_samples = K >= 2: the pass evaluates the K-sample importance-weighted bound.  Shards stay by image; the
    noise of a global minibatch is (gb*K, inf_dim) and rank g takes rows [lo*K, hi*K)."""
    rule = SCRIPTS[script]
    p_net, q_net = step.p_net, step.q_net
    K = int(num_samples)
    p_net.train(train)
    q_net.train(train)
    mean = RunningMean()
    total = sum(idx.numel() for idx in batches)     # images of the pass, for the progress line
    pending = []
    for it, idx in enumerate(batches):
        gb = idx.numel()
        lo, hi = dp.shard_bounds(gb, rank, world)
        sel = idx[lo:hi]
        y = _take(data["y"], sel, x.device)
        args = (y,)
        if rule.mask_ctf:
            ctf = _take(data["ctf"], sel, x.device) if data.get("ctf") is not None else None
            args = (y, mask, ctf)
        call_kw = dict(kw or {})
        if noise is not None:
            r = noise[it]
        else:       # no prepared draws: the reference's per-minibatch draw from the global CPU generator (train_mnist.py:38)
            r = torch.empty(gb * K, inf_dim).normal_().to(x.device, non_blocking=True)
        call_kw["noise"] = r[lo * K:hi * K]
        if K > 1:
            call_kw["num_samples"] = K
        out = None
        if train:
            call_kw.update(train_kw or {})              # augmentation applies to training steps only (train_galaxy.py:204)
            if world > 1 and call_kw.get("augment_rotation") and step.eval_kwargs.get("rotate"):
                call_kw["offset"] = E.draw_offsets(step.eval_kwargs["rotate"], gb)[lo:hi]   # np.random is seeded alike on all ranks
            out = step(x, *args, weight=(hi - lo) / gb, global_batch=gb, **call_kw)
            # the data-parallel metric tail (also the one-rank RCCL rehearsal, and any weight != 1) is overwritten by the
            # next step: keep a copy of it, not a reference
            mean.update(gb, step.metrics, volatile=step.metrics is step.grads.tail)
        else:
            vals = torch.zeros(3, device=x.device)
            if hi > lo:
                with torch.no_grad():
                    out = step.eval_minibatch(x, *args, p_net, q_net, **dict(step.eval_kwargs, **call_kw))
                vals = dp.metric_vector(out)
            if world > 1:
                pending.append((gb, vals * ((hi - lo) / gb)))
            else:
                mean.update(gb, vals)
        if it == 0 and dump and rank == 0 and out is not None:   # first batch of a save-interval epoch (train_mnist.py:214-224)
            # the posed reconstruction shown is each image's first sample
            dump(y, (out[3] if K == 1 else out[3][::K]) if len(out) > 3 else None)
        if train and rank == 0 and progress_every > 0 and (it + 1) % progress_every == 0:
            e, g, k = mean.values()
            print("# [{}/{}] training {:.1%}, ELBO={:.5f}, Error={:.5f}, KL={:.5f}".format(
                epoch + 1, num_epochs, mean.seen / total, e, g, k), end="\r", file=sys.stderr)
    if pending:
        allv = torch.stack([v for _, v in pending])
        torch.distributed.all_reduce(allv)
        for (gb, _), v in zip(pending, allv):
            mean.update(gb, v)
    if train and rank == 0 and progress_every > 0:
        print(" " * 80, end="\r", file=sys.stderr)
    return mean.values()


def train_main(script, args, build):
    """`build(args, device)` returns dict(y_train, y_test, ctf_train, ctf_test, mask, n, m, channels,
    p_net, q_net, rotate, translate, table)."""
    rule = SCRIPTS[script]
    rank, world, local = dp.init_process_group(device_is_gpu=True)
    device = pick_device(args.device, world, local)
    # --resume: every rank opens the file itself and checks it against its own (identical) arguments before the first
    # collective, so a rank that cannot read it -- or a run that does not match -- ends here and not inside a broadcast
    resume = None
    if args.resume:
        resume = read_checkpoint(args.resume)
        check_resume_args(resume, args, script)
    ckpt_every = args.checkpoint_interval
    if ckpt_every < 0:
        raise SystemExit("the checkpoint interval must be >= 0")
    if ckpt_every and not rule.prefix_required and args.save_prefix is None:
        raise SystemExit("--checkpoint-interval needs --save-prefix (the state files are written beside the .sav files)")
    clip = args.clip_grad_norm
    if clip is not None and not clip > 0:
        raise SystemExit("the gradient-norm threshold must be > 0")
    train_k, eval_k = args.num_samples, args.eval_num_samples
    # Randomness is consumed from torch's GLOBAL CPU generator and np.random in the order the reference's main() consumes
    # them: default initialisation of p_net then q_net, one draw for the sample-image pass over the validation
    # loader, then per epoch the two draws of iter(DataLoader(shuffle=True)), one N(0,1) draw per training minibatch, one draw
    # for the validation loader and one N(0,1) draw per validation minibatch (plus the display helpers' on dump epochs).  So
    # torch.manual_seed(s) in front of this function -- or --seed s, an addition: the reference has no such flag -- follows the
    # trajectory of the reference's CPU path under the same seed.  Under data-parallel execution every rank seeds alike
    # (--seed, else rank 0's seed), makes the same draws and slices [lo:hi) of each global minibatch; np.random (the dataset
    # shuffle of train_galaxy.py:372 inside build(), the augmentation angles) is seeded alike too.
    seed = args.seed
    if seed is None and world > 1:
        seed = dp.shared_seed(device)
    if seed is not None:
        torch.manual_seed(seed)
        np.random.seed(seed % (2 ** 32))
    if args.gemm:                                   # before the first decoder call: buffer sizes depend on the mode
        from . import _lib
        _lib.set_gemm_mode(args.gemm)
    start = time.time()
    prefix = args.save_prefix
    out_dir = trained = None
    if rule.prefix_required and prefix is None:
        raise SystemExit("--save_prefix is required (the reference crashes without it: src/misc_tools.py:22)")
    if rule.run_dir and rank == 0:
        out_dir, trained = make_run_dir(prefix, args)
    cfg = build(args, device)
    p_net, q_net = cfg["p_net"].to(device), cfg["q_net"].to(device)
    if rank == 0 and out_dir:
        with open(os.path.join(out_dir, "models.txt"), "w") as f:
            print(p_net, file=f)
            print(q_net, file=f)
    x = coord_grid(cfg["n"], cfg["m"]).to(device)
    # the dataset is resident in HBM (the reference preloads it too: train_mnist.py:329-332) unless --no-preload
    # (train_particles.py:317, :405-413) keeps it in host memory, from where each minibatch is gathered and uploaded
    home = torch.device("cpu") if getattr(args, "no_preload", False) else device
    tr = {"y": cfg["y_train"].to(home), "ctf": None if cfg.get("ctf_train") is None else cfg["ctf_train"].to(home)}
    te = {"y": cfg["y_test"].to(home), "ctf": None if cfg.get("ctf_test") is None else cfg["ctf_test"].to(home)}
    mask = cfg.get("mask")
    mask = mask.to(device) if mask is not None else None
    N = tr["y"].size(0)
    sums = fingerprint = None
    if resume is not None or ckpt_every or world > 1:
        sums = dataset_sums(tr["y"], te["y"])
    if resume is not None or ckpt_every:
        fingerprint = dataset_fingerprint(tr["y"], te["y"], sums)
        if resume is not None:
            check_resume_fingerprint(resume, fingerprint)
    step = dp.TrainStep(p_net, q_net, getattr(E, rule.eval_fn), lr=args.learning_rate, rotate=cfg["rotate"],
                        translate=cfg["translate"], dx_scale=args.dx_scale, theta_prior=args.theta_prior, clip_grad_norm=clip,
                        skip_nonfinite=args.skip_nonfinite)
    print("# using priors: theta={}, dx={}".format(args.theta_prior, args.dx_scale), file=sys.stderr)
    num_epochs = args.num_epochs
    digits = int(math.log10(num_epochs)) + 1
    bs = args.minibatch_size
    if world > 1:       # every rank must hold the SAME dataset: the ranks slice one global minibatch by index
        dp.assert_same_on_all_ranks(sums.to(device), "the dataset")
    inf_dim = q_net.latent_dim
    out = sys.stdout
    header = cfg["table"]
    if rank == 0:
        print("\t".join(header), file=out)
    train_lines, val_lines = ["\t".join(header)], ["\t".join(header)]
    z_delay = getattr(args, "z_delay", 0)               # mnist has no such option
    label = save_label(args) if out_dir else None
    ntest = te["y"].size(0)
    if rule.run_dir:                                                 # MiscTools.sample_images: one pass is started over the
        loader_order(ntest, False)                                   # validation loader (train_mnist.py:402) -> one draw
        if out_dir:
            export_batch_as_image(te["y"][:bs], "{}/images/_sample_{}.png".format(out_dir, label), [cfg["n"], cfg["m"]])
    first_epoch = 0
    rows = []                                                        # particles: the table rows printed so far
    if resume is not None:
        # the networks were built and the pre-loop draws made exactly as a fresh run makes them; now the trained state
        # replaces the initial one and -- last, immediately before the first resumed epoch -- the two generators continue
        # where the stored run's were after its last evaluation pass
        step.load_state_dict(resume["train_step"])
        first_epoch = int(resume["completed"])
        stored = resume["lines"]
        train_lines = list(stored.get("train_lines", train_lines))
        val_lines = list(stored.get("val_lines", val_lines))
        rows = list(stored.get("rows", rows))
        if rank == 0:
            print("# resuming {} after epoch {} of {} (written under {} rank(s), now {})".format(
                args.resume, first_epoch, num_epochs, resume["world"], world), file=sys.stderr)
        set_rng_state(resume["rng"])
    state_prefix = None
    if ckpt_every and rank == 0:
        state_prefix = os.path.join(trained, prefix) if rule.run_dir else prefix
    for epoch in range(first_epoch, num_epochs):
        kw = {"z_scale": 0 if epoch < z_delay else 1} if rule.z_schedule else {}
        batches, noise = train_pass_plan(N, bs, inf_dim, device, home, train_k)    # same order and draws on every rank
        train_kw = {"augment_rotation": True} if cfg.get("augment") and rule.augment else {}
        t_epoch = time.time()
        e, g, k = run_epoch(script, step, x, batches, True, data=tr, inf_dim=inf_dim, noise=noise, mask=mask, kw=kw,
                            train_kw=train_kw, num_samples=train_k, epoch=epoch, num_epochs=num_epochs, rank=rank, world=world,
                            progress_every=args.progress_every)
        if rank == 0:       # run_epoch's values() synchronised: the epoch's training pass is complete
            print("# epoch {}: {} training images in {:.3f} s = {:.0f} images/s".format(
                epoch + 1, N, time.time() - t_epoch, N / max(time.time() - t_epoch, 1e-9)), file=sys.stderr)
        if step.guarded:    # every rank clears its (identical) record; the pass has just synchronised for its row
            gs = step.guard_stats(reset=True)
            if rank == 0:
                print("# grad norm: mean {:.6g} max {:.6g} clipped {}/{} skipped {}".format(
                    gs["mean_norm"], gs["max_norm"], gs["clipped"], gs["steps"], gs["skipped"]), file=sys.stderr)
        dump = None
        shapes = None
        if rule.dumps and (epoch + 1) % args.save_interval == 0:
            # the display helpers' draws are made on every rank (one random stream), the files written by rank 0
            shapes = display_draw_shapes(script, inf_dim, args.z_dim)
        tb, noise, shown = eval_pass_plan(ntest, bs, inf_dim, device, home, shapes, eval_k)
        if shapes and out_dir:
            dump = _image_dumper(script, step, x, cfg, out_dir, str(epoch + 1).zfill(digits), label, kw, args.z_dim, shown)
        ev = run_epoch(script, step, x, tb, False, data=te, inf_dim=inf_dim, noise=noise, mask=mask, kw=kw, dump=dump,
                       num_samples=eval_k, rank=rank, world=world)
        if rank == 0:
            if rule.split_rows:
                rows.append("\t".join([str(epoch + 1), "train", str(e), str(g), str(k)]))
                rows.append("\t".join([str(epoch + 1), "test", str(ev[0]), str(ev[1]), str(ev[2])]))
                print(rows[-2], file=out)
                print(rows[-1], file=out)
            else:
                line = "\t".join(map(str, [epoch, e, g, k]))
                train_lines.append(line)
                print(line, file=out)
                line = "\t".join(map(str, [epoch, ev[0], ev[1], ev[2]]))
                val_lines.append(line)
                print(line, file=out)
            out.flush()
            if not rule.run_dir and prefix is not None and (epoch + 1) % args.save_interval == 0:
                save_models(prefix, str(epoch + 1).zfill(digits), p_net, q_net, device)
            if state_prefix is not None and ((epoch + 1) % ckpt_every == 0 or epoch + 1 == num_epochs):
                write_checkpoint(checkpoint_path(state_prefix, str(epoch + 1).zfill(digits)), step.state_dict(), epoch + 1,
                                 args, world, fingerprint, dict(train_lines=train_lines, val_lines=val_lines, rows=rows))
    if rank == 0 and rule.run_dir:
        save_models(os.path.join(trained, prefix), str(num_epochs).zfill(digits), p_net, q_net, device)
        with open(os.path.join(out_dir, "train.txt"), "w") as f:
            print("\n".join(train_lines), file=f)
        with open(os.path.join(out_dir, "val.txt"), "w") as f:
            print("\n".join(val_lines), file=f)
        print("Elapsed time: {:.1f} s".format(time.time() - start))
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


def display_draw_shapes(script, inf_dim, z_dim):
    """Shapes of the N(0,1) draws eval_model's image dump makes for a first minibatch of B images: minibatch_for_display
    draws (B, inf_dim) (train_mnist.py:107, train_galaxy.py:146); galaxy's random_minibatch_generator then (B, z_dim)
    (train_galaxy.py:177)."""
    width = {"dis": inf_dim, "rnd": z_dim}
    return lambda B: [(B, width[d]) for d in SCRIPTS[script].dumps]


def _image_dumper(script, step, x, cfg, out_dir, epoch_str, label, kw, z_dim, shown=(None, None)):
    """The PNG dumps of eval_model (train_mnist.py:214-224, train_galaxy.py:275-292): <epoch>_dis_ = decoded from the
    content latents on the unposed grid, <epoch>_ = the posed reconstruction y_hat of the same batch, galaxy also
    <epoch>_rnd_ = decoded prior samples.  `shown`: the helpers' N(0,1) draws, made by pass_noise in the reference's order."""
    rule = SCRIPTS[script]
    dims = [cfg["n"], cfg["m"]]
    p_net, q_net = step.p_net, step.q_net
    shown = list(shown) + [None, None]

    def dump(y, y_hat):
        base = "{}/images/{}".format(out_dir, epoch_str)
        rows = y.size(0)                        # data parallel: rank 0's slice [0, rows) of the first global minibatch
        shown[0] = shown[0][:rows] if shown[0] is not None else None
        shown[1] = shown[1][:rows] if shown[1] is not None else None
        zs = kw.get("z_scale", 1)
        if not rule.z_schedule:
            dis = E.minibatch_for_display(x, y, p_net, q_net, rotate=cfg["rotate"], translate=cfg["translate"], noise=shown[0])
        else:
            dis = E.minibatch_for_display_galaxy(x, y, q_net, p_net, rotate=cfg["rotate"], translate=cfg["translate"], z_scale=zs,
                                                 noise=shown[0])
        if "rnd" in rule.dumps:
            rnd = E.random_minibatch_generator(x, y, p_net, z_dim, z_scale=zs, noise=shown[1])
            export_batch_as_image(rnd, "{}_rnd_{}.png".format(base, label), dims)
        export_batch_as_image(dis, "{}_dis_{}.png".format(base, label), dims)
        if y_hat is not None:
            export_batch_as_image(y_hat, "{}_{}.png".format(base, label), dims)

    return dump


def synthetic_images(kind, count, n, m, channels, seed):
    rs = np.random.RandomState(seed)
    if kind == "particles":
        return rs.normal(size=(count, n, m)).astype(np.float32)
    shape = (count, n, m) if channels == 1 else (count, n, m, channels)
    u = rs.uniform(size=shape)
    keep = rs.uniform(size=shape) > (0.8 if channels == 1 else 0.0)
    return np.floor(u * keep * 255.0).astype(np.float32)
