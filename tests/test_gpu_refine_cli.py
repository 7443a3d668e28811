"""infer.py --refine end to end on the MI355X: train a small model with the command line, apply it without the option, with an
empty search and with two rounds, read the files back, and replay round 1 in numpy (tests/refine_ref.py) from the half-set
arrays the plain run wrote.  Each subprocess runs under its own timeout."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
MARGIN = 1e-9       # tests/test_gpu_refine.py's: the replay compares winners where the reference's best beats its second best by more
PLAIN_KEYS = ["average", "count", "members", "sum"]
FRC_KEYS = ["average_filtered", "frc", "frc_mask", "frc_never_below", "frc_sums", "frc_weight", "half_count", "half_members", "half_sum",
            "resolution_0143", "resolution_05", "ring_count", "ring_frequency"]
REFINE_CLASS_KEYS = ["average_unrefined", "frc_unrefined", "resolution_0143_unrefined", "resolution_05_unrefined"]
REFINE_SCORE_KEYS = ["pose_refined", "refine_offset", "refine_score"]


def _run(args, cwd, code=0):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, args[0])] + args[1:], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=LIMIT)
    assert out.returncode == code, out.stdout[-1500:] + out.stderr[-3000:]
    return out


def _npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _bit_equal(a, b, keys=None):
    keys = sorted(a) if keys is None else keys
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def test_mnist_refined_class_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py --class_averages
    --labels --frc (classes 0..2 and -1):
    without --refine, and with --refine 1 --refine_angles 0 --refine_shift 0: every array of the plain class file is in the
    other bit for bit, its average_unrefined / frc_unrefined / resolution_*_unrefined equal its own average / frc / resolution_*
    bit for bit, pose_refined is (theta_iw, dx_iw), every refine_offset row is 0 (flags 4 for the images in no class);
    with --refine 2 --aligned: the score arrays the plain run has are bit-equal, meta gains the four options, average_unrefined
    and the *_unrefined curves are the plain run's average and curves bit for bit, the sums of the last round are the sums of
    the aligned stack by label (1e-12 relative), the images in no class keep their pose; the same command again gives bit-equal
    arrays and leaves no .tmp file;
    a numpy replay of round 1 (refine_ref on the split's images, references half_sum / half_count of the plain run, index
    2 label + (i & 1), elbo.refine_mask) reproduces refine_offset[:, 0] for every image whose margin exceeds 1e-9, and those
    are at least 0.9 of the images;
    --cluster 3 --refine 2 and then --labels on the labels it wrote give bit-equal class files and refined arrays.
    MI355X: all 50 images have a margin above 1e-9 (least 1.1e-3) and the replayed scores differ by at most 1.1e-16."""
    import torch
    import train_mnist
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    images, n, m, K = 50, 28, 28, 3
    label = np.random.RandomState(5).randint(-1, K, size=images)
    label[:4] = [0, 1, 2, -1]
    np.save(os.path.join(cwd, "l.npy"), label)
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1"]
    classes = ["--labels", "l.npy", "--frc"]
    _run(common + ["--out", "p.npz", "--class_averages", "c0.npz"] + classes, cwd)
    p, c0 = _npz(os.path.join(cwd, "p.npz")), _npz(os.path.join(cwd, "c0.npz"))
    assert sorted(c0) == sorted(PLAIN_KEYS + FRC_KEYS) and not set(REFINE_SCORE_KEYS) & set(p)
    pose0 = np.concatenate([p["theta_iw"][:, None], p["dx_iw"]], 1)

    # an empty search changes nothing
    _run(common + ["--out", "e.npz", "--class_averages", "ce.npz", "--refine", "1", "--refine_angles", "0", "--refine_shift", "0"] + classes, cwd)
    e, ce = _npz(os.path.join(cwd, "e.npz")), _npz(os.path.join(cwd, "ce.npz"))
    assert sorted(ce) == sorted(PLAIN_KEYS + FRC_KEYS + REFINE_CLASS_KEYS) and sorted(e) == sorted(list(p) + REFINE_SCORE_KEYS)
    _bit_equal(c0, ce, PLAIN_KEYS + FRC_KEYS)
    for k in ("average", "frc", "resolution_0143", "resolution_05"):
        assert ce[k + "_unrefined"].dtype == ce[k].dtype and ce[k + "_unrefined"].tobytes() == ce[k].tobytes(), k
    assert e["pose_refined"].dtype == np.float32 and e["pose_refined"].tobytes() == pose0.astype(np.float32).tobytes()
    assert e["refine_offset"].shape == (images, 1, 4) and e["refine_offset"].dtype == np.int32 and e["refine_score"].shape == (images, 1)
    assert (e["refine_offset"][label >= 0] == 0).all() and (e["refine_offset"][label < 0, 0] == [0, 0, 0, R.SKIPPED]).all()
    assert (e["refine_score"][label < 0] == 0).all() and (e["refine_score"][label >= 0] != 0).all()

    # two rounds
    refine = ["--refine", "2", "--aligned", "a.npy"]
    _run(common + ["--out", "s.npz", "--class_averages", "c.npz"] + classes + refine, cwd)
    s, c = _npz(os.path.join(cwd, "s.npz")), _npz(os.path.join(cwd, "c.npz"))
    _bit_equal(p, s, [k for k in p if k != "meta"])
    meta, meta_plain = json.loads(str(s["meta"])), json.loads(str(p["meta"]))
    assert dict(meta_plain, class_averages="c.npz", aligned="a.npy", refine=2, refine_angles=5, refine_step=2.0, refine_shift=2) == meta
    assert not {"refine", "refine_angles", "refine_step", "refine_shift"} & set(meta_plain)
    assert sorted(c) == sorted(PLAIN_KEYS + FRC_KEYS + REFINE_CLASS_KEYS)
    for k in ("average", "frc", "resolution_0143", "resolution_05"):
        assert c[k + "_unrefined"].dtype == c0[k].dtype and c[k + "_unrefined"].tobytes() == c0[k].tobytes(), k
    _bit_equal(c0, c, ["members", "half_members", "ring_count", "ring_frequency", "frc_mask"])
    assert s["pose_refined"].shape == (images, 3) and s["refine_score"].shape == (images, 2) and s["refine_offset"].shape == (images, 2, 4)
    assert s["refine_score"].dtype == np.float64 and (np.abs(s["refine_score"]) <= 1 + 1e-12).all()
    assert s["pose_refined"][label < 0].tobytes() == pose0[label < 0].astype(np.float32).tobytes()
    assert (s["refine_offset"][label < 0] == [0, 0, 0, R.SKIPPED]).all() and (s["refine_offset"][label >= 0, :, 3] & R.SKIPPED == 0).all()
    assert (s["refine_offset"][label >= 0, 0, :3] != 0).any() and not np.array_equal(c["sum"], c0["sum"])
    a = np.load(os.path.join(cwd, "a.npy"))
    for k in range(K):                              # --aligned holds the last round's alignment: what the sums are of
        want = a[label == k].astype(np.float64).sum(0)
        assert np.abs(c["sum"][k] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(c["half_count"][:, 0] + c["half_count"][:, 1], c["count"])
    live = label >= 0
    print("refine scores: round 1 mean %.4f, round 2 mean %.4f; resolution at 0.143 %s -> %s pixels"
          % (s["refine_score"][live, 0].mean(), s["refine_score"][live, 1].mean(), c["resolution_0143_unrefined"][:, 0].tolist(),
             c["resolution_0143"][:, 0].tolist()))

    _run(common + ["--out", "s.npz", "--class_averages", "c.npz"] + classes + refine, cwd)      # again, over its own files
    _bit_equal(s, _npz(os.path.join(cwd, "s.npz")))
    _bit_equal(c, _npz(os.path.join(cwd, "c.npz")))
    assert np.array_equal(a, np.load(os.path.join(cwd, "a.npy"))) and not [f for f in os.listdir(cwd) if ".tmp" in f]

    # round 1 again, in numpy, from what the plain run wrote
    cfg = train_mnist.build(train_mnist.mnist_arguments(train), torch.device("cpu"))    # the split, as infer.infer_main obtains it
    y = cfg["y_test"].numpy().reshape(images, n * m, 1)
    count = c0["half_count"][..., None]
    ref = np.divide(c0["half_sum"], count, out=np.zeros_like(c0["half_sum"]), where=count > 0).reshape(2 * K, n * m, 1)
    index = np.where(label >= 0, 2 * label + (np.arange(images) & 1), -1).astype(np.int32)
    want = R.pose_search(y, ref, E.refine_mask(n, m, 2).reshape(-1), index, pose0, n, m, 5, math.radians(2.0), 2, "bicubic")
    clear = want["margin"] > MARGIN
    share = float(clear.mean())
    print("round 1 replayed: %d of %d images have a margin above %.0e (least %.2e); score error %.2e"
          % (clear.sum(), images, MARGIN, want["margin"].min(), np.abs(want["score"] - s["refine_score"][:, 0]).max()))
    assert share >= 0.9
    assert np.array_equal(s["refine_offset"][clear, 0], want["offset"][clear])
    assert np.abs(want["score"] - s["refine_score"][:, 0])[clear].max() <= 1e-10

    # --cluster makes the labels; --labels on what it wrote repeats the refinement
    _run(common + ["--out", "k.npz", "--cluster", "3", "--cluster_out", "f.npz", "--cluster_labels", "l2.npy", "--class_averages", "cc.npz",
                   "--frc", "--refine", "2"], cwd)
    _run(common + ["--out", "k2.npz", "--labels", "l2.npy", "--class_averages", "cl.npz", "--frc", "--refine", "2"], cwd)
    cc, cl = _npz(os.path.join(cwd, "cc.npz")), _npz(os.path.join(cwd, "cl.npz"))
    assert sorted(cc) == sorted(cl) == sorted(PLAIN_KEYS + FRC_KEYS + REFINE_CLASS_KEYS)
    _bit_equal(cc, cl)
    _bit_equal(_npz(os.path.join(cwd, "k.npz")), _npz(os.path.join(cwd, "k2.npz")), REFINE_SCORE_KEYS)
