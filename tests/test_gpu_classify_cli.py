"""infer.py --refine --reassign end to end on the MI355X: train a small model with the command line, apply it with one class
(where re-assigning can change nothing) and with labels under --frc, read the files back, and replay round 1 in numpy
(tests/classify_ref.py) from the half-set arrays a plain run wrote.  Each subprocess runs under its own timeout."""
import json
import math
import os

import numpy as np
import pytest

import classify_ref as CR
from test_gpu_refine_cli import FRC_KEYS, MARGIN, PLAIN_KEYS, REFINE_CLASS_KEYS, REFINE_SCORE_KEYS, _bit_equal, _npz, _run

pytestmark = pytest.mark.gpu
REASSIGN_SCORE_KEYS = ["label_refined", "refine_class_margin", "refine_class_score", "refine_label", "refine_moved"]


def test_mnist_reassigned_class_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py --class_averages:
    --refine 2 with and without --reassign and no --labels (one class): every array the two runs share is bit-equal,
    label_refined and refine_moved are all 0, members_unrefined equals members;
    --labels (classes 0..2 and -1) --frc --refine 2 --reassign --aligned --reassign_labels: the score arrays of the plain run are
    bit-equal, meta gains reassign and reassign_labels, members is bincount(label_refined) and half_members agree with it,
    members_unrefined is the plain run's members, sum[k] is the sum of the aligned stack over label_refined == k (1e-12
    relative), the half counts add to count, the images labelled -1 keep label and pose, the .npy written is label_refined,
    refine_moved[r] counts the changes between consecutive columns of refine_label, label_refined is its last column; the same
    command again gives bit-equal files and leaves no .tmp file;
    a numpy replay of round 1 (classify_ref on the split's images, references half_sum / half_count of the plain --frc run, slot k
    = 2k + (i & 1), elbo.refine_mask) reproduces refine_label[:, 0] for every image whose reference margin exceeds 1e-9, and
    those are at least 0.9 of the labelled images.
    MI355X: all 37 labelled images have a margin above 1e-9 (least 1.13e-2) and the replayed margins differ by at most 1.1e-16;
    with these random labels no image moves (each average holds the image itself), so what moving changes in the sums is the
    planted case's and the bincount identities' to show."""
    import torch
    import train_mnist
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    images, n, m, K = 50, 28, 28, 3
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1"]

    # one class: nothing can move, and nothing else may change
    _run(common + ["--out", "r1.npz", "--class_averages", "cr1.npz", "--refine", "2"], cwd)
    _run(common + ["--out", "m1.npz", "--class_averages", "cm1.npz", "--refine", "2", "--reassign"], cwd)
    r1, m1 = _npz(os.path.join(cwd, "r1.npz")), _npz(os.path.join(cwd, "m1.npz"))
    cr1, cm1 = _npz(os.path.join(cwd, "cr1.npz")), _npz(os.path.join(cwd, "cm1.npz"))
    assert sorted(m1) == sorted(list(r1) + REASSIGN_SCORE_KEYS) and sorted(cm1) == sorted(list(cr1) + ["members_unrefined"])
    _bit_equal(r1, m1, [k for k in r1 if k != "meta"])
    _bit_equal(cr1, cm1, list(cr1))
    assert m1["label_refined"].dtype == np.int64 and m1["label_refined"].shape == (images,) and (m1["label_refined"] == 0).all()
    assert m1["refine_moved"].dtype == np.int64 and m1["refine_moved"].tolist() == [0, 0] and (m1["refine_label"] == 0).all()
    assert np.isinf(m1["refine_class_margin"]).all() and m1["refine_class_score"].tobytes() == r1["refine_score"][:, 1:].tobytes()
    assert np.array_equal(cm1["members_unrefined"], cm1["members"]) and cm1["members"].tolist() == [images]
    meta = json.loads(str(m1["meta"]))
    assert dict(json.loads(str(r1["meta"])), class_averages="cm1.npz", reassign=True, reassign_labels=None) == meta

    # labels, half sets
    label = np.random.RandomState(5).randint(-1, K, size=images)
    label[:4] = [0, 1, 2, -1]
    np.save(os.path.join(cwd, "l.npy"), label)
    classes = ["--labels", "l.npy", "--frc"]
    _run(common + ["--out", "p.npz", "--class_averages", "c0.npz"] + classes, cwd)
    p, c0 = _npz(os.path.join(cwd, "p.npz")), _npz(os.path.join(cwd, "c0.npz"))
    pose0 = np.concatenate([p["theta_iw"][:, None], p["dx_iw"]], 1)
    moving = ["--refine", "2", "--reassign", "--aligned", "a.npy", "--reassign_labels", "new.npy"]
    _run(common + ["--out", "s.npz", "--class_averages", "c.npz"] + classes + moving, cwd)
    s, c = _npz(os.path.join(cwd, "s.npz")), _npz(os.path.join(cwd, "c.npz"))
    _bit_equal(p, s, [k for k in p if k != "meta"])
    assert sorted(s) == sorted(list(p) + REFINE_SCORE_KEYS + REASSIGN_SCORE_KEYS)
    assert sorted(c) == sorted(PLAIN_KEYS + FRC_KEYS + REFINE_CLASS_KEYS + ["members_unrefined"])
    meta, meta_plain = json.loads(str(s["meta"])), json.loads(str(p["meta"]))
    assert dict(meta_plain, class_averages="c.npz", aligned="a.npy", refine=2, refine_angles=5, refine_step=2.0, refine_shift=2,
                reassign=True, reassign_labels="new.npy") == meta
    assert not {"reassign", "reassign_labels"} & set(meta_plain)
    final, rounds = s["label_refined"], s["refine_label"]
    assert final.dtype == np.int64 and final.shape == (images,) and rounds.dtype == np.int32 and rounds.shape == (images, 2)
    assert s["refine_moved"].dtype == np.int64 and s["refine_class_score"].shape == (images, K) and s["refine_class_score"].dtype == np.float64
    assert s["refine_class_margin"].shape == (images, 2) and s["refine_class_margin"].dtype == np.float64
    assert np.array_equal(final, rounds[:, 1]) and final.min() == -1 and final.max() < K
    assert s["refine_moved"].tolist() == [int((rounds[:, 0] != label).sum()), int((rounds[:, 1] != rounds[:, 0]).sum())]
    out = label < 0
    assert (final[out] == -1).all() and (rounds[out] == -1).all() and (final[~out] >= 0).all()
    assert s["pose_refined"][out].tobytes() == pose0[out].astype(np.float32).tobytes()
    assert np.isneginf(s["refine_class_score"][out]).all() and np.isinf(s["refine_class_margin"][out]).all()
    live_score = s["refine_class_score"][~out]
    assert np.isfinite(live_score).any(1).all() and np.array_equal(live_score.argmax(1), final[~out])
    assert np.array_equal(live_score.max(1), s["refine_score"][~out, 1])       # the search against the chosen class: the same bits
    saved = np.load(os.path.join(cwd, "new.npy"))
    assert saved.dtype == np.int64 and np.array_equal(saved, final)
    assert np.array_equal(c["members"], np.bincount(final[final >= 0], minlength=K)) and c["members"].sum() == (~out).sum()
    halves = np.bincount(2 * final[~out] + (np.arange(images)[~out] & 1), minlength=2 * K).reshape(K, 2)
    assert np.array_equal(c["half_members"], halves) and np.array_equal(c["half_members"].sum(1), c["members"])
    assert np.array_equal(c["members_unrefined"], c0["members"]) and np.array_equal(c0["members"], np.bincount(label[~out], minlength=K))
    a = np.load(os.path.join(cwd, "a.npy"))
    for k in range(K):                              # --aligned holds the last round's alignment: what the sums are of
        want = a[final == k].astype(np.float64).sum(0)
        assert np.abs(c["sum"][k] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(c["half_count"][:, 0] + c["half_count"][:, 1], c["count"])
    for k in ("average", "frc"):
        assert c[k + "_unrefined"].tobytes() == c0[k].tobytes(), k
    print("re-assignment: moved %s of %d labelled images; members %s -> %s"
          % (s["refine_moved"].tolist(), (~out).sum(), c0["members"].tolist(), c["members"].tolist()))

    _run(common + ["--out", "s.npz", "--class_averages", "c.npz"] + classes + moving, cwd)      # again, over its own files
    _bit_equal(s, _npz(os.path.join(cwd, "s.npz")))
    _bit_equal(c, _npz(os.path.join(cwd, "c.npz")))
    assert np.array_equal(a, np.load(os.path.join(cwd, "a.npy"))) and np.array_equal(saved, np.load(os.path.join(cwd, "new.npy")))
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    # round 1 again, in numpy, from what the plain run wrote
    cfg = train_mnist.build(train_mnist.mnist_arguments(train), torch.device("cpu"))    # the split, as infer.infer_main obtains it
    y = cfg["y_test"].numpy().reshape(images, n * m, 1)
    count = c0["half_count"][..., None]
    ref = np.divide(c0["half_sum"], count, out=np.zeros_like(c0["half_sum"]), where=count > 0).reshape(2 * K, n * m, 1)
    cand = np.where(label[:, None] >= 0, 2 * np.arange(K)[None, :] + (np.arange(images)[:, None] & 1), -1).astype(np.int32)
    want = CR.pose_classify(y, ref, E.refine_mask(n, m, 2).reshape(-1), cand, pose0, n, m, 5, math.radians(2.0), 2, "bicubic")
    clear = (want["margin"] > MARGIN) & ~out
    print("round 1 replayed: %d of %d labelled images have a margin above %.0e (least %.2e); margin error %.2e"
          % (clear.sum(), (~out).sum(), MARGIN, want["margin"][~out].min(),
             np.abs(want["margin"][~out] - s["refine_class_margin"][~out, 0]).max()))
    assert clear.sum() >= 0.9 * (~out).sum()
    assert np.array_equal(rounds[clear, 0], want["choice"][clear])
    assert (want["choice"][out] == -1).all()
    assert np.abs(want["margin"][clear] - s["refine_class_margin"][clear, 0]).max() <= 1e-10
