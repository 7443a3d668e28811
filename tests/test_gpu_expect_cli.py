"""infer.py --refine --reassign --refine_soft end to end on the MI355X: train a small model with the command line, apply it with
labels with and without --frc, read the files back; the sharp limit against the hard run; a repeat; the refusals.  Each
subprocess runs under its own timeout."""
import json
import os

import numpy as np
import pytest

from test_gpu_classify_cli import REASSIGN_SCORE_KEYS
from test_gpu_refine_cli import REFINE_SCORE_KEYS, _bit_equal, _npz, _run

pytestmark = pytest.mark.gpu
SOFT_SCORE_KEYS = ["refine_class_post", "refine_log_evidence", "refine_post_max", "refine_soft_sigma2"]


def test_mnist_soft_class_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py --class_averages
    --labels (classes 0..2 and -1) --refine 2 --reassign:
    with --frc, hard and then with --refine_soft: the score file gains exactly the four refine_soft arrays with the stated shapes
    and meta the three options, the class file has the hard run's arrays; everything that does not depend on the averages of a
    soft round is the hard run's bit for bit (the plain scores, round 1's labels, scores, offsets and margins); sigma2 is finite
    and positive in both rounds; the refine_class_post rows of labelled images sum to 1 within 1e-12 and the others are zero,
    refine_post_max is its largest entry in the last round; per class count.max() is at most the number of labelled images and
    the counts of all classes add to at most that number at every pixel (1e-9); the half sums add to the full ones (1e-12
    relative); members stays the count of the hard labels; the same command again gives bit-equal files and leaves no .tmp file;
    without --frc the same shapes and bounds.
    The sharp limit: --refine 1 --refine_angles 0 --refine_shift 0 --refine_soft_sigma2 1e-12 against the same run without
    --refine_soft.  With an empty search the hard path's aligned image is the candidate plane P_0 itself rounded to float (an
    integer shift of 0), and the two runs are comparable exactly where every labelled image's posterior is one-hot on the class
    the hard run moved it to -- refine_post_max == 1 and argmax refine_class_post == label_refined, asserted --; then count is
    equal bit for bit and sum and average agree within 1e-6 relative.
    The refusals exit 2 and leave the directory unchanged."""
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    images, n, m, K, R = 50, 28, 28, 3, 2
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1"]
    label = np.random.RandomState(5).randint(-1, K, size=images)
    label[:4] = [0, 1, 2, -1]
    np.save(os.path.join(cwd, "l.npy"), label)
    out = label < 0
    labelled = int((~out).sum())
    moving = ["--labels", "l.npy", "--refine", str(R), "--reassign"]

    def bounds(s, c):
        assert s["refine_soft_sigma2"].shape == (R,) and s["refine_soft_sigma2"].dtype == np.float64
        assert s["refine_log_evidence"].shape == (images, R) and s["refine_post_max"].shape == (images, R)
        assert s["refine_class_post"].shape == (images, K) and s["refine_class_post"].dtype == np.float64
        assert np.isfinite(s["refine_soft_sigma2"]).all() and (s["refine_soft_sigma2"] > 0).all()
        post = s["refine_class_post"]
        assert np.abs(post[~out].sum(1) - 1).max() <= 1e-12 and not post[out].any() and (post >= 0).all()
        assert np.array_equal(s["refine_post_max"][:, R - 1], post.max(1)) and not s["refine_post_max"][out].any()
        assert not s["refine_log_evidence"][out].any() and np.isfinite(s["refine_log_evidence"]).all()
        assert (s["refine_post_max"][~out] > 0).all() and (s["refine_post_max"] <= 1 + 1e-12).all()
        count = c["count"].reshape(K, -1)
        assert count.max() <= labelled and count.sum(0).max() <= labelled + 1e-9 and count.min() >= 0
        final = s["label_refined"]
        assert np.array_equal(c["members"], np.bincount(final[final >= 0], minlength=K)) and c["members"].sum() == labelled
        meta = json.loads(str(s["meta"]))
        assert meta["refine_soft"] is True and meta["refine_soft_classes"] == 8 and meta["refine_soft_sigma2"] is None

    # half sets
    _run(common + ["--out", "h.npz", "--class_averages", "ch.npz", "--frc"] + moving, cwd)
    soft = ["--out", "s.npz", "--class_averages", "c.npz", "--frc", "--aligned", "a.npy"] + moving + ["--refine_soft"]
    _run(common + soft, cwd)
    h, ch = _npz(os.path.join(cwd, "h.npz")), _npz(os.path.join(cwd, "ch.npz"))
    s, c = _npz(os.path.join(cwd, "s.npz")), _npz(os.path.join(cwd, "c.npz"))
    assert sorted(s) == sorted(list(h) + SOFT_SCORE_KEYS) and sorted(c) == sorted(ch)
    assert set(REFINE_SCORE_KEYS + REASSIGN_SCORE_KEYS) <= set(h)
    _bit_equal(h, s, [k for k in h if not k.startswith(("refine_", "pose_refined", "label_refined")) and k != "meta"])
    for k in ("refine_label", "refine_score", "refine_offset", "refine_class_margin"):      # round 1 saw the same references
        assert s[k][:, 0].tobytes() == h[k][:, 0].tobytes(), k
    assert not {"refine_soft", "refine_soft_classes", "refine_soft_sigma2"} & set(json.loads(str(h["meta"])))
    assert json.loads(str(s["meta"])) == dict(json.loads(str(h["meta"])), class_averages="c.npz", aligned="a.npy", refine_soft=True,
                                               refine_soft_classes=8, refine_soft_sigma2=None)
    bounds(s, c)
    for full, half in (("sum", "half_sum"), ("count", "half_count")):
        pair = c[half][:, 0] + c[half][:, 1]
        assert np.abs(c[full] - pair).max() <= 1e-12 * np.abs(pair).max(), full
    assert c["average_unrefined"].tobytes() == ch["average_unrefined"].tobytes()
    print("soft rounds: sigma2 %s, least / median largest posterior %.3f / %.3f, members %s"
          % (s["refine_soft_sigma2"].tolist(), s["refine_post_max"][~out, R - 1].min(), np.median(s["refine_post_max"][~out, R - 1]),
             c["members"].tolist()))
    a = np.load(os.path.join(cwd, "a.npy"))
    _run(common + soft, cwd)                                                # again, over its own files
    _bit_equal(s, _npz(os.path.join(cwd, "s.npz")))
    _bit_equal(c, _npz(os.path.join(cwd, "c.npz")))
    assert np.array_equal(a, np.load(os.path.join(cwd, "a.npy"))) and not [f for f in os.listdir(cwd) if ".tmp" in f]

    # without half sets
    _run(common + ["--out", "s2.npz", "--class_averages", "c2.npz"] + moving + ["--refine_soft"], cwd)
    s2, c2 = _npz(os.path.join(cwd, "s2.npz")), _npz(os.path.join(cwd, "c2.npz"))
    assert set(SOFT_SCORE_KEYS) <= set(s2) and "half_sum" not in c2
    bounds(s2, c2)

    # the sharp limit, on an empty search
    still = ["--labels", "l.npy", "--refine", "1", "--reassign", "--refine_angles", "0", "--refine_shift", "0"]
    _run(common + ["--out", "h0.npz", "--class_averages", "ch0.npz"] + still, cwd)
    _run(common + ["--out", "s0.npz", "--class_averages", "cs0.npz"] + still + ["--refine_soft", "--refine_soft_sigma2", "1e-12"], cwd)
    h0, ch0 = _npz(os.path.join(cwd, "h0.npz")), _npz(os.path.join(cwd, "ch0.npz"))
    s0, cs0 = _npz(os.path.join(cwd, "s0.npz")), _npz(os.path.join(cwd, "cs0.npz"))
    assert s0["refine_soft_sigma2"].tolist() == [1e-12] and json.loads(str(s0["meta"]))["refine_soft_sigma2"] == 1e-12
    assert np.array_equal(s0["label_refined"], h0["label_refined"]) and s0["pose_refined"].tobytes() == h0["pose_refined"].tobytes()
    comparable = (s0["refine_post_max"][~out, 0] == 1).all() and \
        np.array_equal(s0["refine_class_post"][~out].argmax(1), h0["label_refined"][~out])
    assert comparable, (s0["refine_post_max"][~out, 0].min(), s0["refine_class_post"][~out].argmax(1), h0["label_refined"][~out])
    assert cs0["count"].tobytes() == ch0["count"].tobytes()
    for k in ("sum", "average"):
        err = np.abs(cs0[k].astype(np.float64) - ch0[k]).max() / np.abs(ch0[k]).max()
        print("sharp limit, %s: %.2e relative" % (k, err))
        assert err <= 1e-6, k

    # refusals
    before = sorted(os.listdir(cwd))
    for extra, message in ((["--labels", "l.npy", "--refine", "1", "--refine_soft"], "--refine_soft needs --reassign"),
                           (moving + ["--refine_soft_classes", "4"], "--refine_soft_classes needs --refine_soft"),
                           (moving + ["--refine_soft", "--refine_soft_classes", "65"], "--refine_soft_classes must be in [1, 64]"),
                           (moving + ["--refine_soft", "--refine_soft_sigma2", "0"], "--refine_soft_sigma2 must be a finite number > 0")):
        got = _run(common + ["--out", "x.npz", "--class_averages", "cx.npz"] + extra, cwd, code=2)
        assert message in got.stderr and sorted(os.listdir(cwd)) == before
