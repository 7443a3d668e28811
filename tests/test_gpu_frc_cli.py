"""infer.py --frc end to end on the MI355X: train a small model with the command line, apply it with and without the option,
read the files back and hold the new arrays to tests/frc_ref.py on the half-set arrays the same file reports.  Each subprocess
runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frc_ref as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
TOL_SUMS, TOL_FRC, TOL_FILTER = 1e-11, 1e-9, 2e-6      # tests/test_gpu_frc.py's bounds
PLAIN_KEYS = ["average", "count", "members", "sum"]
FRC_KEYS = ["average_filtered", "frc", "frc_mask", "frc_never_below", "frc_sums", "frc_weight", "half_count", "half_members", "half_sum",
            "resolution_0143", "resolution_05", "ring_count", "ring_frequency"]


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


def _check_frc_arrays(c, planes, full, label, radius, edge):
    """The --frc arrays of one file against the reference: planes (n_classes, 2, n, m, C) are the half planes the FRC is of,
    full (n_classes, n, m, C) the average that was filtered.  Returns the worst errors (sums, frc, filter)."""
    K, _, n, m, C = planes.shape
    L, R = F.layout(n, m)
    shapes = {"half_sum": (K, 2, n, m, C), "half_count": (K, 2, n, m), "half_members": (K, 2), "frc": (K, C, R), "frc_sums": (K, C, R, 3),
              "ring_count": (R,), "ring_frequency": (R,), "frc_weight": (K, C, R), "average_filtered": (K, n, m, C),
              "resolution_0143": (K, C), "resolution_05": (K, C), "frc_never_below": (K, C, 2), "frc_mask": (n, m)}
    for k, shape in shapes.items():
        assert c[k].shape == shape, (k, c[k].shape)
    assert c["average_filtered"].dtype == np.float32 and c["frc_never_below"].dtype == np.bool_ and c["half_members"].dtype == np.int64
    assert all(c[k].dtype == np.float64 for k in ("half_sum", "half_count", "frc", "frc_sums", "frc_weight", "ring_frequency",
                                                   "resolution_0143", "resolution_05", "frc_mask"))
    in_class = label >= 0
    members = np.bincount(2 * label[in_class] + (np.arange(len(label))[in_class] & 1), minlength=2 * K).reshape(K, 2)
    assert np.array_equal(c["half_members"], members) and np.array_equal(members.sum(1), c["members"])
    assert np.array_equal(c["ring_count"], F.ring_count(n, m)) and np.array_equal(c["ring_frequency"], np.arange(R) / L)
    assert np.array_equal(c["frc_mask"], F.mask(n, m, radius, edge))
    a = planes[:, 0].transpose(0, 3, 1, 2).reshape(K * C, n, m)
    b = planes[:, 1].transpose(0, 3, 1, 2).reshape(K * C, n, m)
    sums, curve, _ = F.frc(a, b, n, m, radius, edge)
    live = sums[..., 1:].reshape(K * C, -1).max(1) > 0
    scale = np.where(live, sums[..., 1:].reshape(K * C, -1).max(1), 1.0)
    e_sums = float((np.abs(c["frc_sums"].reshape(K * C, R, 3) - sums).reshape(K * C, -1).max(1) / scale).max())
    e_frc = float(np.abs(c["frc"].reshape(K * C, R) - curve).max())
    assert np.abs(c["frc_weight"] - F.weight(c["frc"])).max() <= 1e-15
    want = F.filter_planes(full.transpose(0, 3, 1, 2).reshape(K * C, n, m), c["frc_weight"].reshape(K * C, R), n, m)
    got = c["average_filtered"].transpose(0, 3, 1, 2).reshape(K * C, n, m).astype(np.float64)
    top = np.abs(want).reshape(K * C, -1).max(1)
    e_filter = float((np.abs(got - want).reshape(K * C, -1).max(1) / np.where(top > 0, top, 1.0)).max())
    for j, (name, threshold) in enumerate((("resolution_0143", 0.143), ("resolution_05", 0.5))):
        for k in range(K):
            for ch in range(C):
                res, never = F.resolution(c["frc"][k, ch], threshold, L)
                assert np.array_equal(c[name][k, ch], res, equal_nan=True) and c["frc_never_below"][k, ch, j] == never, (name, k, ch)
    for k in range(K):                              # an empty half: FRC 0, no resolution, a zero filtered average
        if members[k].min() == 0:
            assert (c["frc"][k] == 0).all() and (c["frc_weight"][k] == 0).all() and (c["average_filtered"][k] == 0).all()
            assert np.isnan(c["resolution_0143"][k]).all() and np.isnan(c["resolution_05"][k]).all()
    return e_sums, e_frc, e_filter


def test_mnist_half_sets_frc_and_filtered_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py with --class_averages
    --labels (classes 0..2, -1, and class 3 of a single image, so one of its halves is empty) without and with --frc: the score
    arrays and sum / count / average / members are bit-equal, the plain file keeps exactly its four keys and only the --frc run's
    meta has frc, frc_mask_radius (11.0) and frc_mask_edge (3.0); the half counts add to count exactly and the half sums to sum
    within 1e-12 of its maximum; half_members is the parity count of the labels; frc_sums and frc are frc_ref of half_sum /
    half_count within 1e-11 of the largest power and 1e-9; resolution_* is frc_resolution of the file's frc exactly;
    average_filtered is the reference filter of `average` with the file's frc_weight within 2e-6; class 3 has FRC 0, resolution
    NaN and a zero filtered average.  A second identical run gives bit-equal arrays and no .tmp file remains.  --cluster 3 --frc
    and then --labels on the labels it wrote give bit-equal class files.  MI355X: sums 3.7e-16, frc 4.4e-16, filter 4.7e-8."""
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    images, n, m = 50, 28, 28
    label = np.random.RandomState(5).randint(-1, 3, size=images)
    label[:5] = [0, 1, 2, -1, 3]
    np.save(os.path.join(cwd, "l.npy"), label)
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1"]
    _run(common + ["--out", "p.npz", "--class_averages", "c0.npz", "--labels", "l.npy"], cwd)
    _run(common + ["--out", "s.npz", "--class_averages", "c.npz", "--labels", "l.npy", "--frc"], cwd)
    p, s = _npz(os.path.join(cwd, "p.npz")), _npz(os.path.join(cwd, "s.npz"))
    assert sorted(p) == sorted(s)
    _bit_equal(p, s, [k for k in p if k != "meta"])
    meta, meta_plain = json.loads(str(s["meta"])), json.loads(str(p["meta"]))
    assert dict(meta_plain, class_averages="c.npz", frc=True, frc_mask_radius=11.0, frc_mask_edge=3.0) == meta
    assert not {"frc", "frc_mask_radius", "frc_mask_edge"} & set(meta_plain)
    c0, c = _npz(os.path.join(cwd, "c0.npz")), _npz(os.path.join(cwd, "c.npz"))
    assert sorted(c0) == PLAIN_KEYS and sorted(c) == sorted(PLAIN_KEYS + FRC_KEYS)
    _bit_equal(c0, c, PLAIN_KEYS)
    assert c["sum"].shape == (4, n, m, 1)
    assert np.array_equal(c["half_count"][:, 0] + c["half_count"][:, 1], c["count"])
    assert np.abs(c["half_sum"][:, 0] + c["half_sum"][:, 1] - c["sum"]).max() <= 1e-12 * np.abs(c["sum"]).max()
    assert c["half_members"][3].tolist() == [1, 0]
    count = c["half_count"][..., None]
    planes = np.divide(c["half_sum"], count, out=np.zeros_like(c["half_sum"]), where=count > 0)
    errors = _check_frc_arrays(c, planes, c["average"].astype(np.float64), label, 11.0, 3.0)
    print("mnist --frc against frc_ref: sums %.2e of the largest power, frc %.2e, filter %.2e of the plane maximum" % errors)
    print("resolution at 0.143: %s pixels; frc of class 0: %s" % (c["resolution_0143"][:, 0].tolist(), np.round(c["frc"][0, 0], 3).tolist()))
    assert errors[0] <= TOL_SUMS and errors[1] <= TOL_FRC and errors[2] <= TOL_FILTER

    _run(common + ["--out", "s.npz", "--class_averages", "c.npz", "--labels", "l.npy", "--frc"], cwd)     # again, over its own files
    _bit_equal(s, _npz(os.path.join(cwd, "s.npz")))
    _bit_equal(c, _npz(os.path.join(cwd, "c.npz")))
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    _run(common + ["--out", "k.npz", "--cluster", "3", "--cluster_out", "f.npz", "--cluster_labels", "l2.npy", "--class_averages", "cc.npz",
                   "--frc"], cwd)
    _run(common + ["--out", "k2.npz", "--labels", "l2.npy", "--class_averages", "cl.npz", "--frc"], cwd)
    cc, cl = _npz(os.path.join(cwd, "cc.npz")), _npz(os.path.join(cwd, "cl.npz"))
    assert sorted(cc) == sorted(cl) == sorted(PLAIN_KEYS + FRC_KEYS)
    _bit_equal(cc, cl)
    assert cc["frc"].shape == (3, 1, 15) and np.array_equal(np.load(os.path.join(cwd, "l2.npy")) >= 0, np.ones(images, bool))


def test_particles_wiener_half_sets(tmp_path):
    """train_particles.py --synthetic 200 with two CTF tables for one epoch (50 validation images of 40 x 40), then infer.py
    --ctf_correct wiener --class_averages --labels without and with --frc: the plain and the wiener_* arrays are bit-equal; the
    two halves of half_sum add to wiener_sum within 1e-12 of its maximum; frc_sums and frc are frc_ref of half_sum itself (mask
    17, 3) within 1e-11 and 1e-9; average_filtered is the reference filter of wiener_average within 2e-6; a second identical
    run gives bit-equal arrays and no .tmp file remains.  MI355X: sums 5.4e-16, frc 3.5e-16, filter 3.4e-8."""
    from ctfcorr_ref import random_table
    cwd = str(tmp_path)
    for name, t in (("tr.txt", random_table(200, 40)), ("te.txt", random_table(50, 41))):
        np.savetxt(os.path.join(cwd, name), t)
    train = ["x", "y", "--synthetic", "200", "--ctf-train", os.path.join(cwd, "tr.txt"), "--ctf-test", os.path.join(cwd, "te.txt"),
             "--num-epochs", "1", "--minibatch-size", "64", "--p-hidden-dim", "32", "--q-hidden-dim", "32", "-z", "3",
             "--checkpoint-interval", "1", "--seed", "4", "--progress-every", "0", "--save-prefix", "pp"]
    _run(["train_particles.py"] + train, cwd)
    state = os.path.join(cwd, "pp_state_epoch1.ckpt")
    images, n, m, n_classes = 50, 40, 40, 3
    label = np.random.RandomState(2).randint(-1, n_classes, size=images)
    label[:4] = [0, 1, 2, -1]
    np.save(os.path.join(cwd, "l.npy"), label)
    common = ["infer.py", "particles", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1",
              "--ctf_correct", "wiener", "--labels", "l.npy", "--wiener_lambda", "0.5"]
    _run(common + ["--out", "t0.npz", "--class_averages", "w0.npz"], cwd)
    _run(common + ["--out", "t.npz", "--class_averages", "w.npz", "--frc"], cwd)
    t0, t = _npz(os.path.join(cwd, "t0.npz")), _npz(os.path.join(cwd, "t.npz"))
    _bit_equal(t0, t, [k for k in t0 if k != "meta"])
    meta = json.loads(str(t["meta"]))
    assert (meta["frc"], meta["frc_mask_radius"], meta["frc_mask_edge"]) == (True, 17.0, 3.0) and "frc" not in json.loads(str(t0["meta"]))
    w0, w = _npz(os.path.join(cwd, "w0.npz")), _npz(os.path.join(cwd, "w.npz"))
    wiener = ["wiener_average", "wiener_den", "wiener_lambda", "wiener_sum"]
    assert sorted(w0) == sorted(PLAIN_KEYS + wiener) and sorted(w) == sorted(PLAIN_KEYS + wiener + FRC_KEYS)
    _bit_equal(w0, w, PLAIN_KEYS + wiener)
    assert w["half_sum"].shape == (n_classes, 2, n, m, 1)
    assert np.abs(w["half_sum"][:, 0] + w["half_sum"][:, 1] - w["wiener_sum"]).max() <= 1e-12 * np.abs(w["wiener_sum"]).max()
    assert np.array_equal(w["half_count"][:, 0] + w["half_count"][:, 1], w["count"])
    errors = _check_frc_arrays(w, w["half_sum"], w["wiener_average"].astype(np.float64), label, 17.0, 3.0)
    print("particles wiener --frc against frc_ref: sums %.2e of the largest power, frc %.2e, filter %.2e of the plane maximum" % errors)
    assert errors[0] <= TOL_SUMS and errors[1] <= TOL_FRC and errors[2] <= TOL_FILTER

    _run(common + ["--out", "t.npz", "--class_averages", "w.npz", "--frc"], cwd)
    _bit_equal(t, _npz(os.path.join(cwd, "t.npz")))
    _bit_equal(w, _npz(os.path.join(cwd, "w.npz")))
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]
