"""infer.py --ctf_correct end to end on the MI355X: train a small particle model on CTF tables with the command line, apply it
without the option, with flip and with wiener, read the files back and hold them to tests/ctfcorr_ref.py and tests/align_ref.py
at the poses the same run reports.  Each subprocess runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from align_ref import align_ref, near_threshold, source_positions
from ctfcorr_ref import apply_ref, finish_ref, power_ref, random_table, transfer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
TOL = 2e-6


def _run(args, cwd, code=0):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, args[0])] + args[1:], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=LIMIT)
    assert out.returncode == code, out.stdout[-1500:] + out.stderr[-3000:]
    return out


def _npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_particles_flip_and_wiener(tmp_path):
    """train_particles.py --synthetic 200 with two CTF tables for one epoch (50 validation images of 40 x 40, H = 32), then
    infer.py particles without the option, with flip and with wiener.  The score arrays of all runs are bit-equal and only the
    runs with the option carry ctf_correct / wiener_lambda in their meta.  flip: a.npy is align_ref(apply_ref(y, flip)) at the .npz's theta_iw / dx_iw within
    2^-23 |ref| + 1e-12 max |y| (the alignment kernel's bound) plus 2e-6 of the flipped plane's maximum (the Fourier step), and
    c.npz sums a.npy by label.  wiener: sum / count / average / members are the uncorrected run's bit for bit; wiener_den is
    power_ref to 1e-10; wiener_sum is numpy's sum by label of align_ref(apply_ref(y, multiply)) to 1e-6 of its maximum;
    wiener_average is finish_ref(wiener_sum, wiener_den, 0.5) to 2e-6.  A second identical run of each gives bit-equal files and
    no .tmp file remains; a table shorter than the split exits 2 and leaves nothing.  MI355X: holds; a.npy,
    wiener_sum and wiener_average equal their references in every element, wiener_den is 6.4e-15 from its own."""
    import torch
    import train_particles
    cwd = str(tmp_path)
    tables = {"tr.txt": random_table(200, 40), "te.txt": random_table(50, 41)}
    for name, t in tables.items():
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
    common = ["infer.py", "particles", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "20", "--seed", "1"]
    _run(common + ["--out", "p.npz", "--aligned", "a0.npy", "--class_averages", "c0.npz", "--labels", "l.npy"], cwd)
    flip = ["--ctf_correct", "flip", "--aligned", "a.npy", "--class_averages", "c.npz", "--labels", "l.npy"]
    wien = ["--ctf_correct", "wiener", "--class_averages", "w.npz", "--labels", "l.npy", "--wiener_lambda", "0.5"]
    _run(common + ["--out", "s.npz"] + flip, cwd)
    _run(common + ["--out", "t.npz"] + wien, cwd)
    p, s, t = (_npz(os.path.join(cwd, k)) for k in ("p.npz", "s.npz", "t.npz"))
    for other in (s, t):
        assert sorted(other) == sorted(p) and all(np.array_equal(p[k], other[k]) for k in p if k != "meta")
    metas = {k: json.loads(str(v["meta"])) for k, v in (("p", p), ("s", s), ("t", t))}
    assert "ctf_correct" not in metas["p"] and "wiener_lambda" not in metas["p"]
    assert (metas["s"]["ctf_correct"], metas["s"]["wiener_lambda"]) == ("flip", None)
    assert (metas["t"]["ctf_correct"], metas["t"]["wiener_lambda"]) == ("wiener", 0.5)
    assert set(metas["s"]) - set(metas["p"]) == set(metas["t"]) - set(metas["p"]) == {"ctf_correct", "wiener_lambda"}

    cfg = train_particles.build(train_particles.particle_arguments(train), torch.device("cuda:0"))      # the split, as infer.infer_main has it
    y = cfg["y_test"].numpy()
    table, scale = cfg["ctf_params_test"], cfg["ctf_scale"]
    assert np.array_equal(table, tables["te.txt"]) and scale == 1.0 and y.shape == (images, n * m)
    H, u = transfer(table, n, m, scale)
    assert np.abs(u).min() >= 1e-9                  # no flip depends on the last bit of u
    theta, dx = s["theta_iw"], s["dx_iw"]
    fx, fy = source_positions(theta, dx, images, n, m)
    assert int(near_threshold(fx, fy, n, m).sum()) == 0

    # flip: --aligned and the class averages hold phase-flipped particles
    a = np.load(os.path.join(cwd, "a.npy"))
    flipped = apply_ref(y, table, n, m, scale, "flip").reshape(images, n * m)
    ref, cover = align_ref(flipped, theta, dx, n, m, "bicubic")
    assert a.shape == (images, n, m, 1) and a.dtype == np.float32 and 0 < cover.sum() < cover.size
    got, want = a.reshape(images, -1).astype(np.float64), ref.reshape(images, -1).astype(np.float64)
    bound = 2.0 ** -23 * np.abs(want) + 1e-12 * np.abs(y).max() + TOL * np.abs(flipped).max(1, keepdims=True)
    print("a.npy against align_ref(apply_ref(flip)): max |out - ref| %.3e of the plane maximum"
          % (np.abs(got - want).max(1) / np.abs(flipped).max(1)).max())
    assert (np.abs(got - want) - bound).max() <= 0
    a0 = np.load(os.path.join(cwd, "a0.npy"))
    assert a0.shape == a.shape and not np.array_equal(a0, a)
    c, c0 = _npz(os.path.join(cwd, "c.npz")), _npz(os.path.join(cwd, "c0.npz"))
    assert sorted(c) == sorted(c0) == ["average", "count", "members", "sum"] and np.array_equal(c["count"], c0["count"])
    for k in range(n_classes):
        by_label = a[label == k].astype(np.float64).sum(0)
        assert np.abs(c["sum"][k] - by_label).max() <= 1e-12 * np.abs(by_label).max()

    # wiener: the plain arrays are untouched, the Wiener arrays are added
    w = _npz(os.path.join(cwd, "w.npz"))
    assert sorted(w) == sorted(list(c0) + ["wiener_average", "wiener_den", "wiener_lambda", "wiener_sum"])
    assert all(np.array_equal(w[k], c0[k]) and w[k].dtype == c0[k].dtype for k in c0)
    assert w["wiener_sum"].shape == (n_classes, n, m, 1) and w["wiener_sum"].dtype == np.float64
    assert w["wiener_den"].shape == (n_classes, n, m) and w["wiener_den"].dtype == np.float64
    assert w["wiener_average"].shape == (n_classes, n, m, 1) and w["wiener_average"].dtype == np.float32
    assert float(w["wiener_lambda"]) == 0.5
    den = power_ref([(table, label)], n_classes, n, m, scale)
    e_den = np.abs(w["wiener_den"] - den).max() / den.max()
    g, g_cover = align_ref(apply_ref(y, table, n, m, scale, "multiply").reshape(images, n * m), theta, dx, n, m, "bicubic")
    assert np.array_equal(g_cover, cover)
    by_label = np.stack([g[label == k].astype(np.float64).sum(0) for k in range(n_classes)]).reshape(n_classes, n, m, 1)
    e_sum = np.abs(w["wiener_sum"] - by_label).max() / np.abs(by_label).max()
    average = finish_ref(w["wiener_sum"], w["wiener_den"], 0.5, n, m).reshape(n_classes, n, m, 1)
    e_avg = np.abs(w["wiener_average"].astype(np.float64) - average).max() / np.abs(average).max()
    print("wiener_den %.2e, wiener_sum %.2e, wiener_average %.2e of their maxima from the references" % (e_den, e_sum, e_avg))
    assert e_den <= 1e-10 and e_sum <= 1e-6 and e_avg <= TOL

    # the same command lines again: the same bytes, and nothing temporary is left
    _run(common + ["--out", "s2.npz", "--ctf_correct", "flip", "--aligned", "a2.npy", "--class_averages", "c2.npz", "--labels", "l.npy"], cwd)
    _run(common + ["--out", "t2.npz", "--ctf_correct", "wiener", "--class_averages", "w2.npz", "--labels", "l.npy", "--wiener_lambda", "0.5"],
         cwd)
    assert _bytes(os.path.join(cwd, "a2.npy")) == _bytes(os.path.join(cwd, "a.npy"))
    c2, w2 = _npz(os.path.join(cwd, "c2.npz")), _npz(os.path.join(cwd, "w2.npz"))
    assert sorted(c2) == sorted(c) and all(np.array_equal(c[k], c2[k]) for k in c)
    assert sorted(w2) == sorted(w) and all(np.array_equal(w[k], w2[k]) for k in w)
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    # a table shorter than the split: refused before anything is written
    np.savetxt(os.path.join(cwd, "short.txt"), tables["te.txt"][:-1])
    before = sorted(os.listdir(cwd))
    out = _run(common + ["--out", "s5.npz", "--ctf_test", os.path.join(cwd, "short.txt")] + flip[:2] + ["--aligned", "a5.npy"], cwd, code=2)
    assert "49 rows" in out.stderr and sorted(os.listdir(cwd)) == before


def test_no_table_is_refused(tmp_path):
    """A particle run trained without CTF tables has nothing to correct by: --ctf_correct exits 2 with the reason and writes
    nothing.  MI355X: holds."""
    cwd = str(tmp_path)
    _run(["train_particles.py", "x", "y", "--synthetic", "40", "--num-epochs", "1", "--minibatch-size", "32", "--p-hidden-dim", "16",
          "--q-hidden-dim", "16", "--checkpoint-interval", "1", "--seed", "4", "--progress-every", "0", "--save-prefix", "pp"], cwd)
    before = sorted(os.listdir(cwd))
    out = _run(["infer.py", "particles", "--state", os.path.join(cwd, "pp_state_epoch1.ckpt"), "--num_samples", "2", "--out", "s.npz",
                "--ctf_correct", "wiener", "--class_averages", "w.npz"], cwd, code=2)
    assert "no --ctf-test table" in out.stderr and sorted(os.listdir(cwd)) == before
