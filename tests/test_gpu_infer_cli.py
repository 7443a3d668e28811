"""infer.py end to end on the MI355X: train a small model with the command line, apply it to the dataset, read the .npz.
Each subprocess runs under its own timeout."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
TOL = 2e-5


def _run(script, args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=LIMIT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return out.stdout


def _npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_mnist_state_file_and_sav_pair(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images), then infer.py on the state file with K = 8 in
    chunks of 3 and minibatches of 50: every array with its shape (theta_* and dx_* present), all finite, 1 <= ess <= 8, index
    = arange, meta's means = the arrays' means = the printed line; a second identical run gives bit-equal arrays; the .sav pair
    of the same run with the training flags after `--` gives the same bound to 2e-5; --split train scores the 200 training
    images.  MI355X: holds; the .sav pair's bound equals the state file's bit for bit."""
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run("train_mnist.py", train, cwd)
    trained = os.path.join(cwd, "outputs_run", "trained")
    state = os.path.join(trained, "run_state_epoch1.ckpt")
    sav = {t: [os.path.join(trained, f) for f in os.listdir(trained) if f.endswith(".sav") and "_%s_" % t in f] for t in ("generator", "inference")}
    assert os.path.isfile(state) and len(sav["generator"]) == 1 and len(sav["inference"]) == 1
    common = ["--num_samples", "8", "--chunk", "3", "--minibatch_size", "50", "--seed", "1"]
    printed = _run("infer.py", ["mnist", "--state", state, "--out", "s.npz"] + common, cwd)
    a = _npz(os.path.join(cwd, "s.npz"))
    n, z = 50, 2
    shapes = {"bound": (n,), "loglik": (n,), "kl": (n,), "ess": (n,), "index": (n,), "meta": (),
              "theta_q": (n,), "theta_q_std": (n,), "theta_iw": (n,), "theta_R": (n,), "theta_best": (n,),
              "dx_q": (n, 2), "dx_q_std": (n, 2), "dx_iw": (n, 2), "dx_best": (n, 2),
              "z_q": (n, z), "z_q_std": (n, z), "z_iw": (n, z), "z_best": (n, z)}
    assert {k: v.shape for k, v in a.items()} == shapes
    for k, v in a.items():
        if k not in ("meta", "index"):
            assert v.dtype == np.float32 and np.isfinite(v).all(), k
    assert (a["ess"] >= 1 - 1e-6).all() and (a["ess"] <= 8 * (1 + 1e-6)).all()
    assert (a["theta_R"] > 0).all() and (a["theta_R"] <= 1 + 1e-6).all() and (a["theta_q_std"] > 0).all()
    assert np.array_equal(a["index"], np.arange(n))
    meta = json.loads(str(a["meta"]))
    assert (meta["script"], meta["num_samples"], meta["chunk"], meta["seed"], meta["split"]) == ("mnist", 8, 3, 1, "test")
    assert meta["state"] == state and meta["images"] == n
    means = [float(np.mean(a[k], dtype=np.float64)) for k in ("bound", "loglik", "kl")]
    assert [meta["mean_bound"], meta["mean_loglik"], meta["mean_kl"]] == means
    line = [l for l in printed.splitlines() if l.startswith("images ")]
    assert len(line) == 1
    nums = [float(v) for v in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", line[0])]
    assert line[0].startswith("images %d\t" % n) and nums[:3] == means and abs(nums[3] - float(np.median(a["ess"]))) <= 1e-3
    print(line[0])
    _run("infer.py", ["mnist", "--state", state, "--out", "s2.npz"] + common, cwd)
    b = _npz(os.path.join(cwd, "s2.npz"))
    assert all(np.array_equal(a[k], b[k]) for k in a if k != "meta") and sorted(a) == sorted(b)
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]
    _run("infer.py", ["mnist", "--generator", sav["generator"][0], "--inference", sav["inference"][0], "--out", "s3.npz"] + common
         + ["--"] + train, cwd)
    c = _npz(os.path.join(cwd, "s3.npz"))
    err = np.abs(c["bound"].astype(np.float64) - a["bound"]).max() / np.abs(a["bound"]).max()
    print("state file against .sav pair: bound differs by %.2e" % err)
    assert err <= TOL
    _run("infer.py", ["mnist", "--state", state, "--out", "s4.npz", "--split", "train"] + common, cwd)
    assert _npz(os.path.join(cwd, "s4.npz"))["bound"].shape == (200,)


def test_particles_without_translation(tmp_path):
    """train_particles.py --synthetic 60 --no-translate --mask, then infer.py particles: theta_* keys, no dx_* key, z arrays of
    the model's z-dim, everything finite.  A state file read under another script's name is refused with exit code 2.
    MI355X: holds."""
    cwd = str(tmp_path)
    _run("train_particles.py", ["x", "y", "--synthetic", "60", "--no-translate", "--mask", "--num-epochs", "1", "--minibatch-size", "32",
                                "--p-hidden-dim", "32", "--q-hidden-dim", "32", "-z", "3", "--checkpoint-interval", "1", "--seed", "4",
                                "--progress-every", "0", "--save-prefix", "pp"], cwd)
    state = os.path.join(cwd, "pp_state_epoch1.ckpt")
    assert os.path.isfile(state)
    _run("infer.py", ["particles", "--state", state, "--out", "p.npz", "--num_samples", "5", "--chunk", "2", "--minibatch_size", "8"], cwd)
    a = _npz(os.path.join(cwd, "p.npz"))
    assert all(k in a for k in ("theta_q", "theta_q_std", "theta_iw", "theta_R", "theta_best")) and not [k for k in a if k.startswith("dx_")]
    assert a["bound"].shape == (15,) and a["z_iw"].shape == (15, 3) and a["z_best"].shape == (15, 3)
    assert all(np.isfinite(v).all() for k, v in a.items() if k != "meta")
    assert (a["ess"] >= 1 - 1e-6).all() and (a["ess"] <= 5 * (1 + 1e-6)).all()
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "mnist", "--state", state, "--out", "q.npz"], cwd=cwd, env=env,
                         capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 2 and "not written by train_mnist.py" in out.stderr and not os.path.exists(os.path.join(cwd, "q.npz"))
