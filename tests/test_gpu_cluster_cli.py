"""infer.py --cluster end to end on the MI355X: train a small model with the command line, apply it with and without the
option, read the files back and hold them to float64 numpy on the latents the same run reports.  Each subprocess runs under its
own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
TOL = 2e-5          # tests/test_gpu_align_cli.py's bound for a reconstruction against the in-process decoder


def _infer(args, cwd, code=0):
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


def test_mnist_cluster_labels_centres_and_class_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py plain and with
    --cluster 3 --cluster_out k.npz --cluster_labels l.npy --class_averages c.npz: the score arrays of the two runs are bit-equal
    and only meta differs; l.npy is k.npz's label, which is the float64 argmin of z_iw against the centres on every point whose
    relative best/second gap is >= 1e-9 (at most 2 % may fall under it); if the run converged, the centres are the member means
    to 1e-12 (1 + |c|) and the inertia matches to 1e-12 relative; a third run with --labels l.npy gives bit-equal sum, count,
    average and members; centre_recon is the in-process un-posed decoder at the float centres to 2e-5 of the largest value; a
    repeated run gives byte-equal arrays in every file (and a byte-equal l.npy) and leaves no .tmp file; --cluster with --labels and --cluster 500 on 50 images exit 2 and
    write nothing."""
    import torch
    import train_mnist
    from spatial_vae_amd import cli
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _infer(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    n, rows, cols, k = 50, 28, 28, 3
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "8", "--chunk", "3", "--minibatch_size", "20", "--seed", "1"]
    _infer(common + ["--out", "plain.npz"], cwd)
    clustered = ["--cluster", str(k), "--cluster_out", "k.npz", "--cluster_labels", "l.npy", "--class_averages", "c.npz"]
    _infer(common + ["--out", "s.npz"] + clustered, cwd)
    plain, s = _npz(os.path.join(cwd, "plain.npz")), _npz(os.path.join(cwd, "s.npz"))
    assert sorted(plain) == sorted(s) and all(np.array_equal(plain[key], s[key]) for key in s if key != "meta")
    meta, meta_plain = json.loads(str(s["meta"])), json.loads(str(plain["meta"]))
    added = {"pose": "iw", "interp": "bicubic", "labels": None, "aligned": None, "recon": None, "class_averages": "c.npz", "cluster": k,
             "cluster_out": "k.npz", "cluster_labels": "l.npy", "cluster_iters": 100, "cluster_restarts": 1, "cluster_seed": 1}
    assert dict(meta_plain, **added) == meta

    found, label = _npz(os.path.join(cwd, "k.npz")), np.load(os.path.join(cwd, "l.npy"))
    assert sorted(found) == ["centre_recon", "centres", "chosen_restart", "converged_at", "inertia", "iterations", "label", "members", "meta",
                             "restart_inertia", "seed_index"]
    assert label.dtype == found["label"].dtype == np.int64 and np.array_equal(label, found["label"]) and label.shape == (n,)
    assert json.loads(str(found["meta"])) == meta
    centres, z = found["centres"], s["z_iw"].astype(np.float64)
    assert centres.shape == (k, 3) and centres.dtype == np.float64 and found["members"].dtype == np.int64
    dist = ((z[:, None, :] - centres[None]) ** 2).sum(2)
    order = np.sort(dist, 1)
    clear = (order[:, 1] - order[:, 0]) >= 1e-9 * order[:, 1]
    print("points under the 1e-9 gap: %d of %d; converged_at %d; members %s" % (int((~clear).sum()), n, int(found["converged_at"]),
                                                                                found["members"].tolist()))
    assert (~clear).sum() <= 0.02 * n
    assert np.array_equal(label[clear], dist.argmin(1)[clear]) and label.min() >= 0
    assert np.array_equal(found["members"], np.bincount(label, minlength=k))
    assert found["iterations"] == 100 and found["chosen_restart"] == 0 and found["restart_inertia"].shape == (1,)
    assert found["restart_inertia"][0] == found["inertia"]
    assert found["seed_index"].shape == (k,) and (0 <= found["seed_index"]).all() and (found["seed_index"] < n).all()
    if found["converged_at"] > 0:
        for j in range(k):
            if found["members"][j]:
                mean = z[label == j].mean(0)
                assert (np.abs(centres[j] - mean) <= 1e-12 * (1 + np.abs(centres[j]))).all(), j
    inertia = dist[np.arange(n), label].sum()
    assert abs(found["inertia"] - inertia) <= 1e-12 * inertia

    c = _npz(os.path.join(cwd, "c.npz"))
    _infer(common + ["--out", "s3.npz", "--labels", "l.npy", "--class_averages", "c3.npz"], cwd)
    c3 = _npz(os.path.join(cwd, "c3.npz"))
    assert sorted(c) == sorted(c3) == ["average", "count", "members", "sum"]
    for key in c:
        assert c[key].shape == c3[key].shape and np.array_equal(c[key].view(np.uint8), c3[key].view(np.uint8)), key
    assert c["sum"].shape == (k, rows, cols, 1) and np.array_equal(c["members"], found["members"])

    targs = train_mnist.mnist_arguments(train)
    cfg = train_mnist.build(targs, torch.device("cpu"))
    dev = torch.device("cuda:0")
    p_net = cfg["p_net"]
    p_net.load_state_dict(cli.read_checkpoint(state)["train_step"]["p_net"])
    p_net = p_net.to(dev).eval()
    zc = torch.from_numpy(centres.astype(np.float32)).to(dev)
    mine = E.reconstruct_unposed(cli.coord_grid(rows, cols).to(dev), p_net, k, zc).cpu().numpy()
    recon = found["centre_recon"]
    assert recon.shape == (k, rows, cols, 1) and recon.dtype == np.float32
    err = np.abs(mine.reshape(k, -1).astype(np.float64) - recon.reshape(k, -1)).max() / np.abs(mine).max()
    print("centre_recon against the un-posed decoder at the float centres: %.2e of the largest value" % err)
    assert err <= TOL

    l_bytes = _bytes(os.path.join(cwd, "l.npy"))
    _infer(common + ["--out", "s.npz"] + clustered, cwd)                                   # the same command again, over its own files
    assert _bytes(os.path.join(cwd, "l.npy")) == l_bytes
    for name, first in (("s.npz", s), ("k.npz", found), ("c.npz", c)):                      # (a .npz carries the time it was written)
        again = _npz(os.path.join(cwd, name))
        assert sorted(again) == sorted(first), name
        for key in first:
            assert again[key].dtype == first[key].dtype and again[key].tobytes() == first[key].tobytes(), (name, key)
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    before = sorted(os.listdir(cwd))
    out = _infer(common + ["--out", "s4.npz", "--cluster", "3", "--cluster_out", "k4.npz", "--class_averages", "c4.npz", "--labels", "l.npy"],
                 cwd, code=2)
    assert "excludes --labels" in out.stderr
    out = _infer(common + ["--out", "s5.npz", "--cluster", "500", "--cluster_out", "k5.npz"], cwd, code=2)
    assert "exceeds the 50 images" in out.stderr and sorted(os.listdir(cwd)) == before


def test_models_without_usable_content_latents_are_refused(tmp_path):
    """Two states whose content latents cannot be clustered, each refused with exit code 2 before anything is written: an MNIST
    model trained with --z_dim 0 (it has none), and a particle model saved after 1 of --z-delay 5 epochs (z_scale is still 0,
    so every content latent is 0)."""
    cwd = str(tmp_path)
    _infer(["train_mnist.py", "--synthetic", "100", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "32", "--q_hidden_dim",
            "32", "--z_dim", "0", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "z0"], cwd)
    _infer(["train_particles.py", "x", "y", "--synthetic", "60", "--no-translate", "--num-epochs", "1", "--minibatch-size", "32",
            "--p-hidden-dim", "32", "--q-hidden-dim", "32", "-z", "3", "--z-delay", "5", "--checkpoint-interval", "1", "--seed", "4",
            "--progress-every", "0", "--save-prefix", "pp"], cwd)
    before = sorted(os.listdir(cwd))
    tail = ["--num_samples", "4", "--out", "s.npz", "--cluster", "2", "--cluster_out", "k.npz"]
    out = _infer(["infer.py", "mnist", "--state", os.path.join(cwd, "outputs_z0", "trained", "z0_state_epoch1.ckpt")] + tail, cwd, code=2)
    assert "has none" in out.stderr
    out = _infer(["infer.py", "particles", "--state", os.path.join(cwd, "pp_state_epoch1.ckpt")] + tail, cwd, code=2)
    assert "z_scale = 0" in out.stderr and sorted(os.listdir(cwd)) == before
