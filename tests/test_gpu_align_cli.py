"""infer.py's image outputs end to end on the MI355X: --aligned, --recon, --class_averages / --labels, --pose, --interp.  Train a
small model with the command line, apply it, read the files back and hold them to tests/align_ref.py at the poses the same run
reports.  Each subprocess runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from align_ref import align_ref, near_threshold, source_positions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
TOL = 2e-5


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


def _within_kernel_bound(out, ref, y, what):
    out, ref = out.astype(np.float64), ref.astype(np.float64)
    excess = np.abs(out - ref) - (2.0 ** -23 * np.abs(ref) + 1e-12 * np.abs(y).max())
    print("%s: max |out - ref| %.3e, %d of %d elements differ" % (what, np.abs(out - ref).max(), int((out != ref).sum()), out.size))
    assert excess.max() <= 0


def test_mnist_aligned_recon_and_class_averages(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64), then infer.py with and without the image
    outputs: the score arrays of the two runs are bit-equal and only the run with the options has pose / interp / paths in its
    meta; a.npy is align_ref of the split's images at the .npz's theta_iw / dx_iw within the kernel's bound; r.npy is the un-posed
    decoder at z_iw to 2e-5 of the largest value; c.npz's sum / count / members are numpy's sums of a.npy by label (sum to 1e-12
    relative) and its average their quotient; a second identical run gives bit-equal files and no .tmp file remains; --pose best
    changes a.npy; a labels file of the wrong length exits 2 and leaves nothing.  MI355X: holds; a.npy equals the reference in
    every element and r.npy is 1.1e-7 of the largest value from the in-process decoder."""
    import torch
    import train_mnist
    from spatial_vae_amd import cli
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _infer(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    n, rows, cols = 50, 28, 28
    label = np.random.RandomState(2).randint(-1, 3, size=n)
    np.save(os.path.join(cwd, "l.npy"), label)
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "8", "--chunk", "3", "--minibatch_size", "20", "--seed", "1"]
    _infer(common + ["--out", "plain.npz"], cwd)
    outputs = ["--aligned", "a.npy", "--recon", "r.npy", "--labels", "l.npy", "--class_averages", "c.npz"]
    _infer(common + ["--out", "s.npz"] + outputs, cwd)
    plain, s = _npz(os.path.join(cwd, "plain.npz")), _npz(os.path.join(cwd, "s.npz"))
    assert sorted(plain) == sorted(s) and all(np.array_equal(plain[k], s[k]) for k in s if k != "meta")
    meta, meta_plain = json.loads(str(s["meta"])), json.loads(str(plain["meta"]))
    added = {"pose": "iw", "interp": "bicubic", "aligned": "a.npy", "recon": "r.npy", "class_averages": "c.npz", "labels": "l.npy"}
    assert {k: meta[k] for k in added} == added and dict(meta_plain, **added) == meta

    a, r, c = np.load(os.path.join(cwd, "a.npy")), np.load(os.path.join(cwd, "r.npy")), _npz(os.path.join(cwd, "c.npz"))
    assert a.shape == r.shape == (n, rows, cols, 1) and a.dtype == r.dtype == np.float32
    targs = train_mnist.mnist_arguments(train)
    cfg = train_mnist.build(targs, torch.device("cpu"))             # the split, as infer.infer_main obtains it
    y = cfg["y_test"].numpy()
    fx, fy = source_positions(s["theta_iw"], s["dx_iw"], n, rows, cols)
    assert int(near_threshold(fx, fy, rows, cols).sum()) == 0
    ref, cover = align_ref(y, s["theta_iw"], s["dx_iw"], rows, cols, "bicubic")
    assert 0 < cover.sum() < cover.size
    _within_kernel_bound(a.reshape(n, -1), ref.reshape(n, -1), y, "a.npy against align_ref at theta_iw / dx_iw")

    dev = torch.device("cuda:0")
    p_net = cfg["p_net"]
    p_net.load_state_dict(cli.read_checkpoint(state)["train_step"]["p_net"])
    p_net = p_net.to(dev).eval()
    mine = E.reconstruct_unposed(cli.coord_grid(rows, cols).to(dev), p_net, n, torch.from_numpy(s["z_iw"]).to(dev)).cpu().numpy()
    err = np.abs(mine.reshape(n, -1).astype(np.float64) - r.reshape(n, -1)).max() / np.abs(mine).max()
    print("r.npy against the un-posed decoder at z_iw: %.2e of the largest value" % err)
    assert err <= TOL

    n_classes = 3
    assert c["sum"].shape == (n_classes, rows, cols, 1) and c["count"].shape == (n_classes, rows, cols) and c["average"].shape == c["sum"].shape
    assert (c["sum"].dtype, c["count"].dtype, c["average"].dtype, c["members"].dtype) == (np.float64, np.float64, np.float32, np.int64)
    for k in range(n_classes):
        want = a[label == k].astype(np.float64).sum(0)
        assert np.abs(c["sum"][k] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(c["count"][k], cover[label == k].astype(np.float64).sum(0).reshape(rows, cols))
    assert np.array_equal(c["members"], np.bincount(label[label >= 0], minlength=n_classes))
    on = c["count"] > 0
    assert on.any() and np.array_equal(c["average"][on], (c["sum"][on] / c["count"][on][..., None]).astype(np.float32))
    assert (c["average"][~on] == 0).all()

    _infer(common + ["--out", "s2.npz"] + ["--aligned", "a2.npy", "--recon", "r2.npy", "--labels", "l.npy", "--class_averages", "c2.npz"], cwd)
    assert _bytes(os.path.join(cwd, "a2.npy")) == _bytes(os.path.join(cwd, "a.npy"))
    assert _bytes(os.path.join(cwd, "r2.npy")) == _bytes(os.path.join(cwd, "r.npy"))
    c2 = _npz(os.path.join(cwd, "c2.npz"))
    assert sorted(c2) == sorted(c) == ["average", "count", "members", "sum"] and all(np.array_equal(c[k], c2[k]) for k in c)
    _infer(common + ["--out", "s3.npz", "--aligned", "a3.npy", "--pose", "best", "--class_averages", "c3.npz"], cwd)
    a3, c3 = np.load(os.path.join(cwd, "a3.npy")), _npz(os.path.join(cwd, "c3.npz"))
    assert a3.shape == a.shape and not np.array_equal(a3, a)
    best, _ = align_ref(y, s["theta_best"], s["dx_best"], rows, cols, "bicubic")
    _within_kernel_bound(a3.reshape(n, -1), best.reshape(n, -1), y, "--pose best against align_ref at theta_best / dx_best")
    assert c3["sum"].shape == (1, rows, cols, 1) and c3["members"].tolist() == [n]        # no --labels: one class of all images
    assert np.abs(c3["sum"][0] - a3.astype(np.float64).sum(0)).max() <= 1e-12 * np.abs(c3["sum"]).max()
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    np.save(os.path.join(cwd, "short.npy"), label[:-1])
    before = sorted(os.listdir(cwd))
    out = _infer(common + ["--out", "s4.npz", "--aligned", "a4.npy", "--labels", "short.npy", "--class_averages", "c4.npz"], cwd, code=2)
    assert "49 entries" in out.stderr and sorted(os.listdir(cwd)) == before


def test_particles_mrcs_stacks(tmp_path):
    """train_particles.py --synthetic 60 --no-translate (one channel, 40x40, 15 validation images), then infer.py particles writing
    --aligned / --recon once as .mrcs and once as .npy: mrc.read returns what the .npy holds, bit for bit; the class averages of
    the run without --labels count every image.  MI355X: holds."""
    from spatial_vae_amd import mrc
    cwd = str(tmp_path)
    _infer(["train_particles.py", "x", "y", "--synthetic", "60", "--no-translate", "--num-epochs", "1", "--minibatch-size", "32",
            "--p-hidden-dim", "32", "--q-hidden-dim", "32", "-z", "3", "--checkpoint-interval", "1", "--seed", "4", "--progress-every", "0",
            "--save-prefix", "pp"], cwd)
    common = ["infer.py", "particles", "--state", os.path.join(cwd, "pp_state_epoch1.ckpt"), "--num_samples", "5", "--chunk", "2",
              "--minibatch_size", "8", "--interp", "bilinear"]
    _infer(common + ["--out", "p.npz", "--aligned", "a.mrcs", "--recon", "r.mrcs", "--class_averages", "c.npz"], cwd)
    _infer(common + ["--out", "q.npz", "--aligned", "a.npy", "--recon", "r.npy"], cwd)
    for name in ("a", "r"):
        stack, header, _ = mrc.read(os.path.join(cwd, name + ".mrcs"))
        plain = np.load(os.path.join(cwd, name + ".npy"))
        assert plain.shape == (15, 40, 40, 1) and (header.nx, header.ny, header.nz) == (40, 40, 15)
        assert np.array_equal(np.asarray(stack), plain[..., 0]) and np.isfinite(plain).all()
    c = _npz(os.path.join(cwd, "c.npz"))
    assert c["members"].tolist() == [15] and c["count"].max() == 15 and c["count"].min() >= 0
    assert json.loads(str(_npz(os.path.join(cwd, "p.npz"))["meta"]))["interp"] == "bilinear"
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]
