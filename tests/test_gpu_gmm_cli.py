"""infer.py --cluster_gmm end to end on the MI355X: train a small model with the command line, apply it with --cluster alone
and with the mixture on top, read the files back and hold them to each other and to float64 numpy on the arrays the same run
reports.  Each subprocess runs under its own timeout."""
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
GMM_KEYS = {"gmm_weight", "gmm_mean", "gmm_var", "gmm_resp", "gmm_max_resp", "gmm_label", "gmm_label_used", "gmm_members",
            "gmm_loglik_point", "gmm_loglik", "gmm_loglik_trace", "gmm_iterations", "gmm_converged_at", "gmm_dead", "gmm_bic", "gmm_aic",
            "gmm_mean_recon"}


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


def test_mnist_mixture_on_top_of_the_kmeans_classes(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3), then infer.py --cluster 3 with its
    files in one folder and the same with --cluster_gmm 20 in another: every array the first run wrote to scores.npz and k.npz is
    byte-equal in the second and meta differs by exactly the four added keys; the gmm_* arrays are present with their shapes
    and dtypes; the rows of gmm_resp sum to 1 within 1e-12; gmm_label is the argmax of gmm_resp wherever the top two differ by
    >= 1e-9 (at most 2 % may fall under it); gmm_members is the bincount of gmm_label_used, which is also l.npy and the members of
    the class averages; BIC and AIC follow from gmm_loglik, gmm_dead and the sizes; gmm_mean_recon is the in-process un-posed
    decoder at the float means to 2e-5 of the largest value; a later run with --labels l.npy gives bit-equal sum, count, average
    and members; a repeated run gives byte-equal files and leaves no .tmp file.  With --cluster_min_resp 0.999 gmm_label_used
    is -1 exactly where gmm_max_resp < 0.999 and those images are in no class count.  The refusals exit 2 and write nothing."""
    import torch
    import train_mnist
    from spatial_vae_amd import cli
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _infer(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    n, rows, cols, k, D = 50, 28, 28, 3, 3
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "8", "--chunk", "3", "--minibatch_size", "20", "--seed", "1"]
    clustered = ["--out", "s.npz", "--cluster", str(k), "--cluster_out", "k.npz", "--cluster_labels", "l.npy", "--class_averages", "c.npz"]
    folders = {name: os.path.join(cwd, name) for name in ("kmeans", "gmm", "junk")}
    for path in folders.values():
        os.mkdir(path)
    _infer(common + clustered, folders["kmeans"])
    _infer(common + clustered + ["--cluster_gmm", "20"], folders["gmm"])
    added = {"cluster_gmm": 20, "cluster_gmm_reg": 1e-6, "cluster_gmm_tol": 1e-8, "cluster_min_resp": 0.0}
    for name in ("s.npz", "k.npz"):
        first, second = _npz(os.path.join(folders["kmeans"], name)), _npz(os.path.join(folders["gmm"], name))
        assert set(second) - set(first) == (GMM_KEYS if name == "k.npz" else set()) and set(first) <= set(second)
        for key in first:
            if key != "meta":
                assert first[key].dtype == second[key].dtype and first[key].tobytes() == second[key].tobytes(), (name, key)
        assert dict(json.loads(str(first["meta"])), **added) == json.loads(str(second["meta"])), name
    found = second
    s = _npz(os.path.join(folders["gmm"], "s.npz"))

    shapes = {"gmm_weight": ((k,), np.float64), "gmm_mean": ((k, D), np.float64), "gmm_var": ((k, D), np.float64),
              "gmm_resp": ((n, k), np.float64), "gmm_max_resp": ((n,), np.float64), "gmm_label": ((n,), np.int64),
              "gmm_label_used": ((n,), np.int64), "gmm_members": ((k,), np.int64), "gmm_loglik_point": ((n,), np.float64),
              "gmm_loglik": ((), np.float64), "gmm_loglik_trace": ((21,), np.float64), "gmm_iterations": ((), np.int64),
              "gmm_converged_at": ((), np.int64), "gmm_dead": ((), np.int64), "gmm_bic": ((), np.float64), "gmm_aic": ((), np.float64),
              "gmm_mean_recon": ((k, rows, cols, 1), np.float32)}
    assert set(shapes) == GMM_KEYS
    for key, (shape, dtype) in shapes.items():
        assert found[key].shape == shape and found[key].dtype == dtype, (key, found[key].shape, found[key].dtype)
    resp = found["gmm_resp"]
    assert np.abs(resp.sum(1) - 1).max() <= 1e-12 and (resp >= 0).all()
    order = np.sort(resp, 1)
    clear = order[:, -1] - order[:, -2] >= 1e-9
    print("points under the 1e-9 gap: %d of %d; iterations %d, converged_at %d, dead %d; members %s; max_resp below 0.999: %d"
          % (int((~clear).sum()), n, int(found["gmm_iterations"]), int(found["gmm_converged_at"]), int(found["gmm_dead"]),
             found["gmm_members"].tolist(), int((found["gmm_max_resp"] < 0.999).sum())))
    assert (~clear).sum() <= 0.02 * n
    assert np.array_equal(found["gmm_label"][clear], resp.argmax(1)[clear]) and found["gmm_label"].min() >= 0
    assert np.array_equal(found["gmm_max_resp"], resp.max(1))
    assert np.array_equal(found["gmm_label_used"], found["gmm_label"])                  # --cluster_min_resp 0: nobody leaves
    assert np.array_equal(found["gmm_members"], np.bincount(found["gmm_label_used"], minlength=k))
    label = np.load(os.path.join(folders["gmm"], "l.npy"))
    assert label.dtype == np.int64 and np.array_equal(label, found["gmm_label_used"])
    assert 1 <= found["gmm_iterations"] <= 20 and found["gmm_loglik"] == found["gmm_loglik_trace"][-1]
    assert abs(found["gmm_loglik"] - found["gmm_loglik_point"].sum()) <= 1e-12 * abs(found["gmm_loglik"])
    assert abs(found["gmm_weight"].sum() - 1) <= 1e-12 and (found["gmm_var"] >= 1e-6).all()
    live = k - int(found["gmm_dead"])
    p = (live - 1) + 2 * live * D
    L = float(found["gmm_loglik"])
    assert abs(found["gmm_bic"] - (-2.0 * L + p * np.log(n))) <= 1e-12 * abs(found["gmm_bic"])
    assert abs(found["gmm_aic"] - (-2.0 * L + 2.0 * p)) <= 1e-12 * abs(found["gmm_aic"])

    c = _npz(os.path.join(folders["gmm"], "c.npz"))
    assert np.array_equal(c["members"], found["gmm_members"]) and c["sum"].shape == (k, rows, cols, 1)
    _infer(common + ["--out", "s3.npz", "--labels", "l.npy", "--class_averages", "c3.npz"], folders["gmm"])
    c3 = _npz(os.path.join(folders["gmm"], "c3.npz"))
    assert sorted(c) == sorted(c3) == ["average", "count", "members", "sum"]
    for key in c:
        assert c[key].shape == c3[key].shape and np.array_equal(c[key].view(np.uint8), c3[key].view(np.uint8)), key

    targs = train_mnist.mnist_arguments(train)
    cfg = train_mnist.build(targs, torch.device("cpu"))
    dev = torch.device("cuda:0")
    p_net = cfg["p_net"]
    p_net.load_state_dict(cli.read_checkpoint(state)["train_step"]["p_net"])
    p_net = p_net.to(dev).eval()
    zc = torch.from_numpy(found["gmm_mean"].astype(np.float32)).to(dev)
    mine = E.reconstruct_unposed(cli.coord_grid(rows, cols).to(dev), p_net, k, zc).cpu().numpy()
    recon = found["gmm_mean_recon"]
    err = np.abs(mine.reshape(k, -1).astype(np.float64) - recon.reshape(k, -1)).max() / np.abs(mine).max()
    print("gmm_mean_recon against the un-posed decoder at the float means: %.2e of the largest value" % err)
    assert err <= TOL

    l_bytes = _bytes(os.path.join(folders["gmm"], "l.npy"))
    _infer(common + clustered + ["--cluster_gmm", "20"], folders["gmm"])                 # the same command again, over its own files
    assert _bytes(os.path.join(folders["gmm"], "l.npy")) == l_bytes
    for name, first in (("s.npz", s), ("k.npz", found), ("c.npz", c)):                  # (a .npz carries the time it was written)
        again = _npz(os.path.join(folders["gmm"], name))
        assert sorted(again) == sorted(first), name
        for key in first:
            assert again[key].dtype == first[key].dtype and again[key].tobytes() == first[key].tobytes(), (name, key)
    assert not [f for f in os.listdir(folders["gmm"]) if ".tmp" in f]

    _infer(common + clustered + ["--cluster_gmm", "20", "--cluster_min_resp", "0.999"], folders["junk"])
    junk, cj = _npz(os.path.join(folders["junk"], "k.npz")), _npz(os.path.join(folders["junk"], "c.npz"))
    for key in GMM_KEYS - {"gmm_label_used", "gmm_members"}:
        assert junk[key].tobytes() == found[key].tobytes(), key
    out_of_class = junk["gmm_max_resp"] < 0.999
    assert np.array_equal(junk["gmm_label_used"], np.where(out_of_class, -1, junk["gmm_label"]))
    kept = junk["gmm_label_used"][~out_of_class]
    assert np.array_equal(junk["gmm_members"], np.bincount(kept, minlength=k)) and np.array_equal(cj["members"], junk["gmm_members"])
    assert junk["gmm_members"].sum() == n - out_of_class.sum() and (cj["count"].reshape(k, -1).max(1) <= junk["gmm_members"]).all()
    assert np.array_equal(np.load(os.path.join(folders["junk"], "l.npy")), junk["gmm_label_used"])
    assert json.loads(str(junk["meta"]))["cluster_min_resp"] == 0.999

    before = sorted(os.listdir(folders["junk"]))
    out = _infer(common + ["--out", "s4.npz", "--cluster_gmm", "20"], folders["junk"], code=2)
    assert "--cluster_gmm needs --cluster" in out.stderr
    out = _infer(common + ["--out", "s5.npz", "--cluster", "3", "--cluster_out", "k5.npz", "--cluster_min_resp", "0.5"], folders["junk"], code=2)
    assert "--cluster_min_resp needs --cluster_gmm" in out.stderr
    out = _infer(common + ["--out", "s6.npz", "--cluster", "3", "--cluster_out", "k6.npz", "--cluster_gmm", "1001"], folders["junk"], code=2)
    assert "--cluster_gmm must be in [1, 1000]" in out.stderr and sorted(os.listdir(folders["junk"])) == before
