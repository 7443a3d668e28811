"""infer.py --pca end to end on the MI355X: train a small model with the command line, apply it with --pca alone, with
--cluster and --pca_per_class, and with --cluster alone; read the files back and hold them to tests/pca_ref.py on the latents
and labels the same runs report, and to each other.  Each subprocess runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pca_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
BOUND = 1e-10
TOL = 2e-5          # tests/test_gpu_align_cli.py's bound for a reconstruction against the in-process decoder
KEYS = {"count", "mean", "cov", "eigenvalues", "components", "explained_variance_ratio", "projections", "sweeps", "off_norm"}
WALKS = {"traverse_latents", "traverse_images"}


def _run(args, cwd, code=0):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, args[0])] + args[1:], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=LIMIT)
    assert out.returncode == code, out.stdout[-1500:] + out.stderr[-3000:]
    return out


def _npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _close(got, want):
    return np.abs(got - want).max() <= BOUND * max(1.0, np.abs(want).max())


def test_mnist_principal_axes_global_and_per_class(tmp_path):
    """train_mnist.py --synthetic 200 for one epoch (50 validation images, H = 64, z_dim 3).

    infer.py --pca p.npz --pca_traverse 2 --pca_steps 2: the listed keys with the listed shapes and dtypes; count, sweeps exactly
    and mean, cov, eigenvalues, components, projections within 1e-10 of pca_ref.fit on the score file's own z_iw;
    explained_variance_ratio sums to 1; traverse_latents follows the formula from the file's own mean, eigenvalues and
    components; the middle frame of both walks is the mean and the same image, the in-process decoder on the float mean to 2e-5.

    With --cluster 3 --pca_per_class --pca_components 2 --pca_traverse 1: the class_* arrays, held to one reference fit with
    k.npz's labels as groups; the global arrays equal the first run's in every shared key but projections, whose two columns are
    the first run's first two.  The same command without the --pca options: c.npz and k.npz equal array for array and byte for
    byte (meta included), s.npz in every array but meta, which differs by the pca keys alone."""
    import torch
    import train_mnist
    from spatial_vae_amd import cli
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "200", "--num_epochs", "1", "--minibatch_size", "64", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "3", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    n, rows, cols, K, D, T = 50, 28, 28, 3, 3, 2
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "8", "--chunk", "3", "--minibatch_size", "20", "--seed", "1"]
    folders = {name: os.path.join(cwd, name) for name in ("alone", "classes", "plain")}
    for path in folders.values():
        os.mkdir(path)

    _run(common + ["--out", "s.npz", "--pca", "p.npz", "--pca_traverse", "2", "--pca_steps", str(T)], folders["alone"])
    s, p = _npz(os.path.join(folders["alone"], "s.npz")), _npz(os.path.join(folders["alone"], "p.npz"))
    shapes = {"count": ((), np.int64), "mean": ((D,), np.float64), "cov": ((D, D), np.float64), "eigenvalues": ((D,), np.float64),
              "components": ((D, D), np.float64), "explained_variance_ratio": ((D,), np.float64), "projections": ((n, D), np.float64),
              "sweeps": ((), np.int32), "off_norm": ((), np.float64), "traverse_latents": ((2, 2 * T + 1, D), np.float32),
              "traverse_images": ((2, 2 * T + 1, rows, cols, 1), np.float32)}
    assert set(p) == KEYS | WALKS | {"meta"} == set(shapes) | {"meta"}
    for key, (shape, dtype) in shapes.items():
        assert p[key].shape == shape and p[key].dtype == dtype, (key, p[key].shape, p[key].dtype)
    z = s["z_iw"]
    assert z.dtype == np.float32 and z.shape == (n, D)
    want = R.fit(z)
    assert p["count"] == want["count"][0] == n and p["sweeps"] == want["sweeps"][0] > 0
    errs = {key: float(np.abs(p[key] - want[ref][0 if ref != "proj" else slice(None)]).max())
            for key, ref in (("mean", "mean"), ("cov", "cov"), ("eigenvalues", "eigenvalues"), ("components", "components"),
                             ("projections", "proj"))}
    gap = R.min_gap(want["eigenvalues"][0])
    print("against pca_ref on the file's z_iw: %s; smallest eigenvalue gap %.2e" % (", ".join("%s %.1e" % kv for kv in errs.items()), gap))
    assert _close(p["cov"], want["cov"][0]) and _close(p["mean"], want["mean"][0]) and _close(p["eigenvalues"], want["eigenvalues"][0])
    assert gap >= R.GAP and _close(p["components"], want["components"][0]) and _close(p["projections"], want["proj"])
    assert abs(p["explained_variance_ratio"].sum() - 1) <= 1e-14
    assert np.abs(p["explained_variance_ratio"] - p["eigenvalues"] / p["eigenvalues"].sum()).max() <= 1e-15
    meta = json.loads(str(p["meta"]))
    added = {"pca": "p.npz", "pca_pose": "iw", "pca_components": None, "pca_traverse": 2, "pca_steps": T, "pca_span": 2.0,
             "pca_per_class": False}
    assert {k: meta[k] for k in added} == added and meta == json.loads(str(s["meta"]))
    frames = np.arange(-T, T + 1, dtype=np.float64) / T
    walk = p["mean"] + (frames * 2.0)[None, :, None] * np.sqrt(np.maximum(p["eigenvalues"][:2], 0))[:, None, None] * p["components"][:2, None, :]
    assert np.abs(p["traverse_latents"] - walk).max() <= 2.0 ** -23 * max(1.0, np.abs(walk).max())       # one rounding to float
    assert np.array_equal(p["traverse_latents"][:, T], np.broadcast_to(p["mean"].astype(np.float32), (2, D)))
    images = p["traverse_images"]
    assert np.array_equal(images[0, T], images[1, T]) and not np.array_equal(images[0, 0], images[0, 2 * T])

    targs = train_mnist.mnist_arguments(train)
    cfg = train_mnist.build(targs, torch.device("cpu"))
    dev = torch.device("cuda:0")
    p_net = cfg["p_net"]
    p_net.load_state_dict(cli.read_checkpoint(state)["train_step"]["p_net"])
    p_net = p_net.to(dev).eval()
    zc = torch.from_numpy(p["mean"].astype(np.float32)[None]).to(dev)
    mine = E.reconstruct_unposed(cli.coord_grid(rows, cols).to(dev), p_net, 1, zc).cpu().numpy().reshape(-1)
    err = np.abs(mine.astype(np.float64) - images[0, T].reshape(-1)).max() / np.abs(mine).max()
    print("the middle frame against the un-posed decoder at the float mean: %.2e of the largest value" % err)
    assert err <= TOL

    clustered = ["--out", "s.npz", "--cluster", str(K), "--cluster_out", "k.npz", "--class_averages", "c.npz"]
    _run(common + clustered + ["--pca", "p.npz", "--pca_per_class", "--pca_components", "2", "--pca_traverse", "1", "--pca_steps", str(T)],
         folders["classes"])
    _run(common + clustered, folders["plain"])
    q, k = _npz(os.path.join(folders["classes"], "p.npz")), _npz(os.path.join(folders["classes"], "k.npz"))
    assert set(q) == KEYS | WALKS | {"class_" + key for key in KEYS | WALKS} | {"meta"}
    for key in KEYS - {"projections"}:
        assert q[key].tobytes() == p[key].tobytes(), key
    assert q["projections"].tobytes() == np.ascontiguousarray(p["projections"][:, :2]).tobytes()
    assert q["traverse_latents"].tobytes() == p["traverse_latents"][:1].tobytes()
    label = k["label"]
    per = R.fit(s["z_iw"], label.astype(np.int32), K, 2)
    class_shapes = {"class_count": (K,), "class_mean": (K, D), "class_cov": (K, D, D), "class_eigenvalues": (K, D),
                    "class_components": (K, D, D), "class_explained_variance_ratio": (K, D), "class_projections": (n, 2),
                    "class_sweeps": (K,), "class_off_norm": (K,), "class_traverse_latents": (K, 1, 2 * T + 1, D),
                    "class_traverse_images": (K, 1, 2 * T + 1, rows, cols, 1)}
    for key, shape in class_shapes.items():
        assert q[key].shape == shape, (key, q[key].shape)
    assert np.array_equal(q["class_count"], per["count"]) and np.array_equal(q["class_count"], k["members"])
    assert np.array_equal(q["class_sweeps"], per["sweeps"])
    print("classes of %s members; smallest eigenvalue gaps %s" % (per["count"].tolist(), ["%.1e" % R.min_gap(e) for e in per["eigenvalues"]]))
    for key, ref in (("class_mean", "mean"), ("class_cov", "cov"), ("class_eigenvalues", "eigenvalues")):
        assert _close(q[key], per[ref]), key
    clear = [c for c in range(K) if per["count"][c] >= 2 and R.min_gap(per["eigenvalues"][c]) >= R.GAP]
    assert clear, "no class of this model has eigenvalues %g apart: no vectors to compare" % R.GAP
    for c in clear:                                 # vectors only where the reference's own are well defined
        assert _close(q["class_components"][c], per["components"][c]), c
        assert _close(q["class_projections"][label == c], per["proj"][label == c]), c
    dead = per["count"][np.maximum(label, 0)] < 2
    assert not q["class_projections"][(label < 0) | dead].any()
    for c in range(K):
        assert np.array_equal(q["class_traverse_latents"][c, 0, T], q["class_mean"][c].astype(np.float32))

    plain_dir, with_dir = folders["plain"], folders["classes"]
    for name in ("c.npz", "k.npz", "s.npz"):
        first, second = _npz(os.path.join(plain_dir, name)), _npz(os.path.join(with_dir, name))
        assert sorted(first) == sorted(second), name
        for key in first:
            if name != "s.npz" or key != "meta":
                assert first[key].dtype == second[key].dtype and first[key].tobytes() == second[key].tobytes(), (name, key)
    m0 = json.loads(str(_npz(os.path.join(plain_dir, "s.npz"))["meta"]))
    m1 = json.loads(str(_npz(os.path.join(with_dir, "s.npz"))["meta"]))
    assert set(m1) - set(m0) == set(added) and {key: m1[key] for key in m0} == m0
    assert m1["pca_per_class"] is True and m1["pca_components"] == 2
    assert not [f for folder in folders.values() for f in os.listdir(folder) if ".tmp" in f]
