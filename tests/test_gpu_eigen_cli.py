"""eigenimages.py end to end on the MI355X: train a small model with the command line, apply it with infer.py, run eigenimages.py
on what infer.py wrote, read the file back and replay it in numpy (tests/eigen_ref.py) from the same aligned images.  Each
subprocess runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eigen_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
BOUND = 1e-10
KEYS = ["coords", "count", "eigenimages", "eigenvalues", "explained_variance_ratio", "label", "mean", "members", "meta", "pose",
        "residual", "total_variance", "variance"]


def _run(args, cwd, code=0):
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, args[0])] + args[1:], cwd=cwd, env=env, capture_output=True, text=True,
                         timeout=LIMIT)
    assert out.returncode == code, out.stdout[-1500:] + out.stderr[-3000:]
    return out


def _npz(path):
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _scaled(got, want):
    top = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max() / (top if top > 0 else 1.0)) if want.size else 0.0


def test_mnist_eigenimages_from_what_infer_wrote(tmp_path):
    """train_mnist.py --synthetic 64 for one epoch, infer.py --num_samples 4 --class_averages --labels (classes 0..2 and one -1),
    then eigenimages.py --components 3 --oversample 2 --passes 3 on its score file:
    `mean` is infer.py's `average` bit for bit, count and members are its count and members; every array is within 1e-10 (of the
    array's largest reference value) of eigen_ref.fit driven with the same aligned images and covers, made here by
    elbo.align_at from the stored poses; label and pose are what went in, the image in no class has coords +0; meta records the
    options, the score file's state, the images and the classes; a second run gives a byte-identical file and leaves no .tmp
    file.  --pose refined works on the score file of infer.py --refine 1 (its `mean` is that run's refined `average` bit for bit)
    and is refused (exit code 2, nothing written) on the one without it."""
    import torch
    import train_mnist
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "64", "--num_epochs", "1", "--minibatch_size", "32", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "2", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    cfg = train_mnist.build(train_mnist.mnist_arguments(train), torch.device("cpu"))    # the split, as infer.infer_main obtains it
    images, n, m, K, P, S, I = cfg["y_test"].size(0), 28, 28, 3, 3, 2, 3
    assert images >= 10
    label = (np.arange(images) % K).astype(np.int64)
    label[5] = -1
    np.save(os.path.join(cwd, "l.npy"), label)
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "7", "--seed", "1"]
    _run(common + ["--out", "s.npz", "--class_averages", "c.npz", "--labels", "l.npy"], cwd)
    s, c = _npz(os.path.join(cwd, "s.npz")), _npz(os.path.join(cwd, "c.npz"))
    eigen = ["eigenimages.py", "mnist", "--state", state, "--scores", "s.npz", "--labels", "l.npy", "--components", str(P),
             "--oversample", str(S), "--passes", str(I), "--minibatch_size", "5", "--seed", "2"]
    _run(eigen + ["--out", "e.npz"], cwd)
    with open(os.path.join(cwd, "e.npz"), "rb") as f:
        first = f.read()
    e = _npz(os.path.join(cwd, "e.npz"))
    assert sorted(e) == KEYS
    assert e["mean"].dtype == c["average"].dtype and e["mean"].shape == c["average"].shape == (K, n, m, 1)
    assert e["mean"].tobytes() == c["average"].tobytes(), "mean is not infer.py's average"
    assert np.array_equal(e["count"], c["count"]) and np.array_equal(e["members"], c["members"])
    pose = np.concatenate([s["theta_iw"][:, None], s["dx_iw"]], 1).astype(np.float32)
    assert e["pose"].tobytes() == pose.tobytes() and np.array_equal(e["label"], label) and e["label"].dtype == np.int64
    meta = json.loads(str(e["meta"]))
    assert meta == {"script": "mnist", "state": state, "generator": None, "inference": None, "scores": "s.npz", "split": "test",
                    "labels": "l.npy", "pose": "iw", "interp": "bicubic", "components": P, "oversample": S, "passes": I, "seed": 2,
                    "scores_state": json.loads(str(s["meta"]))["state"], "images": images, "classes": K}

    # the same aligned images through the float64 reference
    dev = torch.device("cuda:0")
    aligned, cover = E.align_at(cfg["y_test"].to(dev), n, m, torch.from_numpy(pose).to(dev), True, True, "bicubic")
    aligned, cover = aligned.cpu().numpy().reshape(images, n * m, 1), cover.cpu().numpy()
    gen = torch.Generator()
    gen.manual_seed(2)
    start = torch.empty(K, n * m, P + S, dtype=torch.float64).normal_(generator=gen).numpy()
    want = R.fit(aligned, cover, label, K, P + S, P, I, start, batch=5)
    host = R.host_outputs(want, P)
    assert np.array_equal(want["count"].reshape(K, n, m), e["count"]) and np.array_equal(want["members"], e["members"])
    assert want["mean"].astype(np.float32).tobytes() == e["mean"].tobytes()
    pairs = {"variance": host["variance"].reshape(K, n, m, 1), "total_variance": host["total_variance"], "eigenvalues": host["eigenvalues"],
             "eigenimages": want["eigenimages"].reshape(K, P, n, m, 1), "explained_variance_ratio": host["explained_variance_ratio"],
             "residual": want["residual"], "coords": want["coords"]}
    errs = {k: _scaled(e[k], v) for k, v in pairs.items()}
    print("eigenimages.py against the reference: %s; eigenvalues %s, residual / eigenvalue %s"
          % (", ".join("%s %.1e" % kv for kv in errs.items()), e["eigenvalues"].round(4).tolist(),
             (e["residual"] / e["eigenvalues"][:, :1]).round(4).tolist()))
    for k, v in pairs.items():
        assert e[k].shape == v.shape and e[k].dtype == np.float64, k
        assert errs[k] <= BOUND, (k, errs[k])
    assert not e["coords"][5].any() and not np.signbit(e["coords"][5]).any() and e["coords"][label >= 0].any(1).all()
    assert (e["eigenvalues"] > 0).all() and (np.diff(e["eigenvalues"], axis=1) <= 0).all()
    assert (e["explained_variance_ratio"].sum(1) <= 1 + 1e-12).all()

    _run(eigen + ["--out", "e.npz"], cwd)                     # again, over its own file
    with open(os.path.join(cwd, "e.npz"), "rb") as f:
        assert f.read() == first, "two runs differ"
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    # --pose refined
    before = sorted(os.listdir(cwd))
    out = _run(eigen + ["--out", "r.npz", "--pose", "refined"], cwd, code=2)
    assert "--pose refined needs the pose_refined of infer.py --refine" in out.stderr.strip().splitlines()[-1]
    assert sorted(os.listdir(cwd)) == before
    _run(common + ["--out", "sr.npz", "--class_averages", "cr.npz", "--labels", "l.npy", "--refine", "1"], cwd)
    sr, cr = _npz(os.path.join(cwd, "sr.npz")), _npz(os.path.join(cwd, "cr.npz"))
    refined = [a if a != "s.npz" else "sr.npz" for a in eigen]
    _run(refined + ["--out", "r.npz", "--pose", "refined"], cwd)
    r = _npz(os.path.join(cwd, "r.npz"))
    assert sorted(r) == KEYS and r["pose"].tobytes() == sr["pose_refined"].tobytes() and json.loads(str(r["meta"]))["pose"] == "refined"
    assert not np.array_equal(r["pose"], e["pose"]) and np.array_equal(r["members"], e["members"])
    assert all(np.isfinite(r[k]).all() for k in KEYS if r[k].dtype.kind == "f") and (r["eigenvalues"] > 0).all()
    assert r["mean"].tobytes() == cr["average"].tobytes(), "mean is not the refined average of infer.py --refine"
    print("--pose refined: total variance %s -> %s" % (e["total_variance"].round(3).tolist(), r["total_variance"].round(3).tolist()))
