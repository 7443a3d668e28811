"""neighbours.py end to end on the MI355X: train a small model with the command line, apply it with infer.py, run neighbours.py on
what infer.py wrote, read the files back and replay them in numpy (tests/neighbours_ref.py) from the score file's latents and
the same aligned images.  Each subprocess runs under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbours_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240
KEYS = ["average_index", "found", "in_degree", "index", "meta", "pose", "sqdist", "weight"]


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


def test_mnist_neighbour_averages_from_what_infer_wrote(tmp_path):
    """train_mnist.py --synthetic 64 for one epoch, infer.py --num_samples 4, then neighbours.py --neighbours 6 --averages a.npy
    --support s.npy --minibatch_size 5 on its score file: the keys, dtypes and shapes; index and sqdist bit-equal to the
    reference on the score file's z_iw widened to float64; found and in_degree exact; average and support match the reference
    replayed from elbo.align_at at the stored poses with the file's own average_index and weight (support bit for bit, every
    average within one float32 of the single division); pose and meta are what went in; a second run gives byte-identical
    files and leaves no .tmp file.  --weights gaussian --exclude_self: slot 0 is -1, the weights are within 1e-12 of numpy's
    formula and the averages again replay from the file.  --latent q --pose refined works on the score file of infer.py
    --refine 1 and is refused (exit code 2, nothing written) on the one without pose_refined."""
    import torch
    import train_mnist
    from spatial_vae_amd import elbo as E
    cwd = str(tmp_path)
    train = ["--synthetic", "64", "--num_epochs", "1", "--minibatch_size", "32", "--p_hidden_dim", "64", "--q_hidden_dim", "32",
             "--z_dim", "2", "--checkpoint_interval", "1", "--seed", "3", "--progress_every", "0", "--save_prefix", "run"]
    _run(["train_mnist.py"] + train, cwd)
    state = os.path.join(cwd, "outputs_run", "trained", "run_state_epoch1.ckpt")
    cfg = train_mnist.build(train_mnist.mnist_arguments(train), torch.device("cpu"))    # the split, as infer.infer_main obtains it
    images, n, m, K = cfg["y_test"].size(0), 28, 28, 6
    assert images >= 10
    common = ["infer.py", "mnist", "--state", state, "--num_samples", "4", "--chunk", "2", "--minibatch_size", "7", "--seed", "1"]
    _run(common + ["--out", "s.npz"], cwd)
    s = _npz(os.path.join(cwd, "s.npz"))
    nbr = ["neighbours.py", "mnist", "--state", state, "--scores", "s.npz", "--neighbours", str(K), "--minibatch_size", "5"]
    files = ["--out", "n.npz", "--averages", "a.npy", "--support", "s.npy"]
    _run(nbr + files, cwd)
    first = [_bytes(os.path.join(cwd, f)) for f in ("n.npz", "a.npy", "s.npy")]
    e = _npz(os.path.join(cwd, "n.npz"))
    assert sorted(e) == KEYS
    T = K + 1
    for key, dtype, shape in (("index", np.int64, (images, K)), ("sqdist", np.float64, (images, K)), ("found", np.int64, (images,)),
                              ("in_degree", np.int64, (images,)), ("average_index", np.int64, (images, T)),
                              ("weight", np.float64, (images, T)), ("pose", np.float32, (images, 3))):
        assert e[key].dtype == dtype and e[key].shape == shape, key
    z = s["z_iw"].astype(np.float64)
    want_d, want_i = R.brute_force(z, K)
    assert e["index"].tobytes() == want_i.tobytes() and e["sqdist"].tobytes() == want_d.tobytes()
    assert np.array_equal(e["found"], (want_i >= 0).sum(1)) and (e["found"] == K).all()
    assert np.array_equal(e["in_degree"], np.bincount(want_i[want_i >= 0], minlength=images)) and e["in_degree"].sum() == images * K
    assert np.array_equal(e["average_index"], np.concatenate([np.arange(images)[:, None], want_i], 1)) and (e["weight"] == 1).all()
    pose = np.concatenate([s["theta_iw"][:, None], s["dx_iw"]], 1).astype(np.float32)
    assert e["pose"].tobytes() == pose.tobytes()
    meta = json.loads(str(e["meta"]))
    assert meta == {"script": "mnist", "state": state, "generator": None, "inference": None, "scores": "s.npz", "split": "test",
                    "averages": "a.npy", "support": "s.npy", "neighbours": K, "latent": "iw", "pose": "iw", "interp": "bicubic",
                    "weights": "uniform", "exclude_self": False, "stack_gib": 32.0,
                    "scores_state": json.loads(str(s["meta"]))["state"], "images": images, "z_dim": 2}

    # the same aligned images through the float64 reference, with the file's own slots and weights
    dev = torch.device("cuda:0")

    def aligned_at(pose3):
        aligned, cover = E.align_at(cfg["y_test"].to(dev), n, m, torch.from_numpy(pose3.copy()).to(dev), True, True, "bicubic")
        return aligned.cpu().numpy().reshape(images, n * m, 1), cover.cpu().numpy()

    def replayed(path_avg, path_sup, arrays, stack, cover):
        avg, sup = np.load(os.path.join(cwd, path_avg)), np.load(os.path.join(cwd, path_sup))
        assert avg.dtype == np.float32 and avg.shape == (images, n, m, 1) and sup.dtype == np.float64 and sup.shape == (images, n, m)
        _, want_sup, exact = R.average(stack, cover, arrays["average_index"], arrays["weight"])
        assert sup.reshape(images, n * m).tobytes() == want_sup.tobytes(), "support"
        ok, same = R.within_one_float(np.ascontiguousarray(avg.reshape(images, n * m, 1)), exact)
        print("%s: %d of %d averages not identical to the reference's float32" % (path_avg, (~same).sum(), same.size))
        assert ok.all()
        return avg, sup

    stack, cover = aligned_at(pose)
    avg, sup = replayed("a.npy", "s.npy", e, stack, cover)
    assert sup.max() == T and np.isfinite(avg).all()

    _run(nbr + files, cwd)                                        # again, over its own files
    assert [_bytes(os.path.join(cwd, f)) for f in ("n.npz", "a.npy", "s.npy")] == first, "two runs differ"
    assert not [f for f in os.listdir(cwd) if ".tmp" in f]

    # --weights gaussian --exclude_self
    _run(nbr + ["--out", "g.npz", "--averages", "ga.npy", "--support", "gs.npy", "--weights", "gaussian", "--exclude_self"], cwd)
    g = _npz(os.path.join(cwd, "g.npz"))
    assert sorted(g) == KEYS and g["index"].tobytes() == e["index"].tobytes() and g["sqdist"].tobytes() == e["sqdist"].tobytes()
    assert (g["average_index"][:, 0] == -1).all() and np.array_equal(g["average_index"][:, 1:], e["index"])
    want_w = R.gaussian_weights(g["sqdist"], g["index"])
    assert np.abs(g["weight"] - want_w).max() <= 1e-12 and (g["weight"][:, 0] == 1).all() and (g["weight"][:, 1:] <= 1).all()
    gmeta = json.loads(str(g["meta"]))
    assert gmeta["weights"] == "gaussian" and gmeta["exclude_self"] is True
    gavg, gsup = replayed("ga.npy", "gs.npy", g, stack, cover)
    assert gsup.max() < K and not np.array_equal(gavg, avg)

    # --latent q --pose refined
    before = sorted(os.listdir(cwd))
    out = _run(nbr + ["--out", "r.npz", "--averages", "ra.npy", "--support", "rs.npy", "--latent", "q", "--pose", "refined"], cwd, code=2)
    assert "--pose refined needs the pose_refined of infer.py --refine" in out.stderr.strip().splitlines()[-1]
    assert sorted(os.listdir(cwd)) == before
    _run(common + ["--out", "sr.npz", "--class_averages", "cr.npz", "--refine", "1"], cwd)
    sr = _npz(os.path.join(cwd, "sr.npz"))
    refined = [a if a != "s.npz" else "sr.npz" for a in nbr]
    _run(refined + ["--out", "r.npz", "--averages", "ra.npy", "--support", "rs.npy", "--latent", "q", "--pose", "refined"], cwd)
    r = _npz(os.path.join(cwd, "r.npz"))
    rmeta = json.loads(str(r["meta"]))
    assert sorted(r) == KEYS and r["pose"].tobytes() == sr["pose_refined"].tobytes() and (rmeta["pose"], rmeta["latent"]) == ("refined", "q")
    rd, ri = R.brute_force(sr["z_q"].astype(np.float64), K)
    assert r["index"].tobytes() == ri.tobytes() and r["sqdist"].tobytes() == rd.tobytes()
    rstack, rcover = aligned_at(sr["pose_refined"])
    replayed("ra.npy", "rs.npy", r, rstack, rcover)
