"""CPU-only: what is include/svae_eigen.h's own in its binding, the float64 reference of the eigenimage kernels
(tests/eigen_ref.py) held to numpy's eigh of the explicit covariance and to the header's conventions for
dead classes and dead columns, and eigenimages.py's command line: its defaults and every refusal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eigen_ref as R
from test_binding_cpu import binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the header and its table
def test_eigen_binding_matches_its_header():
    """What is include/svae_eigen.h's own (the rules every added header shares are tests/test_binding_cpu.py's): six functions
    and their argument names, no struct; the header's two constants are _lib.EIGEN_LIMITS, and none of this adds an upper-case
    integer to the binding; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_eigen.h")[1]
    assert _lib.HEADERS["svae_eigen.h"] is _lib.EIGEN_SIGNATURES
    assert H["structs"] == {} and len(H["functions"]) == 6
    assert H["constants"] == {"SVAE_EIG_" + k.upper(): v for k, v in _lib.EIGEN_LIMITS.items()}
    assert H["constants"]["SVAE_EIG_MAX_R"] == R.MAX_R and 2.0 ** H["constants"]["SVAE_EIG_DEAD_LOG2"] == R.DEAD
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_eig_project"] == ["aligned", "cover", "label", "mean", "Q", "B", "N", "C", "K", "R", "T", "stream"]
    assert names["svae_eig_accumulate"] == ["aligned", "cover", "label", "mean", "T", "B", "N", "C", "K", "R", "Y", "ssq", "stream"]
    assert names["svae_eig_orthonormalise"] == ["Y", "K", "D", "R", "Q", "stream"]
    assert names["svae_eig_gram"] == ["Q", "Y", "members", "K", "D", "R", "G", "stream"]
    assert names["svae_eig_rotate"] == ["Q", "Y", "W", "lambda", "members", "K", "D", "R", "P", "eigenimages", "residual", "rot",
                                        "stream"]
    assert names["svae_eig_coords"] == ["T", "label", "rot", "B", "K", "R", "P", "coords", "stream"]
    assert not [k for k in binding_constants(_lib) if "EIG" in k]
    assert ops._POINTER_ARGS["svae_eig_project"] == (0, 1, 2, 3, 4, 10)
    assert ops._POINTER_ARGS["svae_eig_accumulate"] == (0, 1, 2, 3, 4, 10, 11)
    assert ops._POINTER_ARGS["svae_eig_orthonormalise"] == (0, 4)
    assert ops._POINTER_ARGS["svae_eig_gram"] == (0, 1, 2, 6)
    assert ops._POINTER_ARGS["svae_eig_rotate"] == (0, 1, 2, 3, 4, 9, 10, 11)
    assert ops._POINTER_ARGS["svae_eig_coords"] == (0, 1, 2, 7)


# ---------------------------------------------------------------- the reference against numpy
def _eigh(S):
    w, U = np.linalg.eigh(S)
    return w[::-1], U[:, ::-1].T


# (seed, B, N, K, rank, R, P)
LOW_RANK = [(0, 24, 35, 1, 3, 5, 3), (1, 40, 105, 2, 4, 8, 4), (2, 30, 64, 3, 2, 3, 2)]


@pytest.mark.parametrize("case", LOW_RANK, ids=["N%d_K%d_rank%d_R%d" % c[2:6] for c in LOW_RANK])
def test_reference_against_eigh_on_exactly_low_rank_members(case):
    """Members in a rank-dimensional affine subspace per class, rank <= R: one application of the covariance spans its range
    exactly, so the Rayleigh-Ritz step of the second pass is exact.  Eigenvalues and eigenimages agree with np.linalg.eigh of the
    explicit covariance within 1e-10 of the largest eigenvalue; the nonzero eigenvalues are at least 1e-4 of the largest apart;
    the columns past the rank are dead: eigenvalue +0, eigenimage all +0."""
    seed, B, N, K, rank, Rc, P = case
    aligned, cover, label = R.low_rank_images(seed, B, N, K, rank)
    fit = R.fit(aligned, cover, label, K, Rc, Rc, 2, R.start_array(seed + 50, K, N, Rc))
    host = R.host_outputs(fit, Rc)
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        S, n = R.covariance(aligned, cover, label, k, fit["mean"])
        w, U = _eigh(S)
        top = w[0]
        assert n == fit["members"][k] and top > 0
        assert R.pca_ref.min_gap(w[:rank + 1]) >= 1e-4
        lam, V = host["eigenvalues"][k], fit["eigenimages"][k]
        worst[0] = max(worst[0], np.abs(lam[:rank] - w[:rank]).max() / top)
        signs = np.sign((V[:rank] * U[:rank]).sum(1))
        worst[1] = max(worst[1], np.abs(V[:rank] - signs[:, None] * U[:rank]).max())
        worst[2] = max(worst[2], fit["residual"][k].max() / top)
        assert not lam[rank:].any() and not np.signbit(lam[rank:]).any()
        assert not V[rank:].any() and not np.signbit(V[rank:]).any()
        assert not fit["Q"][k][:, rank:].any()
        assert abs(host["total_variance"][k] - np.trace(S)) <= 1e-12 * np.trace(S)
        assert abs(host["explained_variance_ratio"][k][:rank].sum() - 1.0) <= 1e-10
        assert np.abs(host["variance"][k] - np.diag(S)).max() <= 1e-12 * top
        at = np.abs(V[:rank]).argmax(1)
        assert (V[np.arange(rank), at] > 0).all()
    print("low rank %s: eigenvalues %.1e, eigenimages %.1e, residual %.1e (of the largest eigenvalue)" % ((case,) + tuple(worst)))
    assert worst[0] <= 1e-10 and worst[1] <= 1e-10 and worst[2] <= 1e-10
    assert P <= Rc


def test_reference_on_a_full_rank_planted_spectrum():
    """Sixty members with a planted full-rank spectrum in a 35-pixel box, R = 8, five passes.  Each Ritz value is at most the
    matching eigenvalue of the explicit covariance times (1 + 1e-12) (Cauchy interlacing: a property, not a tuned number);
    `residual` is |S v - lambda v| formed directly; the eigenimages are orthonormal within 1e-12; coords are the members'
    residuals along the eigenimages."""
    N, B, Rc, P = 35, 60, 8, 6
    spectrum = np.concatenate([[40.0, 25.0, 14.0, 8.0], np.linspace(2.0, 0.5, N - 4)])
    aligned, cover, label = R.planted_images(7, B, N, spectrum)
    fit = R.fit(aligned, cover, label, 1, Rc, P, 5, R.start_array(8, 1, N, Rc), batch=17)
    S, n = R.covariance(aligned, cover, label, 0, fit["mean"])
    w, _ = _eigh(S)
    lam, V = fit["lambda"][0], fit["eigenimages"][0]
    assert n == B and (np.diff(lam) <= 0).all()
    assert (lam <= w[:Rc] * (1 + 1e-12)).all()
    direct = np.sqrt((((S.dot(V.T)) - V.T * lam[:P]) ** 2).sum(0))
    assert np.abs(fit["residual"][0] - direct).max() <= 1e-12 * w[0]
    assert np.abs(V.dot(V.T) - np.eye(P)).max() <= 1e-12
    d, _, _ = R.residuals(aligned, cover, label.astype(np.int64), fit["mean"])
    assert np.abs(fit["coords"] - d.dot(V.T)).max() <= 1e-12 * np.abs(d).max() * np.sqrt(N)
    whole = R.fit(aligned, cover, label, 1, Rc, P, 5, R.start_array(8, 1, N, Rc))
    assert all(np.array_equal(fit[k], whole[k]) for k in fit), "minibatch boundaries must not change a bit"
    print("planted: lambda / eigh %s, residual / top %s" % (np.round(lam[:P] / w[:P], 6), fit["residual"][0] / w[0]))


def test_dead_classes_and_rank_deficient_classes_follow_the_header():
    """K = 5 in a 5 x 7 box with R = 5: class 0 has three members (rank 2: three dead columns), class 3 one member, class 4
    none; labels -1 and K + 1 are in no class.  Dead classes: every output +0 (the mean of the one-member class is that member).
    The rank-deficient class: two positive eigenvalues, then +0 and all-zero eigenimages.  Images in no class: coords +0."""
    K, Rc = 5, 5
    aligned, cover, label = R.images(3, 37, 5, 7, 1, K)
    fit = R.fit(aligned, cover, label, K, Rc, Rc, 3, R.start_array(4, K, 35, Rc), batch=10)
    host = R.host_outputs(fit, Rc)
    members = [int(v) for v in fit["members"]]
    assert members[0] == 3 and members[3:] == [1, 0] and min(members[1:3]) > Rc and sum(members) == 35
    for k in (3, 4):
        for key in ("ssq", "G", "eigenimages", "residual", "rot"):
            assert not fit[key][k].any() and not np.signbit(fit[key][k]).any(), (k, key)
        for key in ("variance", "total_variance", "eigenvalues", "explained_variance_ratio"):
            assert not np.any(host[key][k]) and not np.signbit(host[key][k]).any(), (k, key)
    one = int(np.flatnonzero(label == 3)[0])
    assert np.array_equal(fit["mean"][3].reshape(-1)[cover[one] != 0], aligned[one].reshape(-1)[cover[one] != 0].astype(np.float64))
    lam = host["eigenvalues"][0]
    assert (lam[:2] > 0).all() and not lam[2:].any() and not np.signbit(lam[2:]).any()
    assert not fit["eigenimages"][0][2:].any() and fit["eigenimages"][0][:2].any(1).all()
    assert (fit["Q"][0].any(0) == [True, True, False, False, False]).all()
    outside = (label < 0) | (label >= K) | (label == 3)
    assert not fit["coords"][outside].any() and fit["coords"][label == 1].any()
    S, _ = R.covariance(aligned, cover, label, 0, fit["mean"])
    w, _ = _eigh(S)
    assert np.abs(lam[:2] - w[:2]).max() <= 1e-10 * w[0]


# ---------------------------------------------------------------- the command line
def _pipeline():
    from spatial_vae_amd import eigen_images
    return eigen_images


def _base(tmp_path, arrays=None, **meta):
    """A command line that passes, with stand-in files: a state file (never opened by the parser) and a score file."""
    (tmp_path / "a.ckpt").write_bytes(b"x")
    record = dict({"script": "mnist", "split": "test", "images": 50, "state": "a.ckpt"}, **meta)
    stored = {"theta_iw": np.zeros(50, np.float32), "dx_iw": np.zeros((50, 2), np.float32), "meta": np.array(json.dumps(record))}
    stored.update(arrays or {})
    np.savez(str(tmp_path / "s.npz"), **stored)
    return ["mnist", "--state", str(tmp_path / "a.ckpt"), "--scores", str(tmp_path / "s.npz"), "--out", str(tmp_path / "e.npz")]


def test_defaults_are_the_stated_conventions(tmp_path):
    args = _pipeline().eigen_arguments(_base(tmp_path))
    assert (args.components, args.oversample, args.passes, args.pose, args.interp) == (8, 8, 8, "iw", "bicubic")
    assert (args.split, args.seed, args.minibatch_size, args.labels, args.label_array) == ("test", 0, 100, None, None)
    assert args.score_meta["images"] == 50 and sorted(args.score_arrays) == ["dx_iw", "theta_iw"]
    assert all(vars(args)[k] is None for k in _pipeline().PATH_OVERRIDES)


REFUSALS = [
    (["--out", "e.npy"], "--out must end in .npz"),
    (["--scores", "s.npy"], "--scores must end in .npz"),
    (["--labels", "l.npz"], "--labels must end in .npy"),
    (["--components", "0"], "--components must be in [1, 64]"),
    (["--components", "65"], "--components must be in [1, 64]"),
    (["--oversample=-1"], "--oversample must be in [0, 63]"),
    (["--oversample", "64"], "--oversample must be in [0, 63]"),
    (["--passes", "0"], "--passes must be in [1, 1000]"),
    (["--passes", "1001"], "--passes must be in [1, 1000]"),
    (["--minibatch_size", "0"], "--minibatch_size must be in [1, 2147483647]"),
    (["--components", "60", "--oversample", "5"], "--components + --oversample must not exceed 64 (got 60 + 5)"),
    (["--generator", "g.sav"], "give either --state or --generator with --inference"),
    (["--", "--z-dim", "2"], "--state carries the training arguments"),
    (["--scores", "missing.npz"], "no such file: missing.npz"),
    (["--labels", "missing.npy"], "no such file: missing.npy"),
    (["--split", "train"], "was written for the split 'test', not 'train'"),
    (["--pose", "refined"], "--pose refined needs the pose_refined of infer.py --refine"),
    (["--pose", "worst"], "invalid choice"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_made_by_the_parser(tmp_path, capsys, extra, message):
    """eigen_arguments exits with code 2 and the reason on the last line of stderr."""
    with pytest.raises(SystemExit) as e:
        _pipeline().eigen_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err.strip().splitlines()[-1]


def test_refusals_made_from_the_input_files(tmp_path, capsys):
    """Another script's score file, a file that is no score file, a label file with too many classes: code 2 from the parser."""
    P = _pipeline()

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            P.eigen_arguments(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err.strip().splitlines()[-1]

    refused(_base(tmp_path, script="galaxy"), "was written for the script 'galaxy', not 'mnist'")
    base = _base(tmp_path)
    np.savez(str(tmp_path / "s.npz"), theta_iw=np.zeros(50, np.float32))
    refused(base, "is not a score file of infer.py")
    base = _base(tmp_path)
    np.save(str(tmp_path / "l.npy"), np.array([0, 4096]))
    refused(base + ["--labels", str(tmp_path / "l.npy")], "has 4097 classes, at most 4096 are supported")
    np.save(str(tmp_path / "l.npy"), np.array([0, -2]))
    refused(base + ["--labels", str(tmp_path / "l.npy")], "has a value below -1")
    np.save(str(tmp_path / "l.npy"), np.array([0, -1, 2]))
    assert list(P.eigen_arguments(base + ["--labels", str(tmp_path / "l.npy")]).label_array) == [0, -1, 2]
    refined = _base(tmp_path, arrays={"pose_refined": np.zeros((50, 3), np.float32)})
    assert P.eigen_arguments(refined + ["--pose", "refined"]).score_arrays["pose_refined"].shape == (50, 3)


def test_refusals_that_need_the_split(tmp_path, capsys):
    """Where the split is known: the score file's image count, a missing pose array, the labels' length and the size of the
    basis -- each exits with code 2; the same requests within the limits pass."""
    from spatial_vae_amd.infer_request import SplitFacts
    P = _pipeline()
    base = dict(n=28, m=28, channels=1, rotate=True, translate=True, inf_dim=5, z_scale=1, split="test", ctf_rows=None)
    f50, f49 = SplitFacts(images=50, **base), SplitFacts(images=49, **base)
    big = SplitFacts(images=50, **dict(base, n=1024, m=1024))

    def refused(fn, message):
        with pytest.raises(SystemExit) as e:
            fn()
        assert e.value.code == 2 and message in capsys.readouterr().err.strip().splitlines()[-1]

    argv = _base(tmp_path)
    args = P.eigen_arguments(argv)
    pose = P.stored_poses(args, f50)
    assert pose.shape == (50, 3) and pose.dtype == np.float32
    labels, classes = P.check_request(args, f50)
    assert classes == 1 and not labels.any() and labels.shape == (50,)
    refused(lambda: P.stored_poses(args, f49), "holds 50 images, the test split has 49")
    refused(lambda: P.stored_poses(P.eigen_arguments(argv + ["--pose", "q"]), f50), "has no theta_q of shape (50,)")
    np.save(str(tmp_path / "l.npy"), np.arange(49) % 3)
    with_labels = P.eigen_arguments(argv + ["--labels", str(tmp_path / "l.npy")])
    refused(lambda: P.check_request(with_labels, f50), "--labels has 49 entries, the test split has 50 images")
    assert P.check_request(with_labels, f49)[1] == 3
    np.save(str(tmp_path / "l.npy"), np.arange(50) % 22)
    many = P.eigen_arguments(argv + ["--labels", str(tmp_path / "l.npy")])
    assert P.check_request(many, f50)[1] == 22            # 22 x 784 x 16 <= 2^28
    refused(lambda: P.check_request(many, big), "22 x 1048576 x 16 exceed 2^28")
    widest = P.eigen_arguments(argv + ["--oversample", "56"])
    assert P.check_request(widest, SplitFacts(images=50, **dict(base, n=2048, m=2048)))[1] == 1      # 2^22 x 64 = 2^28 exactly
    refused(lambda: P.check_request(widest, SplitFacts(images=50, **dict(base, n=2048, m=2049))), "1 x 4196352 x 64 exceed 2^28")


def test_a_refusal_exits_with_code_2_before_the_library_or_the_device_is_touched(tmp_path):
    """Through the real command line in a fresh process: exit code 2, the reason on the last line of stderr, no output file, and
    the process neither loaded the kernel library nor initialised torch.cuda."""
    argv = _base(tmp_path) + ["--components", "60", "--oversample", "5"]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['eigenimages.py'] + %r\n"
            "import torch\nfrom spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, 'CUDA', torch.cuda.is_initialized(), file=sys.stderr))\n"
            "import eigenimages; sys.exit(eigenimages.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    lines = out.stderr.strip().splitlines()
    assert "--components + --oversample must not exceed 64" in lines[-2] and lines[-1] == "LIB True CUDA False"
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt", "s.npz"]
