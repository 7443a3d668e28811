"""CPU-only: the binding of include/svae_cluster.h held to that header (functions, the record's mirror), the float64 reference
of the k-means (tests/kmeans_ref.py) held to what k-means means, and infer.py's --cluster options: their defaults and every
refusal its argument parser makes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kmeans_ref as K
from test_binding_cpu import SCALARS, binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_cluster_binding_matches_its_header():
    """What is include/svae_cluster.h's own (the rules every added header shares are tests/test_binding_cpu.py's, `rec` as the
    address of a record in device memory among them): three functions and their argument names, no constant and one struct,
    whose mirror _lib.KMeansRecord has its fields, size and offsets; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_cluster.h")[1]
    assert _lib.HEADERS["svae_cluster.h"] is _lib.CLUSTER_SIGNATURES
    assert H["constants"] == {} and list(H["structs"]) == ["svae_kmeans_record"] and len(H["functions"]) == 3
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_kmeans_workspace_bytes"] == ["N", "D", "k"]
    assert names["svae_kmeans_seed"] == ["x", "N", "D", "k", "u", "centres", "seed_index", "ws", "ws_bytes", "stream"]
    assert names["svae_kmeans_step"] == ["x", "N", "D", "k", "update", "centres", "label", "members", "rec", "ws", "ws_bytes", "stream"]
    # the record: field for field, and the layout a C compiler gives it (every field is 8 bytes wide, so there is no padding)
    fields = H["structs"]["svae_kmeans_record"]
    assert [f[2] for f in fields] == [f[0] for f in _lib.KMeansRecord._fields_]
    assert [f[2] for f in fields] == ["iterations", "changed", "converged_at", "assigned", "empty", "inertia"]
    offset = 0
    for (base, pointer, field, length), (_, ctype) in zip(fields, _lib.KMeansRecord._fields_):
        assert not pointer and length is None and ctype is SCALARS[base], field
        assert getattr(_lib.KMeansRecord, field).offset == offset and ctypes.sizeof(ctype) == 8, field
        offset += 8
    assert ctypes.sizeof(_lib.KMeansRecord) == offset == 48
    assert bytes(_lib.KMeansRecord()) == bytes(48)                  # a fresh record is all zero bytes
    assert not [k for k in binding_constants(_lib) if "KMEANS" in k or "CLUSTER" in k]
    assert ops._POINTER_ARGS["svae_kmeans_seed"] == (0, 4, 5, 6, 7) and ops._POINTER_ARGS["svae_kmeans_step"] == (0, 5, 6, 7, 8, 9)
    assert ops.KMeans.RECORD_WORDS == 6


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: 8 (N + 3 C + C k + C k D) bytes with C = ceil(N / P), P = 256 doubled until C <= 1024; 0 outside the
    header's limits."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_kmeans_workspace_bytes
    for N, D, k in [(1000, 3, 5), (4097, 1, 2), (262144, 2, 3), (262145, 2, 3), (2048, 64, 1024), (5, 1, 5), (2 ** 31 - 1, 1, 1)]:
        P = K.chunk_len(N)
        C = -(-N // P)
        assert C <= 1024 and (P == 256 or -(-N // (P // 2)) > 1024)
        assert fn(N, D, k) == 8 * (N + 3 * C + C * k + C * k * D), (N, D, k)
    assert K.chunk_len(262144) == 256 and K.chunk_len(262145) == 512
    for N, D, k in [(4, 3, 5), (100, 0, 5), (100, 65, 5), (100, 3, 0), (2000, 3, 1025), (2 ** 31, 3, 5), (-1, 3, 5)]:
        assert fn(N, D, k) == 0, (N, D, k)


# ---------------------------------------------------------------- the reference, held to what k-means means
def test_reference_labels_are_the_argmin_and_centres_the_means_at_convergence():
    x, u = K.blobs(0, 1000, 3, 5)
    out = K.fit(x, 5, u, 40)
    assert 0 < out["converged_at"] <= 40 and out["iterations"] == 40 and out["changed"] == 0
    x64 = x.astype(np.float64)
    dist = ((x64[:, None, :] - out["centres"][None]) ** 2).sum(2)
    assert np.array_equal(out["label"], dist.argmin(1))
    assert np.array_equal(out["members"], np.bincount(out["label"], minlength=5)) and out["members"].sum() == 1000
    for j in range(5):
        mean = x64[out["label"] == j].mean(0)
        assert np.abs(out["centres"][j] - mean).max() <= 1e-12 * (1 + np.abs(mean).max())
    assert abs(out["inertia"] - dist.min(1).sum()) <= 1e-12 * out["inertia"]
    assert len(set(out["seed_index"].tolist())) == 5 and out["seed_index"][0] == K.fallback(u[0], 1000)


def test_reference_order_ties_and_unassigned_points():
    """The two-level sum differs from numpy's pairwise sum in the last bits but is the plain loop's; equal distances keep the
    lowest centre; a non-finite point is labelled -1 and enters nothing."""
    rs = np.random.RandomState(3)
    v = rs.rand(700)
    chunks = [0.0, 0.0, 0.0]
    for i, a in enumerate(v):
        chunks[i // 256] += a
    assert K.ordered_sum(v) == (0.0 + chunks[0] + chunks[1]) + chunks[2]
    x = np.array([[0.0, 0.0], [1.0, 0.0], [np.nan, 0.0], [0.5, np.inf], [0.5, 0.0]], np.float32)
    c = np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    out = K.step(x, c, None, 0)
    assert out["label"].tolist() == [1, 0, -1, -1, 0] and out["members"].tolist() == [2, 1, 0]
    assert (out["assigned"], out["changed"], out["empty"], out["inertia"]) == (3, 3, 1, 0.25)
    assert np.array_equal(out["centres"], np.array([[0.75, 0.0], [0.0, 0.0], [0.0, 0.0]]))
    again = K.step(x, out["centres"], out["label"], 1, update=False)
    assert again["changed"] == 0 and again["iterations"] == 1 and np.array_equal(again["centres"], out["centres"])


def test_reference_seeding_falls_back_on_coincident_points():
    x = np.ones((300, 2), np.float32)
    u = np.array([0.5, 0.25, 0.999])
    index, centres, rounds = K.seed(x, 3, u)
    assert index.tolist() == [150, 75, 299] and all(T == 0 for _, T in rounds[1:]) and (centres == 1).all()


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


def test_cluster_options_default_to_off_and_fill_in(tmp_path):
    base = _base(tmp_path)
    a = _infer().infer_arguments(base)
    assert (a.cluster, a.cluster_out, a.cluster_labels, a.cluster_iters, a.cluster_restarts, a.cluster_seed) == (None,) * 6
    a = _infer().infer_arguments(base + ["--seed", "7", "--cluster", "3", "--cluster_out", "k.npz"])
    assert (a.cluster, a.cluster_out, a.cluster_labels, a.cluster_iters, a.cluster_restarts, a.cluster_seed) == (3, "k.npz", None, 100, 1, 7)
    assert a.pose == "iw" and a.class_averages is None
    a = _infer().infer_arguments(base + ["--cluster", "1024", "--cluster_out", "k.npz", "--cluster_labels", "l.npy", "--cluster_iters", "1",
                                       "--cluster_restarts", "16", "--cluster_seed", "5", "--pose", "q"])       # --pose with --cluster alone
    assert (a.cluster, a.cluster_labels, a.cluster_iters, a.cluster_restarts, a.cluster_seed, a.pose) == (1024, "l.npy", 1, 16, 5, "q")
    assert _infer().INFER_MAX_CLUSTERS == 1024 <= _infer().INFER_MAX_CLASSES


REFUSALS = [
    (["--cluster", "3", "--cluster_out", "k.npz", "--class_averages", "c.npz", "--labels", "{int1d}"], "excludes --labels"),
    (["--cluster_out", "k.npz"], "--cluster_out needs --cluster"),
    (["--cluster_labels", "l.npy"], "--cluster_labels needs --cluster"),
    (["--cluster_iters", "5"], "--cluster_iters needs --cluster"),
    (["--cluster_restarts", "2"], "--cluster_restarts needs --cluster"),
    (["--cluster_seed", "2"], "--cluster_seed needs --cluster"),
    (["--cluster", "3"], "--cluster needs --cluster_out"),
    (["--cluster", "1", "--cluster_out", "k.npz"], "--cluster must be in [2, 1024]"),
    (["--cluster", "1025", "--cluster_out", "k.npz"], "--cluster must be in [2, 1024]"),
    (["--cluster", "3", "--cluster_out", "k.npy"], "--cluster_out must end in .npz"),
    (["--cluster", "3", "--cluster_out", "k.npz", "--cluster_labels", "l.npz"], "--cluster_labels must end in .npy"),
    (["--cluster", "3", "--cluster_out", "k.npz", "--cluster_iters", "0"], "--cluster_iters must be >= 1"),
    (["--cluster", "3", "--cluster_out", "k.npz", "--cluster_restarts", "0"], "--cluster_restarts must be in [1, 16]"),
    (["--cluster", "3", "--cluster_out", "k.npz", "--cluster_restarts", "17"], "--cluster_restarts must be in [1, 16]"),
    (["--cluster", "3", "--cluster_out", "k.npz", "--interp", "bilinear"], "--interp needs one of"),
    (["--pose", "best"], "--pose needs one of"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_cluster_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    np.save(tmp_path / "int1d.npy", np.array([0, 1, 1]))
    argv = _base(tmp_path) + [a.format(int1d=tmp_path / "int1d.npy") for a in extra]
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(argv)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_a_cluster_refusal_exits_with_code_2_before_the_library_is_loaded(tmp_path):
    """Through the real command line in a fresh process: exit code 2, no output file, and the process never loaded the kernel
    library."""
    np.save(tmp_path / "l.npy", np.array([0, 1, 1]))
    argv = _base(tmp_path) + ["--cluster", "3", "--cluster_out", "k.npz", "--class_averages", "c.npz", "--labels", str(tmp_path / "l.npy")]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert "excludes --labels" in out.stderr and "LIB True" in out.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt", "l.npy"]
