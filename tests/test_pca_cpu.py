"""CPU-only: the binding of include/svae_pca.h held to that header, the float64 reference of the PCA kernels (tests/pca_ref.py)
held to numpy's own covariance and eigen-solver and to the conditions the GPU test relies on, infer.py's --pca options (their
defaults and every refusal), elbo.traverse_latents against its formula, and the build's header check."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pca_ref as R
from kmeans_ref import chunk_len
from test_binding_cpu import binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.fixture_id(f) for f in R.FIXTURES]


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_pca_binding_matches_its_header():
    """What is include/svae_pca.h's own (the rules every added header shares are tests/test_binding_cpu.py's): four functions
    and their argument names, no constant and no struct; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_pca.h")[1]
    assert _lib.HEADERS["svae_pca.h"] is _lib.PCA_SIGNATURES
    assert H["constants"] == {} and H["structs"] == {} and len(H["functions"]) == 4
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_pca_workspace_bytes"] == ["N", "D", "G"]
    assert names["svae_pca_moments"] == ["x", "N", "D", "G", "group", "count", "mean", "cov", "ws", "ws_bytes", "stream"]
    assert names["svae_pca_eigen"] == ["cov", "D", "G", "eigenvalues", "components", "sweeps", "off_norm", "stream"]
    assert names["svae_pca_project"] == ["x", "N", "D", "G", "P", "group", "count", "mean", "components", "proj", "stream"]
    assert not [k for k in binding_constants(_lib) if "PCA" in k]
    assert ops._POINTER_ARGS["svae_pca_moments"] == (0, 4, 5, 6, 7, 8)
    assert ops._POINTER_ARGS["svae_pca_eigen"] == (0, 3, 4, 5, 6)
    assert ops._POINTER_ARGS["svae_pca_project"] == (0, 5, 6, 7, 8, 9)


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: 8 (C G (1 + D + D (D + 1) / 2) + ceil(N / 2)) bytes with C = ceil(N / L); 0 outside the header's limits,
    G D (D + 1) / 2 <= 32768 among them; the per-chunk products stay within 256 MiB."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_pca_workspace_bytes
    for N, D, G in [(1, 1, 1), (1000, 3, 5), (4097, 1, 2), (262144, 2, 3), (262145, 2, 3), (2048, 64, 15), (5, 7, 1024),
                    (2 ** 31 - 1, 1, 1), (100, 8, 910)]:
        C = -(-N // chunk_len(N))
        assert fn(N, D, G) == 8 * (C * G * (1 + D + D * (D + 1) // 2) + (N + 1) // 2) == R.workspace_bytes(N, D, G), (N, D, G)
        assert 8 * C * G * (D * (D + 1) // 2) <= 2 ** 28
    for N, D, G in [(0, 3, 1), (100, 0, 5), (100, 65, 1), (100, 3, 0), (2000, 3, 1025), (2 ** 31, 3, 5), (-1, 3, 5), (100, 64, 16),
                    (100, 8, 911)]:
        assert fn(N, D, G) == 0 == R.workspace_bytes(N, D, G), (N, D, G)


# ---------------------------------------------------------------- the reference against numpy, and the fixtures' conditions
@pytest.mark.parametrize("fixture", R.FIXTURES, ids=IDS)
def test_reference_against_numpy_and_the_gap_the_gpu_test_relies_on(fixture):
    """Per live group: cov against np.cov(ddof=1) and the eigenvalues against eigvalsh within 1e-12 of the largest; the residual
    |C V^T - V^T L| and the orthogonality |V V^T - I| within 1e-12 (relative to the largest eigenvalue, resp. absolute); the
    eigenvalues descend and every axis has its largest entry positive.  Every live group's smallest adjacent eigenvalue gap is
    at least 1e-4 of the largest eigenvalue: tests/test_gpu_pca.py compares the vectors of all of them.  The vectors agree with
    numpy's eigh to 1e-9.  Dead groups follow the header's conventions."""
    x, group = R.fixture(*fixture)
    N, D, G = fixture[1:]
    out = R.fixture_fit(*fixture)
    member = R.members(x, group, G)
    worst = [0.0] * 5
    gap = float("inf")
    for g in range(G):
        mine = x[member == g].astype(np.float64)
        assert out["count"][g] == mine.shape[0]
        lam, comp = out["eigenvalues"][g], out["components"][g]
        if mine.shape[0] < 2:
            assert not out["cov"][g].any() and not lam.any() and np.array_equal(comp, np.eye(D)) and out["sweeps"][g] == 0
            assert np.array_equal(out["mean"][g], mine[0] if mine.shape[0] else np.zeros(D))
            continue
        C = np.cov(mine.T, ddof=1).reshape(D, D)
        w, U = np.linalg.eigh(C)
        w, U = w[::-1], U[:, ::-1]
        top = w[0]
        assert top > 0 and 0 <= out["sweeps"][g] < R.MAX_SWEEPS
        worst[0] = max(worst[0], np.abs(out["cov"][g] - C).max() / np.abs(C).max())
        worst[1] = max(worst[1], np.abs(lam - w).max() / top)
        worst[2] = max(worst[2], np.abs(out["cov"][g].dot(comp.T) - comp.T * lam).max() / top)
        worst[3] = max(worst[3], np.abs(comp.dot(comp.T) - np.eye(D)).max())
        assert (np.diff(lam) <= 0).all()
        at = np.abs(comp).argmax(1)
        assert (comp[np.arange(D), at] > 0).all()
        gap = min(gap, R.min_gap(lam))
        signs = np.sign((comp * U.T).sum(1))
        worst[4] = max(worst[4], np.abs(comp - signs[:, None] * U.T).max())
        assert np.abs(out["mean"][g] - mine.mean(0)).max() <= 1e-12 * max(1.0, np.abs(mine).max())
    print("%s: cov %.1e, eigenvalues %.1e, residual %.1e, orthogonality %.1e, vectors against eigh %.1e, smallest gap %.2e"
          % ((R.fixture_id(fixture),) + tuple(worst) + (gap,)))
    assert max(worst[:4]) <= 1e-12
    assert gap >= R.GAP
    assert worst[4] <= 1e-9
    live = out["count"][np.maximum(member, 0)] >= 2
    live &= member >= 0
    want = np.einsum("nt,npt->np", x.astype(np.float64) - out["mean"][np.maximum(member, 0)], out["components"][np.maximum(member, 0)])
    assert not out["proj"][~live].any()
    if live.any():
        assert np.abs(out["proj"][live] - want[live]).max() <= 1e-12 * max(1.0, np.abs(want[live]).max())


def test_reference_tournament_meets_every_pair_once():
    for D in range(1, 66):
        n = D + (D & 1)
        seen = []
        for s in range(n - 1):
            pairs = R.step_pairs(D, s)
            flat = [i for pair in pairs for i in pair]
            assert len(set(flat)) == len(flat) and all(p < q < D for p, q in pairs)       # disjoint within a step
            seen += pairs
        assert sorted(seen) == [(p, q) for p in range(D) for q in range(p + 1, D)]


def test_reference_special_matrices():
    """A diagonal matrix takes 0 sweeps and comes back sorted, equal values by ascending column; a matrix of rank below D, one
    with columns scaled over six decades and one that needs the full precision of the stopping rule decompose to 1e-12; a
    non-finite entry skips the matrix."""
    D = 9
    out = R.eigen(R.diagonal_cov(D))
    d = np.diag(R.diagonal_cov(D)[0])
    order = np.argsort(-d, kind="stable")
    assert out["sweeps"][0] == 0 and out["off_norm"][0] == 0 and np.array_equal(out["eigenvalues"][0], d[order])
    assert np.array_equal(out["components"][0], np.eye(D)[order])
    low = R.moments(R.low_rank(3, 200, 12, 4))
    scaled = R.moments((R.spread_points(4, 300, 7) * np.logspace(-3, 3, 7)).astype(np.float32))
    for name, m in (("rank 4 of 12", low), ("six decades", scaled)):
        got = R.eigen(m["cov"])
        C, lam, comp = m["cov"][0], got["eigenvalues"][0], got["components"][0]
        w = np.linalg.eigvalsh(C)[::-1]
        errs = (np.abs(lam - w).max() / w[0], np.abs(C.dot(comp.T) - comp.T * lam).max() / w[0], np.abs(comp.dot(comp.T) - np.eye(len(w))).max())
        print("%s: %d sweeps, eigenvalues %.1e, residual %.1e, orthogonality %.1e" % ((name, got["sweeps"][0]) + errs))
        assert max(errs) <= 1e-12 and 0 < got["sweeps"][0] < R.MAX_SWEEPS
    assert np.abs(R.eigen(low["cov"])["eigenvalues"][0][4:]).max() <= 1e-12 * R.eigen(low["cov"])["eigenvalues"][0][0]
    bad = scaled["cov"].copy()
    bad[0, 2, 3] = np.nan
    got = R.eigen(bad)
    assert got["sweeps"][0] == -1 and not got["eigenvalues"].any() and not got["components"].any() and got["off_norm"][0] == 0


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


CLUSTER = ["--cluster", "3", "--cluster_out", "k.npz"]
PCA = ["--pca", "p.npz"]
NAMES = ("pca", "pca_components", "pca_traverse", "pca_steps", "pca_span", "pca_per_class")


def test_pca_options_default_to_off_and_fill_in(tmp_path):
    base = _base(tmp_path)
    a = _infer().infer_arguments(base)
    assert tuple(vars(a)[n] for n in NAMES) == (None, None, None, None, None, False)
    a = _infer().infer_arguments(base + PCA)
    assert tuple(vars(a)[n] for n in NAMES) == ("p.npz", None, 0, 5, 2.0, False)        # components: z_dim, once it is known
    assert a.pose == "iw"
    a = _infer().infer_arguments(base + PCA + ["--pose", "q"])                            # --pose is allowed with --pca alone
    assert a.pose == "q"
    a = _infer().infer_arguments(base + CLUSTER + PCA + ["--pca_components", "2", "--pca_traverse", "1", "--pca_steps", "50",
                                                         "--pca_span", "0.5", "--pca_per_class"])
    assert tuple(vars(a)[n] for n in NAMES) == ("p.npz", 2, 1, 50, 0.5, True)
    assert _infer().INFER_MAX_PCA_STEPS == 50 and _infer().INFER_MAX_PCA_PARTIALS == 32768


REFUSALS = [
    (["--pca_components", "2"], "--pca_components needs --pca"),
    (["--pca_traverse", "2"], "--pca_traverse needs --pca"),
    (["--pca_steps", "2"], "--pca_steps needs --pca"),
    (["--pca_span", "2"], "--pca_span needs --pca"),
    (["--pca_per_class"], "--pca_per_class needs --pca"),
    (CLUSTER + ["--pca_per_class"], "--pca_per_class needs --pca"),
    (PCA + ["--pca_per_class"], "--pca_per_class needs --cluster"),
    (["--pca", "p.npy"], "--pca must end in .npz"),
    (PCA + ["--pca_components", "0"], "--pca_components must be >= 1"),
    (PCA + ["--pca_traverse=-1"], "--pca_traverse must be >= 0"),
    (PCA + ["--pca_steps", "0"], "--pca_steps must be in [1, 50]"),
    (PCA + ["--pca_steps", "51"], "--pca_steps must be in [1, 50]"),
    (PCA + ["--pca_span", "0"], "--pca_span must be a finite number > 0"),
    (PCA + ["--pca_span=-1"], "--pca_span must be a finite number > 0"),
    (PCA + ["--pca_span", "inf"], "--pca_span must be a finite number > 0"),
    (PCA + ["--pca_span", "nan"], "--pca_span must be a finite number > 0"),
    (["--pose", "q"], "--pose needs one of --aligned, --recon, --class_averages"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_pca_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_refusals_that_need_z_dim_are_made_by_check_request(tmp_path, capsys):
    """Where z_dim is known: --pca_components in 1..z_dim, --pca_traverse in 0..z_dim, a model without content latents, and a
    class count beyond the header's G D (D + 1) / 2 <= 32768 -- each exits with code 2; the same requests within the limits pass,
    and without --pca nothing of this is looked at."""
    infer = _infer()
    base = dict(images=2000, n=28, m=28, channels=1, rotate=True, translate=True, z_scale=1, split="test", ctf_rows=None)
    z3, z0, z64 = infer.SplitFacts(inf_dim=6, **base), infer.SplitFacts(inf_dim=3, **base), infer.SplitFacts(inf_dim=67, **base)

    def refused(extra, facts, message):
        args = infer.infer_arguments(_base(tmp_path) + extra)
        with pytest.raises(SystemExit) as e:
            infer.check_request(args, facts)
        assert e.value.code == 2 and message in capsys.readouterr().err

    def passes(extra, facts):
        assert infer.check_request(infer.infer_arguments(_base(tmp_path) + extra), facts) is None

    passes(PCA + ["--pca_components", "3", "--pca_traverse", "3"], z3)
    passes(PCA, z3)
    refused(PCA + ["--pca_components", "4"], z3, "--pca_components must be in [1, 3]")
    refused(PCA + ["--pca_traverse", "4"], z3, "--pca_traverse must be in [0, 3]")
    refused(PCA, z0, "this model has none (z_dim = 0)")
    passes([], z0)
    passes(["--cluster", "15", "--cluster_out", "k.npz"] + PCA + ["--pca_per_class"], z64)
    refused(["--cluster", "16", "--cluster_out", "k.npz"] + PCA + ["--pca_per_class"], z64, "16 classes x 2080 exceed 32768")
    passes(["--cluster", "16", "--cluster_out", "k.npz"] + PCA, z64)
    passes(["--cluster", "1024", "--cluster_out", "k.npz"] + PCA + ["--pca_per_class"], z3)


def test_a_pca_refusal_exits_with_code_2_before_the_library_is_loaded(tmp_path):
    """Through the real command line in a fresh process: exit code 2, no output file, and the process never loaded the kernel
    library."""
    argv = _base(tmp_path) + ["--pca_traverse", "2"]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert "--pca_traverse needs --pca" in out.stderr and "LIB True" in out.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"]


# ---------------------------------------------------------------- the traversal, and the build's check
def test_traverse_latents_against_the_formula():
    """z[p, s] = mean + (s / steps) * span * sqrt(max(lambda_p, 0)) * v_p in double, rounded to float once: bit-equal to the same
    expression in numpy float64 (every operation is one IEEE operation in both); a negative eigenvalue counts as 0; the middle
    frame is the mean; leading axes pass through."""
    from spatial_vae_amd import elbo as E
    rs = np.random.RandomState(5)
    K, D, Q, T, span = 3, 4, 2, 3, 1.5
    mean, lam = rs.randn(K, D), np.abs(rs.randn(K, D)) + 0.1
    lam[1, 1] = -1e-3
    comp = np.stack([np.linalg.qr(rs.randn(D, D))[0] for _ in range(K)])
    got = E.traverse_latents(torch.from_numpy(mean), torch.from_numpy(lam), torch.from_numpy(comp), Q, T, span)
    assert got.dtype == torch.float32 and tuple(got.shape) == (K, Q, 2 * T + 1, D)
    want = np.empty((K, Q, 2 * T + 1, D))
    for k in range(K):
        for p in range(Q):
            for s in range(-T, T + 1):
                want[k, p, s + T] = mean[k] + ((np.float64(s) / T) * span) * np.sqrt(max(lam[k, p], 0.0)) * comp[k, p]
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert np.array_equal(got.numpy()[:, :, T], np.broadcast_to(mean.astype(np.float32)[:, None], (K, Q, D)))
    assert np.array_equal(got.numpy()[1, 1], np.broadcast_to(mean[1].astype(np.float32), (2 * T + 1, D)))
    one = E.traverse_latents(torch.from_numpy(mean[0]), torch.from_numpy(lam[0]), torch.from_numpy(comp[0]), D, 1, 2.0)
    assert tuple(one.shape) == (D, 3, D) and np.array_equal(one.numpy(), E.traverse_latents(
        torch.from_numpy(mean[:1]), torch.from_numpy(lam[:1]), torch.from_numpy(comp[:1]), D, 1, 2.0).numpy()[0])
