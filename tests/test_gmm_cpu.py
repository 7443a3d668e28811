"""CPU-only: the binding of include/svae_gmm.h held to that header (functions, the record's mirror), the float64 reference of
the mixture (tests/gmm_ref.py) held to what a Gaussian mixture means and to the room the device bound of the kernel tests
leaves, and infer.py's --cluster_gmm options: their defaults and every refusal its argument parser makes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gmm_ref as G
import kmeans_ref as K
from test_binding_cpu import SCALARS, binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_IDS = ["N%d_D%d_k%d" % f[1:4] for f in G.FIXTURES]


def _infer():
    from spatial_vae_amd import infer
    return infer


# ---------------------------------------------------------------- the header and its table
def test_gmm_binding_matches_its_header():
    """What is include/svae_gmm.h's own (the rules every added header shares are tests/test_binding_cpu.py's, `rec` as the
    address of a record in device memory among them): three functions and their argument names, no constant and one struct,
    whose mirror _lib.GmmRecord has its fields, size and offsets; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_gmm.h")[1]
    assert _lib.HEADERS["svae_gmm.h"] is _lib.GMM_SIGNATURES
    assert H["constants"] == {} and list(H["structs"]) == ["svae_gmm_record"] and len(H["functions"]) == 3
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_gmm_workspace_bytes"] == ["N", "D", "k"]
    assert names["svae_gmm_init"] == ["x", "N", "D", "k", "label_in", "reg", "weight", "mean", "var", "resp", "rec", "ws", "ws_bytes",
                                      "stream"]
    assert names["svae_gmm_step"] == ["x", "N", "D", "k", "update", "reg", "tol", "weight", "mean", "var", "resp", "label", "loglik_point",
                                      "rec", "ws", "ws_bytes", "stream"]
    fields = H["structs"]["svae_gmm_record"]
    assert [f[2] for f in fields] == [f[0] for f in _lib.GmmRecord._fields_]
    assert [f[2] for f in fields] == ["iterations", "converged_at", "assigned", "dead", "loglik", "previous"]
    offset = 0
    for (base, pointer, field, length), (_, ctype) in zip(fields, _lib.GmmRecord._fields_):
        assert not pointer and length is None and ctype is SCALARS[base], field
        assert getattr(_lib.GmmRecord, field).offset == offset and ctypes.sizeof(ctype) == 8, field
        offset += 8
    assert ctypes.sizeof(_lib.GmmRecord) == offset == 48
    assert bytes(_lib.GmmRecord()) == bytes(48)                     # a fresh record is all zero bytes
    assert not [k for k in binding_constants(_lib) if "GMM" in k]
    assert ops._POINTER_ARGS["svae_gmm_init"] == (0, 4, 6, 7, 8, 9, 10, 11)
    assert ops._POINTER_ARGS["svae_gmm_step"] == (0, 7, 8, 9, 10, 11, 12, 13, 14)
    assert ops.GaussianMixture.RECORD_WORDS == 6


def test_workspace_size_needs_no_gpu():
    """Host arithmetic: 8 (C (2 + k (2 D + 1)) + k (D + 1) + 4) bytes with C = ceil(N / P), which covers the per-chunk partials
    C (1 + k (2 D + 1)) and the per-component iv and c; 0 outside the header's limits."""
    from spatial_vae_amd import _lib
    fn = _lib.lib().svae_gmm_workspace_bytes
    for N, D, k in [(1000, 3, 5), (4097, 1, 2), (262144, 2, 3), (262145, 2, 3), (2048, 64, 1024), (5, 1, 5), (2 ** 31 - 1, 1, 1)]:
        C = -(-N // K.chunk_len(N))
        assert fn(N, D, k) == 8 * (C * (2 + k * (2 * D + 1)) + k * (D + 1) + 4), (N, D, k)
        assert fn(N, D, k) >= 8 * (C * (1 + k * (2 * D + 1)) + k * D + k)
    for N, D, k in [(4, 3, 5), (100, 0, 5), (100, 65, 5), (100, 3, 0), (2000, 3, 1025), (2 ** 31, 3, 5), (-1, 3, 5)]:
        assert fn(N, D, k) == 0, (N, D, k)


# ---------------------------------------------------------------- the reference, held to what a mixture means
def test_reference_init_is_the_plain_class_mean_and_variance():
    x, u = K.blobs(0, 1000, 3, 5)
    km = K.fit(x, 5, u, 20)
    reg = 1e-6
    s = G.init(x, km["label"], km["centres"], reg)
    x64 = x.astype(np.float64)
    for j in range(5):
        mine = x64[km["label"] == j]
        assert np.abs(s["mean"][j] - mine.mean(0)).max() <= 1e-12
        assert np.abs(s["var"][j] - (mine.var(0) + reg)).max() <= 1e-12
        assert abs(s["weight"][j] - mine.shape[0] / 1000.0) <= 1e-12
    assert s["assigned"] == 1000 and s["dead"] == 0 and s["iterations"] == 0 and abs(s["weight"].sum() - 1) <= 1e-12
    assert np.array_equal(s["resp"].argmax(1), km["label"]) and (s["resp"].sum(1) == 1).all()


def test_reference_loglik_never_falls_and_a_frozen_fit_is_bit_identical():
    """Along a fit of overlapping blobs the log-likelihood never falls by more than 1e-12 |L|; rows of resp sum to 1; after
    converged_at further update steps change no bit of the state."""
    x, label_in, centres = G.fixture(*G.FIXTURES[2])
    state = G.init(x, label_in, centres, 1e-6)
    trace = []
    for i in range(400):
        state = G.step(x, state, 1, 1e-6, 1e-7)
        trace.append(state["loglik"])
        if state["converged_at"]:
            break
    assert 1 < state["converged_at"] == state["iterations"] < 400
    trace = np.array(trace)
    assert (np.diff(trace) >= -1e-12 * np.abs(trace[1:])).all() and trace[-1] > trace[0]
    assert np.abs(state["resp"].sum(1) - 1).max() <= 1e-14
    full = ((x.astype(np.float64)[:, None, :] - state["mean"][None]) ** 2 / state["var"][None]).sum(2)
    dens = np.log(state["weight"])[None] - 0.5 * (full + np.log(state["var"]).sum(1)[None] + 8 * np.log(2 * np.pi))
    top = dens.max(1)
    assert abs(state["loglik"] - (top + np.log(np.exp(dens - top[:, None]).sum(1))).sum()) <= 1e-10 * abs(state["loglik"])
    frozen = state
    for _ in range(3):
        again = G.step(x, frozen, 1, 1e-6, 1e-7)
        for key in ("weight", "mean", "var", "resp", "label", "loglik_point"):
            assert np.array_equal(np.asarray(again[key]).view(np.uint8), np.asarray(frozen[key]).view(np.uint8)), key
        assert [again[k] for k in ("iterations", "converged_at", "assigned", "dead", "loglik", "previous")] == \
            [frozen[k] for k in ("iterations", "converged_at", "assigned", "dead", "loglik", "previous")]
        frozen = again


def test_reference_dead_component_and_non_finite_point():
    """A label_in lacking class 2 gives a dead component that stays dead and is never a label; a NaN point is label -1 with an
    all-zero resp row, loglik_point 0 and no part in `assigned`."""
    x, u = K.blobs(1, 600, 3, 4)
    km = K.fit(x, 4, u, 10)
    label_in = km["label"].copy()
    label_in[label_in == 2] = 1
    x = x.copy()
    x[17, 1] = np.nan
    out = G.fit(x, label_in, km["centres"], 6, 1e-6, 0.0)
    assert out["dead"] == 1 and out["weight"][2] == 0 and not (out["label"] == 2).any() and (out["resp"][:, 2] == 0).all()
    assert np.array_equal(out["mean"][2], km["centres"][2]) and (out["var"][2] == 0).all()          # kept as they came in
    assert out["label"][17] == -1 and (out["resp"][17] == 0).all() and out["loglik_point"][17] == 0 and out["assigned"] == 599
    assert np.isfinite(out["loglik"]) and np.isfinite(out["mean"]).all() and abs(out["weight"].sum() - 1) <= 1e-12


PLANTED = [(0, 300, 3, 4), (4, 600, 17, 5), (6, 5000, 4, 3)]


@pytest.mark.parametrize("seed,N,D,k", PLANTED, ids=["N%d_D%d_k%d" % c[1:] for c in PLANTED])
def test_reference_recovers_planted_blobs(seed, N, D, k):
    """kmeans_ref.blobs, 20 k-means steps, 25 EM steps: every label is the planted one (components matched to the nearest planted
    centre) and every mean within 4 * 0.35 / sqrt(n_j) of its planted centre in every coordinate.  Observed: agreement 1.0 and
    worst mean errors of 2.69, 2.40 and 1.93 of 0.35 / sqrt(n_j)."""
    x, u = K.blobs(seed, N, D, k)
    x2, planted_label, centres = G.planted(seed, N, D, k)
    assert np.array_equal(x, x2)
    km = K.fit(x, k, u, 20)
    out = G.fit(x, km["label"], km["centres"], 25, 1e-6, 1e-8)
    match = np.array([((centres - out["mean"][j]) ** 2).sum(1).argmin() for j in range(k)])
    assert sorted(match.tolist()) == list(range(k))
    assert np.array_equal(match[out["label"]], planted_label)
    worst = 0.0
    for j in range(k):
        unit = 0.35 / np.sqrt((planted_label == match[j]).sum())
        worst = max(worst, np.abs(out["mean"][j] - centres[match[j]]).max() / unit)
    print("seed %d: worst mean error %.2f of 0.35 / sqrt(n_j)" % (seed, worst))
    assert worst <= 4.0


# ---------------------------------------------------------------- the fixtures of the kernel tests
@pytest.mark.parametrize("fixture", G.FIXTURES, ids=FIXTURE_IDS)
def test_fixtures_leave_room_under_the_device_bound(fixture):
    """What tests/test_gpu_gmm.py relies on.  (a) The fit run again with every exp and log result moved by a random +-4 ulp
    stays within 1e-12 of the exact one in weight, mean, var, resp (absolute) and loglik (relative): the device bound of 1e-10,
    the project's customary double bound, sits far above what a few ulps in exp and log can do.  Observed: at most 2.1e-14.
    (b) The smallest top-two gap of the scores a is >= 1e-6 at every E part, so the label comparison leaves no point out.
    Observed: at least 3.9e-4.  (c) No deciding gain is within 1e-10 |L| of tol |L|, so converged_at must be equal."""
    x, label_in, centres = G.fixture(*fixture)
    states = G.fixture_states(*fixture)
    fn = G.Ulps(fixture[0] + 50)
    moved = G.init(x, label_in, centres, G.FIT_REG)
    spread = 0.0
    for want in states[1:-1]:
        moved = G.step(x, moved, 1, G.FIT_REG, G.FIT_TOL, fn)
        for key in ("weight", "mean", "var", "resp"):
            spread = max(spread, float(np.abs(moved[key] - want[key]).max()))
        spread = max(spread, abs(moved["loglik"] - want["loglik"]) / abs(want["loglik"]))
        assert moved["iterations"] == want["iterations"] and moved["converged_at"] == want["converged_at"]
    gap = min(G.top_two_gap(s["a"]) for s in states[1:])
    decided = [(s["gain"], s["loglik"]) for s in states[1:-1] if s["gain"] is not None]
    margin = min(abs(g - G.FIT_TOL * abs(L)) / abs(L) for g, L in decided)
    print("spread under +-4 ulp %.2e, smallest top-two gap %.3g, deciding gains off tol |L| by at least %.2e |L|" % (spread, gap, margin))
    assert spread < 1e-12
    assert gap >= 1e-6
    assert decided and margin > 1e-10


# ---------------------------------------------------------------- infer.py's new options
def _base(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    return ["mnist", "--state", str(state), "--out", "s.npz"]


CLUSTER = ["--cluster", "3", "--cluster_out", "k.npz"]


def test_gmm_options_default_to_off_and_fill_in(tmp_path):
    base = _base(tmp_path)
    a = _infer().infer_arguments(base + CLUSTER)
    assert (a.cluster_gmm, a.cluster_gmm_reg, a.cluster_gmm_tol, a.cluster_min_resp) == (None,) * 4
    a = _infer().infer_arguments(base + CLUSTER + ["--cluster_gmm", "20"])
    assert (a.cluster_gmm, a.cluster_gmm_reg, a.cluster_gmm_tol, a.cluster_min_resp) == (20, 1e-6, 1e-8, 0.0)
    a = _infer().infer_arguments(base + CLUSTER + ["--cluster_gmm", "1000", "--cluster_gmm_reg", "1e-3", "--cluster_gmm_tol", "0",
                                                   "--cluster_min_resp", "0.9"])
    assert (a.cluster_gmm, a.cluster_gmm_reg, a.cluster_gmm_tol, a.cluster_min_resp) == (1000, 1e-3, 0.0, 0.9)
    assert _infer().INFER_MAX_GMM_ITERS == 1000 and _infer().INFER_MAX_GMM_RESP == 2 ** 28


REFUSALS = [
    (["--cluster_gmm", "5"], "--cluster_gmm needs --cluster"),
    (CLUSTER + ["--cluster_gmm_reg", "1e-3"], "--cluster_gmm_reg needs --cluster_gmm"),
    (CLUSTER + ["--cluster_gmm_tol", "1e-3"], "--cluster_gmm_tol needs --cluster_gmm"),
    (CLUSTER + ["--cluster_min_resp", "0.5"], "--cluster_min_resp needs --cluster_gmm"),
    (CLUSTER + ["--cluster_gmm", "0"], "--cluster_gmm must be in [1, 1000]"),
    (CLUSTER + ["--cluster_gmm", "1001"], "--cluster_gmm must be in [1, 1000]"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_gmm_reg", "0"], "--cluster_gmm_reg must be a finite number > 0"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_gmm_reg", "inf"], "--cluster_gmm_reg must be a finite number > 0"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_gmm_reg", "nan"], "--cluster_gmm_reg must be a finite number > 0"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_gmm_tol=-1e-9"], "--cluster_gmm_tol must be a finite number >= 0"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_gmm_tol", "inf"], "--cluster_gmm_tol must be a finite number >= 0"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_min_resp", "1"], "--cluster_min_resp must be in [0, 1)"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_min_resp=-0.1"], "--cluster_min_resp must be in [0, 1)"),
    (CLUSTER + ["--cluster_gmm", "5", "--cluster_min_resp", "nan"], "--cluster_min_resp must be in [0, 1)"),
]


@pytest.mark.parametrize("extra,message", REFUSALS)
def test_gmm_refusals_are_made_by_the_parser(tmp_path, capsys, extra, message):
    """infer_arguments exits with code 2 and the reason on stderr."""
    with pytest.raises(SystemExit) as e:
        _infer().infer_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_too_many_responsibilities_are_refused_before_anything_is_allocated(tmp_path, capsys):
    """images * K > 2^28: check_request, a function of the arguments and the facts alone, exits with code 2."""
    infer = _infer()
    args = infer.infer_arguments(_base(tmp_path) + ["--cluster", "1024", "--cluster_out", "k.npz", "--cluster_gmm", "5"])
    base = dict(n=28, m=28, channels=1, rotate=True, translate=True, inf_dim=6, z_scale=1, split="test", ctf_rows=None)
    assert infer.check_request(args, infer.SplitFacts(images=2 ** 18, **base)) is None
    with pytest.raises(SystemExit) as e:
        infer.check_request(args, infer.SplitFacts(images=2 ** 18 + 1, **base))
    assert e.value.code == 2 and "exceed 2^28" in capsys.readouterr().err
    plain = infer.infer_arguments(_base(tmp_path) + ["--cluster", "1024", "--cluster_out", "k.npz"])
    assert infer.check_request(plain, infer.SplitFacts(images=2 ** 18 + 1, **base)) is None


def test_a_gmm_refusal_exits_with_code_2_before_the_library_is_loaded(tmp_path):
    """Through the real command line in a fresh process: exit code 2, no output file, and the process never loaded the kernel
    library."""
    argv = _base(tmp_path) + ["--cluster_gmm", "5"]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert "--cluster_gmm needs --cluster" in out.stderr and "LIB True" in out.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt"]
