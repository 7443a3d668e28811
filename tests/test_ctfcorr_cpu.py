"""CPU-only: the binding of include/svae_ctfcorr.h held to that header, the float64 reference of the CTF correction
(tests/ctfcorr_ref.py) held to the sign of the reference's training filters and to the recovery example it exists for, infer.py's
--ctf_correct / --wiener_lambda rules, and the CTF tables train_particles.build now hands on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ctfcorr_ref import apply_ref, example_image, finish_ref, power_ref, transfer
from helpers import GOLDEN_DIR
from test_binding_cpu import binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _infer():
    from spatial_vae_amd import infer
    return infer


def _golden_table():
    return np.loadtxt(os.path.join(GOLDEN_DIR, "ctf_table.txt"), ndmin=2)


def _norm(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


# ---------------------------------------------------------------- the header and its table
def test_ctfcorr_binding_matches_its_header():
    """What is include/svae_ctfcorr.h's own (the rules every added header shares are tests/test_binding_cpu.py's): five
    functions and their argument names, no struct; the header's two constants are _lib.CTF_MODE, and none of this adds an
    upper-case integer to the binding; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_ctfcorr.h")[1]
    assert _lib.HEADERS["svae_ctfcorr.h"] is _lib.CTFCORR_SIGNATURES
    assert H["structs"] == {} and len(H["functions"]) == 5
    assert H["constants"] == {"SVAE_CTF_" + k.upper(): v for k, v in _lib.CTF_MODE.items()} == {"SVAE_CTF_FLIP": 0, "SVAE_CTF_MULTIPLY": 1}
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_ctf_apply_workspace_bytes"] == ["B", "n", "m"]
    assert names["svae_ctf_apply"] == ["y", "params", "B", "n", "m", "scale", "mode", "out", "ws", "ws_bytes", "stream"]
    assert names["svae_ctf_power_update"] == ["params", "label", "B", "n", "m", "scale", "n_classes", "den", "stream"]
    assert names["svae_wiener_finish_workspace_bytes"] == ["n_classes", "n", "m"]
    assert names["svae_wiener_finish"] == ["sum", "den", "lambda", "n_classes", "n", "m", "average", "ws", "ws_bytes", "stream"]
    assert not [k for k in binding_constants(_lib) if "CTF" in k or "WIENER" in k]
    assert ops._POINTER_ARGS["svae_ctf_apply"] == (0, 1, 7, 8) and ops._POINTER_ARGS["svae_ctf_power_update"] == (0, 1, 7)
    assert ops._POINTER_ARGS["svae_wiener_finish"] == (0, 1, 6, 7)


def test_workspace_sizes_need_no_gpu():
    """The size calls are host arithmetic: 0 while 32 n m + 16 (n + m) bytes fit 160 KiB (up to 71 x 71), else one slice of two
    complex planes per workgroup, at most 512 workgroups."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    for fn in (L.svae_ctf_apply_workspace_bytes, L.svae_wiener_finish_workspace_bytes):
        assert fn(100, 40, 40) == 0 and fn(3, 71, 71) == 0 and fn(0, 200, 200) == 0
        assert fn(3, 72, 72) == 3 * 72 * 72 * 32 and fn(3, 96, 90) == 3 * 96 * 90 * 32
        assert fn(700, 72, 72) == 512 * 72 * 72 * 32


# ---------------------------------------------------------------- the reference, held to what it restates
def _correlate_zero_padded(img, filt):
    """The training path's use of a filter (a cross-correlation with zero padding k // 2, what conv2d does), in float64."""
    k = filt.shape[0]
    n, m = img.shape
    padded = np.zeros((n + k - 1, m + k - 1))
    padded[k // 2:k // 2 + n, k // 2:k // 2 + m] = img
    out = np.zeros((n, m))
    for p in range(k):
        for q in range(k):
            out += filt[p, q] * padded[p:p + n, q:q + m]
    return out


def test_sign_is_the_training_filters():
    """For the golden table at 40 x 40, the zero-padded cross-correlation of an image with the 39 x 39 filter the training path
    uses (oracle.ctf_oracle.ctf_filter) is closer to ifft2(H fft2(image)) than to its negative: H = -c.  The ordering is what is
    asserted; the distance that remains (0.18 and 0.25 of the norm for the first two rows, against 1.98 with the opposite sign)
    is the 39-point frequency grid and the zero padding of the training filters."""
    from oracle import ctf_oracle as C
    table = _golden_table()
    A = example_image()
    filters = C.ctf_filter({k: table[:, i] for i, k in enumerate(C.COLUMNS)}, 39, 39).astype(np.float64)
    H, _ = transfer(table, 40, 40)
    for i in range(len(table)):
        trained = _correlate_zero_padded(A, filters[i])
        mine = np.fft.ifft2(H[i] * np.fft.fft2(A)).real
        same, opposite = _norm(trained - mine) / _norm(trained), _norm(trained + mine) / _norm(trained)
        print("row %d: %.3f of the norm from H, %.3f from -H" % (i, same, opposite))
        assert same < opposite


@pytest.mark.parametrize("n,m", [(40, 40), (13, 10)])
def test_wiener_recovers_what_the_plain_mean_loses(n, m):
    """Six copies of one image through the six golden transfer functions, no noise, identity pose: the Wiener combination
    sum(H y) / (sum(H^2) + 1e-3) is closer to the image than the plain mean of the copies (0.012 against 0.72 of its norm at
    40 x 40, 0.0023 against 1.06 at 13 x 10); the ordering is what is asserted.  apply_ref(multiply) is H times the spectrum and
    flipping twice is the identity."""
    table = _golden_table()
    A = example_image()[:n, :m]
    A = A - A.mean()
    H, u = transfer(table, n, m)
    assert np.abs(u).min() >= 1e-9
    copies = np.fft.ifft2(H * np.fft.fft2(A)[None]).real
    from spatial_vae_amd import _lib
    assert sorted(_lib.CTF_MODE) == ["flip", "multiply"]        # the reference restates every mode the binding names
    g = apply_ref(copies, table, n, m, mode="multiply", dtype=np.float64)
    assert np.allclose(np.fft.fft2(g), H * np.fft.fft2(copies), rtol=0, atol=1e-9)
    twice = apply_ref(apply_ref(copies, table, n, m, mode="flip", dtype=np.float64), table, n, m, mode="flip", dtype=np.float64)
    assert np.abs(twice - copies).max() <= 1e-12
    den = power_ref([(table[:2], [0, 0]), (table[2:], [0, 0, 0, 0])], 1, n, m)
    assert np.array_equal(den, power_ref([(table, np.zeros(6, int))], 1, n, m)) and np.allclose(den[0], (H ** 2).sum(0), rtol=1e-14)
    wiener = finish_ref(g.sum(0)[None], den, 1e-3, n, m, dtype=np.float64)[0]
    plain = copies.mean(0)
    e_wiener, e_plain = _norm(wiener - A) / _norm(A), _norm(plain - A) / _norm(A)
    print("%dx%d: Wiener %.4f of the image's norm away, plain mean %.4f" % (n, m, e_wiener, e_plain))
    assert e_wiener < e_plain
    # a zero denominator contributes nothing, so lambda = 0 is legal (a frequency and its conjugate partner, or the real part
    # would bring half of the partner back)
    den0 = den.copy()
    den0[0, 1, 2] = den0[0, -1, -2] = 0.0
    out = finish_ref(g.sum(0)[None], den0, 0.0, n, m, dtype=np.float64)
    F = np.fft.fft2(out[0])
    assert np.isfinite(out).all() and abs(F[1, 2]) <= 1e-9 * np.abs(F).max()


# ---------------------------------------------------------------- infer.py's new options
def test_ctf_options_default_to_off(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    base = ["particles", "--state", str(state), "--out", "s.npz"]
    a = _infer().infer_arguments(base)
    assert (a.ctf_correct, a.wiener_lambda) == (None, None)
    a = _infer().infer_arguments(base + ["--ctf_correct", "flip", "--aligned", "a.npy"])
    assert (a.ctf_correct, a.wiener_lambda) == ("flip", None)
    a = _infer().infer_arguments(base + ["--ctf_correct", "wiener", "--class_averages", "c.npz"])
    assert (a.ctf_correct, a.wiener_lambda) == ("wiener", 1.0)
    a = _infer().infer_arguments(base + ["--ctf_correct", "wiener", "--class_averages", "c.npz", "--wiener_lambda", "0"])
    assert (a.ctf_correct, a.wiener_lambda) == ("wiener", 0.0)


@pytest.mark.parametrize("script,extra,message", [
    ("mnist", ["--ctf_correct", "flip", "--aligned", "a.npy"], "--ctf_correct is for particles"),
    ("galaxy", ["--ctf_correct", "wiener", "--class_averages", "c.npz"], "--ctf_correct is for particles"),
    ("particles", ["--ctf_correct", "flip"], "--ctf_correct flip needs one of --aligned, --class_averages"),
    ("particles", ["--ctf_correct", "flip", "--recon", "r.npy"], "--ctf_correct flip needs one of --aligned, --class_averages"),
    ("particles", ["--ctf_correct", "wiener", "--aligned", "a.npy"], "--ctf_correct wiener needs --class_averages"),
    ("particles", ["--ctf_correct", "both", "--aligned", "a.npy"], "invalid choice"),
    ("particles", ["--class_averages", "c.npz", "--wiener_lambda", "0.5"], "--wiener_lambda needs --ctf_correct wiener"),
    ("particles", ["--ctf_correct", "flip", "--class_averages", "c.npz", "--wiener_lambda", "0.5"], "--wiener_lambda needs --ctf_correct wiener"),
    ("particles", ["--ctf_correct", "wiener", "--class_averages", "c.npz", "--wiener_lambda", "-0.1"], "--wiener_lambda must be"),
    ("particles", ["--ctf_correct", "wiener", "--class_averages", "c.npz", "--wiener_lambda", "nan"], "--wiener_lambda must be"),
    ("particles", ["--ctf_correct", "wiener", "--class_averages", "c.npz", "--wiener_lambda", "inf"], "--wiener_lambda must be"),
])
def test_ctf_refusals_exit_with_code_2_before_the_library_is_loaded(tmp_path, script, extra, message):
    """Through the real command line in a fresh process: exit code 2, the reason on stderr, no output file, and the process
    never loaded the kernel library."""
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    argv = [script, "--state", str(state), "--out", "s.npz"] + extra
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert message in out.stderr and "LIB True" in out.stderr
    assert os.listdir(tmp_path) == ["a.ckpt"]


# ---------------------------------------------------------------- train_particles.build hands the tables on
def test_build_returns_the_ctf_tables_and_scale(tmp_path, monkeypatch):
    """train_particles.build on 8 synthetic particles with two written tables returns them as (P, 8) float64 arrays beside the
    filters built from the same arrays, and the --scale it built them at; without tables both are None.  The filter bank itself
    is a device computation (tests/test_gpu_ctf.py), so ops.ctf_filter is replaced by a recorder here."""
    import torch
    import train_particles
    from ctfcorr_ref import random_table
    from spatial_vae_amd import ops
    seen = []

    def recorder(table, n, m, scale=1.0, device=None):
        seen.append((np.array(table), n, m, scale))
        return torch.zeros(len(table), n, m)

    monkeypatch.setattr(ops, "ctf_filter", recorder)
    tables = {"train": random_table(8, 1), "test": random_table(2, 2)}
    for k, t in tables.items():
        np.savetxt(tmp_path / (k + ".txt"), t)
    small = ["x", "y", "--synthetic", "8", "--p-hidden-dim", "8", "--q-hidden-dim", "8"]
    args = train_particles.particle_arguments(small + ["--ctf-train", str(tmp_path / "train.txt"), "--ctf-test", str(tmp_path / "test.txt"),
                                                       "--scale", "1.5"])
    cfg = train_particles.build(args, torch.device("cpu"))
    for k, t in tables.items():
        got = cfg["ctf_params_" + k]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == t.shape and np.array_equal(got, t)
        assert cfg["ctf_" + k].shape == (len(t), 1, 39, 39)
    assert cfg["ctf_scale"] == 1.5 and isinstance(cfg["ctf_scale"], float)
    assert [(s[1], s[2], s[3]) for s in seen] == [(39, 39, 1.5)] * 2
    assert np.array_equal(seen[0][0], tables["train"]) and np.array_equal(seen[1][0], tables["test"])
    plain = train_particles.build(train_particles.particle_arguments(small), torch.device("cpu"))
    assert plain["ctf_params_train"] is None and plain["ctf_params_test"] is None and plain["ctf_scale"] == 1.0
    assert plain["ctf_train"] is None and plain["ctf_test"] is None
