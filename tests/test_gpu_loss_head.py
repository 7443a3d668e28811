"""The kernels behind the decoder, each called on its own and compared with float64 on the CPU (tests/ref64.py):
gaussian_ctf_lds_kernel and gaussian_kernel (svae_gaussian_loglik), bce_kernel and the fused logits_finish_bce_kernel +
loglik_reduce_kernel, latent_fwd/bwd_kernel, elbo_head_fwd/bwd_kernel and colsum_reduce_kernel behind svae_colsum.

Bounds are formed at run time from a reference's own fp32 error, never from the kernel's output: a kernel may be 4x as far
from float64 as the fp32 CPU evaluation of the same formula on the same inputs (it adds as many terms, FMA-contracted and in
another grouping; random-walk rounding differs by a small factor between orders), with a floor of a few units of 2^-24 where
that evaluation happens to be exact.  Errors are helpers.rel_err: max |error| over the largest reference entry.

Which Gaussian kernel a case runs is not reported by the library (both forms are the profile kind 'gaussian'); it follows
from the LDS size svae_gaussian_loglik computes, restated as ref64.ctf_lds_bytes and asserted per case in
test_ctf_cases_reach_the_intended_launch.  The Bernoulli cases assert theirs through svae_profile_read kinds.

The maxima observed on the MI355X are recorded in each test's docstring (error, and the bound it was held to)."""
import ctypes
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import ref64
from helpers import rel_err
from loss_head_child import run_ctf
from ref64 import U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_IDS = ["n%d_k%d" % p for p in ref64.CTF_PAIRS]
SENTINEL = -12345.5


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bound(oracle_err, floor_units=8):
    return max(4.0 * oracle_err, floor_units * U)


def _default_ctf_env():
    """The parent process must run the library's default choice of CTF kernel, or the LDS cases below test nothing."""
    assert not os.environ.get("SVAE_CTF_LDS", "1").startswith("0"), "run this file without SVAE_CTF_LDS=0"


# ---------------------------------------------------------------------------------------------------------------------
# 1. Gaussian log-likelihood with a CTF
# ---------------------------------------------------------------------------------------------------------------------
def test_ctf_cases_reach_the_intended_launch():
    """svae_gaussian_loglik takes the LDS kernel up to 150 KB of dynamic LDS and sets the kernel's attribute above 48 KB;
    the sizes of the table's rows, from the library's own formula."""
    form = {p: ref64.ctf_form(*p) for p in ref64.CTF_PAIRS}
    assert [p for p in ref64.CTF_PAIRS if form[p] == "lds_attr"] == [(56, 55), (80, 79)]
    assert [p for p in ref64.CTF_PAIRS if form[p] == "global"] == [(88, 87)]
    assert (ref64.ctf_lds_bytes(56, 55), ref64.ctf_lds_bytes(80, 79), ref64.ctf_lds_bytes(88, 87)) == (66880, 133984, 161472)
    assert all(ref64.ctf_form(*p) != "global" for p in ref64.CTF_BOTH_FORMS)   # the child's cases differ from the parent's
    _default_ctf_env()


@functools.lru_cache(maxsize=None)
def _ctf_integer_case(n, k, masked):
    img, tgt, f = ref64.ctf_inputs_integer(n, k)
    ref = ref64.gaussian64(img, tgt, ref64.ctf_mask(n, masked), f)
    ref64.assert_fp32_exact(ref, f)
    return img, tgt, f, ref


@functools.lru_cache(maxsize=None)
def _ctf_random_case(n, k, masked):
    from oracle import elbo_oracle as O
    img, tgt, f = ref64.ctf_inputs_random(n, k)
    mask = ref64.ctf_mask(n, masked)
    ref = ref64.gaussian64(img, tgt, mask, f)
    o_ll, o_dll = O.gaussian_loglik(img, tgt, mask=mask, ctf=f[:, None])
    bound = dict(loglik=_bound(rel_err(o_ll, ref["loglik"])), dll=_bound(rel_err(o_dll, ref["dll"])))
    return img, tgt, f, ref, bound


@pytest.mark.parametrize("want_dll", [True, False], ids=["dll", "nodll"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("pair", ref64.CTF_PAIRS, ids=PAIR_IDS)
def test_ctf_loglik_exact_on_integers(pair, masked, want_dll):
    """Integer images, targets and taps: every fp32 intermediate is exact (asserted on the float64 reference itself), so
    loglik and dll must EQUAL float64 -- a wrong, shifted, dropped or doubled tap cannot hide in rounding.
    MI355X: equal in all 52 cases."""
    _default_ctf_env()
    n, k = pair
    img, tgt, f, ref = _ctf_integer_case(n, k, masked)
    ll, dll = run_ctf(img, tgt, f, ref64.ctf_mask(n, masked), want_dll)
    assert np.array_equal(ll.astype(np.float64), ref["loglik"]), (ll, ref["loglik"])
    if want_dll:
        bad = np.argwhere(dll.astype(np.float64) != ref["dll"])
        assert bad.size == 0, "dll differs at (image, pixel) %s ..." % bad[:5].tolist()


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("pair", [p for p in ref64.CTF_PAIRS if p[1] <= 11], ids=lambda p: "n%d_k%d" % p)
def test_ctf_one_hot_images_pick_the_right_taps(pair, masked):
    """A single 1 at each corner and at the centre, all taps distinct: the filtered image IS a window of the filter, placed
    by the padding, so a mirrored, transposed or shifted read gives other integers.  Exact as above.  MI355X: equal."""
    _default_ctf_env()
    n, k = pair
    img, tgt, f = ref64.ctf_inputs_one_hot(n, k)
    mask = ref64.ctf_mask(n, masked)
    ref = ref64.gaussian64(img, tgt, mask, f)
    ref64.assert_fp32_exact(ref, f)
    ll, dll = run_ctf(img, tgt, f, mask)
    assert np.array_equal(ll.astype(np.float64), ref["loglik"]), (ll, ref["loglik"])
    assert np.array_equal(dll.astype(np.float64), ref["dll"])


@pytest.mark.parametrize("want_dll", [True, False], ids=["dll", "nodll"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("pair", ref64.CTF_PAIRS, ids=PAIR_IDS)
def test_ctf_loglik_rounded_against_float64(pair, masked, want_dll):
    """Normal images, targets and filters (normal / k plus a unit centre tap).  The kernel may be 4x as far from float64 as
    oracle.elbo_oracle.gaussian_loglik (numpy fp32) is on the same inputs, floor 8 * 2^-24.
    MI355X maxima over the 52 cases: loglik 1.5e-7 (n = 6, k = 11; bound 4.8e-7), dll 2.6e-6 at (88, 87) (bound 1.0e-5);
    never above 0.32 of the bound (dll at (9, 9): 3.2e-7 of 1.0e-6)."""
    _default_ctf_env()
    n, k = pair
    img, tgt, f, ref, bound = _ctf_random_case(n, k, masked)
    ll, dll = run_ctf(img, tgt, f, ref64.ctf_mask(n, masked), want_dll)
    errs = dict(loglik=rel_err(ll, ref["loglik"]))
    if want_dll:
        errs["dll"] = rel_err(dll, ref["dll"])
    print("ctf_rounded n=%d k=%d mask=%d %s bound %s" % (n, k, masked, errs, bound))
    for name, e in errs.items():
        assert e <= bound[name], (name, e, bound[name])


@pytest.fixture(scope="module")
def global_form(tmp_path_factory):
    """Results of tests/loss_head_child.py under SVAE_CTF_LDS=0: one fresh process for all the both-forms cases."""
    out = str(tmp_path_factory.mktemp("loss_head") / "ctf_global.npz")
    env = dict(os.environ, SVAE_CTF_LDS="0")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "loss_head_child.py"), "ctf", out], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert json.loads(run.stdout.strip().splitlines()[-1])["SVAE_CTF_LDS"] == "0"
    with np.load(out, allow_pickle=False) as z:
        return {key: z[key] for key in z.files}


@pytest.mark.parametrize("pair", ref64.CTF_BOTH_FORMS, ids=lambda p: "n%d_k%d" % p)
def test_ctf_lds_and_global_forms_agree(pair, global_form):
    """gaussian_kernel (child process, SVAE_CTF_LDS=0) against gaussian_ctf_lds_kernel (this process) on identical inputs,
    mask and dll on.  The filtered image and dll are the same sums in the same (u, v) order in both: dll must be equal bit
    for bit.  loglik is summed over the pixels by 256 threads in one form and by 512 in the other: equal bit for bit while
    every thread holds at most one pixel (N <= 256), within the rounded bound above it.  On integer inputs the global form
    must equal float64 like the LDS form does.  MI355X: dll equal in all four; loglik equal at N = 25 and 100, 1 ulp apart
    at most at N = 1681 and 3136."""
    _default_ctf_env()
    n, k = pair
    img, tgt, f, ref, bound = _ctf_random_case(n, k, True)
    ll, dll = run_ctf(img, tgt, f, ref64.ctf_mask(n, True))
    g_ll, g_dll = global_form["random_%d_%d_loglik" % pair], global_form["random_%d_%d_dll" % pair]
    print("ctf_forms n=%d k=%d loglik lds %s global %s" % (n, k, ll.tolist(), g_ll.tolist()))
    assert np.array_equal(dll, g_dll)
    assert rel_err(g_dll, ref["dll"]) <= bound["dll"] and rel_err(g_ll, ref["loglik"]) <= bound["loglik"]
    if n * n <= 256:
        assert np.array_equal(ll, g_ll)
    else:
        assert rel_err(ll, g_ll.astype(np.float64)) <= bound["loglik"]
    _, _, _, iref = _ctf_integer_case(n, k, True)
    assert np.array_equal(global_form["integer_%d_%d_loglik" % pair].astype(np.float64), iref["loglik"])
    assert np.array_equal(global_form["integer_%d_%d_dll" % pair].astype(np.float64), iref["dll"])


def test_ctf_call_writes_nothing_outside_its_buffers():
    """One direct svae_gaussian_loglik call at (n, k) = (10, 9): loglik, dll and the workspace each sit inside a larger
    buffer of sentinels; outside [0, B), [0, B N) and svae_gaussian_workspace_bytes nothing may change."""
    from spatial_vae_amd import _lib
    _default_ctf_env()
    L = _lib.lib()
    n, k, B = 10, 9, ref64.CTF_B
    N = n * n
    img, tgt, f, ref, bound = _ctf_random_case(n, k, True)
    dev = _dev()
    G = 64
    ws_bytes = L.svae_gaussian_workspace_bytes(B, N)
    assert ws_bytes >= 2 * B * N * 4
    ll_buf = torch.full((G + B + G,), SENTINEL, device=dev)
    dll_buf = torch.full((G + B * N + G,), SENTINEL, device=dev)
    ws_buf = torch.full((256 + ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    y, t, fd = (torch.from_numpy(a).to(dev) for a in (img, tgt, f))
    m = torch.from_numpy(ref64.ctf_mask(n, True)).to(dev, torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(L.svae_gaussian_loglik(B, N, 1, y.data_ptr(), t.data_ptr(), m.data_ptr(), fd.data_ptr(), k,
                                          ll_buf.data_ptr() + 4 * G, dll_buf.data_ptr() + 4 * G, ws_buf.data_ptr() + 256,
                                          ws_bytes, _stream()))
    torch.cuda.synchronize()
    ll_buf, dll_buf, ws_buf = ll_buf.cpu().numpy(), dll_buf.cpu().numpy(), ws_buf.cpu().numpy()
    for buf, size in ((ll_buf, B), (dll_buf, B * N)):
        assert (buf[:G] == SENTINEL).all() and (buf[G + size:] == SENTINEL).all()
    assert (ws_buf[:256] == 0xA5).all() and (ws_buf[256 + ws_bytes:] == 0xA5).all()
    ll, dll = run_ctf(img, tgt, f, ref64.ctf_mask(n, True))
    assert np.array_equal(ll_buf[G:G + B], ll) and np.array_equal(dll_buf[G:G + B * N].reshape(B, N), dll)
    assert rel_err(dll, ref["dll"]) <= bound["dll"]


# ---------------------------------------------------------------------------------------------------------------------
# 2. Gaussian log-likelihood without a CTF
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("C", [1, 2])
def test_gaussian_loglik_without_ctf(C, N, masked):
    """C = 2: the first N entries of a row are the mean, the last N the log-variance (spread over [-8, 8]).  Bound measured
    against oracle.elbo_oracle.gaussian_loglik as in section 1; masked-out pixels give exactly 0 in both halves of dll.
    MI355X maxima: loglik 9.1e-8, dll 1.1e-7, both against the floor of 4.8e-7."""
    from oracle import elbo_oracle as O
    from spatial_vae_amd import ops
    B = 3
    rs = np.random.RandomState(100 * N + 10 * C + masked)
    y = rs.normal(size=(B, N * C)).astype(np.float32)
    if C == 2:
        y[:, N:] = rs.uniform(-8, 8, size=(B, N)).astype(np.float32)
        y[0, N], y[0, 2 * N - 1] = -8.0, 8.0
    tgt = rs.normal(size=(B, N)).astype(np.float32)
    mask = None
    if masked:
        mask = rs.uniform(size=N) < 0.7
        mask[0] = True
        mask[-1] = N == 1
    ref = ref64.gaussian64(y, tgt, mask)
    o_ll, o_dll = O.gaussian_loglik(y, tgt, mask=mask)
    yd = torch.from_numpy(y).to(_dev()).requires_grad_(True)
    ll = ops.gaussian_loglik(yd, torch.from_numpy(tgt).to(_dev()), None if mask is None else torch.from_numpy(mask).to(_dev()))
    ll.sum().backward()
    dll = yd.grad.cpu().numpy()
    errs = dict(loglik=rel_err(ll.detach().cpu().numpy(), ref["loglik"]), dll=rel_err(dll, ref["dll"]))
    bound = dict(loglik=_bound(rel_err(o_ll, ref["loglik"])), dll=_bound(rel_err(o_dll, ref["dll"])))
    print("gaussian_plain C=%d N=%d mask=%d %s bound %s" % (C, N, masked, errs, bound))
    assert errs["loglik"] <= bound["loglik"] and errs["dll"] <= bound["dll"], (errs, bound)
    if masked:
        off = ~mask
        assert off.any() or N == 1
        for half in range(C):
            assert (dll[:, half * N:(half + 1) * N][:, off] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Bernoulli log-likelihood
# ---------------------------------------------------------------------------------------------------------------------
# 1 rounding in s - t (2^-24 relative; exact when s and t are within a factor 2), max() exact, one division (correctly
# rounded, or 2.5 ulp = 5 * 2^-24 where the compiler's fast division is used): <= 6 * 2^-24 of each entry, held to 8.
DLL_ELEMENTWISE = 8 * U


def _bce_inputs(B, n, seed):
    rs = np.random.RandomState(seed)
    s = rs.uniform(size=B * n).astype(np.float32)
    s = np.clip(s, np.float32(1e-6), np.float32(1.0 - 1e-6))
    t = (np.floor(rs.uniform(size=B * n) * 255) / 255).astype(np.float32)
    special = [0.0, 1.0, float(np.float32(1.4e-45)), 2.0 ** -24, 1.0 - 2.0 ** -24]
    for i, v in enumerate(special):                         # fixed positions; with B * n < 5 the later values win
        s[(7 * i) % (B * n)] = np.float32(v)
    t[(7 * 1 + 1) % (B * n)] = 0.0
    t[(7 * 2 + 2) % (B * n)] = 1.0
    return s.reshape(B, n), t.reshape(B, n)


def _assert_dll_elementwise(dll, y, t):
    want = ref64.bce_dll64(y, t)
    err = np.abs(dll.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
    assert np.isfinite(dll).all()
    assert err.max() <= DLL_ELEMENTWISE, (err.max(), np.argmax(err))
    return float(err.max())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 784, 3 * 1089])
def test_bce_loglik_standalone(n):
    """ops.bce_loglik (bce_kernel) with y_hat at 0, 1, the smallest denormal, 2^-24 and 1 - 2^-24 among ordinary values and
    targets k / 255 including 0 and 1.  loglik against float64 with the clamps at -100, bound 4x the error of
    oracle.elbo_oracle.bce_loglik (floor 8 * 2^-24); dll entry by entry against -(s - t) / max((1 - s) s, 1e-12).
    MI355X maxima: loglik 1.3e-7 (bound 4.8e-7), dll 1.1e-7 of an entry (bound 4.8e-7)."""
    from oracle import elbo_oracle as O
    from spatial_vae_amd import ops
    B = 3
    s, t = _bce_inputs(B, n, 300 + n)
    ref = ref64.bce64(s, t)
    o_ll, _ = O.bce_loglik(s, t)
    sd = torch.from_numpy(s).to(_dev()).requires_grad_(True)
    ll = ops.bce_loglik(sd, torch.from_numpy(t).to(_dev()))
    ll.sum().backward()
    err, bound = rel_err(ll.detach().cpu().numpy(), ref), _bound(rel_err(o_ll, ref))
    derr = _assert_dll_elementwise(sd.grad.cpu().numpy(), s, t)
    print("bce_standalone n=%d loglik %.3e bound %.3e dll %.3e" % (n, err, bound, derr))
    assert err <= bound, (err, bound)
    nograd = ops.bce_loglik(torch.from_numpy(s).to(_dev()), torch.from_numpy(t).to(_dev()))     # dll not requested
    assert torch.equal(nograd, ll.detach())


def _small_decoder(C, seed, out_scale=1.0):
    import contextlib
    import io
    import spatial_vae_amd.models as M
    torch.manual_seed(seed)                      # nn.Linear's init draws from the CPU generator
    with contextlib.redirect_stdout(io.StringIO()):
        p = M.SpatialGenerator(2, 32, n_out=C, num_layers=2, activation=nn.Tanh)
    if out_scale != 1.0:
        with torch.no_grad():
            p.layers[-2].weight.mul_(out_scale)
    return p.to(_dev())


def _decode(p, grid, theta, dx, z, target=None):
    """ops.decoder on the posed grid with the module's parameters; (y, logits[, loglik])."""
    from spatial_vae_amd import ops
    hidden_lin, out_lin = p._linears()
    hidden = [t for m in hidden_lin for t in (m.weight, m.bias)]
    return ops.decoder(p._spec, theta.shape[0], None, grid, theta, dx, z, p.coord_linear.weight, p.coord_linear.bias,
                       p.latent_linear.weight, None, out_lin.weight, out_lin.bias, hidden, bce_target=target)


FUSED = [(n, C, 2, 1.0) for n in (16, 17, 23, 32, 33, 40, 45) for C in (1, 2, 3)] + [(257, 1, 1, 1.0), (33, 2, 2, 600.0)]


@pytest.mark.parametrize("n,C,B,out_scale", FUSED, ids=["n%d_C%d%s" % (n, C, "_saturated" if sc != 1 else "") for n, C, _, sc in FUSED])
def test_bce_loglik_fused_into_the_decoder(n, C, B, out_scale):
    """ops.decoder(..., bce_target=) on a 32-wide two-layer tanh net over n x n posed grids: N = 256 (256 threads), 289
    (512), 529 and 1024 (1024 threads, one chunk), 1089 / 1600 / 2025 (2 chunks, ragged where N is odd), 66 049 (the 64-chunk
    cap, a second trip of the pixel loop); C = 3 is bce_kernel behind out_fwd_kernel.  loglik against float64 of the y the
    call returned; the kept dll bit-equal to a plain ops.bce_loglik on that y; y and logits against the call without a
    target.  One case scales the output weights so that pixels saturate to exactly 0 and 1.  MI355X maxima over the 23
    cases: loglik 1.1e-7 (bound 4.8e-7), dll 1.2e-7 of an entry and bit-equal to bce_kernel's, y and logits identical."""
    from oracle import elbo_oracle as O
    from spatial_vae_amd import ops
    p = _small_decoder(C, 40 + n + C, out_scale)
    rs = np.random.RandomState(500 + n + C)
    dev = _dev()
    grid = torch.from_numpy(cases.coord_grid(n, n).astype(np.float32)).to(dev)
    theta = torch.from_numpy(rs.uniform(-3, 3, size=B).astype(np.float32)).to(dev)
    dx = torch.from_numpy(rs.normal(size=(B, 2)).astype(np.float32) * 0.1).to(dev)
    z = torch.from_numpy(rs.normal(size=(B, 2)).astype(np.float32)).to(dev)
    tgt_np = (np.floor(rs.uniform(size=(B, n * n, C)) * 255) / 255).astype(np.float32)
    tgt_np[0, :2, 0] = (0.0, 1.0)
    tgt = torch.from_numpy(tgt_np).to(dev)
    y, logits, ll = _decode(p, grid, theta, dx, z, tgt)
    assert ll.grad_fn is not None
    # the dll the fused call keeps for its backward pass: position of `dll` in _Decoder.forward's save_for_backward
    kept = ll.grad_fn.saved_tensors[13]
    assert kept.shape == y.shape
    y_np = y.detach().cpu().numpy()
    if out_scale != 1.0:
        assert (y_np == 0.0).any() and (y_np == 1.0).any()
    ref = ref64.bce64(y_np, tgt_np)
    o_ll, _ = O.bce_loglik(y_np, tgt_np)
    err, bound = rel_err(ll.detach().cpu().numpy(), ref), _bound(rel_err(o_ll, ref))
    yd = y.detach().clone().requires_grad_(True)
    ll2 = ops.bce_loglik(yd, tgt)
    ll2.sum().backward()
    assert torch.equal(kept, yd.grad)
    derr = _assert_dll_elementwise(kept.cpu().numpy(), y_np, tgt_np)
    ll.sum().backward()                                     # the fused backward runs from the kept dll
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in p.parameters())
    with torch.no_grad():
        y0, logits0 = _decode(p, grid, theta, dx, z)
    ey, el = rel_err(y_np, y0.cpu().numpy()), rel_err(logits.cpu().numpy(), logits0.cpu().numpy())
    print("bce_fused n=%d C=%d loglik %.3e bound %.3e dll %.3e y %.3e logits %.3e" % (n, C, err, bound, derr, ey, el))
    assert err <= bound, (err, bound)
    assert ey <= 2 * U and el <= 2 * U, (ey, el)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_bce_cases_run_the_intended_kernel(C):
    """svae_profile_read kinds of one forward call at n = 17: C <= 2 finishes inside 'out_fwd' (logits_finish_bce_kernel)
    with no 'bce' launch; C = 3 runs bce_kernel ('bce') behind out_fwd_kernel."""
    from spatial_vae_amd import _lib
    p = _small_decoder(C, 3)
    dev = _dev()
    n, B = 17, 2
    grid = torch.from_numpy(cases.coord_grid(n, n).astype(np.float32)).to(dev)
    theta, dx, z = torch.zeros(B, device=dev), torch.zeros(B, 2, device=dev), torch.ones(B, 2, device=dev)
    tgt = torch.full((B, n * n, C), 0.5, device=dev)
    _lib.profile_enable(2)
    try:
        _lib.profile_read()
        with torch.no_grad():
            _decode(p, grid, theta, dx, z, tgt)
        kinds = _lib.profile_read()
    finally:
        _lib.profile_enable(0)
        _lib.profile_read()
    assert "out_fwd" in kinds and ("bce" in kinds) == (C == 3), kinds


# ---------------------------------------------------------------------------------------------------------------------
# 4. Latent head and the minibatch scalars
# ---------------------------------------------------------------------------------------------------------------------
def _latent_cases():
    out = []
    for rotate, translate, mu_penalty in itertools.product((False, True), (False, True), (0, 1)):
        pose = int(rotate) + 2 * int(translate)
        infs = sorted({d for d in (pose, pose + 1, 5, 23) if d >= max(pose, 1)})
        out += [(rotate, translate, mu_penalty, inf, 3) for inf in infs]
        out += [(rotate, translate, mu_penalty, 5, B) for B in (1, 255, 256, 257, 600)]
    return out


LATENT = _latent_cases()
SUBSETS = [("theta", "dx", "zc", "kl"), ("kl",), ("theta",), ("dx",), ("zc",)]


@pytest.mark.parametrize("rotate,translate,mu_penalty,inf,B", LATENT,
                         ids=["r%d_t%d_mp%d_inf%d_B%d" % tuple(map(int, c)) for c in LATENT])
def test_latent_head_against_float64(rotate, translate, mu_penalty, inf, B):
    """ops.latent_head / svae_latent_forward / _backward against torch float64 autograd of the reference's formulas, for
    (z_scale, theta_prior) = (1, pi) and (0.5, 0.5), dx_scale 0.1, log-std in [-2, 1].  Upstream gradients: all of them
    through autograd, and the subsets {all, kl, theta, dx, zc} through the C ABI with NULL for the absent ones.
    Bound per output: 16 * 2^-24 plus 4x the error of the same formulas in torch float32 on the CPU.
    MI355X: the worst error over the 70 cases is 0.18 of its bound."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    dev = _dev()
    pose = int(rotate) + 2 * int(translate)
    zd = inf - pose
    rs = np.random.RandomState(900 + 7 * inf + B + 2 * pose + mu_penalty)
    q_np = np.concatenate([rs.normal(size=(B, inf)), rs.uniform(-2, 1, size=(B, inf))], 1).astype(np.float32)
    r_np = rs.normal(size=(B, inf)).astype(np.float32)
    ups = dict(theta=rs.normal(size=B), dx=rs.normal(size=(B, 2)), zc=rs.normal(size=(B, zd)), kl=rs.normal(size=B))
    ups = {k: v.astype(np.float32) for k, v in ups.items()}
    present = [k for k in ("theta", "dx", "zc", "kl") if (k != "theta" or rotate) and (k != "dx" or translate) and (k != "zc" or zd)]
    worst = 0.0
    for z_scale, theta_prior in ((1.0, np.pi), (0.5, 0.5)):
        sc = [float(np.float32(v)) for v in (0.1, z_scale, theta_prior)]       # the scalars cross the ABI as floats

        def formulas(dtype, subset):
            q = torch.from_numpy(q_np).to(dtype).requires_grad_(True)
            outs = dict(zip(("theta", "dx", "zc", "kl"),
                            ref64.latent_formulas(q, torch.from_numpy(r_np).to(dtype), rotate, translate, mu_penalty, *sc)))
            loss = sum((outs[k] * torch.from_numpy(ups[k]).to(dtype)).sum() for k in subset if k in present)
            loss.backward()
            return {k: v.detach().numpy() for k, v in outs.items() if v is not None}, q.grad.numpy()

        def bound(f32, f64):
            return 16 * U + 4 * rel_err(f32, f64)

        q = torch.from_numpy(q_np).to(dev).requires_grad_(True)
        r_dev = torch.from_numpy(r_np).to(dev)
        got = dict(zip(("theta", "dx", "zc", "kl"), ops.latent_head(q, r_dev, rotate, translate, mu_penalty, 0.1, z_scale,
                                                                    theta_prior)))
        assert (got["theta"] is None) == (not rotate) and (got["dx"] is None) == (not translate)
        assert tuple(got["zc"].shape) == (B, zd)
        ref_out, ref_gq = formulas(torch.float64, present)
        f32_out, f32_gq = formulas(torch.float32, present)
        for k in present:
            e, b = rel_err(got[k].detach().cpu().numpy(), ref_out[k]), bound(f32_out[k], ref_out[k])
            worst = max(worst, e / b)
            assert e <= b, (k, e, b)
        sum((got[k] * torch.from_numpy(ups[k]).to(dev)).sum() for k in present).backward()
        e, b = rel_err(q.grad.cpu().numpy(), ref_gq), bound(f32_gq, ref_gq)
        worst = max(worst, e / b)
        assert e <= b, ("g_q_out", e, b)
        desc = _lib.LatentDesc(B, inf, int(rotate), int(translate), int(mu_penalty), 0.1, z_scale, theta_prior)
        up_dev = {k: torch.from_numpy(ups[k]).to(dev) for k in present}
        for subset in SUBSETS:
            if not any(k in present for k in subset):
                continue
            _, ref_gq = formulas(torch.float64, subset)
            _, f32_gq = formulas(torch.float32, subset)
            gq = torch.full((B * 2 * inf + 64,), SENTINEL, device=dev)
            ptr = {k: (up_dev[k].data_ptr() if (k in subset and k in present) else None) for k in ("theta", "dx", "zc", "kl")}
            with torch.cuda.device(dev):
                _lib.check(L.svae_latent_backward(ctypes.byref(desc), q.data_ptr(), r_dev.data_ptr(), ptr["theta"], ptr["dx"],
                                                  ptr["zc"], ptr["kl"], gq.data_ptr(), _stream()))
            torch.cuda.synchronize()
            gq = gq.cpu().numpy()
            assert (gq[B * 2 * inf:] == SENTINEL).all()
            e, b = rel_err(gq[:B * 2 * inf].reshape(B, 2 * inf), ref_gq), bound(f32_gq, ref_gq)
            worst = max(worst, e / b)
            assert e <= b, (subset, e, b)
    print("latent r%d t%d mp%d inf%d B%d worst error/bound %.3f" % (rotate, translate, mu_penalty, inf, B, worst))


@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1000])
def test_elbo_head_against_float64(B):
    """ops.elbo_head: {mean(loglik) - mean(kl), mean(loglik), mean(kl)} against float64, and its backward for every
    non-empty subset of the three upstream gradients against (g_elbo + g_logp) / B and (g_kl - g_elbo) / B.
    Forward bound: 4x the error of torch float32 means on the CPU, floor 16 * 2^-24 -- the worst case of the kernel's <= 15
    roundings (<= 4 additions per thread, 6 + 3 to combine lanes and waves, the division, the difference), each at most
    2^-24 of a partial sum of same-sign terms.  Backward: one addition and one division per entry, 8 * 2^-24 of the entry.
    MI355X maxima: forward 7.0e-8 (bound 9.5e-7), backward 6.0e-8 (bound 4.8e-7)."""
    from spatial_vae_amd import ops
    dev = _dev()
    rs = np.random.RandomState(60 + B)
    ll_np = (-50.0 - 100.0 * np.abs(rs.normal(size=B))).astype(np.float32)
    kl_np = (5.0 + 3.0 * np.abs(rs.normal(size=B))).astype(np.float32)
    lp, kk = ll_np.astype(np.float64).mean(), kl_np.astype(np.float64).mean()
    ref = np.array([lp - kk, lp, kk])
    lp32, kk32 = torch.from_numpy(ll_np).mean(), torch.from_numpy(kl_np).mean()
    f32 = np.array([float(lp32 - kk32), float(lp32), float(kk32)])
    ups = rs.normal(size=3).astype(np.float32)
    worst_b = 0.0
    for subset in [s for r in (1, 2, 3) for s in itertools.combinations(range(3), r)]:
        ll = torch.from_numpy(ll_np).to(dev).requires_grad_(True)
        kl = torch.from_numpy(kl_np).to(dev).requires_grad_(True)
        out = ops.elbo_head(ll, kl)
        got = np.array([float(o.detach()) for o in out])
        err, bound = rel_err(got, ref), _bound(rel_err(f32, ref), 16)
        assert err <= bound, (err, bound)
        sum(out[i] * float(ups[i]) for i in subset).backward()
        g = [float(ups[i]) if i in subset else 0.0 for i in range(3)]
        want_l, want_k = (g[0] + g[1]) / B, (g[2] - g[0]) / B
        for grad, want in ((ll.grad, want_l), (kl.grad, want_k)):
            gn = grad.cpu().numpy().astype(np.float64)
            assert gn.shape == (B,) and (gn == gn[0]).all()
            e = abs(gn[0] - want) / abs(want) if want != 0.0 else abs(gn[0])
            worst_b = max(worst_b, e)
            assert e <= 8 * U, (subset, e)
    print("elbo_head B=%d forward %.3e bound %.3e backward %.3e" % (B, err, bound, worst_b))


# ---------------------------------------------------------------------------------------------------------------------
# 5. Column sums
# ---------------------------------------------------------------------------------------------------------------------
COLSUM = [(r, c) for r in (1, 7, 8, 9, 24, 25, 32, 33, 57, 256, 257) for c in (1, 31, 32, 33, 46, 500)] + [(256, 5000)]


@pytest.mark.parametrize("rows,cols", COLSUM, ids=["%dx%d" % rc for rc in COLSUM])
def test_colsum_against_float64(rows, cols):
    """svae_colsum (colsum_reduce_kernel: 8 row lanes per column, four chains of the main loop while i + 24 < rows, then the
    remainder loop) against float64 column sums.  Bound: 4x the error of x.sum(0) in torch float32 on the CPU, floor
    4 * 2^-24.  Two calls are bit-equal and the 64 elements behind out[cols] stay untouched.  MI355X: the worst error over
    the 67 shapes is 0.47 of its bound (largest: 1.5e-6 of 5.9e-6, where the largest column sum is itself small)."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * rows + cols)
    x = torch.randn(rows, cols, generator=g)
    ref = x.double().sum(0).numpy()
    bound = _bound(rel_err(x.sum(0).numpy(), ref), 4)
    xd = x.to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((cols + 64,), SENTINEL, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.svae_colsum(xd.data_ptr(), rows, cols, out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert (outs[0][cols:] == SENTINEL).all()
    assert np.array_equal(outs[0], outs[1])
    err = rel_err(outs[0][:cols], ref)
    print("colsum %dx%d %.3e bound %.3e" % (rows, cols, err, bound))
    assert err <= bound, (err, bound)
