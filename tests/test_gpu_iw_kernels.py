"""The four entries behind the K-sample importance-weighted bound, each called on its own and compared with torch float64
autograd on the CPU: svae_latent_iw_forward / _backward (ops.latent_head_iw) and svae_iw_head_forward / _backward
(ops.iw_head).  Row b*K + k is sample k of image b.

Bounds as in tests/test_gpu_loss_head.py, formed from a reference's own fp32 error and never from the kernel's output: a kernel
may be 4x as far from float64 as the fp32 CPU evaluation of the same formula on the same inputs, floor 8 * 2^-24; errors are
helpers.rel_err.  Each test prints its figures before it asserts; what an MI355X gave is in each docstring."""
import ctypes
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import ref64
from helpers import rel_err
from iw_ref import iw_latent_formulas
from ref64 import U

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
BS, KS, INFS = (1, 3, 257), (1, 2, 5, 64, 65), (1, 3, 5, 12)
PRIORS = ((math.pi, 1.0), (0.3, 0.5))                  # (theta_prior, z_scale); dx_scale is 0.1 throughout
NAMES = ("theta", "dx", "zc", "log_ratio")
SUBSETS = [("log_ratio",), ("theta",), ("dx",), ("zc",), ("theta", "dx", "zc")]


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bound(oracle_err):
    return max(4.0 * oracle_err, 8 * U)


def _poses(inf):
    """Every (rotate, translate, mu_penalty) whose pose coordinates fit inf_dim; inf == pose is the zd = 0 case."""
    return [(r, t, mp) for r, t, mp in itertools.product((False, True), (False, True), (0, 1)) if int(r) + 2 * int(t) <= inf]


def _latent_inputs(B, K, inf, seed):
    rs = np.random.RandomState(seed)
    q = np.concatenate([rs.uniform(-2, 2, size=(B, inf)), rs.uniform(-3, 1, size=(B, inf))], 1).astype(np.float32)
    r = rs.normal(size=(B * K, inf)).astype(np.float32)
    ups = dict(theta=rs.normal(size=B * K), dx=rs.normal(size=(B * K, 2)), zc=rs.normal(size=(B * K, max(inf, 1))),
               log_ratio=rs.normal(size=B * K))
    return q, r, {k: v.astype(np.float32) for k, v in ups.items()}


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_latent_iw_against_float64(B, K):
    """ops.latent_head_iw forward and backward (all upstream gradients, through autograd) for inf_dim in {1, 3, 5, 12}, every
    pose / mu_penalty combination that fits (zd = 0 included) and (theta_prior, z_scale) in {(pi, 1), (0.3, 0.5)}; log-std
    in [-3, 1], mu in [-2, 2].  For K <= 5 also svae_latent_iw_backward with NULL for the absent gradients, g_q_out inside
    sentinels.  MI355X: the worst error is 0.089 to 0.123 of its bound over the fifteen (B, K) cases."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    dev = _dev()
    worst = 0.0
    for inf in INFS:
        q_np, r_np, ups = _latent_inputs(B, K, inf, 4000 + 100 * inf + 7 * B + K)
        q_dev, r_dev = torch.from_numpy(q_np).to(dev), torch.from_numpy(r_np).to(dev)
        for (rotate, translate, mu_penalty), (theta_prior, z_scale) in itertools.product(_poses(inf), PRIORS):
            zd = inf - int(rotate) - 2 * int(translate)
            sc = [float(np.float32(v)) for v in (0.1, z_scale, theta_prior)]    # the scalars cross the ABI as floats
            present = [k for k in NAMES if (k != "theta" or rotate) and (k != "dx" or translate) and (k != "zc" or zd)]
            up = {k: (ups[k][:, :zd] if k == "zc" else ups[k]) for k in present}

            def formulas(dtype, subset):
                q = torch.from_numpy(q_np).to(dtype).requires_grad_(True)
                outs = dict(zip(NAMES, iw_latent_formulas(q, torch.from_numpy(r_np).to(dtype), K, rotate, translate,
                                                          mu_penalty, *sc)))
                sum((outs[k] * torch.from_numpy(up[k]).to(dtype)).sum() for k in subset if k in present).backward()
                return {k: v.detach().numpy() for k, v in outs.items() if v is not None}, q.grad.numpy()

            q = q_dev.clone().requires_grad_(True)
            got = dict(zip(NAMES, ops.latent_head_iw(q, r_dev, K, rotate, translate, mu_penalty, 0.1, z_scale, theta_prior)))
            assert (got["theta"] is None) == (not rotate) and (got["dx"] is None) == (not translate)
            assert tuple(got["zc"].shape) == (B * K, zd) and tuple(got["log_ratio"].shape) == (B * K,)
            ref_out, ref_gq = formulas(torch.float64, present)
            f32_out, f32_gq = formulas(torch.float32, present)
            tag = (inf, rotate, translate, mu_penalty, theta_prior)
            for k in present:
                e, b = rel_err(got[k].detach().cpu().numpy(), ref_out[k]), _bound(rel_err(f32_out[k], ref_out[k]))
                worst = max(worst, e / b)
                assert e <= b, (tag, k, e, b)
            sum((got[k] * torch.from_numpy(up[k]).to(dev)).sum() for k in present).backward()
            e, b = rel_err(q.grad.cpu().numpy(), ref_gq), _bound(rel_err(f32_gq, ref_gq))
            worst = max(worst, e / b)
            assert e <= b, (tag, "g_q_out", e, b)
            if K > 5:
                continue
            desc = _lib.LatentDesc(B, inf, int(rotate), int(translate), int(mu_penalty), 0.1, z_scale, theta_prior)
            up_dev = {k: torch.from_numpy(np.ascontiguousarray(up[k])).to(dev) for k in present}
            for subset in SUBSETS:
                if not any(k in present for k in subset):
                    continue
                _, ref_gq = formulas(torch.float64, subset)
                _, f32_gq = formulas(torch.float32, subset)
                gq = torch.full((B * 2 * inf + 64,), SENTINEL, device=dev)
                ptr = {k: (up_dev[k].data_ptr() if (k in subset and k in present) else None) for k in NAMES}
                with torch.cuda.device(dev):
                    _lib.check(L.svae_latent_iw_backward(ctypes.byref(desc), K, q_dev.data_ptr(), r_dev.data_ptr(), ptr["theta"],
                                                         ptr["dx"], ptr["zc"], ptr["log_ratio"], gq.data_ptr(), _stream()))
                torch.cuda.synchronize()
                gq = gq.cpu().numpy()
                assert (gq[B * 2 * inf:] == SENTINEL).all()
                e, b = rel_err(gq[:B * 2 * inf].reshape(B, 2 * inf), ref_gq), _bound(rel_err(f32_gq, ref_gq))
                worst = max(worst, e / b)
                assert e <= b, (tag, subset, e, b)
    print("latent_iw B%d K%d worst error/bound %.3f" % (B, K, worst))


@pytest.mark.parametrize("rotate,translate,mu_penalty", _poses(5), ids=lambda v: str(int(v)))
def test_minus_log_ratio_averages_to_the_analytic_kl(rotate, translate, mu_penalty):
    """Over 4096 fixed draws per image (four calls at K = 1024, the largest K the interface takes) the float64 mean of
    -log_ratio is svae_latent_forward's kl of the same descriptor, for both priors.  Tolerance: five standard errors of the
    float64 reference's own -log_ratio over those draws (its standard deviation / sqrt(4096)) -- the draws are fixed, so this
    is a property of the formulas, not a chance -- plus 8 * 2^-24 of the kl.  A prior with the wrong centre or width, a
    dropped log(theta_prior) or a sample read from another image's row moves the mean by many standard errors.
    MI355X: |mean - kl| is at most 0.50 of its tolerance (0.080 of 0.163)."""
    from spatial_vae_amd import ops
    dev = _dev()
    B, K, inf, calls = 3, 1024, 5, 4
    q_np, _, _ = _latent_inputs(B, 1, inf, 77)
    q_dev = torch.from_numpy(q_np).to(dev)
    rs = np.random.RandomState(78)
    for theta_prior, z_scale in PRIORS:
        tp = float(np.float32(theta_prior))
        kl = ops.latent_head(q_dev, torch.zeros(B, inf, device=dev), rotate, translate, mu_penalty, 0.1, z_scale, theta_prior)[3]
        kl = kl.cpu().numpy().astype(np.float64)
        kl64 = ref64.latent_formulas(torch.from_numpy(q_np).double(), torch.zeros(B, inf, dtype=torch.float64), rotate, translate,
                                     mu_penalty, 0.1, z_scale, tp)[3].numpy()
        kl32 = ref64.latent_formulas(torch.from_numpy(q_np), torch.zeros(B, inf), rotate, translate, mu_penalty, 0.1, z_scale,
                                     tp)[3].numpy()
        assert rel_err(kl, kl64) <= 16 * U + 4 * rel_err(kl32, kl64)                # the bound tests/test_gpu_loss_head.py holds it to
        got, ref = [], []
        for _ in range(calls):
            r_np = rs.normal(size=(B * K, inf)).astype(np.float32)
            lr = ops.latent_head_iw(q_dev, torch.from_numpy(r_np).to(dev), K, rotate, translate, mu_penalty, 0.1, z_scale,
                                    theta_prior)[3]
            got.append(lr.cpu().numpy().astype(np.float64).reshape(B, K))
            ref.append(iw_latent_formulas(torch.from_numpy(q_np).double(), torch.from_numpy(r_np).double(), K, rotate, translate,
                                          mu_penalty, 0.1, z_scale, tp)[3].numpy().reshape(B, K))
        got, ref = -np.concatenate(got, 1), -np.concatenate(ref, 1)
        tol = 5.0 * ref.std(1) / math.sqrt(calls * K) + 8 * U * np.abs(kl)
        print("kl r%d t%d mp%d prior %.2f: mean %s kl %s tol %s" % (rotate, translate, mu_penalty, theta_prior,
                                                                    got.mean(1).tolist(), kl.tolist(), tol.tolist()))
        assert (np.abs(got.mean(1) - kl) <= tol).all(), (got.mean(1), kl, tol)


@functools.lru_cache(maxsize=None)
def _head_case(B, K):
    """loglik around -300 (the image's own level, then sigma = 1.5 between its samples), log_ratio around -4.  For K >= 2 the
    float64 reference must give every image two weights above 1e-3 before anything runs on the GPU."""
    rs = np.random.RandomState(500 + 11 * B + K)
    ll = (-300.0 + 5.0 * rs.normal(size=(B, 1)) + 1.5 * rs.normal(size=(B, K))).astype(np.float32)
    lr = (-4.0 + 0.3 * rs.normal(size=(B, K))).astype(np.float32)
    ups = rs.normal(size=3).astype(np.float32)

    def formulas(dtype, subset):
        l, r = torch.from_numpy(ll).to(dtype).requires_grad_(True), torch.from_numpy(lr).to(dtype).requires_grad_(True)
        a = l + r
        bound = (torch.logsumexp(a, 1) - math.log(K)).mean()
        out = torch.stack([bound, l.mean(), -r.mean()])
        sum(out[i] * float(ups[i]) for i in subset).backward()
        return out.detach().numpy(), torch.softmax(a, 1).detach().numpy(), l.grad.numpy(), r.grad.numpy()

    w64 = formulas(torch.float64, (0,))[1]
    if K >= 2:
        assert ((w64 > 1e-3).sum(1) >= 2).all(), "a degenerate row would hide a softmax error"
    return ll, lr, ups, formulas


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", BS)
def test_iw_head_against_float64(B, K):
    """ops.iw_head: {mean_b log mean_k exp(loglik + log_ratio), mean loglik, mean -log_ratio} and the softmax weights against
    float64, and the backward for every non-empty subset of the three upstream gradients.  With K = 1 the bound is
    mean(loglik + log_ratio) and every weight is exactly 1.
    MI355X: scalars at most 4.9e-8, weights 3.8e-8, gradients 5.6e-8 (bounds 4.8e-7 and up)."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    ll_np, lr_np, ups, formulas = _head_case(B, K)
    dev = _dev()
    ll_dev, lr_dev = torch.from_numpy(ll_np).to(dev).reshape(-1), torch.from_numpy(lr_np).to(dev).reshape(-1)
    out = torch.full((3 + 64,), SENTINEL, device=dev)
    w = torch.full((B * K + 64,), SENTINEL, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.svae_iw_head_forward(ll_dev.data_ptr(), lr_dev.data_ptr(), B, K, out.data_ptr(), w.data_ptr(), _stream()))
    torch.cuda.synchronize()
    out, w = out.cpu().numpy(), w.cpu().numpy()
    assert (out[3:] == SENTINEL).all() and (w[B * K:] == SENTINEL).all()
    ref = formulas(torch.float64, (0, 1, 2))
    f32 = formulas(torch.float32, (0, 1, 2))
    errs = {}
    for i, name in enumerate(("bound", "log_p", "kl")):
        errs[name] = (rel_err(out[i:i + 1], ref[0][i:i + 1]), _bound(rel_err(f32[0][i:i + 1], ref[0][i:i + 1])))
    errs["weights"] = (rel_err(w[:B * K].reshape(B, K), ref[1]), _bound(rel_err(f32[1], ref[1])))
    if K == 1:
        assert (w[:B] == 1.0).all()
        mean = (ll_np.astype(np.float64) + lr_np.astype(np.float64)).mean()
        assert abs(out[0] - mean) <= 8 * U * abs(mean)
    for subset in [s for n in (1, 2, 3) for s in itertools.combinations(range(3), n)]:
        l, r = ll_dev.clone().requires_grad_(True), lr_dev.clone().requires_grad_(True)
        got = ops.iw_head(l, r, K)
        assert got[0]._base is not None and got[0]._base.numel() == 3 and got[2]._base is got[0]._base
        assert np.array_equal(np.array([float(g.detach()) for g in got], np.float32), out[:3])
        sum(got[i] * float(ups[i]) for i in subset).backward()
        ref = formulas(torch.float64, subset)
        f32 = formulas(torch.float32, subset)
        for name, g, j in (("dloglik", l.grad, 2), ("dlog_ratio", r.grad, 3)):
            e, b = rel_err(g.cpu().numpy().reshape(B, K), ref[j]), _bound(rel_err(f32[j], ref[j]))
            prev = errs.get(name, (0.0, b))
            errs[name] = max(prev, (e, b), key=lambda t: t[0] / t[1])
            assert e <= b, (name, subset, e, b)
    print("iw_head B%d K%d %s" % (B, K, {k: "%.2e of %.2e" % v for k, v in errs.items()}))
    for name, (e, b) in errs.items():
        assert e <= b, (name, e, b)


def _edge_rows(K):
    equal = np.full(K, -300.0, np.float32)
    spike = np.full(K, -300.0, np.float32) - np.arange(K, dtype=np.float32) / K
    spike[K // 2] = -100.0                                        # 200 above the rest
    holes = -300.0 + np.arange(K, dtype=np.float32)
    holes[::2] = -np.inf                                          # some but not all
    return {"equal": equal, "spike": spike, "holes": holes}


@pytest.mark.parametrize("K", [2, 5, 65])
@pytest.mark.parametrize("row", ["equal", "spike", "holes"])
def test_iw_head_edge_rows(row, K):
    """One image each: all a equal (weights 1/K, bound = a); one a 200 above the rest (its weight exactly 1, the others
    exactly 0, bound = a_max - log K); a = -inf for every other sample (those weights exactly 0, the rest the softmax of the
    finite ones).  The bound, every weight and every gradient are finite; the -inf enters through log_ratio, so only the
    Monte-Carlo KL column is infinite there.
    MI355X: every case holds; each bound is its float64 value rounded to fp32."""
    from spatial_vae_amd import ops
    dev = _dev()
    a = _edge_rows(K)[row]
    ll_np = np.full(K, -290.0, np.float32)
    lr_np = (a - ll_np).astype(np.float32)                        # exact: small integers and multiples of 1/K ... or -inf
    l = torch.from_numpy(ll_np).to(dev).requires_grad_(True)
    r = torch.from_numpy(lr_np).to(dev).requires_grad_(True)
    bound, log_p, kl = ops.iw_head(l, r, K)
    (bound + 0.5 * log_p).backward()
    a64 = ll_np.astype(np.float64) + lr_np.astype(np.float64)
    w64 = np.exp(a64 - a64.max())
    w64 /= w64.sum()
    want = a64.max() + math.log(np.exp(a64 - a64.max()).sum()) - math.log(K)
    got, gl, gr = float(bound), l.grad.cpu().numpy(), r.grad.cpu().numpy()
    print("edge %s K%d bound %r want %r" % (row, K, got, want))
    assert math.isfinite(got) and abs(got - want) <= 8 * U * abs(want)
    assert float(log_p) == -290.0 and not math.isnan(float(kl))
    assert np.isfinite(gl).all() and np.isfinite(gr).all()
    w = gr.astype(np.float64)                                     # d bound / d log_ratio = w / B with B = 1
    assert rel_err(w, w64) <= 8 * U and rel_err(gl - 0.5 / K, w64) <= 16 * U
    if row == "equal":
        assert (gr == np.float32(1.0 / K)).all()
    if row == "spike":
        assert gr[K // 2] == 1.0 and (np.delete(gr, K // 2) == 0.0).all()
    if row == "holes":
        assert (gr[::2] == 0.0).all() and (gr[1::2] > 0.0).all() and math.isinf(float(kl))


@pytest.mark.parametrize("B,K", [(3, 5), (257, 65)])
def test_two_runs_are_bit_identical(B, K):
    """All four entries twice on the same inputs, fresh output buffers: equal bit for bit (fixed summation order over K and
    B, no atomics).  MI355X: equal."""
    from spatial_vae_amd import ops
    dev = _dev()
    inf = 12
    q_np, r_np, ups = _latent_inputs(B, K, inf, 31)
    ll_np, lr_np, _, _ = _head_case(B, K)
    runs = []
    for _ in range(2):
        q = torch.from_numpy(q_np).to(dev).requires_grad_(True)
        theta, dx, zc, lr = ops.latent_head_iw(q, torch.from_numpy(r_np).to(dev), K, True, True, False, 0.1, 0.5, 0.3)
        ll = torch.from_numpy(ll_np).to(dev).reshape(-1).requires_grad_(True)
        lr_in = torch.from_numpy(lr_np).to(dev).reshape(-1).requires_grad_(True)
        out = ops.iw_head(ll, lr_in, K)
        (out[0] - 0.25 * out[2]).backward()
        (theta * torch.from_numpy(ups["theta"]).to(dev)).sum().backward(retain_graph=True)
        ((lr * lr_in.grad).sum() + (zc * torch.from_numpy(ups["zc"][:, :inf - 3]).to(dev)).sum() + dx.sum()).backward()
        runs.append([t.detach().cpu().numpy() for t in (theta, dx, zc, lr, out[0]._base, ll.grad, lr_in.grad, q.grad)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_out_of_range_K_is_refused():
    """K = 0, -1 and 1025 return SVAE_E_INVALID from each of the four entries and write nothing; 1024 is taken; ops raises."""
    from spatial_vae_amd import _lib, ops
    L = _lib.lib()
    dev = _dev()
    B, inf = 2, 3
    desc = _lib.LatentDesc(B, inf, 1, 1, 1, 0.1, 1.0, math.pi)
    q = torch.zeros(B, 2 * inf, device=dev)
    big = torch.full((B * 1025 * inf,), SENTINEL, device=dev)
    outs = [torch.full((B * 1025 * 2,), SENTINEL, device=dev) for _ in range(4)]
    ptrs = [o.data_ptr() for o in outs]
    with torch.cuda.device(dev):
        for K in (0, -1, 1025):
            calls = (L.svae_latent_iw_forward(ctypes.byref(desc), K, q.data_ptr(), big.data_ptr(), ptrs[0], ptrs[1], None, ptrs[2],
                                              _stream()),
                     L.svae_latent_iw_backward(ctypes.byref(desc), K, q.data_ptr(), big.data_ptr(), None, None, None, ptrs[0],
                                               ptrs[1], _stream()),
                     L.svae_iw_head_forward(big.data_ptr(), big.data_ptr(), B, K, ptrs[2], ptrs[3], _stream()),
                     L.svae_iw_head_backward(None, None, None, big.data_ptr(), B, K, ptrs[0], ptrs[1], _stream()))
            assert calls == (-1, -1, -1, -1), (K, calls)
            assert b"K" in L.svae_last_error()
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in outs)
        big.zero_()
        assert L.svae_iw_head_forward(big.data_ptr(), big.data_ptr(), B, 1024, ptrs[2], ptrs[3], _stream()) == 0
        torch.cuda.synchronize()
    assert bool((outs[3][:B * 1024] == np.float32(1.0 / 1024)).all()) and bool((outs[3][B * 1024:] == SENTINEL).all())
    for K in (0, 1025):
        with pytest.raises(RuntimeError, match="num_samples"):
            ops.iw_head(torch.zeros(4, device=dev), torch.zeros(4, device=dev), K)
        with pytest.raises(RuntimeError, match="num_samples"):
            ops.latent_head_iw(q, torch.zeros(4, inf, device=dev), K, True, True, True, 0.1, 1.0, math.pi)
