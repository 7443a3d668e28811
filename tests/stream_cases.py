"""Helper of tests/test_gpu_streams.py, tests/test_gpu_graph.py and tests/test_stream_cases_cpu.py (not collected): one table
of enqueue-only callers, at least one per entry point of include/*.h that takes a stream.  A new header needs a row here (or in
tests/stream_cases_analysis.py, which holds the rows of the analysis headers), not a test file of its own.

A case knows three things.  inputs(seed): its input set as numpy arrays by name -- seed 0 (set A) and 1 (set B) have equal
shapes and dtypes and different values, but for the inputs the case names in same_in_both_sets; integer inputs (labels,
quarter-turn codes, masks, reference and class indices) are valid in both.  alloc(dev):
every device buffer its calls read or write -- the real inputs (case.real), a staging copy of each (case.stage), the outputs
(case.outs, each inside guard bytes, the in-place ones listed in case.state too) and the scratch areas (case.scratch:
workspaces, `saved`, records the calls initialise themselves).  steps(): the C-ABI calls in order, each a callable of the
stream handle that returns the call's status and does nothing else: no allocation, no synchronisation, no readback, no copy.
enqueue(stream) issues all of them.  Entry points that only make sense together are one case with several steps.

Everything else here (load, poison, stage_to_real, collect) is what a test does AROUND the calls; none of it is called by
enqueue.  check(out, seed) holds a default-stream result to the case's reference; must_differ names the outputs that set B has
to change.  The table is checked against _lib.ALL_SIGNATURES, the signature tables of every header, by
tests/test_stream_cases_cpu.py."""
import ctypes
import math

import numpy as np
import torch

import decoder_abi as A
import ref64
from ctfcorr_ref import random_table
from decoder_abi import GUARD_BYTE, SENTINEL, Guarded
from spatial_vae_amd import _lib, ops

# Entry points a HIP graph cannot hold for a reason that lies in the runtime and not in this project: {name: reason}.  At most
# three, none of those dp.TrainStep needs.  Empty: every entry point is captured and replayed by tests/test_gpu_graph.py.
NOT_CAPTURABLE = {}


def stream_entry_points():
    """Every function of _lib.ALL_SIGNATURES (one table per header of _lib.HEADERS) whose last argument is the stream: it
    returns a status and its last argument is a bare address (size queries return size_t; svae_profile_read ends in a typed
    pointer)."""
    return sorted(name for name, (res, args) in _lib.ALL_SIGNATURES.items() if res is _lib.cint and args and args[-1] is _lib.vp)


_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
          np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8}


def _view(g, shape, dtype):
    """The payload of a Guarded allocation as a typed torch tensor."""
    return g.buf[g.off:g.off + g.nbytes].view(_TORCH[np.dtype(dtype)]).view(*shape)


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return Guarded(max(n, 1), dev), tuple(shape), np.dtype(dtype)


def _fill_poison(t):
    """Finite poison for float data; integer data is left as it is (valid)."""
    if t.dtype in (torch.float32, torch.float64):
        t.fill_(SENTINEL)


def _fill_sentinel(t):
    t.fill_(SENTINEL if t.dtype in (torch.float32, torch.float64) else GUARD_BYTE)


class Case(object):
    """Base of the table's rows; a subclass states name, entry_points, inputs(), _outputs(), _scratch_bytes() and steps()."""
    name = None
    entry_points = ()
    state = ()                      # inputs the calls update in place: collected like outputs
    has_reference = False           # check(out) compares with float64 (else: finite, no sentinel, not constant)
    same_in_both_sets = ()          # inputs that are deliberately equal in set A and set B (every other input differs)
    must_differ = ()                # outputs that have to differ between the baselines of set A and set B
    non_finite_inputs = ()          # float inputs that hold an inf or a NaN on purpose (every other one is finite in both sets)

    def inputs(self, seed):
        raise NotImplementedError

    def _outputs(self):
        return {}

    def _scratch_bytes(self):
        return {}

    def steps(self):
        raise NotImplementedError

    # ---- allocation ---------------------------------------------------------------------------------
    def alloc(self, dev):
        self.dev = dev
        self.L = _lib.lib()
        self.real, self.stage, self.outs, self.scratch = {}, {}, {}, {}
        for k, a in self.inputs(0).items():
            g, shape, dt = _guarded(a.shape, a.dtype, dev)
            self.real[k] = _view(g, shape, dt)
            self.real[k].copy_(torch.from_numpy(np.ascontiguousarray(a)))
            self.stage[k] = torch.empty_like(self.real[k])
            if k in self.state:
                self.outs[k] = (g, shape, dt)
            else:
                self.scratch["input:" + k] = g          # read-only: only its guards are looked at
        for k, (shape, dt) in self._outputs().items():
            self.outs[k] = _guarded(shape, dt, dev)
        for k, n in self._scratch_bytes().items():
            if n:
                self.scratch[k] = Guarded(n, dev)
        self.fill_outputs()
        return self

    def ptr(self, k):
        if k in self.real:
            return self.real[k].data_ptr()
        return self.outs[k][0].ptr if k in self.outs else (self.scratch[k].ptr if k in self.scratch else None)

    # ---- what a test does around the calls ----------------------------------------------------------------
    def load(self, seed):
        """Host to device: input set `seed` into the staging copies."""
        for k, a in self.inputs(seed).items():
            self.stage[k].copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def stage_to_real(self):
        """Device-to-device copies, on the current stream, from staging to the real inputs."""
        for k, t in self.stage.items():
            self.real[k].copy_(t, non_blocking=True)

    def poison(self):
        """Real float inputs to -12345.5, scratch to 0xA5 bytes, outputs to the sentinel."""
        for t in self.real.values():
            _fill_poison(t)
        for k, g in self.scratch.items():
            if not k.startswith("input:"):
                g.fill_byte(GUARD_BYTE)
        self.fill_outputs()

    def zero_scratch(self):
        for k, g in self.scratch.items():
            if not k.startswith("input:"):
                g.buf[g.off:g.off + g.nbytes].zero_()

    def fill_outputs(self):
        for k, (g, shape, dt) in self.outs.items():
            if k not in self.state:
                _fill_sentinel(_view(g, shape, dt))

    def enqueue(self, stream):
        """Every call of the case on `stream`; the list of their statuses."""
        return [step(stream) for step in self.steps()]

    def collect(self):
        """({output name: numpy array}, names of buffers whose guard bytes changed) -- after a synchronisation."""
        out, bad = {}, []
        for k, (g, shape, dt) in self.outs.items():
            a = g.buf.cpu().numpy()
            if not ((a[:g.off] == GUARD_BYTE).all() and (a[g.off + g.nbytes:] == GUARD_BYTE).all()):
                bad.append(k)
            out[k] = a[g.off:g.off + int(np.prod(shape)) * dt.itemsize].copy().view(dt).reshape(shape)
        bad += [k for k, g in self.scratch.items() if not g.read()[1]]
        return out, bad

    def check(self, out, seed=0):
        """The baseline of input set `seed` is live: by default every output is finite, free of the sentinel and not constant.
        A row whose check takes the seed is held to its reference on both sets; one that takes `out` alone, on set A."""
        for k, a in out.items():
            if a.dtype.kind == "f":
                assert np.isfinite(a).all(), (self.name, k)
                assert not (a == SENTINEL).any(), (self.name, k)
            if a.size > 1 and k not in getattr(self, "may_be_constant", ()):
                assert (a != a.flat[0]).any(), (self.name, k, "constant")


def statuses_ok(rcs):
    for rc in rcs:
        _lib.check(rc)


# ---------------------------------------------------------------------------------------------------------------------
# the decoder: forward [+ BCE] -> backward, on tests/decoder_abi.py's buffers
# ---------------------------------------------------------------------------------------------------------------------
class Decoder(Case):
    has_reference = True

    def __init__(self, case, bce=None):
        self.case, self.bce = case, bce
        self.name = "decoder_" + case + ("_bce" if bce else "")
        self.entry_points = ("svae_decoder_forward_bce" if bce else "svae_decoder_forward", "svae_decoder_backward")

    def inputs(self, seed):
        p, d = A.inputs(self.case, seed)
        out = dict(p)
        out.update(d)
        c = A.case(self.case)
        if c["Zd"] == 0:
            out.pop("z")                # (B, 0): nothing to differ in
        if self.bce:
            out.pop("dy")               # the backward call reads the forward's dll_dy in its place
            out["dy_scale"] = np.random.RandomState(50 + seed).normal(size=c["B"]).astype(np.float32)
        else:
            out.pop("target")
        return out

    def alloc(self, dev):
        self.dev = dev
        self.L = _lib.lib()
        self.f = f = A.Forward(self.case, bce="dll" if self.bce else None, run=False)
        f.alloc_backward(dy_scale=self.inputs(0)["dy_scale"] if self.bce else None)
        if self.bce:
            f.tens["dy_scale"] = f.bwd["scale"]
        self.real = {k: f.tens[k] for k in self.inputs(0)}
        self.stage = {k: torch.empty_like(t) for k, t in self.real.items()}
        c = f.c
        self.outs = {k: (g, A._shape(c, k), np.dtype(np.float32)) for k, g in list(f.bufs.items()) + list(f.bwd["bufs"].items())}
        self.scratch = {"ws": f.ws, "saved": f.saved}
        return self

    def steps(self):
        f = self.f
        if not self.bce:
            return [f.enqueue, f.enqueue_backward]

        def backward(stream):           # dy = the forward's dll_dy, dy_scale = the upstream gradient of loglik
            w = f.bwd
            bufs = w["bufs"]
            return f.L.svae_decoder_backward(ctypes.byref(f.desc), ctypes.byref(f.params), ctypes.byref(f.pose), f.z,
                                             f.bufs["logits"].ptr, f.bufs["dll_dy"].ptr, w["scale"].data_ptr(), f.saved.ptr,
                                             ctypes.byref(w["grads"]), bufs["dz"].ptr if "dz" in bufs else None,
                                             ctypes.byref(w["pg"]), w["ws"].ptr, f.ws_bytes, stream)
        return [f.enqueue, backward]

    def check(self, out):
        """Against decoder_abi.reference in float64 under tests/test_gpu_decoder_abi.py's own bounds (input set A is the set
        those references are computed on); the fused likelihood against decoder_abi.bce64 of the returned y."""
        Case.check(self, out)
        import test_gpu_decoder_abi as T
        if not self.bce:
            T._assert_values(self.case, out, tag=" [stream case]")
            return
        T._assert_values(self.case, {k: out[k] for k in ("y", "logits")}, tag=" [stream case, bce]")
        from helpers import rel_err
        from oracle import elbo_oracle as O
        target = A.inputs(self.case)[1]["target"]
        want = A.bce64(out["y"], target)        # tests/test_gpu_loss_head.py's bound for the fused likelihood
        assert rel_err(out["loglik"], want) <= max(4.0 * rel_err(O.bce_loglik(out["y"], target)[0], want), 8 * ref64.U)


DECODER_CASES = ["rank1_tanh", "stream_c2_L3", "leaky_resid_L4", "expand_bilinear", "z0_sigmoid_w128", "many_images",
                 "rank1_tanh_b20"]


# ---------------------------------------------------------------------------------------------------------------------
# likelihoods
# ---------------------------------------------------------------------------------------------------------------------
class Bce(Case):
    name, entry_points, has_reference = "bce_B3_n257", ("svae_bce_loglik",), True
    B, n = 3, 257

    def inputs(self, seed):
        rs = np.random.RandomState(310 + seed)
        s = np.clip(rs.uniform(size=(self.B, self.n)), 1e-6, 1 - 1e-6).astype(np.float32)
        t = (np.floor(rs.uniform(size=(self.B, self.n)) * 255) / 255).astype(np.float32)
        return {"y_hat": s, "target": t}

    def _outputs(self):
        return {"loglik": ((self.B,), np.float32), "dll_dy": ((self.B, self.n), np.float32)}

    def steps(self):
        return [lambda st: self.L.svae_bce_loglik(self.B, self.n, self.ptr("y_hat"), self.ptr("target"), self.ptr("loglik"),
                                                  self.ptr("dll_dy"), st)]

    def check(self, out):
        from helpers import rel_err
        Case.check(self, out)
        i = self.inputs(0)
        # tests/test_gpu_loss_head.py: 4x the fp32 oracle's error, floor 8 * 2^-24; the entries of dll to 8 * 2^-24 each
        from oracle import elbo_oracle as O
        ref = ref64.bce64(i["y_hat"], i["target"])
        assert rel_err(out["loglik"], ref) <= max(4 * rel_err(O.bce_loglik(i["y_hat"], i["target"])[0], ref), 8 * ref64.U)
        want = ref64.bce_dll64(i["y_hat"], i["target"])
        assert (np.abs(out["dll_dy"] - want) <= 8 * ref64.U * np.abs(want)).all()


class Gaussian(Case):
    """svae_gaussian_loglik: plain (C = 1 or 2, with or without the pixel mask) or with a CTF pair (n, k) of tests/ref64.py."""
    entry_points, has_reference = ("svae_gaussian_loglik",), True

    def __init__(self, C=1, N=None, masked=False, ctf=None):
        self.C, self.masked, self.ctf = C, masked, ctf
        self.B = ref64.CTF_B if ctf else 3
        self.N = ctf[0] * ctf[0] if ctf else N
        self.k = ctf[1] if ctf else 0
        self.name = "gaussian_" + ("ctf_n%d_k%d_%s" % (ctf + (ref64.ctf_form(*ctf),)) if ctf else "C%d_N%d" % (C, N)) + \
                    ("_mask" if masked else "")

    def inputs(self, seed):
        B, N, C = self.B, self.N, self.C
        rs = np.random.RandomState(1000 * N + 10 * C + self.masked + 77 * seed)
        y = rs.normal(size=(B, N * C)).astype(np.float32)
        if C == 2:
            y[:, N:] = rs.uniform(-8, 8, size=(B, N)).astype(np.float32)
        out = {"y_params": y, "target": rs.normal(size=(B, N)).astype(np.float32)}
        if self.ctf:
            f = rs.normal(size=(B, self.k, self.k)) / self.k
            f[:, self.k // 2, self.k // 2] += 1.0
            out["ctf"] = f.astype(np.float32)
        if self.masked:
            if self.ctf:
                m = np.asarray(ref64.ctf_mask(self.ctf[0], True), bool).reshape(-1).copy()
            else:
                m = rs.uniform(size=N) < 0.7
            m[0] = True
            m[1 + seed] = not m[1 + seed]           # the two sets' masks differ, both valid
            out["mask"] = m.astype(np.uint8)
        return out

    def _outputs(self):
        return {"loglik": ((self.B,), np.float32), "dll_dy": ((self.B, self.N * self.C), np.float32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_gaussian_workspace_bytes(self.B, self.N) if self.ctf else 0}

    def steps(self):
        ws = self.scratch.get("ws")
        return [lambda st: self.L.svae_gaussian_loglik(self.B, self.N, self.C, self.ptr("y_params"), self.ptr("target"),
                                                       self.ptr("mask"), self.ptr("ctf"), self.k, self.ptr("loglik"),
                                                       self.ptr("dll_dy"), ws.ptr if ws else None, ws.nbytes if ws else 0, st)]

    def check(self, out):
        """tests/test_gpu_loss_head.py's bound: 4x the error of oracle.elbo_oracle.gaussian_loglik, floor 8 * 2^-24."""
        from helpers import rel_err
        from oracle import elbo_oracle as O
        Case.check(self, out)
        i = self.inputs(0)
        mask = i["mask"].astype(bool) if self.masked else None
        ref = ref64.gaussian64(i["y_params"], i["target"], mask, i.get("ctf"))
        o_ll, o_dll = O.gaussian_loglik(i["y_params"], i["target"], mask=mask, ctf=i["ctf"][:, None] if self.ctf else None)
        for got, want, oracle in ((out["loglik"], ref["loglik"], o_ll), (out["dll_dy"], ref["dll"], o_dll)):
            assert rel_err(got, want) <= max(4.0 * rel_err(oracle, want), 8 * ref64.U), self.name


# ---------------------------------------------------------------------------------------------------------------------
# latent heads and minibatch scalars
# ---------------------------------------------------------------------------------------------------------------------
class Latent(Case):
    """svae_latent_forward -> _backward (K = None) or the K-sample pair: B = 257, inf_dim 5 with rotate + translate + z."""
    B, inf, has_reference = 257, 5, True

    def __init__(self, K=None):
        self.K = K
        self.rows = self.B * (K or 1)
        self.name = "latent_B257_inf5" + ("_K%d" % K if K else "")
        self.entry_points = ("svae_latent_iw_forward", "svae_latent_iw_backward") if K else \
            ("svae_latent_forward", "svae_latent_backward")
        self.last = "log_ratio" if K else "kl"
        self.last_rows = self.rows if K else self.B

    def inputs(self, seed):
        rs = np.random.RandomState(4000 + (self.K or 0) + 13 * seed)
        B, inf, R = self.B, self.inf, self.rows
        q = np.concatenate([rs.uniform(-2, 2, size=(B, inf)), rs.uniform(-3, 1, size=(B, inf))], 1).astype(np.float32)
        f = lambda *s: rs.normal(size=s).astype(np.float32)
        return {"q_out": q, "r": f(R, inf), "g_theta": f(R), "g_dx": f(R, 2), "g_zc": f(R, inf - 3),
                "g_" + self.last: f(self.last_rows)}

    def _outputs(self):
        R, f = self.rows, np.float32
        return {"theta": ((R,), f), "dx": ((R, 2), f), "zc": ((R, self.inf - 3), f), self.last: ((self.last_rows,), f),
                "g_q_out": ((self.B, 2 * self.inf), f)}

    def steps(self):
        d = self.desc = _lib.LatentDesc(self.B, self.inf, 1, 1, 0, 0.1, 0.5, 0.3)
        p = self.ptr
        if self.K:
            return [lambda st: self.L.svae_latent_iw_forward(ctypes.byref(d), self.K, p("q_out"), p("r"), p("theta"), p("dx"),
                                                             p("zc"), p("log_ratio"), st),
                    lambda st: self.L.svae_latent_iw_backward(ctypes.byref(d), self.K, p("q_out"), p("r"), p("g_theta"), p("g_dx"),
                                                              p("g_zc"), p("g_log_ratio"), p("g_q_out"), st)]
        return [lambda st: self.L.svae_latent_forward(ctypes.byref(d), p("q_out"), p("r"), p("theta"), p("dx"), p("zc"), p("kl"), st),
                lambda st: self.L.svae_latent_backward(ctypes.byref(d), p("q_out"), p("r"), p("g_theta"), p("g_dx"), p("g_zc"),
                                                       p("g_kl"), p("g_q_out"), st)]

    def check(self, out):
        """ref64.latent_formulas / iw_ref.iw_latent_formulas in torch float64 with autograd, under the bounds of
        tests/test_gpu_loss_head.py (16 * 2^-24 + 4x the fp32 error) and tests/test_gpu_iw_kernels.py (its _bound)."""
        from helpers import rel_err
        from iw_ref import iw_latent_formulas
        Case.check(self, out)
        i = self.inputs(0)
        sc = [float(np.float32(v)) for v in (0.1, 0.5, 0.3)]                   # dx_scale, z_scale, theta_prior of steps()
        names = ("theta", "dx", "zc", self.last)

        def formulas(dtype):
            q = torch.from_numpy(i["q_out"]).to(dtype).requires_grad_(True)
            r = torch.from_numpy(i["r"]).to(dtype)
            res = iw_latent_formulas(q, r, self.K, True, True, 0, *sc) if self.K else ref64.latent_formulas(q, r, True, True, 0, *sc)
            outs = dict(zip(names, res))
            sum((outs[k] * torch.from_numpy(i["g_" + k]).to(dtype)).sum() for k in names).backward()
            return dict({k: v.detach().numpy() for k, v in outs.items()}, g_q_out=q.grad.numpy())

        r64, r32 = formulas(torch.float64), formulas(torch.float32)
        if self.K:
            from test_gpu_iw_kernels import _bound
        else:
            _bound = lambda e: 16 * ref64.U + 4 * e
        for k, want in r64.items():
            assert rel_err(out[k], want) <= _bound(rel_err(r32[k], want)), (self.name, k)


class ElboHead(Case):
    name, entry_points, B, has_reference = "elbo_head_B257", ("svae_elbo_head_forward", "svae_elbo_head_backward"), 257, True
    may_be_constant = ("dloglik", "dkl")

    def inputs(self, seed):
        rs = np.random.RandomState(60 + seed)
        return {"loglik": (-50.0 - 100.0 * np.abs(rs.normal(size=self.B))).astype(np.float32),
                "kl": (5.0 + 3.0 * np.abs(rs.normal(size=self.B))).astype(np.float32), "g": rs.normal(size=3).astype(np.float32)}

    def _outputs(self):
        return {"out3": ((3,), np.float32), "dloglik": ((self.B,), np.float32), "dkl": ((self.B,), np.float32)}

    def steps(self):
        p, g = self.ptr, self.real["g"].data_ptr()
        return [lambda st: self.L.svae_elbo_head_forward(p("loglik"), p("kl"), self.B, p("out3"), st),
                lambda st: self.L.svae_elbo_head_backward(g, g + 4, g + 8, self.B, p("dloglik"), p("dkl"), st)]

    def check(self, out):
        """tests/test_gpu_loss_head.py: the means against float64 within its _bound (floor 16 * 2^-24), the gradients
        (g_elbo + g_logp) / B and (g_kl - g_elbo) / B to 8 * 2^-24 of the entry."""
        from helpers import rel_err
        from test_gpu_loss_head import _bound
        Case.check(self, out)
        i = self.inputs(0)
        lp, kk = i["loglik"].astype(np.float64).mean(), i["kl"].astype(np.float64).mean()
        lp32, kk32 = torch.from_numpy(i["loglik"]).mean(), torch.from_numpy(i["kl"]).mean()
        ref, f32 = np.array([lp - kk, lp, kk]), np.array([float(lp32 - kk32), float(lp32), float(kk32)])
        assert rel_err(out["out3"], ref) <= _bound(rel_err(f32, ref), 16)
        g = i["g"].astype(np.float64)
        for got, want in ((out["dloglik"], (g[0] + g[1]) / self.B), (out["dkl"], (g[2] - g[0]) / self.B)):
            assert (got == got[0]).all() and abs(got[0] - want) <= 8 * ref64.U * abs(want)


class IwHead(Case):
    name, entry_points, B, K = "iw_head_B257_K5", ("svae_iw_head_forward", "svae_iw_head_backward"), 257, 5
    has_reference = True

    def inputs(self, seed):
        rs = np.random.RandomState(500 + seed)
        B, K = self.B, self.K
        return {"loglik": (-300.0 + 5.0 * rs.normal(size=(B, 1)) + 1.5 * rs.normal(size=(B, K))).astype(np.float32),
                "log_ratio": (-4.0 + 0.3 * rs.normal(size=(B, K))).astype(np.float32), "g": rs.normal(size=3).astype(np.float32)}

    def _outputs(self):
        n, f = self.B * self.K, np.float32
        return {"out3": ((3,), f), "weights": ((n,), f), "dloglik": ((n,), f), "dlog_ratio": ((n,), f)}

    def steps(self):
        p, g = self.ptr, self.real["g"].data_ptr()
        return [lambda st: self.L.svae_iw_head_forward(p("loglik"), p("log_ratio"), self.B, self.K, p("out3"), p("weights"), st),
                lambda st: self.L.svae_iw_head_backward(g, g + 4, g + 8, p("weights"), self.B, self.K, p("dloglik"),
                                                        p("dlog_ratio"), st)]

    def check(self, out):
        """The formulas of tests/test_gpu_iw_kernels.py's _head_case in torch float64, under that file's _bound."""
        from helpers import rel_err
        from test_gpu_iw_kernels import _bound
        Case.check(self, out)
        i = self.inputs(0)

        def formulas(dtype):
            l, r = (torch.from_numpy(i[k]).to(dtype).requires_grad_(True) for k in ("loglik", "log_ratio"))
            a = l + r
            out3 = torch.stack([(torch.logsumexp(a, 1) - math.log(self.K)).mean(), l.mean(), -r.mean()])
            (out3 * torch.from_numpy(i["g"]).to(dtype)).sum().backward()
            return {"out3": out3.detach().numpy(), "weights": torch.softmax(a, 1).detach().numpy().reshape(-1),
                    "dloglik": l.grad.numpy().reshape(-1), "dlog_ratio": r.grad.numpy().reshape(-1)}

        r64, r32 = formulas(torch.float64), formulas(torch.float32)
        for j in range(3):
            assert rel_err(out["out3"][j:j + 1], r64["out3"][j:j + 1]) <= _bound(rel_err(r32["out3"][j:j + 1], r64["out3"][j:j + 1]))
        for k in ("weights", "dloglik", "dlog_ratio"):
            assert rel_err(out[k], r64[k]) <= _bound(rel_err(r32[k], r64[k])), k


class IwStream(Case):
    """reset -> update (2 samples) -> update (3 samples) -> finish; the state record is the calls' own to initialise."""
    name = "iw_stream_B3_inf5_chunks_2_3"
    entry_points = ("svae_iw_stream_reset", "svae_iw_stream_update", "svae_iw_stream_finish")
    B, inf, chunks, has_reference = 3, 5, (2, 3), True

    def inputs(self, seed):
        rs = np.random.RandomState(9000 + seed)
        out = {}
        for i, k in enumerate(self.chunks):
            R = self.B * k
            out.update({"ll%d" % i: 3 * rs.normal(size=R), "lr%d" % i: 3 * rs.normal(size=R), "theta%d" % i: 0.3 + 0.5 * rs.normal(size=R),
                        "dx%d" % i: rs.normal(size=(R, 2)), "zc%d" % i: rs.normal(size=(R, self.inf - 3))})
        return {k: v.astype(np.float32) for k, v in out.items()}

    def _outputs(self):
        return {"per_image": ((self.B, _lib.iw_stream_cols(self.inf)), np.float32), "out3": ((3,), np.float32)}

    def _scratch_bytes(self):
        return {"state": _lib.lib().svae_iw_stream_state_bytes(self.B, self.inf)}

    def steps(self):
        d = self.desc = _lib.LatentDesc(self.B, self.inf, 1, 1, 0, 0.1, 1.0, math.pi)
        p, state = self.ptr, self.scratch["state"].ptr
        out = [lambda st: self.L.svae_iw_stream_reset(state, self.B, self.inf, st)]
        for i, k in enumerate(self.chunks):
            out.append(lambda st, i=i, k=k: self.L.svae_iw_stream_update(state, ctypes.byref(d), k, p("ll%d" % i), p("lr%d" % i),
                                                                        p("theta%d" % i), p("dx%d" % i), p("zc%d" % i), st))
        out.append(lambda st: self.L.svae_iw_stream_finish(state, ctypes.byref(d), p("per_image"), p("out3"), st))
        return out

    def check(self, out):
        """tests/iw_stream_ref.py on all five samples at once, column by column under tests/test_gpu_iw_stream.py's bounds."""
        from helpers import rel_err
        from iw_stream_ref import iw_stream_ref
        from test_gpu_iw_stream import _bound, _column_errors
        Case.check(self, out)
        i = self.inputs(0)
        B = self.B
        cat = lambda nm: np.concatenate([i["%s%d" % (nm, c)].reshape(B, k, -1) for c, k in enumerate(self.chunks)], 1)
        ll, lr = cat("ll")[:, :, 0], cat("lr")[:, :, 0]
        v = np.concatenate([cat("theta"), cat("dx"), cat("zc")], 2)
        ref, f32 = iw_stream_ref(ll, lr, v, True), iw_stream_ref(ll, lr, v, True, np.float32)
        errs = _column_errors(out["per_image"], ref[0], f32[0], self.inf, True)
        for j in range(3):
            errs["out3[%d]" % j] = (rel_err(out["out3"][j:j + 1], ref[1][j:j + 1]), _bound(rel_err(f32[1][j:j + 1], ref[1][j:j + 1])))
        assert not {c: e for c, e in errs.items() if not e[0] <= e[1]}, errs


# ---------------------------------------------------------------------------------------------------------------------
# the encoder's kernels
# ---------------------------------------------------------------------------------------------------------------------
class Colsum(Case):
    name, entry_points, has_reference = "colsum_57x33", ("svae_colsum",), True
    rows, cols = 57, 33

    def inputs(self, seed):
        return {"x": np.random.RandomState(57033 + seed).normal(size=(self.rows, self.cols)).astype(np.float32)}

    def _outputs(self):
        return {"out": ((self.cols,), np.float32)}

    def steps(self):
        return [lambda st: self.L.svae_colsum(self.ptr("x"), self.rows, self.cols, self.ptr("out"), st)]

    def check(self, out):
        """tests/test_gpu_loss_head.py: 4x the error of the fp32 column sums on the CPU, floor 4 * 2^-24."""
        from helpers import rel_err
        Case.check(self, out)
        x = self.inputs(0)["x"]
        ref = x.astype(np.float64).sum(0)
        assert rel_err(out["out"], ref) <= max(4 * rel_err(torch.from_numpy(x).sum(0).numpy(), ref), 4 * ref64.U)


class Linear(Case):
    entry_points, has_reference = ("svae_linear_forward", "svae_linear_backward"), True

    def __init__(self, M, K, N, act):
        self.M, self.K, self.N, self.act = M, K, N, act
        self.name = "linear_%dx%dx%d_%s" % (M, K, N, act)

    def inputs(self, seed):
        rs = np.random.RandomState(self.M * 1000 + self.K + self.N + 5 * seed)
        f = lambda *s: rs.normal(size=s).astype(np.float32)
        return {"x": f(self.M, self.K), "weight": (f(self.N, self.K) / np.sqrt(self.K)).astype(np.float32),
                "bias": (0.1 * f(self.N)).astype(np.float32), "dout": f(self.M, self.N)}

    def _outputs(self):
        f = np.float32
        return {"out": ((self.M, self.N), f), "dweight": ((self.N, self.K), f), "dbias": ((self.N,), f), "dx": ((self.M, self.K), f)}

    def steps(self):
        p, act = self.ptr, _lib.ACT[self.act]
        return [lambda st: self.L.svae_linear_forward(p("x"), p("weight"), p("bias"), p("out"), self.M, self.K, self.N, act, st),
                lambda st: self.L.svae_linear_backward(p("x"), p("weight"), p("out"), p("dout"), self.M, self.K, self.N, act,
                                                       p("dweight"), p("dbias"), p("dx"), st)]

    def check(self, out):
        """tests/test_gpu_encoder.py's reference and its bound of 5e-6 of the largest entry."""
        import torch.nn.functional as F
        from helpers import rel_err
        Case.check(self, out)
        i = {k: torch.from_numpy(v).double() for k, v in self.inputs(0).items()}
        x, w, b = (i[k].requires_grad_(True) for k in ("x", "weight", "bias"))
        pre = F.linear(x, w, b)
        ref = torch.tanh(pre) if self.act == "tanh" else F.leaky_relu(pre, 0.01)
        ref.backward(i["dout"])
        want = {"out": ref.detach(), "dweight": w.grad, "dbias": b.grad, "dx": x.grad}
        for k, v in want.items():
            assert rel_err(out[k], v.numpy()) < 5e-6, (self.name, k)


# ---------------------------------------------------------------------------------------------------------------------
# Adam and the gradient guard: n = 4 * 256 * 3 + 3 (three full rounds of a 256-thread float4 grid and a scalar tail)
# ---------------------------------------------------------------------------------------------------------------------
ADAM_N = 4 * 256 * 3 + 3
# the hyper-parameters cross the ABI as floats: the references below start from the numbers the library receives
LR, BETA1, BETA2, EPS = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8))


def _adam_inputs(rs, n):
    return {"param": rs.normal(size=n).astype(np.float32), "grad": rs.normal(size=n).astype(np.float32),
            "exp_avg": (0.1 * rs.normal(size=n)).astype(np.float32),
            "exp_avg_sq": (0.01 * rs.uniform(0.1, 1.0, size=n)).astype(np.float32)}


class Adam(Case):
    """svae_adam_step: the step number is a host argument (case.step, 4 unless a test sets another)."""
    entry_points, has_reference = ("svae_adam_step",), True
    state = ("param", "grad", "exp_avg", "exp_avg_sq")
    may_be_constant = ("grad",)

    def __init__(self, zero_grad):
        self.zero_grad, self.step, self.n = zero_grad, 4, ADAM_N
        self.name = "adam_zero%d" % zero_grad

    def inputs(self, seed):
        return _adam_inputs(np.random.RandomState(810 + seed), self.n)

    def steps(self):
        p = self.ptr
        return [lambda st: self.L.svae_adam_step(p("param"), p("grad"), p("exp_avg"), p("exp_avg_sq"), self.n, LR, BETA1, BETA2,
                                                 EPS, self.step, self.zero_grad, st)]

    def reference(self, i, step):
        """The header's formulas in float64 from fp32 inputs."""
        g, m, v, p = (i[k].astype(np.float64) for k in ("grad", "exp_avg", "exp_avg_sq", "param"))
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        p = p - (LR / (1 - BETA1 ** step)) * m / (np.sqrt(v) / np.sqrt(1 - BETA2 ** step) + EPS)
        return {"param": p, "exp_avg": m, "exp_avg_sq": v}

    def check(self, out):
        """A handful of fp32 roundings per entry: 8 * 2^-24 of the largest entry (the update is lr-sized against a unit
        parameter, so a wrong bias correction moves it by 1e-4, a thousand times the bound)."""
        from helpers import rel_err
        for k, want in self.reference(self.inputs(0), self.step).items():
            assert rel_err(out[k], want) <= 8 * ref64.U, (self.name, k)
        g0 = self.inputs(0)["grad"]
        assert np.array_equal(out["grad"], np.zeros_like(g0) if self.zero_grad else g0)


def _control_bytes(t):
    rec = _lib.GuardControl()
    rec.t = t
    return np.frombuffer(bytes(rec), np.int64).copy()


class Guard(Case):
    """svae_grad_guard_norm -> svae_adam_step_guarded with a max_norm that clips (|g| ~ 55 against 1); set B holds one inf,
    which must leave param, both moments and t alone."""
    name, entry_points = "guard_clip", ("svae_grad_guard_norm", "svae_adam_step_guarded")
    state = ("param", "grad", "exp_avg", "exp_avg_sq", "control")
    may_be_constant = non_finite_inputs = ("grad",)
    n, max_norm, zero_grad = ADAM_N, 1.0, 1

    def inputs(self, seed, finite=None):
        out = _adam_inputs(np.random.RandomState(910 + seed), self.n)
        if seed == 1 if finite is None else not finite:
            out["grad"][1234] = np.inf
        out["control"] = _control_bytes(3 + 4 * seed)
        return out

    def _scratch_bytes(self):
        return {"ws": max(_lib.lib().svae_grad_guard_workspace_bytes(self.n), 256)}

    def steps(self):
        p, ws = self.ptr, self.scratch["ws"]
        return [lambda st: self.L.svae_grad_guard_norm(p("grad"), self.n, self.max_norm, LR, BETA1, BETA2, p("control"), ws.ptr,
                                                       ws.nbytes, st),
                lambda st: self.L.svae_adam_step_guarded(p("param"), p("grad"), p("exp_avg"), p("exp_avg_sq"), self.n, BETA1,
                                                         BETA2, EPS, self.zero_grad, p("control"), st)]

    @staticmethod
    def record(control):
        rec = _lib.GuardControl()
        ctypes.memmove(ctypes.byref(rec), np.ascontiguousarray(control).tobytes(), ctypes.sizeof(rec))
        return rec

    def check(self, out):
        i = self.inputs(0)
        rec = self.record(out["control"])
        assert rec.t == 4 and rec.apply == 1 and rec.finite == 1 and rec.clipped == 1 and rec.coef < 1.0
        assert (out["param"] != i["param"]).any() and (out["grad"] == 0).all()
        assert abs(rec.total - np.sqrt((i["grad"].astype(np.float64) ** 2).sum())) <= 4 * np.spacing(np.float32(rec.total))


# ---------------------------------------------------------------------------------------------------------------------
# images: rotation, CTF filters, alignment and class sums, CTF correction
# ---------------------------------------------------------------------------------------------------------------------
class Rotate(Case):
    entry_points, has_reference, B = ("svae_rotate_bicubic",), True, 6

    def __init__(self, side, C, u8):
        self.side, self.C, self.u8 = side, C, u8
        self.name = "rotate_%d_C%d_%s" % (side, C, "u8" if u8 else "float")

    def offsets(self, seed):
        rs = np.random.RandomState(self.side + self.C + 3 * seed)
        quarter = [0.0, np.pi / 2, np.pi, 3 * np.pi / 2]
        return np.array((quarter if seed == 0 else quarter[::-1]) + [np.pi / 4, rs.uniform(0, 2 * np.pi)])

    def inputs(self, seed):
        rs = np.random.RandomState(100 + self.side + self.C + 3 * seed)
        n = self.side * self.side
        if self.u8:
            y = (np.floor(rs.uniform(size=(self.B, n, self.C)) * 255.0) / 255.0).astype(np.float32)
        else:
            y = rs.normal(size=(self.B, n, self.C)).astype(np.float32)
        mat, quarter = ops.rotation_matrices(self.offsets(seed), self.side, self.side)
        return {"y": y, "matrix": mat, "quarter": quarter}

    def _outputs(self):
        return {"y_rot": ((self.B, self.side * self.side, self.C), np.float32)}

    def steps(self):
        p = self.ptr
        return [lambda st: self.L.svae_rotate_bicubic(p("y"), p("y_rot"), p("matrix"), p("quarter"), self.B, self.side, self.side,
                                                      self.C, int(self.u8), st)]

    def check(self, out):
        """Bit-equal to oracle.pil_rotate, as tests/test_gpu_augment.py holds it."""
        from oracle import pil_rotate as R
        Case.check(self, out)
        y = self.inputs(0)["y"]
        want = R.augment_galaxy(y, self.offsets(0)) if self.u8 else R.augment_particles(y[:, :, 0], self.offsets(0))
        assert np.array_equal(out["y_rot"].reshape(want.shape), want)


class CtfFilter(Case):
    entry_points, has_reference, P, scale = ("svae_ctf_filter",), True, 9, 1.5

    def __init__(self, n):
        self.n = n
        self.name = "ctf_filter_%dx%d" % (n, n)

    def inputs(self, seed):
        return {"params": random_table(self.P, self.n + 1000 * seed)}

    def _outputs(self):
        return {"filters": ((self.P, self.n, self.n), np.float32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_ctf_filter_workspace_bytes(self.P, self.n, self.n)}

    def steps(self):
        ws = self.scratch.get("ws")
        return [lambda st: self.L.svae_ctf_filter(self.ptr("params"), self.ptr("filters"), self.P, self.n, self.n, self.scale,
                                                  ws.ptr if ws else None, ws.nbytes if ws else 0, st)]

    def check(self, out):
        """oracle.ctf_oracle.ctf_filter within tests/test_gpu_ctf.py's TOL."""
        from oracle import ctf_oracle as C
        from test_gpu_ctf import TOL, _rel
        Case.check(self, out)
        tab = self.inputs(0)["params"]
        want = C.ctf_filter({k: tab[:, i] for i, k in enumerate(C.COLUMNS)}, self.n, self.n, scale=self.scale)
        assert _rel(out["filters"], want) < TOL


class AlignAndSums(Case):
    """svae_align_images at tests/test_gpu_align.py's smallest ordinary shape, then svae_class_sums_update on what it wrote."""
    name, entry_points, has_reference = "align_3x9x9_sums", ("svae_align_images", "svae_class_sums_update"), True
    state = ("sum", "count")
    B, rows, cols, C, n_classes = 3, 9, 9, 1, 3

    def inputs(self, seed):
        rs = np.random.RandomState(100 * self.rows + self.cols + self.C + 17 * seed)
        B, N = self.B, self.rows * self.cols
        theta = rs.uniform(-np.pi, np.pi, B).astype(np.float32)
        dx = rs.uniform(-0.25, 0.25, (B, 2)).astype(np.float32)
        theta[0], dx[0] = 0.0, 0.0
        return {"y": rs.uniform(-1, 2, size=(B, N, self.C)).astype(np.float32), "theta": theta, "dx": dx,
                "label": np.array([[0, 2, -1], [2, 1, 1]][seed], np.int32),
                "sum": rs.normal(size=(self.n_classes, N, self.C)), "count": np.floor(rs.uniform(0, 5, size=(self.n_classes, N)))}

    def _outputs(self):
        N = self.rows * self.cols
        return {"aligned": ((self.B, N, self.C), np.float32), "cover": ((self.B, N), np.uint8)}

    def steps(self):
        p, N = self.ptr, self.rows * self.cols
        return [lambda st: self.L.svae_align_images(p("y"), p("theta"), p("dx"), self.B, self.rows, self.cols, self.C,
                                                    _lib.ALIGN_INTERP["bicubic"], p("aligned"), p("cover"), st),
                lambda st: self.L.svae_class_sums_update(p("aligned"), p("cover"), p("label"), self.B, N, self.C, self.n_classes,
                                                         p("sum"), p("count"), st)]

    def check(self, out):
        """tests/test_gpu_align.py's bound against align_ref; the sums bit-equal to class_sums_ref added to the start values."""
        from align_ref import align_ref, class_sums_ref
        i = self.inputs(0)
        ref, ref_cover = align_ref(i["y"], i["theta"], i["dx"], self.rows, self.cols, "bicubic")[:2]
        assert np.array_equal(out["cover"], ref_cover)
        r64 = ref.astype(np.float64)
        assert (np.abs(out["aligned"] - r64) <= 2.0 ** -23 * np.abs(r64) + 1e-12 * np.abs(i["y"]).max()).all()
        s, c = class_sums_ref([(out["aligned"], out["cover"], i["label"])], self.n_classes, self.rows * self.cols, self.C)
        assert np.array_equal(out["sum"], i["sum"] + s) and np.array_equal(out["count"], i["count"] + c)


class CtfApply(Case):
    entry_points, has_reference = ("svae_ctf_apply",), True

    def __init__(self, n, m, P):
        self.n, self.m, self.P, self.scale = n, m, P, 1.0
        self.name = "ctf_apply_%dx%d_P%d" % (n, m, P)

    def inputs(self, seed):
        rs = np.random.RandomState(1000 + self.n * self.m + self.P + 31 * seed)
        return {"y": rs.normal(size=(self.P, self.n, self.m)).astype(np.float32), "params": random_table(self.P, self.n + 500 * seed)}

    def _outputs(self):
        return {"out": ((self.P, self.n, self.m), np.float32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_ctf_apply_workspace_bytes(self.P, self.n, self.m)}

    def steps(self):
        ws = self.scratch.get("ws")
        return [lambda st: self.L.svae_ctf_apply(self.ptr("y"), self.ptr("params"), self.P, self.n, self.m, self.scale,
                                                 _lib.CTF_MODE["flip"], self.ptr("out"), ws.ptr if ws else None,
                                                 ws.nbytes if ws else 0, st)]

    def check(self, out):
        from ctfcorr_ref import apply_ref
        from test_gpu_ctfcorr import TOL, _plane_err
        Case.check(self, out)
        i = self.inputs(0)
        assert _plane_err(out["out"], apply_ref(i["y"], i["params"], self.n, self.m, self.scale, "flip")) <= TOL


class PowerAndWiener(Case):
    """svae_ctf_power_update onto a denominator that starts at set values, then svae_wiener_finish with it."""
    name, entry_points, has_reference = "ctf_power_wiener_7x10", ("svae_ctf_power_update", "svae_wiener_finish"), True
    state = ("den",)
    n, m, P, n_classes, scale, lam = 7, 10, 5, 4, 1.0, 1e-3

    def inputs(self, seed):
        rs = np.random.RandomState(7100 + seed)
        return {"params": random_table(self.P, 7 + 500 * seed), "label": np.array([[0, -1, 3, 1, 0], [1, 3, 0, -1, 3]][seed], np.int32),
                "den": rs.uniform(0.5, 2.0, size=(self.n_classes, self.n, self.m)),
                "sum": rs.normal(size=(self.n_classes, self.n * self.m))}

    def _outputs(self):
        return {"average": ((self.n_classes, self.n, self.m), np.float32)}

    def _scratch_bytes(self):
        return {"ws": _lib.lib().svae_wiener_finish_workspace_bytes(self.n_classes, self.n, self.m)}

    def steps(self):
        p, ws = self.ptr, self.scratch.get("ws")
        return [lambda st: self.L.svae_ctf_power_update(p("params"), p("label"), self.P, self.n, self.m, self.scale, self.n_classes,
                                                        p("den"), st),
                lambda st: self.L.svae_wiener_finish(p("sum"), p("den"), self.lam, self.n_classes, self.n, self.m, p("average"),
                                                     ws.ptr if ws else None, ws.nbytes if ws else 0, st)]

    def check(self, out):
        from ctfcorr_ref import finish_ref, power_ref
        from test_gpu_ctfcorr import TOL, TOL_POWER
        Case.check(self, out)
        i = self.inputs(0)
        den = i["den"] + power_ref([(i["params"], i["label"])], self.n_classes, self.n, self.m, self.scale)
        assert np.abs(out["den"] - den).max() <= TOL_POWER * np.abs(den).max()
        want = finish_ref(i["sum"].reshape(self.n_classes, self.n, self.m), den, self.lam, self.n, self.m)
        assert np.abs(out["average"] - want).max() <= TOL * np.abs(want).max()


# the global form of the CTF likelihood is taken above 150 KB of LDS: (88, 87) is ref64.CTF_PAIRS' one such pair (every pair
# of CTF_BOTH_FORMS takes the LDS form in a process that does not set SVAE_CTF_LDS=0)
CTF_LDS_PAIR = (10, 9)
CTF_GLOBAL_PAIR = (88, 87)

# the rows of the analysis headers (k-means, mixture, PCA, ring correlation, pose search, classification, soft averages,
# eigenimages, neighbour averages) live in a sibling file that subclasses Case, so it is imported here, below everything it needs
from stream_cases_analysis import analysis_cases            # noqa: E402


def make_cases():
    """Fresh, unallocated instances of every row of the table, in a fixed order."""
    out = [Decoder(n) for n in DECODER_CASES] + [Decoder("rank1_tanh", bce=True)]
    out += [Bce(), Gaussian(C=1, N=257), Gaussian(C=2, N=256, masked=True), Gaussian(ctf=CTF_LDS_PAIR, masked=True),
            Gaussian(ctf=CTF_GLOBAL_PAIR)]
    out += [Latent(), Latent(K=5), ElboHead(), IwHead(), IwStream(), Colsum(), Linear(17, 130, 33, "tanh"),
            Linear(5, 49, 24, "leakyrelu"), Adam(0), Adam(1), Guard(), Rotate(17, 1, False), Rotate(32, 3, True), CtfFilter(39),
            CtfFilter(81), AlignAndSums(), CtfApply(7, 10, 5), CtfApply(72, 72, 3), PowerAndWiener()]
    return out + analysis_cases()


NAMES = [c.name for c in make_cases()]
ANALYSIS_NAMES = [c.name for c in analysis_cases()]


def make_case(name):
    return next(c for c in make_cases() if c.name == name)


def covered_entry_points():
    return sorted({e for c in make_cases() for e in c.entry_points})
