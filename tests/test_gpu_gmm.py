"""The mixture kernels (include/svae_gmm.h: svae_gmm_init, svae_gmm_step; ops.GaussianMixture, elbo.mixture_latents) on the
MI355X against tests/gmm_ref.py, the float64 restatement of the header: labels, counts and iterations exactly equal, doubles
within 1e-10 (the device's exp and log are not numpy's; tests/test_gmm_cpu.py shows that a few ulps in them move nothing by
more than 1e-12, and that the fixtures' labels and convergence decisions are clear-cut).  Every buffer the calls write sits
inside guard bytes (decoder_abi.Guarded) and the workspace is exactly svae_gmm_workspace_bytes long."""
import ctypes

import numpy as np
import pytest
import torch

import gmm_ref as G
import kmeans_ref as K
from decoder_abi import GUARD_BYTE, Guarded

pytestmark = pytest.mark.gpu
E_INVALID, E_WORKSPACE = -1, -2
BOUND = 1e-10
FIXTURE_IDS = ["N%d_D%d_k%d" % f[1:4] for f in G.FIXTURES]
PARAMS = ("weight", "mean", "var")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


class Run(object):
    """One mixture problem through ctypes alone: x and label_in on the device, every output inside guard bytes."""

    def __init__(self, x, k, label_in=None):
        from spatial_vae_amd import _lib
        self.L = _lib.lib()
        dev = _dev()
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
        self.N, self.D, self.k = x.shape[0], x.shape[1], k
        self.label_in = None if label_in is None else torch.from_numpy(np.ascontiguousarray(label_in, np.int32)).to(dev)
        self.ws_bytes = self.L.svae_gmm_workspace_bytes(self.N, self.D, k)
        assert self.ws_bytes > 0
        N, D = self.N, self.D
        self.bufs = {"weight": (Guarded(k * 8, dev), np.float64, (k,)), "mean": (Guarded(k * D * 8, dev), np.float64, (k, D)),
                     "var": (Guarded(k * D * 8, dev), np.float64, (k, D)), "resp": (Guarded(N * k * 8, dev), np.float64, (N, k)),
                     "label": (Guarded(N * 4, dev), np.int32, (N,)), "loglik_point": (Guarded(N * 8, dev), np.float64, (N,)),
                     "rec": (Guarded(48, dev), np.int64, (6,)), "ws": (Guarded(self.ws_bytes, dev), np.uint8, (self.ws_bytes,))}
        self.bufs["rec"][0].fill_byte(0)           # all zero bytes = a fresh record

    def ptr(self, name):
        return self.bufs[name][0].ptr

    def put(self, name, array):
        g, dt, shape = self.bufs[name]
        raw = torch.from_numpy(np.ascontiguousarray(array, dt).reshape(-1).view(np.uint8).copy()).to(_dev())
        g.buf[g.off:g.off + g.nbytes].copy_(raw)

    def put_state(self, state):
        for key in PARAMS:
            self.put(key, state[key])

    def init(self, reg=G.FIT_REG):
        p = self.ptr
        return self.L.svae_gmm_init(self.x.data_ptr(), self.N, self.D, self.k, self.label_in.data_ptr(), reg, p("weight"), p("mean"), p("var"),
                                    p("resp"), p("rec"), p("ws"), self.ws_bytes, _stream())

    def step(self, update=1, reg=G.FIT_REG, tol=G.FIT_TOL, loglik_point=True):
        p = self.ptr
        return self.L.svae_gmm_step(self.x.data_ptr(), self.N, self.D, self.k, update, reg, tol, p("weight"), p("mean"), p("var"), p("resp"),
                                    p("label"), p("loglik_point") if loglik_point else None, p("rec"), p("ws"), self.ws_bytes, _stream())

    def read(self, names=None):
        """The named buffers (default: all) as numpy, the record's fields by name; asserts the guard bytes are intact."""
        torch.cuda.synchronize()
        out = {}
        for name, (g, dt, shape) in self.bufs.items():
            if names is not None and name not in names and name != "rec":
                continue
            pay, intact = g.read()
            assert intact, "written outside " + name
            out[name] = pay.view(dt).reshape(shape).copy()
        rec = out["rec"]
        out.update(iterations=int(rec[0]), converged_at=int(rec[1]), assigned=int(rec[2]), dead=int(rec[3]),
                   loglik=float(rec[4:5].view(np.float64)[0]), previous=float(rec[5:6].view(np.float64)[0]))
        return out


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _rel(got, want):
    """The largest |got - want| / max(1, |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _assert_e_part(got, want, what):
    """resp within 1e-10 absolute, loglik_point and loglik within 1e-10 max(1, |.|), every label and the counts equal.  Returns
    the three errors."""
    assert np.array_equal(got["label"], want["label"]), (what, "label", int((got["label"] != want["label"]).sum()))
    errs = (float(np.abs(got["resp"] - want["resp"]).max()), _rel(got["loglik_point"], want["loglik_point"]), _rel(got["loglik"], want["loglik"]))
    assert errs[0] <= BOUND and errs[1] <= BOUND and errs[2] <= BOUND, (what, errs)
    assert got["assigned"] == want["assigned"] and got["dead"] == want["dead"], (what, got["assigned"], got["dead"])
    return errs


def _assert_params(got, want, what):
    """weight, mean and var within 1e-10 relative (of max(1, |.|)); returns the largest error."""
    errs = [_rel(got[key], want[key]) for key in PARAMS]
    assert max(errs) <= BOUND, (what, errs)
    return max(errs)


@pytest.mark.parametrize("fixture", G.FIXTURES, ids=FIXTURE_IDS)
def test_one_e_part_from_given_parameters(fixture):
    """The reference's parameters after three update steps uploaded, one update = 0 call on a fresh record, once more without
    loglik_point: resp, loglik_point, loglik and every label held to the reference; the parameters and the record's iterations,
    converged_at and previous come back bit-equal.  MI355X, the largest over the fixtures: resp 5.6e-16, loglik_point 6.9e-16,
    loglik 1.7e-16."""
    x, label_in, centres = G.fixture(*fixture)
    state = G.fixture_states(*fixture)[3]
    want = G.step(x, state, 0, G.FIT_REG, G.FIT_TOL)
    run = Run(x, fixture[3])
    run.put_state(state)
    assert run.step(0) == 0
    got = run.read()
    errs = _assert_e_part(got, want, "E part")
    print("N %d D %d k %d: resp %.2e, loglik_point %.2e, loglik %.2e" % (fixture[1:4] + errs))
    for key in PARAMS:
        assert _same_bytes(got[key], state[key]), key
    assert (got["iterations"], got["converged_at"], got["previous"]) == (0, 0, 0.0)
    run.bufs["loglik_point"][0].fill_byte(GUARD_BYTE)
    assert run.step(0, loglik_point=False) == 0
    again = run.read()
    assert (again["loglik_point"].view(np.uint8) == GUARD_BYTE).all()
    for key in ("resp", "label", "rec") + PARAMS:
        assert _same_bytes(again[key], got[key]), key


@pytest.mark.parametrize("fixture", G.FIXTURES, ids=FIXTURE_IDS)
def test_init_and_a_25_step_fit_equal_the_reference(fixture):
    """svae_gmm_init from the fixture's k-means start: one-hot resp exactly, parameters within 1e-10 relative, a zeroed record
    with assigned and dead.  Then 25 update steps and the labelling call: after the first step and at the end parameters, resp
    and labels, and after every step the loglik (the trace), iterations and converged_at held to the reference.  The labelling
    call leaves parameters and iterations, converged_at, previous bit-equal.  A second run on fresh buffers is bit-equal
    throughout.  MI355X, the largest over the fixtures: init 0 (bit-equal), parameters 3.9e-16, resp 3.9e-15, trace 3.5e-16."""
    x, label_in, centres = G.fixture(*fixture)
    states = G.fixture_states(*fixture)
    k = fixture[3]
    runs = []
    for attempt in range(2):
        run = Run(x, k, label_in)
        run.put("mean", centres)
        run.put("rec", np.full(6, -1, np.int64))           # init zeroes the record itself
        assert run.init() == 0
        got = run.read()
        if attempt == 0:
            assert _same_bytes(got["resp"], states[0]["resp"])
            e_init = _assert_params(got, states[0], "init")
            assert [got[key] for key in ("iterations", "converged_at", "assigned", "dead", "loglik", "previous")] == \
                [0, 0, states[0]["assigned"], states[0]["dead"], 0.0, 0.0]
        kept = [got]
        e_par = e_resp = e_trace = 0.0
        for i, want in enumerate(states[1:]):
            update = 1 if i < G.FIT_STEPS else 0
            if not update:
                before = run.read(PARAMS)
            assert run.step(update) == 0
            got = run.read(None if i in (0, G.FIT_STEPS) else ())
            kept.append(got)
            if attempt:
                continue
            e_trace = max(e_trace, _rel(got["loglik"], want["loglik"]))
            assert e_trace <= BOUND, (i, got["loglik"], want["loglik"])
            assert got["iterations"] == want["iterations"] and got["converged_at"] == want["converged_at"], (i, got["iterations"], got["converged_at"])
            assert _rel(got["previous"], want["previous"]) <= BOUND
            if "resp" in got:
                e_par = max(e_par, _assert_params(got, want, "step %d" % i))
                e_resp = max(e_resp, _assert_e_part(got, want, "step %d" % i)[0])
            if not update:
                for key in PARAMS:
                    assert _same_bytes(got[key], before[key]), key
                assert np.array_equal(got["rec"][[0, 1, 5]], before["rec"][[0, 1, 5]])
        if attempt == 0:
            print("N %d D %d k %d: init %.2e, parameters %.2e, resp %.2e, trace %.2e; iterations %d, converged_at %d"
                  % (fixture[1:4] + (e_init, e_par, e_resp, e_trace, got["iterations"], got["converged_at"])))
        runs.append(kept)
    for a, b in zip(*runs):
        assert sorted(a) == sorted(b)
        for key in a:
            if isinstance(a[key], np.ndarray) and key != "ws":
                assert _same_bytes(a[key], b[key]), key


def test_steps_after_convergence_change_no_bit():
    """The baseline fixture converges at its first iteration; three further update steps leave every buffer and the record as
    they were."""
    fixture = G.FIXTURES[0]
    x, label_in, centres = G.fixture(*fixture)
    run = Run(x, fixture[3], label_in)
    run.put("mean", centres)
    assert run.init() == 0
    for _ in range(3):
        assert run.step(1) == 0
    a = run.read()
    assert a["converged_at"] == 1 == a["iterations"]
    for _ in range(3):
        assert run.step(1) == 0
    b = run.read()
    for key in a:
        if isinstance(a[key], np.ndarray) and key != "ws":
            assert _same_bytes(a[key], b[key]), key


def test_non_finite_points_and_a_dead_component():
    """Three points carrying NaN, +inf and -inf, and a label_in without class 2 (its members moved to class 1) with one entry out
    of range: the dead component gets weight 0, keeps the mean and var it came with, is never a label and has a zero resp column;
    the three points are label -1 with zero rows, loglik_point 0 and outside `assigned`; everything stays finite and equals the
    reference along six steps."""
    x, u = K.blobs(1, 700, 3, 4)
    km = K.fit(x, 4, u, 10)
    label_in = km["label"].astype(np.int32)
    label_in[label_in == 2] = 1
    label_in[5] = 9
    x = x.copy()
    x[3, 1], x[300, 0], x[699, 2] = np.nan, np.inf, -np.inf
    run = Run(x, 4, label_in)
    run.put("mean", km["centres"])
    run.put("var", np.zeros((4, 3)))
    assert run.init() == 0
    want = G.init(x, label_in, km["centres"], G.FIT_REG)
    got = run.read()
    assert _same_bytes(got["resp"], want["resp"]) and (got["resp"][[3, 5, 300, 699]] == 0).all()
    _assert_params(got, want, "init")
    assert got["assigned"] == 697 and got["dead"] == 1 and got["weight"][2] == 0
    for i, update in enumerate([1] * 5 + [0]):
        want = G.step(x, want, update, G.FIT_REG, 0.0)
        assert run.step(update, tol=0.0) == 0
        got = run.read()
        _assert_e_part(got, want, "step %d" % i)
        _assert_params(got, want, "step %d" % i)
        assert got["iterations"] == want["iterations"] and got["converged_at"] == want["converged_at"]
    assert got["label"][[3, 300, 699]].tolist() == [-1, -1, -1] and (got["resp"][[3, 300, 699]] == 0).all()
    assert (got["loglik_point"][[3, 300, 699]] == 0).all() and got["assigned"] == 697
    assert got["dead"] == 1 and got["weight"][2] == 0 and not (got["label"] == 2).any() and (got["resp"][:, 2] == 0).all()
    assert _same_bytes(got["mean"][2], km["centres"][2]) and (got["var"][2] == 0).all()
    for key in PARAMS + ("resp", "loglik_point"):
        assert np.isfinite(got[key]).all(), key
    assert np.isfinite(got["loglik"]) and abs(got["weight"].sum() - 1) <= 1e-12


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_buffers_untouched():
    """Every SVAE_E_INVALID case of the header, and the workspace refusals: the status, a message, and every output still the
    fill bytes inside intact guards."""
    x, label_in, centres = G.fixture(*G.FIXTURES[0])
    run = Run(x, 4, label_in)
    for name, (g, _, _) in run.bufs.items():
        g.fill_byte(GUARD_BYTE)
    L, X, LAB, st = run.L, run.x.data_ptr(), run.label_in.data_ptr(), _stream()
    p = run.ptr
    ws, wb = p("ws"), run.ws_bytes
    inf, nan = float("inf"), float("nan")

    def init(x=X, N=300, D=3, k=4, label_in=LAB, reg=1e-6, weight=p("weight"), mean=p("mean"), var=p("var"), resp=p("resp"), rec=p("rec"),
             ws=ws, wb=wb):
        return L.svae_gmm_init(x, N, D, k, label_in, reg, weight, mean, var, resp, rec, ws, wb, st)

    def step(x=X, N=300, D=3, k=4, reg=1e-6, tol=1e-8, weight=p("weight"), mean=p("mean"), var=p("var"), resp=p("resp"), label=p("label"),
             point=p("loglik_point"), rec=p("rec"), ws=ws, wb=wb):
        return L.svae_gmm_step(x, N, D, k, 1, reg, tol, weight, mean, var, resp, label, point, rec, ws, wb, st)

    assert L.svae_gmm_workspace_bytes(2 ** 31, 3, 4) == 0
    invalid = [init(D=0), init(D=65), init(k=0), init(k=1025), init(N=3), init(N=2 ** 31), init(x=None), init(label_in=None),
               init(weight=None), init(mean=None), init(var=None), init(resp=None), init(rec=None), init(weight=p("weight") + 4),
               init(mean=p("mean") + 4), init(var=p("var") + 4), init(resp=p("resp") + 4), init(rec=p("rec") + 4), init(reg=0.0),
               init(reg=-1.0), init(reg=inf), init(reg=nan),
               step(D=0), step(D=65), step(k=0), step(k=1025), step(N=3), step(N=2 ** 31), step(x=None), step(label=None),
               step(weight=None), step(mean=None), step(var=None), step(resp=None), step(rec=None), step(weight=p("weight") + 4),
               step(mean=p("mean") + 4), step(var=p("var") + 4), step(resp=p("resp") + 4), step(rec=p("rec") + 4),
               step(point=p("loglik_point") + 4), step(reg=0.0), step(reg=inf), step(reg=nan), step(tol=-1e-9), step(tol=inf),
               step(tol=nan)]
    assert invalid == [E_INVALID] * len(invalid), invalid
    assert b"svae_gmm_step" in L.svae_last_error()
    workspace = [init(ws=None), init(ws=ws + 8), init(wb=wb - 1), step(ws=None), step(ws=ws + 8), step(wb=wb - 1)]
    assert workspace == [E_WORKSPACE] * len(workspace), workspace
    torch.cuda.synchronize()
    for name, (g, _, _) in run.bufs.items():
        pay, intact = g.read()
        assert intact and (pay == GUARD_BYTE).all(), name
    run.put("mean", centres)
    assert init() == 0 and step() == 0              # the same buffers are fine with valid arguments
    run.read()


def test_ops_refuses_shape_and_dtype_mistakes():
    from spatial_vae_amd import ops
    dev = _dev()
    gm = ops.GaussianMixture(3, 2, dev)
    x = torch.zeros(10, 2, device=dev)
    lab = torch.zeros(10, dtype=torch.int32, device=dev)
    cen = torch.zeros(3, 2, dtype=torch.float64, device=dev)
    for points, label, centres, reg, tol in [(x.cpu(), lab, cen, 1e-6, 0), (x.double(), lab, cen, 1e-6, 0), (x[:2], lab[:2], cen, 1e-6, 0),
                                             (x, lab.long(), cen, 1e-6, 0), (x, lab[:9], cen, 1e-6, 0), (x, lab.cpu(), cen, 1e-6, 0),
                                             (x, lab, cen.float(), 1e-6, 0), (x, lab, cen[:2], 1e-6, 0), (x, lab, cen, 0.0, 0),
                                             (x, lab, cen, 1e-6, -1.0), (x, lab, cen, float("nan"), 0)]:
        with pytest.raises(RuntimeError):
            gm.fit(points, label, centres, 2, reg, tol)
    for k, D, device in [(0, 2, dev), (1025, 2, dev), (3, 65, dev), (3, 2, "cpu")]:
        with pytest.raises(RuntimeError):
            ops.GaussianMixture(k, D, device)


# ---------------------------------------------------------------- the host side: ops.GaussianMixture.fit and elbo.mixture_latents
def test_mixture_latents_fit_trace_and_the_threshold_on_the_device():
    """elbo.mixture_latents on the (1000, 8, 6) fixture from device k-means tensors: the GmmFit equals gmm_ref.fit (trace of
    iters + 1 logliks included), max_resp is the row maximum and label_used is the label where max_resp >= min_resp, else -1;
    the k-means inputs are left as they were."""
    from spatial_vae_amd import elbo as E
    from spatial_vae_amd import ops
    fixture = G.FIXTURES[2]
    x, label_in, centres = G.fixture(*fixture)
    dev = _dev()
    km = {"label": torch.from_numpy(label_in).to(dev), "centres": torch.from_numpy(centres).to(dev)}
    iters, min_resp = 6, 0.9
    out = E.mixture_latents(torch.from_numpy(x).to(dev), km, iters, G.FIT_REG, G.FIT_TOL, min_resp)
    want = G.fit(x, label_in, centres, iters, G.FIT_REG, G.FIT_TOL)
    got = {key: v.cpu().numpy() for key, v in out.items()}
    assert np.array_equal(km["label"].cpu().numpy(), label_in) and _same_bytes(km["centres"].cpu().numpy(), centres)
    assert got["trace"].shape == (iters + 1,) and _rel(got["trace"], want["trace"]) <= BOUND
    _assert_params(got, want, "fit")
    assert np.array_equal(got["label"], want["label"]) and out["label"].dtype == torch.int32 and out["label_used"].dtype == torch.int32
    assert np.abs(got["resp"] - want["resp"]).max() <= BOUND and _rel(got["loglik_point"], want["loglik_point"]) <= BOUND
    rec = ops.GaussianMixture.read_record(out["record"])
    assert rec["iterations"] == want["iterations"] == iters and rec["converged_at"] == want["converged_at"] == 0
    assert rec["assigned"] == 1000 and rec["dead"] == 0 and rec["loglik"] == got["trace"][-1]
    assert np.array_equal(got["max_resp"], got["resp"].max(1))
    low = got["max_resp"] < min_resp
    assert 0 < low.sum() < 1000
    assert np.array_equal(got["label_used"], np.where(low, -1, got["label"]))
