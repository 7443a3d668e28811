"""The PCA kernels (include/svae_pca.h: svae_pca_moments, svae_pca_eigen, svae_pca_project; ops.LatentPCA, elbo.principal_axes)
on the MI355X against tests/pca_ref.py, the float64 restatement of the header: counts, sweeps and the dead and skipped
conventions exactly equal, doubles within 1e-10 (the project's bound for its double kernels; tests/test_pca_cpu.py asserts the
eigenvalue gaps that make the vectors comparable).  Every buffer the calls write sits inside guard bytes (decoder_abi.Guarded)
and the workspace is exactly svae_pca_workspace_bytes long."""
import ctypes

import numpy as np
import pytest
import torch

import pca_ref as R
from decoder_abi import GUARD_BYTE, Guarded

pytestmark = pytest.mark.gpu
E_INVALID, E_WORKSPACE = -1, -2
BOUND = 1e-10
IDS = [R.fixture_id(f) for f in R.FIXTURES]
OUTPUTS = ("count", "mean", "cov", "eigenvalues", "components", "sweeps", "off_norm", "proj")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


class Run(object):
    """One PCA problem through ctypes alone: x and group on the device, every output inside guard bytes."""

    def __init__(self, x, group, G, P=None):
        from spatial_vae_amd import _lib
        self.L = _lib.lib()
        dev = _dev()
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
        self.N, self.D = x.shape
        self.G, self.P = G, self.D if P is None else P
        self.group = None if group is None else torch.from_numpy(np.ascontiguousarray(group, np.int32)).to(dev)
        self.ws_bytes = self.L.svae_pca_workspace_bytes(self.N, self.D, G)
        assert self.ws_bytes == R.workspace_bytes(self.N, self.D, G) > 0
        N, D, P = self.N, self.D, self.P
        self.bufs = {"count": (Guarded(G * 8, dev), np.int64, (G,)), "mean": (Guarded(G * D * 8, dev), np.float64, (G, D)),
                     "cov": (Guarded(G * D * D * 8, dev), np.float64, (G, D, D)),
                     "eigenvalues": (Guarded(G * D * 8, dev), np.float64, (G, D)),
                     "components": (Guarded(G * D * D * 8, dev), np.float64, (G, D, D)),
                     "sweeps": (Guarded(G * 4, dev), np.int32, (G,)), "off_norm": (Guarded(G * 8, dev), np.float64, (G,)),
                     "proj": (Guarded(N * P * 8, dev), np.float64, (N, P)), "ws": (Guarded(self.ws_bytes, dev), np.uint8, (self.ws_bytes,))}

    def ptr(self, name):
        return self.bufs[name][0].ptr

    def put(self, name, array):
        g, dt, shape = self.bufs[name]
        raw = torch.from_numpy(np.ascontiguousarray(array, dt).reshape(-1).view(np.uint8).copy()).to(_dev())
        g.buf[g.off:g.off + g.nbytes].copy_(raw)

    def _group(self):
        return None if self.group is None else self.group.data_ptr()

    def moments(self, stream=None):
        p = self.ptr
        return self.L.svae_pca_moments(self.x.data_ptr(), self.N, self.D, self.G, self._group(), p("count"), p("mean"), p("cov"), p("ws"),
                                       self.ws_bytes, stream or _stream())

    def eigen(self, stream=None):
        p = self.ptr
        return self.L.svae_pca_eigen(p("cov"), self.D, self.G, p("eigenvalues"), p("components"), p("sweeps"), p("off_norm"),
                                     stream or _stream())

    def project(self, stream=None):
        p = self.ptr
        return self.L.svae_pca_project(self.x.data_ptr(), self.N, self.D, self.G, self.P, self._group(), p("count"), p("mean"),
                                       p("components"), p("proj"), stream or _stream())

    def fit(self, stream=None):
        assert self.moments(stream) == 0 and self.eigen(stream) == 0 and self.project(stream) == 0
        return self

    def read(self, names=OUTPUTS):
        """The named buffers as numpy; asserts the guard bytes of every buffer are intact."""
        torch.cuda.synchronize()
        out = {}
        for name, (g, dt, shape) in self.bufs.items():
            pay, intact = g.read()
            assert intact, "written outside " + name
            if name in names:
                out[name] = pay.view(dt).reshape(shape).copy()
        return out

    def untouched(self):
        """Whether every output still holds the fill bytes and every guard is intact."""
        torch.cuda.synchronize()
        for name, (g, dt, shape) in self.bufs.items():
            pay, intact = g.read()
            if not intact or not (pay == GUARD_BYTE).all():
                return False
        return True


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _scaled(got, want):
    """The largest |got - want| over the largest |want| (1 where that is 0)."""
    top = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max() / (top if top > 0 else 1.0)) if want.size else 0.0


def _assert_decomposition(cov, lam, comp, what):
    """Against the device's own input: residual |C V^T - V^T L| and orthogonality within 1e-10 of the largest eigenvalue (an
    absolute 1e-10 for the orthogonality of unit vectors); descending order and the sign rule exactly.  Returns both errors."""
    D = lam.shape[0]
    top = max(float(np.abs(lam).max()), np.finfo(np.float64).tiny)
    residual = float(np.abs(cov.dot(comp.T) - comp.T * lam).max() / top)
    ortho = float(np.abs(comp.dot(comp.T) - np.eye(D)).max())
    assert residual <= BOUND and ortho <= BOUND, (what, residual, ortho)
    assert (np.diff(lam) <= 0).all(), (what, "not descending")
    at = np.abs(comp).argmax(1)                     # the first of equal magnitudes
    assert (comp[np.arange(D), at] > 0).all(), (what, "sign rule")
    return residual, ortho


@pytest.mark.parametrize("fixture", R.FIXTURES, ids=IDS)
def test_the_three_calls_against_the_reference(fixture):
    """svae_pca_moments, svae_pca_eigen and svae_pca_project on one fixture: count and sweeps equal; a dead group's mean, cov,
    eigenvalues and components, and the rows of proj of points in no group or in a dead one, bit-equal to the header's
    conventions; mean, cov, eigenvalues and proj within 1e-10 of the group's largest reference value, components within 1e-10;
    residual and orthogonality of every live group against the device's own cov."""
    x, group = R.fixture(*fixture)
    N, D, G = fixture[1:]
    want = R.fixture_fit(*fixture)
    got = Run(x, group, G).fit().read()
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["sweeps"], want["sweeps"])
    member = R.members(x, group, G)
    errs = dict.fromkeys(("mean", "cov", "eigenvalues", "components", "proj", "off_norm", "residual", "orthogonality"), 0.0)
    for g in range(G):
        if want["count"][g] < 2:
            for key in ("mean", "cov", "eigenvalues", "components", "off_norm"):
                assert _same_bytes(got[key][g], want[key][g]), (g, key)
            assert got["sweeps"][g] == 0 and np.array_equal(got["components"][g], np.eye(D))
            continue
        for key in ("mean", "cov", "eigenvalues"):
            errs[key] = max(errs[key], _scaled(got[key][g], want[key][g]))
        errs["components"] = max(errs["components"], float(np.abs(got["components"][g] - want["components"][g]).max()))
        errs["off_norm"] = max(errs["off_norm"], abs(got["off_norm"][g] - want["off_norm"][g]) / want["eigenvalues"][g, 0])
        mine = member == g
        errs["proj"] = max(errs["proj"], _scaled(got["proj"][mine], want["proj"][mine]))
        r, o = _assert_decomposition(got["cov"][g], got["eigenvalues"][g], got["components"][g], (fixture, g))
        errs["residual"], errs["orthogonality"] = max(errs["residual"], r), max(errs["orthogonality"], o)
    out_of_it = (member < 0) | (want["count"][np.maximum(member, 0)] < 2)
    assert _same_bytes(got["proj"][out_of_it], np.zeros((int(out_of_it.sum()), D)))
    bit_equal = all(_same_bytes(got[key], want[key]) for key in ("mean", "cov", "eigenvalues", "components", "proj"))
    print("%s: %s; bit-equal to the reference: %s" % (R.fixture_id(fixture), ", ".join("%s %.1e" % kv for kv in errs.items()), bit_equal))
    for key in ("mean", "cov", "eigenvalues", "components", "proj", "off_norm"):
        assert errs[key] <= BOUND, (key, errs[key])


def test_fewer_components_than_coordinates():
    """P < D: proj is the first P columns of the P == D result, bit for bit."""
    f = R.FIXTURES[4]
    x, group = R.fixture(*f)
    full = Run(x, group, f[3]).fit().read(("proj",))["proj"]
    for P in (1, 3):
        part = Run(x, group, f[3], P).fit().read(("proj",))["proj"]
        assert part.shape == (f[1], P) and _same_bytes(part, full[:, :P])


def test_special_matrices_in_one_eigen_call():
    """Four 12 x 12 matrices in one call: one that is diagonal already (0 sweeps, sorted with equal values by ascending column,
    the unit vectors bit for bit), the covariance of points of rank 4 (eight eigenvalues within 1e-10 of 0 relative to the
    largest), one with a NaN (skipped: zeros and sweeps -1) and the all-zero one (0 sweeps, the identity) -- each held to the
    reference and, where it is decomposed, to its own residual and orthogonality."""
    D = 12
    low = R.moments(R.low_rank(3, 200, D, 4))["cov"][0]
    bad = low.copy()
    bad[5, 2] = np.nan
    cov = np.stack([R.diagonal_cov(D)[0], low, bad, np.zeros((D, D))])
    want = R.eigen(cov)
    run = Run(np.zeros((4, D), np.float32), None, 4)
    run.put("cov", cov)
    assert run.eigen() == 0
    got = run.read(("eigenvalues", "components", "sweeps", "off_norm"))
    assert got["sweeps"].tolist() == want["sweeps"].tolist() and got["sweeps"][0] == 0 and got["sweeps"][2] == -1 and got["sweeps"][3] == 0
    for g in (0, 2, 3):
        for key in ("eigenvalues", "components", "off_norm"):
            assert _same_bytes(got[key][g], want[key][g]), (g, key)
    d = np.diag(cov[0])
    assert np.array_equal(got["components"][0], np.eye(D)[np.argsort(-d, kind="stable")]) and np.array_equal(got["components"][3], np.eye(D))
    assert not got["eigenvalues"][2].any() and not got["components"][2].any()
    assert _scaled(got["eigenvalues"][1], want["eigenvalues"][1]) <= BOUND
    assert np.abs(got["eigenvalues"][1][4:]).max() <= BOUND * got["eigenvalues"][1][0]
    r, o = _assert_decomposition(cov[1], got["eigenvalues"][1], got["components"][1], "rank 4 of 12")
    _assert_decomposition(cov[0], got["eigenvalues"][0], got["components"][0], "diagonal")
    print("rank 4 of 12: %d sweeps, residual %.1e, orthogonality %.1e, off_norm %.1e" % (got["sweeps"][1], r, o, got["off_norm"][1]))


# ---------------------------------------------------------------- bit-equality
@pytest.mark.parametrize("fixture", [R.FIXTURES[5], R.FIXTURES[9]], ids=[IDS[5], IDS[9]])
def test_repeated_and_side_stream_calls_are_bit_equal(fixture):
    """The same calls again into fresh buffers, and once more on a non-default stream: every output bit-equal."""
    x, group = R.fixture(*fixture)
    first = Run(x, group, fixture[3]).fit().read()
    again = Run(x, group, fixture[3]).fit().read()
    side = torch.cuda.Stream(_dev())
    run = Run(x, group, fixture[3])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        run.fit(ctypes.c_void_p(side.cuda_stream))
    side.synchronize()
    other = run.read()
    for key in OUTPUTS:
        assert _same_bytes(first[key], again[key]), ("repeated", key)
        assert _same_bytes(first[key], other[key]), ("side stream", key)


@pytest.mark.parametrize("fixture", [R.FIXTURES[8], R.FIXTURES[10]], ids=[IDS[8], IDS[10]])
def test_groups_in_one_call_equal_single_group_calls(fixture):
    """G groups in one call against G calls with G == 1 on the same rows, the members of the group labelled 0 and everybody else
    -1: count, mean, cov, eigenvalues, components, sweeps, off_norm and the members' rows of proj bit-equal."""
    x, group = R.fixture(*fixture)
    G = fixture[3]
    together = Run(x, group, G).fit().read()
    member = R.members(x, group, G)
    for g in range(G):
        alone = Run(x, np.where(group == g, 0, -1).astype(np.int32), 1).fit().read()
        for key in ("count", "mean", "cov", "eigenvalues", "components", "sweeps", "off_norm"):
            assert _same_bytes(together[key][g], alone[key][0]), (g, key)
        assert _same_bytes(together["proj"][member == g], alone["proj"][member == g]), g
        assert not alone["proj"][member != g].any()


def test_the_wrappers_make_the_same_calls():
    """ops.LatentPCA.fit and elbo.principal_axes return what the three calls write, bit for bit, with explained_variance_ratio =
    eigenvalues / their sum and 0 for a dead group."""
    from spatial_vae_amd import elbo as E
    from spatial_vae_amd import ops
    f = R.FIXTURES[8]
    x, group = R.fixture(*f)
    want = Run(x, group, f[3], 2).fit().read()
    xd, gd = torch.from_numpy(x).to(_dev()), torch.from_numpy(group).to(_dev())
    fit = ops.LatentPCA(f[2], _dev()).fit(xd, gd, f[3], 2)
    axes = E.principal_axes(xd, gd, f[3], 2)
    for key in OUTPUTS:
        assert _same_bytes(getattr(fit, key).cpu().numpy(), want[key]), key
        assert _same_bytes(axes["projections" if key == "proj" else key].cpu().numpy(), want[key]), key
    ratio = axes["explained_variance_ratio"].cpu().numpy()
    total = want["eigenvalues"].sum(1, keepdims=True)
    assert np.abs(ratio - np.where(total != 0, want["eigenvalues"] / np.where(total != 0, total, 1), 0)).max() <= 1e-15
    assert not ratio[want["count"] < 2].any() and np.abs(ratio[want["count"] >= 2].sum(1) - 1).max() <= 1e-14
    whole = E.principal_axes(xd)
    assert whole["mean"].shape == (1, f[2]) and whole["projections"].shape == (f[1], f[2])


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_buffers_untouched():
    """Every SVAE_E_INVALID and SVAE_E_WORKSPACE case of the header, one call each: the status, a message in svae_last_error,
    and afterwards every output and the workspace still hold their fill bytes inside intact guards."""
    x, group = R.fixture(*R.FIXTURES[8])
    N, D, G = R.FIXTURES[8][1:]
    run = Run(x, group, G)
    L, p = run.L, run.ptr
    xp, gp, st = run.x.data_ptr(), run.group.data_ptr(), _stream()

    def moments(x=xp, N=N, D=D, G=G, group=gp, count=p("count"), mean=p("mean"), cov=p("cov"), ws=p("ws"), ws_bytes=run.ws_bytes):
        return L.svae_pca_moments(x, N, D, G, group, count, mean, cov, ws, ws_bytes, st)

    def eigen(cov=p("cov"), D=D, G=G, eigenvalues=p("eigenvalues"), components=p("components"), sweeps=p("sweeps"), off_norm=p("off_norm")):
        return L.svae_pca_eigen(cov, D, G, eigenvalues, components, sweeps, off_norm, st)

    def project(x=xp, N=N, D=D, G=G, P=D, group=gp, count=p("count"), mean=p("mean"), components=p("components"), proj=p("proj")):
        return L.svae_pca_project(x, N, D, G, P, group, count, mean, components, proj, st)

    sizes = [dict(D=0), dict(D=65), dict(G=0), dict(G=1025), dict(D=64, G=16), dict(D=8, G=911)]
    points = [dict(N=0), dict(N=2 ** 31), dict(N=-1)]
    cases = [(moments, kw, E_INVALID) for kw in sizes + points]
    cases += [(moments, {k: None}, E_INVALID) for k in ("x", "count", "mean", "cov")]
    cases += [(moments, dict(group=None), E_INVALID)]                                   # a null group with G == 3
    cases += [(moments, {k: p(k) + 4}, E_INVALID) for k in ("count", "mean", "cov")]
    cases += [(moments, dict(ws=None), E_WORKSPACE), (moments, dict(ws=p("ws") + 128), E_WORKSPACE),
              (moments, dict(ws_bytes=run.ws_bytes - 1), E_WORKSPACE), (moments, dict(ws_bytes=0), E_WORKSPACE)]
    cases += [(eigen, kw, E_INVALID) for kw in sizes]
    cases += [(eigen, {k: None}, E_INVALID) for k in ("cov", "eigenvalues", "components", "sweeps", "off_norm")]
    cases += [(eigen, {k: p(k) + 4}, E_INVALID) for k in ("cov", "eigenvalues", "components", "off_norm")]
    cases += [(project, kw, E_INVALID) for kw in sizes + points + [dict(P=0), dict(P=D + 1), dict(P=-1)]]
    cases += [(project, {k: None}, E_INVALID) for k in ("x", "count", "mean", "components", "proj")]
    cases += [(project, dict(group=None), E_INVALID)]
    cases += [(project, {k: p(k) + 4}, E_INVALID) for k in ("count", "mean", "components", "proj")]
    for call, kw, status in cases:
        assert call(**kw) == status, (call.__name__, kw)
        assert L.svae_last_error(), (call.__name__, kw)
    assert run.untouched()
    assert L.svae_pca_workspace_bytes(N, 64, 16) == 0 and L.svae_pca_workspace_bytes(0, D, G) == 0
    assert moments() == 0 and eigen() == 0 and project() == 0                           # the same buffers, accepted as they stand
    got, want = run.read(), R.fixture_fit(*R.FIXTURES[8])
    assert np.array_equal(got["count"], want["count"]) and _scaled(got["proj"], want["proj"]) <= BOUND
