"""The eigenimage kernels (include/svae_eigen.h: svae_eig_project, svae_eig_accumulate, svae_eig_orthonormalise, svae_eig_gram,
svae_eig_rotate, svae_eig_coords; ops.EigenImages) on the MI355X against tests/eigen_ref.py, the float64 restatement of the
header: doubles within 1e-10 of the largest reference value of the array, the conventions for dead classes, dead columns and
images in no class exactly.  Every buffer the calls write sits inside guard bytes (decoder_abi.Guarded).  The side-stream and
graph-replay checks are the shared stream table's (tests/stream_cases_analysis.py), whose rows run the chain of CASES[1] and
CASES[7] and compare it through chain_errors below."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eigen_ref as R
from decoder_abi import GUARD_BYTE, Guarded

pytestmark = pytest.mark.gpu
E_INVALID = -1
BOUND = 1e-10
CHAIN = ("Q0", "T", "Y", "ssq", "Q1", "G", "lambda", "W", "eigenimages", "residual", "rot", "coords")


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _scaled(got, want):
    """The largest |got - want| over the largest |want| (1 where that is 0)."""
    top = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max() / (top if top > 0 else 1.0)) if want.size else 0.0


def _separated(lam):
    """(K, R) bool: the eigenvalue is at least 1e-4 of the class's largest away from both its neighbours."""
    K = lam.shape[0]
    gap, edge = np.abs(np.diff(lam, axis=1)), np.full((K, 1), np.inf)
    nearest = np.minimum(np.concatenate([edge, gap], 1), np.concatenate([gap, edge], 1))
    return nearest >= 1e-4 * lam[:, :1]


class Run(object):
    """One problem through ctypes alone: the inputs on the device, every output inside guard bytes.  chain() is one pass of the
    iteration from the start array and the Rayleigh-Ritz step: orthonormalise, project, accumulate (in `parts` calls),
    orthonormalise again (what a further pass would start from), gram, svae_pca_eigen, rotate, coords."""

    def __init__(self, aligned, cover, label, K, Rc, P, start=None, mean=None):
        from spatial_vae_amd import _lib
        self.L = _lib.lib()
        dev = _dev()
        self.B, self.N, self.C = aligned.shape
        self.K, self.R, self.P, self.D = K, Rc, P, self.N * self.C
        B, D = self.B, self.D
        self.aligned = torch.from_numpy(np.ascontiguousarray(aligned, np.float32)).to(dev)
        self.cover = None if cover is None else torch.from_numpy(np.ascontiguousarray(cover, np.uint8)).to(dev)
        self.label = torch.from_numpy(np.ascontiguousarray(label, np.int32)).to(dev)
        label64 = np.asarray(label, np.int64)
        self.mean_h = R.class_moments(aligned, cover, label64, K)[0] if mean is None else mean
        self.mean = torch.from_numpy(self.mean_h.reshape(K, D)).to(dev)
        self.members_h = np.array([(label64 == k).sum() for k in range(K)], np.int64)
        self.members = torch.from_numpy(self.members_h).to(dev)
        self.start = None if start is None else torch.from_numpy(np.ascontiguousarray(start, np.float64)).to(dev)
        f8 = np.float64
        self.bufs = {"Q0": (K * D * Rc * 8, f8, (K, D, Rc)), "T": (B * Rc * 8, f8, (B, Rc)), "Y": (K * D * Rc * 8, f8, (K, D, Rc)),
                     "ssq": (K * D * 8, f8, (K, D)), "Q1": (K * D * Rc * 8, f8, (K, D, Rc)), "G": (K * Rc * Rc * 8, f8, (K, Rc, Rc)),
                     "lambda": (K * Rc * 8, f8, (K, Rc)), "W": (K * Rc * Rc * 8, f8, (K, Rc, Rc)), "sweeps": (K * 4, np.int32, (K,)),
                     "off_norm": (K * 8, f8, (K,)), "eigenimages": (K * P * D * 8, f8, (K, P, D)), "residual": (K * P * 8, f8, (K, P)),
                     "rot": (K * P * Rc * 8, f8, (K, P, Rc)), "coords": (B * P * 8, f8, (B, P))}
        self.bufs = {k: (Guarded(n, dev), dt, shape) for k, (n, dt, shape) in self.bufs.items()}

    def ptr(self, name):
        return self.bufs[name][0].ptr

    def put(self, name, array):
        g, dt, shape = self.bufs[name]
        raw = torch.from_numpy(np.ascontiguousarray(array, dt).reshape(-1).view(np.uint8).copy()).to(_dev())
        g.buf[g.off:g.off + g.nbytes].copy_(raw)

    def zero(self, *names):
        for name in names:
            self.bufs[name][0].fill_byte(0)

    def _cover(self, lo=0):
        return None if self.cover is None else self.cover.data_ptr() + lo * self.N

    def orthonormalise(self, src, dst, st=None):
        return self.L.svae_eig_orthonormalise(src, self.K, self.D, self.R, self.ptr(dst), st or _stream())

    def project(self, Q="Q0", st=None):
        return self.L.svae_eig_project(self.aligned.data_ptr(), self._cover(), self.label.data_ptr(), self.mean.data_ptr(), self.ptr(Q),
                                       self.B, self.N, self.C, self.K, self.R, self.ptr("T"), st or _stream())

    def accumulate(self, lo=0, hi=None, ssq=True, st=None):
        hi = self.B if hi is None else hi
        return self.L.svae_eig_accumulate(self.aligned.data_ptr() + lo * self.D * 4, self._cover(lo), self.label.data_ptr() + lo * 4,
                                          self.mean.data_ptr(), self.ptr("T") + lo * self.R * 8, hi - lo, self.N, self.C, self.K, self.R,
                                          self.ptr("Y"), self.ptr("ssq") if ssq else None, st or _stream())

    def gram(self, st=None):
        return self.L.svae_eig_gram(self.ptr("Q0"), self.ptr("Y"), self.members.data_ptr(), self.K, self.D, self.R, self.ptr("G"),
                                    st or _stream())

    def eigen(self, st=None):
        from spatial_vae_amd import ops
        step = ops.LatentPCA.max_groups(self.R)
        for lo in range(0, self.K, step):
            g, RR, Rc = min(step, self.K - lo), self.R * self.R * 8, self.R * 8
            rc = self.L.svae_pca_eigen(self.ptr("G") + lo * RR, self.R, g, self.ptr("lambda") + lo * Rc, self.ptr("W") + lo * RR,
                                       self.ptr("sweeps") + lo * 4, self.ptr("off_norm") + lo * 8, st or _stream())
            if rc:
                return rc
        return 0

    def rotate(self, st=None):
        return self.L.svae_eig_rotate(self.ptr("Q0"), self.ptr("Y"), self.ptr("W"), self.ptr("lambda"), self.members.data_ptr(), self.K,
                                      self.D, self.R, self.P, self.ptr("eigenimages"), self.ptr("residual"), self.ptr("rot"),
                                      st or _stream())

    def coords(self, st=None):
        return self.L.svae_eig_coords(self.ptr("T"), self.label.data_ptr(), self.ptr("rot"), self.B, self.K, self.R, self.P,
                                      self.ptr("coords"), st or _stream())

    def chain(self, st=None, parts=1):
        """Everything but the zeroing of Y and ssq, which the caller does first (under graph capture: outside the graph)."""
        assert self.orthonormalise(self.start.data_ptr(), "Q0", st) == 0 and self.project("Q0", st) == 0
        cuts = [self.B * i // parts for i in range(parts + 1)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if hi > lo:
                assert self.accumulate(lo, hi, True, st) == 0
        assert self.orthonormalise(self.ptr("Y"), "Q1", st) == 0
        assert self.gram(st) == 0 and self.eigen(st) == 0 and self.rotate(st) == 0 and self.coords(st) == 0
        return self

    def read(self, names=CHAIN):
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
        torch.cuda.synchronize()
        for name, (g, dt, shape) in self.bufs.items():
            pay, intact = g.read()
            if not intact or not (pay == GUARD_BYTE).all():
                return False
        return True


@functools.lru_cache(maxsize=None)
def reference(case):
    """The reference of one chain, computed once and shared -- treat as read-only."""
    seed, B, rows, cols, C, K, Rc, P, covered = case
    aligned, cover, label = R.images(seed, B, rows, cols, C, K, covered)
    label64 = label.astype(np.int64)
    D = rows * cols * C
    start = R.start_array(seed + 100, K, D, Rc)
    mean, _ = R.class_moments(aligned, cover, label64, K)
    members = np.array([(label64 == k).sum() for k in range(K)], np.int64)
    want = {"Q0": R.orthonormalise(start)}
    want["T"] = R.project(aligned, cover, label64, mean, want["Q0"])
    want["Y"], want["ssq"] = np.zeros((K, D, Rc)), np.zeros((K, D))
    R.accumulate(aligned, cover, label64, mean, want["T"], want["Y"], want["ssq"])
    want["Q1"] = R.orthonormalise(want["Y"])
    want["G"] = R.gram(want["Q0"], want["Y"], members)
    want["lambda"], want["W"] = R.eigen(want["G"])
    want["eigenimages"], want["residual"], want["rot"] = R.rotate(want["Q0"], want["Y"], want["W"], want["lambda"], members, P)
    want["coords"] = R.coords(want["T"], label64, want["rot"])
    return (aligned, cover, label, start, members), want


def chain_errors(got, want, label, K, Rc, P):
    """({output of CHAIN: the largest error over the largest reference value}, the (K, R) mask of separated eigenvalues).  The
    vectors of svae_pca_eigen are comparable where their eigenvalue is at least 1e-4 of the largest away from both its
    neighbours (the gap tests/test_gpu_pca.py relies on): a class of rank below R has a null space whose basis is arbitrary, so
    W, eigenimages, residual, rot and coords are compared where _separated says so and every other output everywhere."""
    sep = _separated(want["lambda"])
    of_image = sep[np.clip(label, 0, K - 1)]
    masks = {"W": np.broadcast_to(sep[:, :, None], (K, Rc, Rc)), "eigenimages": np.broadcast_to(sep[:, :P, None], want["eigenimages"].shape),
             "residual": sep[:, :P], "rot": np.broadcast_to(sep[:, :P, None], (K, P, Rc)), "coords": of_image[:, :P]}
    errs = {key: _scaled(np.where(masks[key], got[key], 0.0), np.where(masks[key], want[key], 0.0)) if key in masks
            else _scaled(got[key], want[key]) for key in CHAIN}
    return errs, sep


def _run(case, parts=1, st=None):
    (aligned, cover, label, start, _), _ = reference(case)
    run = Run(aligned, cover, label, case[5], case[6], case[7], start)
    run.zero("Y", "ssq")
    return run.chain(st, parts)


# (seed, B, rows, cols, C, K, R, P, covered): D is 35, 105, 256 and 1023; R' is 1, 4, 16 and 64 (S = 256, 64, 16, 4 segments, some
# of them empty at D = 35); K = 3 and 5 have an empty and a one-member class, K = 5 a class of three members, and 37 images in
# one class are rank deficient for R = 64; D = 35 < R = 64 leaves dead columns in the start basis itself.
CASES = [(0, 37, 5, 7, 1, 1, 1, 1, True), (1, 37, 5, 7, 3, 3, 3, 2, True), (2, 37, 16, 16, 1, 5, 16, 5, True),
         (3, 37, 33, 31, 1, 3, 3, 3, False), (4, 37, 5, 7, 1, 5, 64, 8, True), (5, 1, 5, 7, 1, 1, 3, 3, True),
         (6, 37, 16, 16, 1, 1, 64, 4, False), (7, 37, 33, 31, 1, 5, 16, 4, True)]
IDS = ["B%d_%dx%dx%d_K%d_R%d_P%d_%s" % (c[1:8] + ("cover" if c[8] else "nullcover",)) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_pass_and_the_ritz_step_against_the_reference(case):
    """Every call of the chain on one fixture, each output within 1e-10 of the largest reference value of its array (the basis
    arrays hold unit vectors: 1e-10 absolute).  Exactly: the dead columns of both bases, the rows of T and coords of images in no
    class, and every output of a dead class, are +0."""
    (aligned, cover, label, start, members), want = reference(case)
    K, Rc, P = case[5:8]
    run = _run(case)
    got = run.read()
    errs, sep = chain_errors(got, want, label, K, Rc, P)    # what hangs on the other vectors: below, from the reference's W and lambda
    run.put("W", want["W"])
    run.put("lambda", want["lambda"])
    assert run.rotate() == 0 and run.coords() == 0
    fed = run.read(("eigenimages", "residual", "rot", "coords"))
    errs.update({key + " (reference W)": _scaled(fed[key], want[key]) for key in fed})
    print("%s: %d of %d vectors separated; %s" % (IDS[CASES.index(case)], int(sep[:, :P].sum()), K * P,
                                                  ", ".join("%s %.1e" % kv for kv in errs.items())))
    for key in ("Q0", "Q1"):
        assert np.array_equal(got[key].any(1), want[key].any(1)), key + ": other dead columns"
        assert not np.signbit(got[key][:, :, ~want[key].any((0, 1))]).any()
    outside = (label < 0) | (label >= K)
    assert _same_bytes(got["T"][outside], np.zeros((int(outside.sum()), Rc)))
    assert _same_bytes(got["coords"][outside], np.zeros((int(outside.sum()), P)))
    for k in np.flatnonzero(members < 2):
        for key in ("ssq", "Y", "G", "eigenimages", "residual", "rot"):
            assert _same_bytes(got[key][k], np.zeros_like(got[key][k])), (k, key)
    live = np.flatnonzero(members >= 2)
    dead_cols = ~want["Q0"].any(1)
    assert not got["G"][dead_cols[:, :, None] | dead_cols[:, None, :]].any()
    for key in errs:
        assert errs[key] <= BOUND, (key, errs[key])
    if live.size:
        assert np.abs(got["G"] - got["G"].transpose(0, 2, 1)).max() == 0.0
        v = got["eigenimages"][live]
        at = np.abs(v).argmax(2)
        lead = np.take_along_axis(v, at[:, :, None], 2)[:, :, 0]
        assert (lead >= 0).all(), "sign rule"


def test_a_split_minibatch_and_repeated_calls_are_bit_equal():
    """One accumulate call equals two and three calls on the parts of the minibatch, and the whole chain again into fresh
    buffers: every output bit for bit."""
    case = CASES[2]
    first = _run(case).read()
    for parts in (2, 3):
        other = _run(case, parts).read()
        for key in CHAIN:
            assert _same_bytes(first[key], other[key]), (parts, key)
    again = _run(case).read()
    for key in CHAIN:
        assert _same_bytes(first[key], again[key]), ("repeated", key)


def test_later_passes_leave_the_squares_alone_and_fewer_components_are_a_prefix():
    """ssq NULL: Y as before, ssq untouched.  P < R: eigenimages, residual, rot and coords are the leading rows and columns of the
    P == R result, bit for bit."""
    case = CASES[2]
    (aligned, cover, label, start, _), _ = reference(case)
    K, Rc = case[5], case[6]
    full = Run(aligned, cover, label, K, Rc, Rc, start)
    full.zero("Y", "ssq")
    full = full.chain().read()
    part = _run(case).read()
    P = case[7]
    assert _same_bytes(part["eigenimages"], full["eigenimages"][:, :P]) and _same_bytes(part["residual"], full["residual"][:, :P])
    assert _same_bytes(part["rot"], full["rot"][:, :P]) and _same_bytes(part["coords"], full["coords"][:, :P])
    run = Run(aligned, cover, label, K, Rc, P, start)
    run.zero("Y")
    assert run.orthonormalise(run.start.data_ptr(), "Q0") == 0 and run.project() == 0 and run.accumulate(ssq=False) == 0
    got = run.read(("Y", "ssq"))
    assert _same_bytes(got["Y"], part["Y"]) and (got["ssq"].view(np.uint8) == GUARD_BYTE).all()


def test_a_non_finite_pixel_stays_in_its_own_class():
    """One NaN and one inf pixel in two members of class 1 (K = 5): class 1's ssq entries there and its Y at the indices the
    image covers are non-finite, every other
    class's T rows, Y, ssq, G, eigenimages and coords are bit-equal to the run without them."""
    case = CASES[2]
    (aligned, cover, label, start, _), _ = reference(case)
    clean = _run(case).read()
    mean = R.class_moments(aligned, cover, label.astype(np.int64), case[5])[0]
    bad = aligned.copy()
    mine = np.flatnonzero(label == 1)
    spots = [(mine[0], int(np.flatnonzero(cover[mine[0]])[3])), (mine[4], int(np.flatnonzero(cover[mine[4]])[11]))]
    bad[spots[0][0], spots[0][1], 0] = np.nan
    bad[spots[1][0], spots[1][1], 0] = np.inf
    run = Run(bad, cover, label, case[5], case[6], case[7], start, mean=mean)
    run.zero("Y", "ssq")
    got = run.chain().read()
    assert not np.isfinite(got["Y"][1][cover[spots[0][0]] != 0]).any() and not np.isfinite(got["ssq"][1][[s[1] for s in spots]]).any()
    assert not np.isfinite(got["T"][[s[0] for s in spots]]).any()
    others = np.array([k for k in range(case[5]) if k != 1])
    for key in ("Y", "ssq", "Q1", "G", "lambda", "eigenimages", "residual", "rot"):
        assert _same_bytes(got[key][others], clean[key][others]), key
    assert _same_bytes(got["T"][label != 1], clean["T"][label != 1]) and _same_bytes(got["coords"][label != 1], clean["coords"][label != 1])


def test_the_wrapper_makes_the_same_calls():
    """ops.EigenImages over three passes in minibatches of 10 against eigen_ref.fit: every array within the bound, members
    exactly; and its first pass is the chain of ctypes calls above, bit for bit."""
    from spatial_vae_amd import ops
    case = CASES[2]
    (aligned, cover, label, start, members), _ = reference(case)
    K, Rc, P = case[5:8]
    B, N, C = aligned.shape
    dev = _dev()
    want = R.fit(aligned, cover, label, K, Rc, P, 3, start, batch=10)
    a, c, l = torch.from_numpy(aligned).to(dev), torch.from_numpy(cover).to(dev), torch.from_numpy(label).to(dev)
    mean = torch.from_numpy(want["mean"]).to(dev)
    eig = ops.EigenImages(K, N, C, Rc, dev)
    eig.start(torch.from_numpy(start).to(dev))
    for it in range(3):
        if it:
            eig.end_pass()
        eig.begin_pass()
        for lo in range(0, B, 10):
            eig.update(a[lo:lo + 10], c[lo:lo + 10], l[lo:lo + 10], mean)
        if it == 0:
            chain = _run(case).read(("Y", "ssq"))
            assert _same_bytes(eig.Y.cpu().numpy(), chain["Y"]) and _same_bytes(eig.ssq.cpu().numpy(), chain["ssq"])
    fit = eig.finish(P)
    assert np.array_equal(fit.members.cpu().numpy(), members)
    sep = _separated(want["lambda"])[:, :P]                  # as in the chain's test: the null space of class 0 has no fixed basis
    masks = {"eigenimages": sep[:, :, None], "residual": sep, "coords": sep[np.clip(label, 0, K - 1)]}
    pairs = {"ssq": fit.ssq, "lambda": fit.eigenvalues, "eigenimages": fit.eigenimages, "residual": fit.residual, "coords": fit.coords}
    errs = {k: _scaled(np.where(masks.get(k, True), v.cpu().numpy(), 0.0), np.where(masks.get(k, True), want[k], 0.0))
            for k, v in pairs.items()}
    print("wrapper, three passes: %s" % ", ".join("%s %.1e" % kv for kv in errs.items()))
    assert max(errs.values()) <= BOUND
    with pytest.raises(RuntimeError):
        ops.EigenImages(K, N, C, 65, dev)
    with pytest.raises(RuntimeError):
        ops.EigenImages(K, N, C, Rc, "cpu")


def test_every_refusal_leaves_the_buffers_untouched():
    """Every SVAE_E_INVALID case of the header, one call each: the status, a message in svae_last_error, and afterwards every
    output still holds its fill bytes inside intact guards."""
    case = CASES[1]
    (aligned, cover, label, start, _), want = reference(case)
    K, Rc, P = case[5:8]
    run = Run(aligned, cover, label, K, Rc, P, start)
    L, p, st = run.L, run.ptr, _stream()
    B, N, C, D = run.B, run.N, run.C, run.D
    a, cv, lb, mu, mem, s0 = (run.aligned.data_ptr(), run.cover.data_ptr(), run.label.data_ptr(), run.mean.data_ptr(),
                              run.members.data_ptr(), run.start.data_ptr())

    def project(aligned=a, cover=cv, label=lb, mean=mu, Q=p("Q0"), B=B, N=N, C=C, K=K, R=Rc, T=p("T")):
        return L.svae_eig_project(aligned, cover, label, mean, Q, B, N, C, K, R, T, st)

    def accumulate(aligned=a, cover=cv, label=lb, mean=mu, T=p("T"), B=B, N=N, C=C, K=K, R=Rc, Y=p("Y"), ssq=p("ssq")):
        return L.svae_eig_accumulate(aligned, cover, label, mean, T, B, N, C, K, R, Y, ssq, st)

    def orthonormalise(Y=s0, K=K, D=D, R=Rc, Q=p("Q0")):
        return L.svae_eig_orthonormalise(Y, K, D, R, Q, st)

    def gram(Q=p("Q0"), Y=p("Y"), members=mem, K=K, D=D, R=Rc, G=p("G")):
        return L.svae_eig_gram(Q, Y, members, K, D, R, G, st)

    def rotate(Q=p("Q0"), Y=p("Y"), W=p("W"), lam=p("lambda"), members=mem, K=K, D=D, R=Rc, P=P, eigenimages=p("eigenimages"),
               residual=p("residual"), rot=p("rot")):
        return L.svae_eig_rotate(Q, Y, W, lam, members, K, D, R, P, eigenimages, residual, rot, st)

    def coords(T=p("T"), label=lb, rot=p("rot"), B=B, K=K, R=Rc, P=P, coords=p("coords")):
        return L.svae_eig_coords(T, label, rot, B, K, R, P, coords, st)

    basis = [dict(K=0), dict(K=4097), dict(R=0), dict(R=65), dict(K=4096, R=64, D=1025)]
    image_sizes = [dict(B=0), dict(N=0), dict(C=0), dict(C=5), dict(B=2 ** 29, N=4, C=1), dict(K=0), dict(K=4097), dict(R=0), dict(R=65),
                   dict(K=4096, R=64, N=1025, C=1)]
    cases = [(project, kw) for kw in image_sizes] + [(accumulate, kw) for kw in image_sizes]
    cases += [(project, {k: None}) for k in ("aligned", "label", "mean", "Q", "T")]
    cases += [(project, {k: v + 4}) for k, v in (("mean", mu), ("Q", p("Q0")), ("T", p("T")))]
    cases += [(project, dict(T=p("Q0"))), (project, dict(T=mu))]
    cases += [(accumulate, {k: None}) for k in ("aligned", "label", "mean", "T", "Y")]
    cases += [(accumulate, {k: v + 4}) for k, v in (("mean", mu), ("T", p("T")), ("Y", p("Y")), ("ssq", p("ssq")))]
    cases += [(accumulate, dict(Y=p("T"))), (accumulate, dict(ssq=p("Y"))), (accumulate, dict(ssq=mu))]
    cases += [(orthonormalise, kw) for kw in basis + [dict(D=0)]]
    cases += [(orthonormalise, dict(Y=None)), (orthonormalise, dict(Q=None)), (orthonormalise, dict(Y=s0 + 4)),
              (orthonormalise, dict(Q=p("Q0") + 4)), (orthonormalise, dict(Y=p("Q0"))), (orthonormalise, dict(Y=p("Q0") + 8))]
    cases += [(gram, kw) for kw in basis + [dict(D=0)]]
    cases += [(gram, {k: None}) for k in ("Q", "Y", "members", "G")]
    cases += [(gram, {k: v + 4}) for k, v in (("Q", p("Q0")), ("Y", p("Y")), ("members", mem), ("G", p("G")))]
    cases += [(gram, dict(G=p("Y")))]
    cases += [(rotate, kw) for kw in basis + [dict(D=0), dict(P=0), dict(P=Rc + 1)]]
    cases += [(rotate, {k: None}) for k in ("Q", "Y", "W", "lam", "members", "eigenimages", "residual", "rot")]
    cases += [(rotate, {k: v + 4}) for k, v in (("Q", p("Q0")), ("W", p("W")), ("lam", p("lambda")), ("eigenimages", p("eigenimages")),
                                                ("residual", p("residual")), ("rot", p("rot")))]
    cases += [(rotate, dict(eigenimages=p("Y"))), (rotate, dict(rot=p("W"))), (rotate, dict(residual=p("lambda"))),
              (rotate, dict(rot=p("eigenimages")))]
    cases += [(coords, kw) for kw in (dict(B=0), dict(K=0), dict(K=4097), dict(R=0), dict(R=65), dict(P=0), dict(P=Rc + 1))]
    cases += [(coords, {k: None}) for k in ("T", "label", "rot", "coords")]
    cases += [(coords, {k: v + 4}) for k, v in (("T", p("T")), ("rot", p("rot")), ("coords", p("coords")))]
    cases += [(coords, dict(coords=p("T")))]
    for call, kw in cases:
        assert call(**kw) == E_INVALID, (call.__name__, kw)
        assert L.svae_last_error(), (call.__name__, kw)
    assert run.untouched()
    run.zero("Y", "ssq")                                                                # the same buffers, accepted as they stand
    got = run.chain().read()
    for key in CHAIN:
        assert _scaled(got[key], want[key]) <= BOUND, key
