"""The k-means kernels (include/svae_cluster.h: svae_kmeans_seed, svae_kmeans_step; ops.KMeans, elbo.cluster_latents) on the
MI355X against tests/kmeans_ref.py, the float64 restatement of the header's order of operations: labels, members and counts
exactly equal, centres and inertia BIT-equal after every step.  Every buffer the calls write sits inside guard bytes
(decoder_abi.Guarded) and the workspace is exactly svae_kmeans_workspace_bytes long."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kmeans_ref as K
from decoder_abi import GUARD_BYTE, Guarded

pytestmark = pytest.mark.gpu
E_INVALID, E_WORKSPACE = -1, -2


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


class Run(object):
    """One clustering problem through ctypes alone: x on the device, every output inside guard bytes."""

    def __init__(self, x, k):
        from spatial_vae_amd import _lib
        self.L = _lib.lib()
        self.x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(_dev())
        self.N, self.D, self.k = x.shape[0], x.shape[1], k
        self.ws_bytes = self.L.svae_kmeans_workspace_bytes(self.N, self.D, k)
        assert self.ws_bytes > 0
        dev = _dev()
        self.bufs = {"centres": (Guarded(k * self.D * 8, dev), np.float64, (k, self.D)), "label": (Guarded(self.N * 4, dev), np.int32, (self.N,)),
                     "members": (Guarded(k * 8, dev), np.int64, (k,)), "rec": (Guarded(48, dev), np.int64, (6,)),
                     "seed_index": (Guarded(k * 4, dev), np.int32, (k,)), "ws": (Guarded(self.ws_bytes, dev), np.uint8, (self.ws_bytes,))}
        self.bufs["rec"][0].fill_byte(0)           # all zero bytes = a fresh record

    def ptr(self, name):
        return self.bufs[name][0].ptr

    def put(self, name, array):
        g, dt, shape = self.bufs[name]
        raw = torch.from_numpy(np.ascontiguousarray(array, dt).reshape(-1).view(np.uint8).copy()).to(_dev())
        g.buf[g.off:g.off + g.nbytes].copy_(raw)

    def seed(self, u):
        self.u = torch.from_numpy(np.ascontiguousarray(u, np.float64)).to(_dev())
        return self.L.svae_kmeans_seed(self.x.data_ptr(), self.N, self.D, self.k, self.u.data_ptr(), self.ptr("centres"), self.ptr("seed_index"),
                                       self.ptr("ws"), self.ws_bytes, _stream())

    def step(self, update=1):
        return self.L.svae_kmeans_step(self.x.data_ptr(), self.N, self.D, self.k, update, self.ptr("centres"), self.ptr("label"),
                                       self.ptr("members"), self.ptr("rec"), self.ptr("ws"), self.ws_bytes, _stream())

    def read(self):
        """Every buffer as numpy, the record's fields by name; asserts the guard bytes are intact."""
        torch.cuda.synchronize()
        out = {}
        for name, (g, dt, shape) in self.bufs.items():
            pay, intact = g.read()
            assert intact, "written outside " + name
            out[name] = pay.view(dt).reshape(shape).copy()
        rec = out["rec"]
        out.update(iterations=int(rec[0]), changed=int(rec[1]), converged_at=int(rec[2]), assigned=int(rec[3]), empty=int(rec[4]),
                   inertia=float(rec[5:6].view(np.float64)[0]))
        return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_step(got, want, what):
    """labels, members and the counts exactly equal, centres and inertia bit-equal."""
    assert np.array_equal(got["label"], want["label"]), (what, "label", int((got["label"] != want["label"]).sum()))
    assert np.array_equal(got["members"], want["members"]), (what, "members")
    for key in ("changed", "assigned", "empty", "iterations"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert np.array_equal(_bits(got["centres"]), _bits(want["centres"])), (what, "centres", np.abs(got["centres"] - want["centres"]).max())
    assert _bits(got["inertia"]) == _bits(want["inertia"]), (what, "inertia", got["inertia"], want["inertia"])


def _min_gap(x, centres):
    """The smallest relative gap between the best and the second-best distance."""
    d = np.sort(K.d2(x, centres), 1)
    return float(((d[:, 1] - d[:, 0]) / d[:, 1]).min()) if centres.shape[0] > 1 else 1.0


BLOBS = [(0, 1000, 3, 5, 8), (1, 4097, 1, 2, 8), (2, 300, 8, 17, 8), (3, 257, 2, 3, 8), (4, 262145, 2, 3, 12), (5, 2048, 64, 1024, 3),
         (6, 300, 4, 3, 3), (7, 300, 5, 3, 3), (8, 300, 16, 3, 3), (9, 300, 17, 3, 3)]


@pytest.mark.parametrize("seed,N,D,k,steps", BLOBS, ids=["N%d_D%d_k%d" % c[1:4] for c in BLOBS])
def test_seed_and_every_step_equal_the_reference(seed, N, D, k, steps):
    """Blobs (kmeans_ref.blobs): the seeding's picks and centres, then `steps` update steps and one assign-only step, each held
    to the reference.  (4097, 1, 2) has 17 chunks, the last of one point; (262145, 2, 3) doubles the chunk to 512; (2048, 64,
    1024) walks the centres in 16 slabs of 64; D = 4, 5, 16, 17 sit on either side of the 4 / 16 / 64 register bounds, in two
    chunks, the second of 44 points.  MI355X: holds, bit for bit, in every shape."""
    x, u = K.blobs(seed, N, D, k)
    run = Run(x, k)
    assert run.seed(u) == 0
    got = run.read()
    index, centres, _ = K.seed(x, k, u)
    assert np.array_equal(got["seed_index"], index)
    assert np.array_equal(_bits(got["centres"]), _bits(x[index].astype(np.float64))) and np.array_equal(_bits(centres), _bits(got["centres"]))
    label, it, converged, gap = None, 0, 0, 1.0
    for i, update in enumerate([1] * steps + [0]):
        gap = min(gap, _min_gap(x, centres)) if N * k <= 10 ** 6 else gap
        want = K.step(x, centres, label, it, bool(update))
        assert run.step(update) == 0
        got = run.read()
        _assert_step(got, want, "step %d (update %d)" % (i, update))
        centres, label, it = want["centres"], want["label"], want["iterations"]
        if update and not converged and want["changed"] == 0:
            converged = it
        assert got["converged_at"] == converged
    print("N %d D %d k %d: converged_at %d, inertia %.6g, smallest relative best/second gap %.2e" % (N, D, k, converged, want["inertia"], gap))
    assert got["iterations"] == steps and (got["label"] >= 0).all() and got["members"].sum() == N


def test_ties_go_to_the_lower_index_and_the_higher_stays_empty():
    """Explicit initial centres with two identical rows: every tie goes to row 1 and row 3 keeps no member and its coordinates."""
    x, _ = K.blobs(7, 600, 3, 4)
    centres = x[[5, 100, 300, 100]].astype(np.float64)
    run = Run(x, 4)
    run.put("centres", centres)
    assert run.step(1) == 0
    got = run.read()
    _assert_step(got, K.step(x, centres, None, 0), "tied centres")
    assert got["members"][3] == 0 and got["members"][1] > 0 and got["empty"] == 1 and not (got["label"] == 3).any()
    assert np.array_equal(_bits(got["centres"][3]), _bits(centres[3]))


def test_a_far_away_centre_stays_empty_and_bit_unchanged():
    x, _ = K.blobs(8, 500, 2, 3)
    centres = np.concatenate([x[[1, 2]].astype(np.float64), [[1e6 + 0.1, -1e6 / 3]]])
    run = Run(x, 3)
    run.put("centres", centres)
    for i in range(2):
        assert run.step(1) == 0
    got = run.read()
    assert got["empty"] == 1 and got["members"][2] == 0 and np.array_equal(_bits(got["centres"][2]), _bits(centres[2]))
    assert not np.array_equal(got["centres"][:2], centres[:2])


def test_non_finite_points_are_unassigned():
    """Three points carrying NaN, +inf and -inf: label -1, out of `assigned`, the members and every sum."""
    x, _ = K.blobs(9, 700, 3, 4)
    x[3, 1], x[300, 0], x[699, 2] = np.nan, np.inf, -np.inf
    centres = x[[0, 10, 20, 30]].astype(np.float64)
    run = Run(x, 4)
    run.put("centres", centres)
    label, it = None, 0
    for i in range(3):
        want = K.step(x, centres, label, it)
        assert run.step(1) == 0
        got = run.read()
        _assert_step(got, want, "step %d" % i)
        centres, label, it = want["centres"], want["label"], want["iterations"]
    assert got["label"][[3, 300, 699]].tolist() == [-1, -1, -1] and got["assigned"] == 697 and got["members"].sum() == 697
    assert np.isfinite(got["centres"]).all() and np.isfinite(got["inertia"])


def test_steps_after_convergence_change_nothing_and_update_0_leaves_the_centres():
    x, u = K.blobs(0, 1000, 3, 5)
    run = Run(x, 5)
    assert run.seed(u) == 0
    for _ in range(40):
        assert run.step(1) == 0
    a = run.read()
    assert 0 < a["converged_at"] < 40 and a["changed"] == 0 and a["iterations"] == 40
    for _ in range(3):
        assert run.step(1) == 0
    b = run.read()
    assert b["iterations"] == 43 and b["converged_at"] == a["converged_at"]
    for key in ("centres", "label", "members", "seed_index"):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
    assert np.array_equal(a["rec"][1:], b["rec"][1:])
    assert run.step(0) == 0
    c = run.read()
    assert c["iterations"] == 43 and np.array_equal(_bits(c["centres"]), _bits(b["centres"])) and np.array_equal(c["rec"], b["rec"])
    assert np.array_equal(c["label"], K.assign(x, c["centres"])[0])


def test_update_0_on_a_fresh_record():
    """The first call may be the labelling call: incoming labels are ignored, centres and the count stay."""
    x, _ = K.blobs(11, 300, 2, 3)
    centres = x[[0, 1, 2]].astype(np.float64)
    run = Run(x, 3)
    run.put("centres", centres)
    assert run.step(0) == 0
    got = run.read()
    _assert_step(got, K.step(x, centres, None, 0, update=False), "assign only")
    assert got["iterations"] == 0 and got["converged_at"] == 0 and got["changed"] == 300


# ---------------------------------------------------------------- seeding
@pytest.mark.parametrize("seed,N,D,k", [(0, 1000, 3, 5), (1, 4097, 1, 2), (2, 300, 8, 17), (4, 262145, 2, 3)])
def test_seeding_picks_are_valid_under_the_flat_prefix_sums(seed, N, D, k):
    """seed_index[0] is min(floor(u0 N), N - 1); centres[j] is x[seed_index[j]] widened, exactly; every later pick i has m_i > 0
    and cs[i-1] - s <= u_j T <= cs[i] + s, cs the in-order cumulative sum of m in ONE level and s = N 2^-52 T the worst-case
    bound of a length-N double sum; two runs are bit-equal."""
    x, u = K.blobs(seed, N, D, k)
    run = Run(x, k)
    assert run.seed(u) == 0
    got = run.read()
    assert got["seed_index"][0] == min(int(np.floor(u[0] * N)), N - 1)
    assert np.array_equal(_bits(got["centres"]), _bits(x[got["seed_index"]].astype(np.float64)))
    _, _, rounds = K.seed(x, k, u)
    for j in range(1, k):
        m, T = rounds[j]
        i = int(got["seed_index"][j])
        cs = np.cumsum(m)
        s = N * 2.0 ** -52 * T
        assert m[i] > 0 and (cs[i - 1] if i else 0.0) - s <= u[j] * T <= cs[i] + s, (j, i)
    again = Run(x, k)
    assert again.seed(u) == 0
    other = again.read()
    assert np.array_equal(other["seed_index"], got["seed_index"]) and np.array_equal(_bits(other["centres"]), _bits(got["centres"]))


def test_seeding_coincident_points_take_the_fallback_index():
    x = np.full((600, 3), 0.25, np.float32)
    u = np.array([0.5, 0.25, 0.999, 0.0])
    run = Run(x, 4)
    assert run.seed(u) == 0
    got = run.read()
    assert got["seed_index"].tolist() == [300, 150, 599, 0] and (got["centres"] == 0.25).all()


# ---------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_buffers_untouched():
    """Every SVAE_E_INVALID case of the header, and the workspace refusals: the status, a message, and every output still the
    fill bytes inside intact guards."""
    from spatial_vae_amd import _lib
    x, u = K.blobs(0, 300, 3, 5)
    run = Run(x, 5)
    run.u = torch.from_numpy(u).to(_dev())
    for name, (g, _, _) in run.bufs.items():
        g.fill_byte(GUARD_BYTE)
    L, X, U, st = run.L, run.x.data_ptr(), run.u.data_ptr(), _stream()
    p = run.ptr
    ws, wb = p("ws"), run.ws_bytes

    def seed(x=X, N=300, D=3, k=5, u=U, centres=p("centres"), index=p("seed_index"), ws=ws, wb=wb):
        return L.svae_kmeans_seed(x, N, D, k, u, centres, index, ws, wb, st)

    def step(x=X, N=300, D=3, k=5, centres=p("centres"), label=p("label"), members=p("members"), rec=p("rec"), ws=ws, wb=wb):
        return L.svae_kmeans_step(x, N, D, k, 1, centres, label, members, rec, ws, wb, st)

    assert L.svae_kmeans_workspace_bytes(2 ** 31, 3, 5) == 0
    invalid = [seed(D=0), seed(D=65), seed(k=0), seed(k=1025), seed(N=4), seed(N=2 ** 31), seed(x=None), seed(u=None), seed(centres=None),
               seed(index=None), seed(u=U + 4), seed(centres=p("centres") + 4),
               step(D=0), step(D=65), step(k=0), step(k=1025), step(N=4), step(N=2 ** 31), step(x=None), step(centres=None), step(label=None),
               step(members=None), step(rec=None), step(centres=p("centres") + 4), step(members=p("members") + 4), step(rec=p("rec") + 4)]
    assert invalid == [E_INVALID] * len(invalid), invalid
    assert b"svae_kmeans_step" in L.svae_last_error()
    workspace = [seed(ws=None), seed(ws=ws + 8), seed(wb=wb - 1), step(ws=None), step(ws=ws + 8), step(wb=wb - 1)]
    assert workspace == [E_WORKSPACE] * len(workspace), workspace
    torch.cuda.synchronize()
    for name, (g, _, _) in run.bufs.items():
        pay, intact = g.read()
        assert intact and (pay == GUARD_BYTE).all(), name
    assert seed() == 0 and step() == 0              # the same buffers are fine with valid arguments
    run.read()


def test_ops_refuses_shape_and_dtype_mistakes():
    from spatial_vae_amd import ops
    dev = _dev()
    km = ops.KMeans(3, 2, dev)
    good = torch.zeros(10, 2, device=dev)
    for points, u in [(torch.zeros(10, 2), np.zeros(3)), (good.double(), np.zeros(3)), (torch.zeros(10, 3, device=dev), np.zeros(3)),
                      (torch.zeros(2, 10, device=dev).t(), np.zeros(3)), (good[:2], np.zeros(3)), (good, np.zeros(4)),
                      (good, torch.zeros(3))]:
        with pytest.raises(RuntimeError):
            km.fit(points, 2, u)
    for k, D, device in [(0, 2, dev), (1025, 2, dev), (3, 65, dev), (3, 2, "cpu")]:
        with pytest.raises(RuntimeError):
            ops.KMeans(k, D, device)


# ---------------------------------------------------------------- the host side: ops.KMeans.fit and elbo.cluster_latents
def test_restarts_pick_the_lowest_inertia_on_the_device():
    """elbo.cluster_latents with three restarts: every restart's inertia is the reference's from that restart's uniforms, bit for
    bit; chosen_restart is their argmin and the tensors returned are that run's."""
    from spatial_vae_amd import elbo as E
    from spatial_vae_amd import ops
    x, _ = K.blobs(12, 900, 4, 6)
    k, iters, R = 6, 10, 3
    gen = torch.Generator()
    gen.manual_seed(21)
    out = E.cluster_latents(torch.from_numpy(x).to(_dev()), k, iters, R, gen)
    gen.manual_seed(21)
    uniforms = torch.rand(R, k, dtype=torch.float64, generator=gen).numpy()
    refs = [K.fit(x, k, uniforms[r], iters) for r in range(R)]
    inertia = out["restart_inertia"].cpu().numpy()
    assert np.array_equal(_bits(inertia), _bits(np.array([r["inertia"] for r in refs])))
    chosen = int(out["chosen_restart"].item())
    assert chosen == int(np.argmin(inertia)) and len(set(inertia.tolist())) > 1
    want = refs[chosen]
    assert np.array_equal(out["label"].cpu().numpy(), want["label"]) and out["label"].dtype == torch.int32
    assert np.array_equal(_bits(out["centres"].cpu().numpy()), _bits(want["centres"]))
    assert np.array_equal(out["members"].cpu().numpy(), want["members"]) and np.array_equal(out["seed_index"].cpu().numpy(), want["seed_index"])
    rec = ops.KMeans.read_record(out["record"])
    assert rec["iterations"] == iters and rec["converged_at"] == want["converged_at"] and rec["inertia"] == want["inertia"]
