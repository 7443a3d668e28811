"""The neighbour kernels (include/svae_neighbours.h) on the MI355X, through ctypes alone, against the float64 restatement
tests/neighbours_ref.py: the lists bit for bit (only subtraction, multiplication and addition are involved), whatever the split
of candidates and queries into calls; the averages within one float32 of the reference's single division, their support bit
for bit.  Every buffer the calls write sits inside guard bytes (decoder_abi.Guarded).  The side-stream and graph-replay checks
are the shared stream table's (tests/stream_cases_analysis.py), whose row runs search_case("300x7_K64") and
average_case("40x105x3_T257"), each with a second seed for its other input set."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import neighbours_ref as R
from decoder_abi import GUARD_BYTE, Guarded

pytestmark = pytest.mark.gpu
E_INVALID = -1


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _lib():
    from spatial_vae_amd import _lib
    return _lib.lib()


def _view(g, dtype):
    """The payload of a Guarded as a torch view of `dtype`."""
    return g.buf[g.off:g.off + g.nbytes].view(dtype)


def _read(g, dtype, shape):
    pay, intact = g.read()
    assert intact, "guard bytes overwritten"
    return pay.view(dtype).reshape(shape)


# ---------------------------------------------------------------- the search
class Search(object):
    """The latents of `images` images on the device and their running lists inside guard bytes."""

    def __init__(self, latents, K):
        self.L, self.K = _lib(), K
        self.images, self.D = latents.shape
        self.z = torch.from_numpy(np.array(latents, np.float64)).to(_dev())
        self.d2, self.index = Guarded(self.images * K * 8, _dev()), Guarded(self.images * K * 8, _dev())
        self.refill()

    def refill(self):
        _view(self.d2, torch.float64).fill_(float("inf"))
        _view(self.index, torch.int64).fill_(-1)

    def call(self, qlo, qhi, lo, hi, st=None):
        return self.L.svae_nbr_search(self.z.data_ptr() + qlo * self.D * 8, qhi - qlo, qlo, self.z.data_ptr() + lo * self.D * 8, hi - lo, lo,
                                      self.D, self.K, self.d2.ptr + qlo * self.K * 8, self.index.ptr + qlo * self.K * 8, st or _stream())

    def run(self, chunks=None, query_chunks=None, st=None):
        for qlo, qhi in query_chunks or [(0, self.images)]:
            for lo, hi in chunks or [(0, self.images)]:
                assert self.call(qlo, qhi, lo, hi, st) == 0, self.L.svae_last_error()
        return self

    def read(self):
        torch.cuda.synchronize()
        return _read(self.d2, np.float64, (self.images, self.K)), _read(self.index, np.int64, (self.images, self.K))


SEARCH = ["lattice", "300x7_K64", "70x1_K1", "40x33_K256", "1000x3_K100_duplicates"]


@functools.lru_cache(maxsize=None)
def search_case(name, seed=0):
    """(latents, K, reference d2, reference index): the reference is the full sort, made once.  The tests here use seed 0."""
    rs = np.random.RandomState(SEARCH.index(name) + 10 + 100 * seed)
    if name == "lattice":
        z, K = R.lattice(), 5
    elif name == "300x7_K64":
        z, K = rs.randn(300, 7), 64
    elif name == "70x1_K1":
        z, K = rs.randn(70, 1), 1
    elif name == "40x33_K256":
        z, K = rs.randn(40, 33), 256
    else:
        z, K = rs.rand(1000, 3), 100
        z[rs.choice(500, 20, replace=False) + 500] = z[rs.choice(500, 20, replace=False)]      # 20 exact duplicates
    want_d, want_i = R.brute_force(z, K)
    for a in (z, want_d, want_i):
        a.setflags(write=False)
    return z, K, want_d, want_i


@pytest.mark.parametrize("name", SEARCH)
def test_search_is_bit_equal_to_the_full_sort_however_the_calls_are_split(name):
    """One call over all candidates gives best_d2 and best_index bit-equal to the reference's full sort of (d2, index); so do the
    candidates split at 64 / 70 / rest and offered in a shuffled order, and the queries split in three.  (40, 33, 256) leaves 39
    entries and then empty slots (+inf, -1); the duplicates of (1000, 3, 100) sit at distance +0 in index order."""
    z, K, want_d, want_i = search_case(name)
    images = z.shape[0]
    got_d, got_i = Search(z, K).run().read()
    assert _same_bytes(got_i, want_i) and _same_bytes(got_d, want_d), "one call"
    cuts = [c for c in (64, 70) if c < images]
    chunks = list(zip([0] + cuts, cuts + [images]))
    for order in (chunks[::-1], chunks[1:] + chunks[:1]):
        got_d, got_i = Search(z, K).run(order).read()
        assert _same_bytes(got_i, want_i) and _same_bytes(got_d, want_d), ("candidates", order)
    a, b = images // 3, images // 3 + 1
    got_d, got_i = Search(z, K).run(query_chunks=[(b, images), (0, a), (a, b)]).read()
    assert _same_bytes(got_i, want_i) and _same_bytes(got_d, want_d), "queries"
    if name == "40x33_K256":
        assert ((got_i >= 0).sum(1) == 39).all() and (got_i[:, 39:] == -1).all() and np.isposinf(got_d[:, 39:]).all()
    if name == "1000x3_K100_duplicates":
        assert (got_d[:, 0] == 0).sum() == 40
    if name == "lattice":
        assert R.ties_at_cut(z, K)[1].sum() * 2 >= images


def test_non_finite_latents_list_nothing_and_are_listed_by_nobody():
    """A NaN and an inf latent in two images: their lists stay empty, no list names them, and every other row is bit-equal to
    the run that never offers them as candidates."""
    z, K, _, _ = search_case("300x7_K64")
    bad = z.copy()
    bad[17, 3], bad[101, 0] = np.nan, np.inf
    got_d, got_i = Search(bad, K).run().read()
    assert (got_i[[17, 101]] == -1).all() and np.isposinf(got_d[[17, 101]]).all()
    assert not np.isin(got_i, [17, 101]).any()
    clean_d, clean_i = Search(bad, K).run([(0, 17), (18, 101), (102, 300)]).read()
    others = np.array([b for b in range(300) if b not in (17, 101)])
    assert _same_bytes(got_i[others], clean_i[others]) and _same_bytes(got_d[others], clean_d[others])
    want_d, want_i = R.search_all(bad, K)
    assert _same_bytes(got_i, want_i) and _same_bytes(got_d, want_d)


# ---------------------------------------------------------------- the average
class Average(object):
    """One svae_nbr_average problem: the inputs on the device, average and support inside guard bytes."""

    def __init__(self, stack, cover, index, weight):
        self.L = _lib()
        dev = _dev()
        self.images, self.N, self.C = stack.shape
        self.B, self.T = index.shape
        self.stack = torch.from_numpy(np.array(stack, np.float32)).to(dev)
        self.cover = None if cover is None else torch.from_numpy(np.array(cover, np.uint8)).to(dev)
        self.index = torch.from_numpy(np.array(index, np.int64)).to(dev)
        self.weight = None if weight is None else torch.from_numpy(np.array(weight, np.float64)).to(dev)
        self.average, self.support = Guarded(self.B * self.N * self.C * 4, dev), Guarded(self.B * self.N * 8, dev)

    def call(self, weight=True, support=True, st=None):
        w = self.weight.data_ptr() if weight and self.weight is not None else None
        return self.L.svae_nbr_average(self.stack.data_ptr(), None if self.cover is None else self.cover.data_ptr(), self.images, self.N,
                                       self.C, self.index.data_ptr(), w, self.B, self.T, self.average.ptr,
                                       self.support.ptr if support else None, st or _stream())

    def read(self):
        torch.cuda.synchronize()
        return _read(self.average, np.float32, (self.B, self.N, self.C)), _read(self.support, np.float64, (self.B, self.N))


AVERAGE = ["60x35x1_T6", "40x105x3_T257", "10x1x4_T1"]


@functools.lru_cache(maxsize=None)
def average_case(name, seed=0):
    """(stack, cover, index, weight, reference average, reference support, unrounded quotient).  The tests here use seed 0."""
    rs = np.random.RandomState(AVERAGE.index(name) + 30 + 100 * seed)
    if name == "60x35x1_T6":
        images, N, C, B, T = 60, 35, 1, 60, 6
        index = np.concatenate([np.arange(60)[:, None], rs.randint(0, images, (B, T - 1))], 1)
        cover = (rs.rand(images, N) < 0.8).astype(np.uint8)
    elif name == "40x105x3_T257":
        images, N, C, B, T = 40, 105, 3, 17, 257
        index = rs.randint(-1, images, (B, T))                          # repeated images and empty slots
        index[3, 5], index[3, 6], index[8, 0] = images, -7, images      # skipped, not read
        index[11] = -1                                                   # a row that lists nobody
        cover = (rs.rand(images, N) < 0.6).astype(np.uint8)
        cover[:, 0] = 0                                                  # a pixel nobody covers
    else:
        images, N, C, B, T = 10, 1, 4, 10, 1
        index = rs.permutation(images)[:, None]
        cover = None
    stack = rs.randn(images, N, C).astype(np.float32)
    weight = rs.rand(B, T) + 0.25
    index = index.astype(np.int64)
    want_avg, want_sup, exact = R.average(stack, cover, index, weight)
    out = (stack, cover, index, weight, want_avg, want_sup, exact)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", AVERAGE)
def test_average_matches_the_reference(name):
    """support is bit-equal; every average is the reference's float32 or one of its two float32 neighbours (the quotient is one
    double division rounded once: observed on the MI355X, 0 values not identical in every case); a NULL weight equals weights
    of 1.0 bit for bit; a pixel with den == 0 is +0 with the sign bit clear; an index equal to `images`, -7 and -1 are
    skipped; without support the average is the same."""
    stack, cover, index, weight, want_avg, want_sup, exact = average_case(name)
    run = Average(stack, cover, index, weight)
    assert run.call() == 0
    avg, sup = run.read()
    assert _same_bytes(sup, want_sup), "support"
    ok, same = R.within_one_float(avg, exact)
    print("%s: %d of %d averages not identical to the reference's float32" % (name, (~same).sum(), same.size))
    assert ok.all()
    empty = sup == 0
    if name == "40x105x3_T257":
        assert empty[:, 0].all() and empty[11].all() and not empty[:, 1:].all()
    assert not avg[empty].any() and not np.signbit(avg[empty]).any()
    ones = Average(stack, cover, index, np.ones_like(weight))
    assert ones.call() == 0
    one_avg, one_sup = ones.read()
    null = Average(stack, cover, index, None)
    assert null.call() == 0
    null_avg, null_sup = null.read()
    assert _same_bytes(null_avg, one_avg) and _same_bytes(null_sup, one_sup), "NULL weight"
    assert _same_bytes(one_sup, R.average(stack, cover, index)[1])
    bare = Average(stack, cover, index, weight)
    assert bare.call(support=False) == 0
    torch.cuda.synchronize()
    assert _same_bytes(_read(bare.average, np.float32, avg.shape), avg) and (bare.support.read()[0] == GUARD_BYTE).all()


def test_a_non_finite_pixel_reaches_exactly_the_rows_that_list_it():
    """One NaN pixel in one image: NaN in that pixel and channel of the rows that list the image where it covers the pixel, and
    every other value of every row bit-equal to the clean run."""
    stack, cover, index, weight, _, _, _ = average_case("60x35x1_T6")
    i0 = 7
    j0 = int(np.flatnonzero(cover[i0])[2])
    bad = stack.copy()
    bad[i0, j0, 0] = np.nan
    clean, dirty = Average(stack, cover, index, weight), Average(bad, cover, index, weight)
    assert clean.call() == 0 and dirty.call() == 0
    (avg, sup), (got, got_sup) = clean.read(), dirty.read()
    lists_it = (index == i0).any(1)
    assert lists_it.sum() >= 2 and not lists_it.all()
    hit = np.zeros(avg.shape, bool)
    hit[lists_it, j0, 0] = True
    assert np.isnan(got[hit]).all() and _same_bytes(got[~hit], avg[~hit]) and _same_bytes(got_sup, sup)


# ---------------------------------------------------------------- both entries: refusals, the wrappers
def test_every_refusal_leaves_the_buffers_untouched():
    """Every SVAE_E_INVALID case of the header, one call each: the status, a message in svae_last_error, and afterwards every
    output still holds its fill inside intact guards; the same buffers are then accepted as they stand."""
    z, K, want_d, want_i = search_case("70x1_K1")
    s = Search(np.repeat(z, 2, 1), 3)
    L, st = s.L, _stream()
    zp, images, D, K = s.z.data_ptr(), s.images, s.D, s.K

    def search(query=zp, B=images, query_base=0, cand=zp, M=images, cand_base=0, D=D, K=K, best_d2=s.d2.ptr, best_index=s.index.ptr):
        return L.svae_nbr_search(query, B, query_base, cand, M, cand_base, D, K, best_d2, best_index, st)

    stack, cover, index, weight, want_avg, want_sup, exact = average_case("60x35x1_T6")
    a = Average(stack, cover, index, weight)
    a.average.fill_byte(0x3C)
    a.support.fill_byte(0x3C)
    sp, cp, ip, wp = a.stack.data_ptr(), a.cover.data_ptr(), a.index.data_ptr(), a.weight.data_ptr()

    def average(stack=sp, cover=cp, images=a.images, N=a.N, C=a.C, index=ip, weight=wp, B=a.B, T=a.T, average=a.average.ptr,
                support=a.support.ptr):
        return L.svae_nbr_average(stack, cover, images, N, C, index, weight, B, T, average, support, st)

    cases = [(search, kw) for kw in (dict(B=0), dict(M=0), dict(D=0), dict(D=513), dict(K=0), dict(K=257), dict(query_base=-1),
                                     dict(cand_base=-1))]
    cases += [(search, {k: None}) for k in ("query", "cand", "best_d2", "best_index")]
    cases += [(search, {k: v + 4}) for k, v in (("query", zp), ("cand", zp), ("best_d2", s.d2.ptr), ("best_index", s.index.ptr))]
    cases += [(search, dict(best_d2=zp)), (search, dict(best_index=zp + 8)), (search, dict(best_index=s.d2.ptr)),
              (search, dict(best_d2=s.index.ptr + 8))]
    cases += [(average, kw) for kw in (dict(images=0), dict(images=2 ** 31), dict(N=0), dict(C=0), dict(C=5), dict(N=2 ** 30, C=2),
                                       dict(B=0), dict(T=0), dict(T=258))]
    cases += [(average, {k: None}) for k in ("stack", "index", "average")]
    cases += [(average, {k: v + 4}) for k, v in (("index", ip), ("weight", wp), ("support", a.support.ptr))]
    cases += [(average, dict(average=sp)), (average, dict(average=cp)), (average, dict(average=ip)), (average, dict(average=wp)),
              (average, dict(support=sp)), (average, dict(support=ip)), (average, dict(support=wp)), (average, dict(support=a.average.ptr))]
    for call, kw in cases:
        assert call(**kw) == E_INVALID, (call.__name__, kw)
        assert L.svae_last_error(), (call.__name__, kw)
    got_d, got_i = s.read()
    assert np.isposinf(got_d).all() and (got_i == -1).all()
    avg_bytes, intact_a = a.average.read()
    sup_bytes, intact_s = a.support.read()
    assert intact_a and intact_s and (avg_bytes == 0x3C).all() and (sup_bytes == 0x3C).all()
    want = R.brute_force(np.repeat(z, 2, 1), 3)
    got_d, got_i = s.run().read()
    assert _same_bytes(got_d, want[0]) and _same_bytes(got_i, want[1])
    assert a.call() == 0
    avg, sup = a.read()
    assert _same_bytes(sup, want_sup) and R.within_one_float(avg, exact)[0].all()


def test_the_wrappers_make_the_same_calls():
    """ops.NeighbourSearch (queries in two blocks, candidates in two) and ops.neighbour_average give the bits of the ctypes
    calls; bad arguments raise."""
    from spatial_vae_amd import ops
    dev = _dev()
    z, K, want_d, want_i = search_case("300x7_K64")
    zd = torch.from_numpy(z.copy()).to(dev)
    search = ops.NeighbourSearch(300, K, dev)
    for qlo, qhi in ((0, 130), (130, 300)):
        for lo, hi in ((200, 300), (0, 200)):
            search.update(zd[qlo:qhi], qlo, zd[lo:hi], lo)
    d2, index = search.lists()
    assert d2.is_cuda and index.is_cuda
    assert _same_bytes(d2.cpu().numpy(), want_d) and _same_bytes(index.cpu().numpy(), want_i)
    stack, cover, index, weight, _, _, _ = average_case("40x105x3_T257")
    run = Average(stack, cover, index, weight)
    assert run.call() == 0
    avg, sup = run.read()
    t = [torch.from_numpy(x.copy()).to(dev) for x in (stack, cover, index, weight)]
    got, got_sup = ops.neighbour_average(t[0], t[1], t[2], t[3], support=True)
    assert _same_bytes(got.cpu().numpy(), avg) and _same_bytes(got_sup.cpu().numpy(), sup)
    assert _same_bytes(ops.neighbour_average(t[0], t[1], t[2], t[3]).cpu().numpy(), avg)
    ones = Average(stack, cover, index, None)
    assert ones.call() == 0
    assert _same_bytes(ops.neighbour_average(t[0], t[1], t[2]).cpu().numpy(), ones.read()[0])
    with pytest.raises(RuntimeError):
        ops.NeighbourSearch(300, 257, dev)
    with pytest.raises(RuntimeError):
        ops.NeighbourSearch(300, K, "cpu")
    with pytest.raises(RuntimeError):
        search.update(zd[:10].float(), 0, zd, 0)
    with pytest.raises(RuntimeError):
        search.update(zd[:10], 295, zd, 0)
    with pytest.raises(RuntimeError):
        ops.neighbour_average(t[0], t[1], t[2].int())


# ---------------------------------------------------------------- what it is for
def test_neighbour_averages_denoise_towards_the_prototype():
    """200 images of 64 pixels: one of two prototypes plus unit noise; latents in two well separated clusters.  K = 20 with the
    image itself, uniform weights: every neighbour is of the image's own prototype, and the mean squared error of the averages
    to the prototypes is below 0.1 of the raw images' (the reference gives about 1 / 21 of it; the factor of two covers other
    seeds, not kernel error: the kernel must match the reference anyway)."""
    rs = np.random.RandomState(5)
    images, N, K = 200, 64, 20
    kind = np.arange(images) % 2
    proto = rs.randn(2, N) * 2.0
    stack = (proto[kind] + rs.randn(images, N)).astype(np.float32)[:, :, None]
    z = np.where(kind[:, None] == 0, -5.0, 5.0) + 0.5 * rs.randn(images, 2)
    d2, index = Search(z, K).run().read()
    assert (index >= 0).all() and (kind[index] == kind[:, None]).all()
    slots = np.concatenate([np.arange(images)[:, None], index], 1)
    run = Average(stack, None, slots, None)
    assert run.call() == 0
    avg, sup = run.read()
    assert (sup == K + 1).all()
    raw = float(((stack[:, :, 0] - proto[kind]) ** 2).mean())
    den = float(((avg[:, :, 0] - proto[kind]) ** 2).mean())
    ref = float(((R.average(stack, None, slots)[0][:, :, 0] - proto[kind]) ** 2).mean())
    print("neighbour averages: mse %.4f of the raw images' %.4f = %.4f (reference %.4f, ideal %.4f)" % (den, raw, den / raw, ref / raw, 1 / 21.0))
    assert den < 0.1 * raw
