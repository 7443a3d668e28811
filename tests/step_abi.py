"""Helper of tests/test_gpu_step_abi.py and tests/test_step_abi_cpu.py (not collected, needs no GPU): the case tables, the
float64 references and the guarded device buffers for the entry points of the training step that are not the decoder --
svae_linear_forward / _backward, svae_adam_step / _guarded, svae_grad_guard_norm, svae_rotate_bicubic, svae_ctf_filter.

Modelled on tests/decoder_abi.py.  Unlike ops.py's wrappers the callers here own every buffer: an operand of exactly the
advertised size sits at a chosen byte offset (0, 4, 8 or 12) past a 256-byte boundary inside a larger allocation, with GUARD
words on both sides, so an overrun or over-read of a few elements lands inside the allocation and is seen instead of faulting."""
import ctypes
import functools
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
CAP = 5e-6                      # tests/test_gpu_encoder.py's bound for a layer output, and the cap here
MARGIN = 64.0                   # tests/decoder_sweep.py's margin rule for a rectifier's pre-activations
SEEDS_TRIED = 16
LEAK = 0.01

# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 1024                    # 4-byte words on each side, at least
NAN_BITS = 0x7FC00000           # guards of inputs: a lane that reads one too many drags a NaN into its sum
OUT_GUARD_BITS = 0xA5A5A5A5     # guards of outputs
PREFILL_BITS = 0x7FC01234       # outputs before the call: a NaN no arithmetic produces, so an element left unwritten shows


def _i32(bits):
    return int(np.array(bits, np.uint32).view(np.int32))


def dev():
    return torch.device("cuda:0")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


class Guarded(object):
    """`nwords` 4-byte words of device memory starting `off` bytes (a multiple of 4) past a 256-byte boundary, inside one
    allocation with at least GUARD words in front and behind.  role "in": the guards hold NaN and the payload `data`; role
    "out": the guards hold 0xA5A5A5A5 and the payload the prefill NaN, or `data` for a buffer the call updates in place."""

    def __init__(self, nwords, off=0, role="out", data=None):
        assert off % 4 == 0 and role in ("in", "out")
        self.nwords, self.role = int(nwords), role
        self.guard_bits = NAN_BITS if role == "in" else OUT_GUARD_BITS
        self.buf = torch.full((self.nwords + 2 * GUARD + 64 + 4,), _i32(self.guard_bits), dtype=torch.int32, device=dev())
        base = self.buf.data_ptr()
        assert base % 4 == 0
        self.start = GUARD + ((-(base + 4 * GUARD)) % 256) // 4 + off // 4
        self.ptr = base + 4 * self.start
        assert (self.ptr - off) % 256 == 0 and self.start >= GUARD and self.start + self.nwords + GUARD <= self.buf.numel()
        if data is not None:
            self.write(data)
        elif role == "out":
            self.fill_bits(PREFILL_BITS)

    def fill_bits(self, bits):
        self.buf[self.start:self.start + self.nwords].fill_(_i32(bits))
        return self

    def write(self, data):
        words = np.ascontiguousarray(data).reshape(-1).view(np.int32)
        assert words.size == self.nwords, (words.size, self.nwords)
        self.buf[self.start:self.start + self.nwords] = torch.from_numpy(words.copy()).to(self.buf.device)
        return self

    def read(self, dtype=np.float32, shape=None):
        """(payload as `dtype` [reshaped], indices of the guard words that changed, relative to the payload's first word)."""
        a = self.buf.cpu().numpy().view(np.uint32)
        mask = np.ones(a.size, bool)
        mask[self.start:self.start + self.nwords] = False
        changed = (np.nonzero(mask & (a != self.guard_bits))[0] - self.start).tolist()
        pay = a[self.start:self.start + self.nwords].copy().view(dtype)
        return (pay.reshape(shape) if shape is not None else pay), changed


def unwritten(a):
    """Entries of a float32 array that still hold the prefill's bit pattern."""
    return int((np.ascontiguousarray(a).view(np.uint32) == PREFILL_BITS).sum())


def bit_equal(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def rel_err(a, b):
    """max |a - b| relative to the largest reference entry: tests/helpers.py's measure."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------
# the encoder layer: cases
# ---------------------------------------------------------------------------------------------------------------------
ACTS = (None, "tanh", "leakyrelu", "relu", "sigmoid")
RECTIFIERS = ("leakyrelu", "relu")
SMALL = [(1, 1, 1), (3, 37, 10), (16, 16, 16)]
# shape -> the rectifier it runs with besides tanh; what each reaches is in the docstring of test_gpu_step_abi.py
LARGE = [((17, 36, 20), "relu"), ((33, 520, 24), "leakyrelu"), ((20, 258, 7), "relu"), ((260, 44, 264), "leakyrelu"),
         ((5, 260, 262), "relu")]
# 260 x 264 = 68 640 pre-activations of unit scale against a margin of 64 * 1.1e-6 = 7e-5: four of them fall inside it on
# average and none of 16 seeds is free of them.  That one rectifier case draws its inputs on a dyadic grid instead (kind "grid":
# x in k/16, w in k/1024, b in k/1024), fine enough to look like the normal draw and coarse enough that every pre-activation is
# exact in fp32 in any order (multiples of 2^-14 below 2^4); the margin is then 0 and the seed search only has to avoid a
# pre-activation of exactly 0.  The same shape's tanh case keeps the normal draw.
GRID_RECTIFIER = (260, 44, 264)
LATTICE_SHAPES = [(17, 36, 20), (3, 37, 10)]
SATURATE_SHAPE = (17, 36, 20)
SATURATE_SCALE = 8.0            # on x and on w: the grid draw's unit-scale pre-activations times 64
SATURATE_SPAN = 110.0           # both signs reach it: beyond -103.98 a float64 sigmoid rounds to 0 in fp32, not to a denormal

# The input seed of a rectifier case on random inputs: the first of 0, 1, ... (SEEDS_TRIED tried) whose float64
# pre-activations all lie further than MARGIN * max |pre32 - pre64| from the kink; tests/test_step_abi_cpu.py repeats the search.
RECTIFIER_SEED = {
    "1x1x1_leakyrelu": 0, "1x1x1_relu": 0, "3x37x10_leakyrelu": 0, "3x37x10_relu": 0, "16x16x16_leakyrelu": 0,
    "16x16x16_relu": 0, "17x36x20_relu": 0, "33x520x24_leakyrelu": 0, "20x258x7_relu": 0, "260x44x264_leakyrelu_grid": 4,
    "5x260x262_relu": 1,
}


def _name(shape, act, kind):
    return "%s_%s%s" % ("x".join(map(str, shape)), act or "none", "" if kind == "random" else "_" + kind)


def _cases():
    out = []
    for s in SMALL:
        out += [(s, a, "random") for a in ACTS]
    for s, rect in LARGE:
        out += [(s, "tanh", "random"), (s, rect, "grid" if s == GRID_RECTIFIER else "random")]
    for s in LATTICE_SHAPES:
        out += [(s, a, "lattice") for a in ("relu", "leakyrelu", None)]
    out += [(SATURATE_SHAPE, "tanh", "saturate"), (SATURATE_SHAPE, "sigmoid", "saturate")]
    return [dict(name=_name(*c), M=c[0][0], K=c[0][1], N=c[0][2], act=c[1], kind=c[2]) for c in out]


ENC_CASES = _cases()
ENC_BY_NAME = {c["name"]: c for c in ENC_CASES}
ENC_NAMES = [c["name"] for c in ENC_CASES]
ENC_OUTPUTS = ("out", "dw", "db", "dx")


def enc_case(name):
    return ENC_BY_NAME[name] if isinstance(name, str) else name


def is_rectifier_on_random(c):
    c = enc_case(c)
    return c["kind"] in ("random", "grid") and c["act"] in RECTIFIERS


def enc_inputs(name, seed=None):
    """float32 numpy x (M, K), w (N, K), b (N), dout (M, N) of a case.
    random: x ~ normal, w ~ normal / sqrt(K), b ~ 0.1 normal, as tests/test_gpu_encoder.py draws them; the seed of a
            rectifier case comes from RECTIFIER_SEED.
    lattice: x in k/8 (|k| <= 8), w in {-2..2}/8, b in k/8 (|k| <= 8): every product is a multiple of 1/64 and a row's
            sum |x||w| + |b| stays below 2^24 / 64, so the pre-activation is exact in fp32 in any summation order.  Row 0 of x
            and b[0] are zero: pre[0][0] is exactly 0.
    grid:   the random draw rounded to x in k/16, w in k/1024, b in k/1024 (see GRID_RECTIFIER): exact pre-activations.
    saturate: the grid draw with x and w times SATURATE_SCALE each, so that the pre-activations (still exact: a product by
            powers of two) pass SATURATE_SPAN on both sides while a few stay of unit size.  On the normal draw the few
            pre-activations of unit size would carry the fp32 rounding of sums of size 100 straight into the output: 4 * e32
            would be 8e-6, past the cap, for a reason that has nothing to do with saturation."""
    c = enc_case(name)
    M, K, N = c["M"], c["K"], c["N"]
    if seed is None:
        seed = RECTIFIER_SEED[c["name"]] if is_rectifier_on_random(c) else 0
    rs = np.random.RandomState((zlib.crc32(c["name"].encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
    dout = rs.normal(size=(M, N)).astype(np.float32)
    if c["kind"] == "lattice":
        x = (rs.randint(-8, 9, size=(M, K)) / 8.0).astype(np.float32)
        w = (rs.randint(-2, 3, size=(N, K)) / 8.0).astype(np.float32)
        b = (rs.randint(-8, 9, size=N) / 8.0).astype(np.float32)
        x[0], b[0] = 0.0, 0.0
        return dict(x=x, w=w, b=b, dout=dout)
    x = rs.normal(size=(M, K)).astype(np.float32)
    w = (rs.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rs.normal(size=N)).astype(np.float32)
    if c["kind"] in ("grid", "saturate"):
        x, w, b = np.round(x * 16) / 16, np.round(w * 1024) / 1024, np.round(b * 1024) / 1024
    if c["kind"] == "saturate":
        x, w = x * np.float32(SATURATE_SCALE), w * np.float32(SATURATE_SCALE)
    return dict(x=x, w=w, b=b, dout=dout)


# ---------------------------------------------------------------------------------------------------------------------
# the encoder layer: references
# ---------------------------------------------------------------------------------------------------------------------
ENC_MISTAKES = ("drop_last_k", "db_misses_last_row", "leaky_one_at_zero")


def layer(inp, act, dtype, bias=True, mistake=None):
    """act(x W^T + b) and its three gradients, written out in numpy in `dtype` (float64: the reference; float32: the yardstick
    e32 and, with `mistake`, the emulation of a wrong kernel).  act' is taken through the layer's OUTPUT a, as the kernel takes
    it: tanh 1 - a^2, sigmoid a (1 - a), ReLU [a > 0], LeakyReLU [a > 0] + 0.01 [a <= 0] -- so act'(0) is 0 and 0.01.
    Returns dict(pre, out, dw, db, dx)."""
    x, w, b, dout = (inp[k].astype(dtype) for k in ("x", "w", "b", "dout"))
    xk, wk = (x[:, :-1], w[:, :-1]) if mistake == "drop_last_k" else (x, w)
    pre = xk @ wk.T
    if bias:
        pre = pre + b
    leak = dtype(LEAK)
    if act is None:
        out, g = pre, np.ones_like(pre)
    elif act == "tanh":
        out = np.tanh(pre)
        g = 1 - out * out
    elif act == "sigmoid":
        with np.errstate(over="ignore"):
            out = 1 / (1 + np.exp(-pre))
        g = out * (1 - out)
    elif act == "relu":
        out = np.where(pre > 0, pre, dtype(0))
        g = np.where(out > 0, dtype(1), dtype(0))
    else:
        out = np.where(pre > 0, pre, leak * pre)
        g = np.where(out > 0, dtype(1), leak)
        if mistake == "leaky_one_at_zero":
            g = np.where(out >= 0, dtype(1), leak)
    dpre = dout * g
    db = (dpre[:-1] if mistake == "db_misses_last_row" else dpre).sum(0)
    return dict(pre=pre, out=out.astype(dtype), dw=dpre.T @ x, db=db, dx=dpre @ w)


@functools.lru_cache(maxsize=None)
def _layer_cached(name, dtype_name, bias):
    c = enc_case(name)
    return layer(enc_inputs(name), c["act"], getattr(np, dtype_name), bias=bias)


def enc_reference(name, dtype=np.float64, bias=True):
    return _layer_cached(enc_case(name)["name"], np.dtype(dtype).name, bias)


def enc_out32(name):
    """The layer's output as the backward call is handed it: the float64 reference rounded to fp32."""
    return enc_reference(name)["out"].astype(np.float32)


def enc_exact_out32(name):
    """Lattice cases: the one fp32 value the forward can give -- the exact pre-activation through the kernel's own
    activation (LeakyReLU's slope is the fp32 constant 0.01f, one rounding of an exact product)."""
    c = enc_case(name)
    assert c["kind"] == "lattice"
    pre = enc_reference(name)["pre"]
    assert np.array_equal(pre.astype(np.float32).astype(np.float64), pre)
    if c["act"] is None:
        return pre.astype(np.float32)
    if c["act"] == "relu":
        return np.where(pre > 0, pre, 0.0).astype(np.float32)                  # v > 0 ? v : 0.0f -- never -0
    return np.where(pre > 0, pre, float(np.float32(LEAK)) * pre).astype(np.float32)


CONTRACTION = {"out": "K", "dw": "M", "db": "M", "dx": "N"}


def enc_bounds(name, bias=True):
    """{output: min(5e-6, max(4 * e32, floor, 2 sqrt(Kc) u))} relative to the largest reference entry (rel_err), Kc the
    contraction length of that output: 4 * e32 is the rule of tests/test_gpu_decoder_abi.py, 2 sqrt(Kc) u the accumulation
    budget tests/test_gpu_encoder.py derives, and 5e-6 that file's bound, which nothing here passes.
    The floor is 16 u.  It stands for the kernel's tanh / sigmoid on v_exp_f32 / v_rcp_f32, which the CPU evaluation does not
    contain: 1 - 2 / (t + 1) and 1 / (1 + t) round a sum of size 1 to 2 whatever the result, so they leave an ABSOLUTE error of
    the order of u.  Relative to the largest entry that is 16 u only while some output is of size 1; for the `out` of those two
    activations the floor is therefore 16 u / max |ref| (max |ref| <= 1).  This is a widening of the floor, not of the cap, and
    it matters for the single outputs of (1, 1, 1) alone: 0.0279 (tanh: the floor would be 3.4e-5, so the bound is the cap,
    5e-6) and 0.533 (sigmoid: 1.8e-6); everywhere else max |ref| > 0.9.  That fast_tanh loses relative accuracy near 0 (1.4e-6
    of 0.0279 on the MI355X, 3.9e-8 absolute) is accepted: a hidden unit's value enters the next layer by its absolute size."""
    c = enc_case(name)
    r64, r32 = enc_reference(name, np.float64, bias), enc_reference(name, np.float32, bias)
    out = {}
    for k in ENC_OUTPUTS:
        floor = 16 * U
        if k == "out" and c["act"] in ("tanh", "sigmoid"):
            floor /= min(1.0, max(float(np.abs(r64[k]).max()), 1e-30))
        out[k] = min(CAP, max(4.0 * rel_err(r32[k], r64[k]), floor, 2.0 * math.sqrt(c[CONTRACTION[k]]) * U))
    return out


def enc_violations(name, got, bias=True, tag=""):
    """Hold outputs (a dict with some of out, dw, db, dx) to the float64 reference: prints a line per output, returns
    {output: (error, bound)} of those outside their bound."""
    c = enc_case(name)
    r64, b = enc_reference(name, np.float64, bias), enc_bounds(name, bias)
    bad = {}
    for k in ENC_OUTPUTS:
        if k not in got:
            continue
        assert got[k].shape == r64[k].shape, (c["name"], k, got[k].shape)
        e = rel_err(got[k], r64[k]) if np.isfinite(got[k]).all() else float("inf")
        print("step_abi enc %s%s %-3s err %.3e bound %.3e share %.2f" % (c["name"], tag, k, e, b[k], e / b[k]))
        if not e <= b[k]:
            bad[k] = (e, b[k])
    return bad


def enc_margin(name, seed=None):
    """(smallest |pre64|, MARGIN * max |pre32 - pre64|) of a case's inputs (or of another seed's)."""
    c = enc_case(name)
    inp = enc_inputs(name, seed)
    p64, p32 = layer(inp, c["act"], np.float64)["pre"], layer(inp, c["act"], np.float32)["pre"]
    return float(np.abs(p64).min()), MARGIN * float(np.abs(p32.astype(np.float64) - p64).max())


def first_seed_with_margin(name):
    for seed in range(SEEDS_TRIED):
        lo, tau = enc_margin(name, seed)
        if lo > tau:
            return seed
    return None


# ---------------------------------------------------------------------------------------------------------------------
# the encoder layer: raw calls
# ---------------------------------------------------------------------------------------------------------------------
ACT_CODE = {None: -1, "tanh": 0, "leakyrelu": 1, "relu": 2, "sigmoid": 3}


def linear_forward(inp, act, off_x=0, off_w=0, bias=True, act_code=None, dims=None, out_null=False):
    """One svae_linear_forward call on guarded buffers.  Returns dict(rc, out, bad (names of buffers whose guards changed))."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    M, K = inp["x"].shape
    N = inp["w"].shape[0]
    x = Guarded(M * K, off_x, "in", inp["x"])
    w = Guarded(N * K, off_w, "in", inp["w"])
    b = Guarded(N, 0, "in", inp["b"])
    out = Guarded(M * N, 0, "out")
    m, k, n = dims if dims is not None else (M, K, N)
    with torch.cuda.device(dev()):
        rc = L.svae_linear_forward(x.ptr, w.ptr, b.ptr if bias else None, None if out_null else out.ptr, m, k, n,
                                   ACT_CODE[act] if act_code is None else act_code, stream())
    torch.cuda.synchronize()
    o, ch = out.read(np.float32, (M, N))
    bad = ["out"] if ch else []
    bad += [nm for nm, g in (("x", x), ("w", w), ("b", b)) if g.read()[1]]
    return dict(rc=rc, out=o, bad=bad, err=L.svae_last_error().decode() if rc else "")


SINKS = ("dw", "db", "dx")


def linear_backward(inp, out32, act, sinks=SINKS, off_dout=0, off_out=0, out_null=False, act_code=None, dims=None):
    """One svae_linear_backward call on guarded buffers; `sinks`: the outputs requested, every other one NULL (its buffer is
    allocated all the same and must stay as prefilled).  Returns dict(rc, dw, db, dx, bad)."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    M, K = inp["x"].shape
    N = inp["w"].shape[0]
    x = Guarded(M * K, 0, "in", inp["x"])
    w = Guarded(N * K, 0, "in", inp["w"])
    o = Guarded(M * N, off_out, "in", out32)
    d = Guarded(M * N, off_dout, "in", inp["dout"])
    g = {"dw": Guarded(N * K), "db": Guarded(N), "dx": Guarded(M * K)}
    shape = {"dw": (N, K), "db": (N,), "dx": (M, K)}
    m, k, n = dims if dims is not None else (M, K, N)
    with torch.cuda.device(dev()):
        rc = L.svae_linear_backward(x.ptr, w.ptr, None if out_null else o.ptr, d.ptr, m, k, n,
                                    ACT_CODE[act] if act_code is None else act_code,
                                    *[g[s].ptr if s in sinks else None for s in SINKS], stream())
    torch.cuda.synchronize()
    res = dict(rc=rc, bad=[], err=L.svae_last_error().decode() if rc else "")
    for s in SINKS:
        res[s], ch = g[s].read(np.float32, shape[s])
        if ch:
            res["bad"].append(s)
    res["bad"] += [nm for nm, q in (("x", x), ("w", w), ("out", o), ("dout", d)) if q.read()[1]]
    return res


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
ADAM_LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 262147]
ADAM_DEFAULT = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1)
ADAM_STEPS = (1, 2, 1000000)
ADAM_BETAS = ((0.9, 0.999), (0.5, 0.9), (0.0, 0.999))
ADAM_EPS = (1e-8, 1e-3)
ADAM_SWEEP_N = 1027
TINY = 2.0 ** -149               # the spacing of fp32 below the normal range

# (p, g, m, v) of the first elements of every buffer; element 0 alone is what n = 1 updates, so it is one that moves
ADAM_EDGES = [
    (0.0, 0.25, -0.125, 0.0625),      # p == 0
    (0.5, 0.0, 0.5, 0.0),             # g == 0, v == 0, m != 0: the denominator is eps alone
    (0.75, 1e25, 0.1, 0.01),          # g^2 = inf in fp32: v becomes inf and the parameter must not move
    (-0.3, 1e-40, 0.3, 0.2),          # a denormal g beside ordinary moments
    (0.2, 1.0, 0.5, 1e30),            # sqrt(v) dominates eps by far (element 4: the scalar tail of n = 5, so one that moves)
    (1.5, 0.0, 0.0, 0.0),             # g == 0, v == 0, m == 0: nothing moves
    (-2.0, 1e-40, 0.0, 0.0),          # m becomes a denormal, g^2 underflows
    (0.1, -1e25, -0.2, 0.5),          # the overflow with the other sign
]


def adam_inputs(n, seed=0):
    """float32 p, g, m, v of length n: p ~ normal, g and m ~ 0.1 normal, v = (0.1 normal)^2, the first min(n, 8) elements
    overwritten with ADAM_EDGES.  Eight elements, not sixteen: the table holds every edge once (the overflow with both signs,
    the denormal gradient beside ordinary and beside zero moments) and has no more to put there."""
    rs = np.random.RandomState(1000 + 31 * seed + n % 9973)
    p = rs.normal(size=n).astype(np.float32)
    g = (0.1 * rs.normal(size=n)).astype(np.float32)
    m = (0.1 * rs.normal(size=n)).astype(np.float32)
    v = ((0.1 * rs.normal(size=n)) ** 2).astype(np.float32)
    for i, e in enumerate(ADAM_EDGES[:n]):
        p[i], g[i], m[i], v[i] = e
    return dict(p=p, g=g, m=m, v=v)


def adam_scalars(lr, b1, b2, step):
    """step_size and sqrt_bc2 as svae_adam_step forms them: in double from the float arguments, rounded to float once."""
    lr, b1, b2 = (float(np.float32(t)) for t in (lr, b1, b2))
    return np.float32(lr / (1.0 - math.pow(b1, float(step)))), np.float32(math.sqrt(1.0 - math.pow(b2, float(step))))


def adam_reference(inp, b1, b2, eps, step_size, sqrt_bc2, coef=None):
    """The header's formula in ATen's operation order, in float64 from the fp32 scalars:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  denom = sqrt(v) / sqrt_bc2 + eps;  p += -step_size * (m / denom).
    coef: the guarded form's factor; g * coef is rounded to fp32 first, as the kernel forms it on load.
    One exception, in fp32 semantics: where (1 - b2) g^2 is beyond the fp32 range the kernel's v is +inf, so the reference's
    v is +inf too and its p the old p (m / inf = 0).
    Bounds, per element: m within 4u (|b1 m| + |(1 - b1) g|) + 2^-149, v within 4u (|b2 v| + |(1 - b2) g^2|) + 2^-149, p within
    2 spacing(p) + 16u |update|.  The 2^-149 is a widening of the first two by one spacing of the denormal grid: a stored m or
    v below 2^-126 is rounded to a multiple of 2^-149 whatever its size (ADAM_EDGES' element 6 makes m 1e-41, where 4u |m| is
    2e-48), and a kernel that flushed it to zero would still be off by thousands of such spacings."""
    b1, b2, eps = (float(np.float32(t)) for t in (b1, b2, eps))
    ss, bc = float(step_size), float(sqrt_bc2)               # adam_scalars' fp32 values, as the kernel receives them
    g32 = inp["g"] if coef is None else inp["g"] * np.float32(coef)
    p, g, m, v = inp["p"].astype(np.float64), g32.astype(np.float64), inp["m"].astype(np.float64), inp["v"].astype(np.float64)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    over = v1 > float(np.finfo(np.float32).max)
    v1 = np.where(over, np.inf, v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        upd = -ss * (m1 / (np.sqrt(v1) / bc + eps))
    upd = np.where(over, 0.0, upd)
    bound = dict(m=4 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g)) + TINY,
                 v=np.where(over, 0.0, 4 * U * (np.abs(b2 * v) + np.abs((1.0 - b2) * g * g)) + TINY),
                 p=2 * np.spacing(np.abs(p + upd).astype(np.float32)).astype(np.float64) + 16 * U * np.abs(upd))
    return dict(p=p + upd, m=m1, v=v1), bound


ADAM_MISTAKES = ("eps_inside_sqrt", "bias_corrections_swapped", "tail_not_updated")


def adam_emulation(inp, b1, b2, eps, step_size, sqrt_bc2, mistake=None):
    """adam_kernel's arithmetic in numpy float32, operation by operation; `mistake`: one deliberate error (ADAM_MISTAKES; for
    bias_corrections_swapped the caller hands over the swapped scalars)."""
    f = np.float32
    b1, b2, eps, ss, bc = f(b1), f(b2), f(eps), f(step_size), f(sqrt_bc2)
    p, g, m, v = (inp[k].copy() for k in ("p", "g", "m", "v"))
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        m1 = b1 * m + (f(1) - b1) * g
        v1 = b2 * v + (f(1) - b2) * g * g
        den = np.sqrt(v1 + eps) / bc if mistake == "eps_inside_sqrt" else np.sqrt(v1) / bc + eps
        p1 = p + (-ss) * (m1 / den)
    if mistake == "tail_not_updated":
        k = p.size - p.size % 4
        p1[k:], m1[k:], v1[k:] = p[k:], m[k:], v[k:]
    return dict(p=p1.astype(f), m=m1.astype(f), v=v1.astype(f))


def adam_violations(got, ref, bound, tag=""):
    """Per-element comparison of p, m, v with the float64 reference; returns {name: (index, error, bound)} of the worst
    offender per buffer that is outside its bound, and prints the largest share of a bound per buffer."""
    bad = {}
    for k in ("p", "m", "v"):
        a, r, b = got[k].astype(np.float64), ref[k], bound[k]
        with np.errstate(invalid="ignore"):
            err = np.where(a == r, 0.0, np.abs(a - r))
        err = np.where(np.isnan(err), np.inf, err)
        share = np.where(err == 0.0, 0.0, err / np.maximum(b, 1e-300))
        i = int(np.argmax(share))
        print("step_abi adam%s %s worst share %.3f (element %d: err %.3e bound %.3e)" % (tag, k, share[i], i, err[i], b[i]))
        if share[i] > 1.0:
            bad[k] = (i, float(err[i]), float(b[i]))
    return bad


def adam_call(inp, lr, b1, b2, eps, step, zero_grad, control=None, off_p=0, n=None):
    """svae_adam_step (control None) or svae_adam_step_guarded (control: the bytes of an svae_guard_control built on the
    host) on guarded buffers that start 16-byte aligned and end wherever n puts the end.  Returns dict(rc, p, g, m, v, bad)."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    size = inp["p"].size
    bufs = {k: Guarded(size, off_p if k == "p" else 0, "out", inp[k]) for k in ("p", "g", "m", "v")}
    n = size if n is None else n
    with torch.cuda.device(dev()):
        if control is None:
            rc = L.svae_adam_step(bufs["p"].ptr, bufs["g"].ptr, bufs["m"].ptr, bufs["v"].ptr, n, lr, b1, b2, eps, step, zero_grad,
                                  stream())
        else:
            ctl = None
            if control != "null":
                ctl = Guarded(len(control) // 4, 0, "in", np.frombuffer(control, np.uint8))
            rc = L.svae_adam_step_guarded(bufs["p"].ptr, bufs["g"].ptr, bufs["m"].ptr, bufs["v"].ptr, n, b1, b2, eps, zero_grad,
                                          ctl.ptr if ctl is not None else None, stream())
    torch.cuda.synchronize()
    res = dict(rc=rc, bad=[], err=L.svae_last_error().decode() if rc else "")
    for k, q in bufs.items():
        res[k], ch = q.read()
        if ch:
            res["bad"].append(k)
    return res


def control_bytes(apply, coef, step_size, sqrt_bc2, t=7):
    from spatial_vae_amd import _lib
    rec = _lib.GuardControl()
    rec.t, rec.total, rec.coef, rec.step_size, rec.sqrt_bc2, rec.apply, rec.finite = t, 1.0, coef, step_size, sqrt_bc2, apply, 1
    return bytes(bytearray(rec))


# ---------------------------------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------------------------------
NORM_BASE = 4096 * 4096
NORM_LENGTHS = [NORM_BASE - 3, NORM_BASE, NORM_BASE + 1, NORM_BASE + 5]


def norm_chunk(n):
    """include/svae.h: 4096 floats per chunk, doubled until the buffer is at most 4096 chunks."""
    c = 4096
    while -(-n // c) > 4096:
        c *= 2
    return c


def norm_reference(g):
    return math.sqrt(float(np.square(g.astype(np.float64)).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# rotation and CTF bank
# ---------------------------------------------------------------------------------------------------------------------
ROT_SHAPES = [(9, 14, 1), (14, 9, 3), (1, 1, 1), (2, 3, 1), (3, 2, 2), (5, 40, 4)]
ROT_B = 12
CTF_SMALL = [(1, 1), (1, 5), (2, 2), (3, 8)]
CTF_GUARDED = [(39, 39), (81, 81), (82, 82)]        # the planes in LDS, twice (24 n m + 16 (n + m) bytes <= 160 KiB); in the workspace
CTF_COUNT = 3


def rot_offsets(shape):
    rs = np.random.RandomState(sum(shape))
    off = rs.uniform(0, 2 * np.pi, size=ROT_B)
    off[:6] = [0.0, np.pi / 2, np.pi, 3 * np.pi / 2, 2 * np.pi, np.pi / 4]
    return off


def rot_images(shape, u8):
    rows, cols, C = shape
    rs = np.random.RandomState(100 + sum(shape))
    if u8:
        return (np.floor(rs.uniform(size=(ROT_B, rows * cols, C)) * 255.0) / 255.0).astype(np.float32)
    return rs.normal(size=(ROT_B, rows * cols, C)).astype(np.float32)


def rot_oracle(y, offset, shape, u8):
    """oracle.pil_rotate image by image (channel by channel for float32 images, which Pillow keeps as single planes)."""
    from oracle import pil_rotate as R
    rows, cols, C = shape
    out = np.empty_like(y)
    for i in range(y.shape[0]):
        angle = 360 * offset[i] / 2 / np.pi
        im = y[i].reshape(rows, cols, C)
        if u8:
            r = R.rotate_u8((im * 255).astype(np.uint8), angle)
            out[i] = (r.astype(float) / 255).reshape(rows * cols, C).astype(np.float32)
        else:
            r = np.stack([R.rotate_f32(np.ascontiguousarray(im[:, :, c]), angle) for c in range(C)], -1)
            out[i] = r.reshape(rows * cols, C)
    return out


def ctf_table(P, seed):
    """tests/test_gpu_ctf.py's draw of a (P, 8) parameter table."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(0.8, 3.5, P), np.full(P, 2.7), rs.choice([200.0, 300.0], P), rs.uniform(1.0, 2.5, P),
                     rs.uniform(0, 200, P), rs.uniform(5, 15, P), np.zeros(P), rs.uniform(0, 180, P)], 1)
