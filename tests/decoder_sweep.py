"""Helper of tests/test_gpu_kernel_fuzz.py, test_gpu_dense4.py, test_gpu_wgrad2.py and tests/test_decoder_sweep_cpu.py (not
collected, needs no GPU): the float64 / float32 CPU references of test_gpu_dense4._run's cases, the bound each device output
is held to, and the cases whose rectifier gradients can be compared at all.

The three GPU files compare kernels with kernels.  Here every case gets the same decoder (oracle.torch_cpu_step.decoder) on the
CPU, on exactly the inputs _run draws, in float64 (the reference) and float32 (the yardstick), and per output the bound
max(4 * rel_err(r32, r64), 16 * 2^-24) -- the rule, the floor and the caps (2e-5 on y / logits, 1e-4 on gradients) of
test_gpu_decoder_abi.py.

A rectifier has a kink: a hidden pre-activation within rounding of 0 takes the other branch in another precision or summation
order, act' jumps, and no tolerance covers the gradient (fuzz00: 1.3e-2 between float32 and float64 on the CPU).  The forward
value is continuous there.  So the cases fall in classes, decided from the case alone:

  smooth      Tanh, Sigmoid: every output is compared.
  rectifier   ReLU / LeakyReLU on random inputs: y and logits always; gradients only where the float64 reference has no hidden
              pre-activation with |pre| <= tau_l = 64 * max |pre32 - pre64| of that layer ("margin"), else forward only.
  lattice     LATTICE: ReLU cases on inputs that make every hidden pre-activation a small dyadic rational -- exact in fp32
              in any summation order, so no flip is possible (and many are exactly 0: act'(0) = 0 is exercised); every
              gradient is compared.  Explicit coordinates k/8, z k/2, coordinate / latent layer k/4, hidden weights
              {-2..2}/8, hidden biases k/8; the output layer and dy are ordinary floats (nothing non-linear follows).
  pinned      PINNED: small LeakyReLU cases whose input seed (11 in _run) was searched, from 11 upwards over at most 16
              seeds, for the first that meets the margin condition; the seed stands in the table and every gradient is
              compared.

given(case) is what _run's hook takes for the lattice and pinned cases; it is None for every other case."""
import contextlib
import io
import zlib

import numpy as np
import torch
import torch.nn as nn

from helpers import rel_err
from oracle import torch_cpu_step as T

U = 2.0 ** -24
Y_CAP, GRAD_CAP = 2e-5, 1e-4
FLOOR = 16 * U
MARGIN = 64.0
FIRST_SEED, SEEDS_TRIED = 11, 16
SMOOTH, RECTIFIER = (nn.Tanh, nn.Sigmoid), (nn.ReLU, nn.LeakyReLU)
ACT_NAME = {nn.Tanh: "tanh", nn.Sigmoid: "sigmoid", nn.ReLU: "relu", nn.LeakyReLU: "leakyrelu"}
SPLIT_PATHS = ("dense_split_fwd", "dense_split_dgrad", "wgrad_split")

# name, n (image side), B, z, H, L, C, act, posed -- as test_gpu_dense4.CASES.  All on explicit coordinates (a posed grid goes
# through cos / sin and leaves the lattice).  Row tiles = B * ceil(n^2 / 32); dense4 is legal when they come in fours.
LATTICE = [
    ("lat_c1_h64", 8, 4, 2, 64, 2, 1, nn.ReLU, False),             # 8 tiles: dense4_kernel<1> by default, dual under =2
    ("lat_c2_h100_n25", 5, 8, 2, 100, 2, 2, nn.ReLU, False),       # 25 pixels in 32-row tiles, Hp 128: both ragged
    ("lat_c3_h96", 6, 6, 1, 96, 2, 3, nn.ReLU, False),             # three column tiles (NT = 2 illegal), 36 pixels of 64 rows
    ("lat_L3_h96", 8, 4, 2, 96, 3, 2, nn.ReLU, False),             # a plain data gradient and two weight gradients
    ("lat_h500", 28, 4, 2, 500, 2, 1, nn.ReLU, False),             # BASELINE width, 784 pixels (25 tiles per image)
    ("lat_z0_seven_tiles", 5, 7, 0, 64, 2, 1, nn.ReLU, False),     # 7 tiles: dense_kernel whatever is asked, no latent
    ("lat_tail_c1", 8, 20, 2, 64, 2, 1, nn.ReLU, False),           # 1280 rows = 2.5 sets: room for the forced tail split
    ("lat_tail_c2_h100", 8, 20, 2, 100, 2, 2, nn.ReLU, False),     # the same with two channels' logits partials, ragged H
    ("lat_z5_h128_n121", 11, 4, 5, 128, 2, 3, nn.ReLU, False),     # 121 pixels of 128 rows, five latent coordinates
]
LATTICE_TAIL = [c for c in LATTICE if c[0].startswith("lat_tail_")]

# name, n, B, z, H, L, C, act, posed, input seed (the first of 11, 12, ... that meets the margin condition)
_PINNED = [
    ("pin_leaky_L4", 5, 4, 2, 32, 4, 1, nn.LeakyReLU, False, 11),
    ("pin_leaky_c2_posed", 5, 3, 1, 64, 2, 2, nn.LeakyReLU, True, 11),
    ("pin_leaky_c3_h96", 6, 2, 2, 96, 2, 3, nn.LeakyReLU, False, 12),
    ("pin_leaky_z0_L3_posed", 5, 4, 0, 64, 3, 1, nn.LeakyReLU, True, 11),
    ("pin_leaky_c2_h100", 5, 4, 2, 100, 2, 2, nn.LeakyReLU, False, 17),
]
PINNED = [c[:9] for c in _PINNED]
PINNED_SEED = {c[:9]: c[9] for c in _PINNED}
_LATTICE_SET, _PINNED_SET = set(LATTICE), set(PINNED)


def kind(case):
    """'smooth', 'lattice', 'pinned' or 'rectifier' -- from the case alone."""
    case = tuple(case)
    if case in _LATTICE_SET:
        return "lattice"
    if case in _PINNED_SET:
        return "pinned"
    return "smooth" if case[7] in SMOOTH else "rectifier"


def split_eligible(case):
    """fp16x3 mode takes the f16 kernels (decoder_abi.split_eligible): bounded activation, an even number of 32-column tiles,
    at least one hidden GEMM."""
    H, L, act = case[4], case[5], case[7]
    return act in SMOOTH and ((H + 31) // 32) % 2 == 0 and L >= 2


def dispatch(case, dense4):
    """What svae_path_counts must show for one forward + backward of a rectifier case in fp32 mode (launch_dense / launch_wgrad
    of api.hip restated).  dense4: SVAE_DENSE4 as _run sets it -- "0", "1", "2", or "" for the default, which at these sizes
    (far below 2048 wide workgroups) is dense4_kernel<1> wherever dense4 is legal.  The streaming out_bwd pass is the only
    output-layer backward a rectifier has."""
    name, n, B, zd, H, L, C, act, posed = case
    assert act in RECTIFIER and L >= 2
    gemms = L - 1
    tiles, ntile = B * ((n * n + 31) // 32), (H + 31) // 32
    d4 = 2 * gemms if dense4 != "0" and tiles % 4 == 0 else 0           # forward and data gradient of every hidden layer
    wide = d4 if dense4 == "2" and ntile % 2 == 0 else 0
    # three channels: the forward GEMM with the logits epilogue is dense4_kernel<2>, its partials have no room for a tail
    dual = (wide - (1 if C > 2 else 0)) if wide else 0
    return {"dense_fp32_fwd": gemms, "dense_fp32_dgrad": gemms, "wgrad_fp32": gemms, "dense4": d4, "dense4_nt2": wide,
            "dense4_dual": dual, "out_bwd_stream": 1, "out_bwd_rank1": 0, "dense_split_fwd": 0,
            "dense_split_dgrad": 0, "wgrad_split": 0}


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _fresh_state(case):
    """The state dict test_gpu_dense4._run starts from: torch.manual_seed(5), then the constructor (the caller's RNG stream is
    left as it was)."""
    import spatial_vae.models as models
    name, n, B, zd, H, L, C, act, posed = case
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            p = models.SpatialGenerator(zd, H, n_out=C, num_layers=L, activation=act)
    return {k: v.detach().clone() for k, v in p.state_dict().items()}


def drawn_inputs(case, seed=FIRST_SEED):
    """float32 CPU tensors in _run's draw order: z, dy, then theta and dx (posed) or coords."""
    name, n, B, zd, H, L, C, act, posed = case
    N = n * n
    g = torch.Generator().manual_seed(seed)
    d = {"z": torch.randn(B, max(zd, 1), generator=g)[:, :zd].contiguous(), "dy": torch.randn(B, N, C, generator=g) / N}
    if posed:
        d["theta"] = torch.randn(B, generator=g)
        d["dx"] = 0.1 * torch.randn(B, 2, generator=g)
    else:
        d["coords"] = torch.rand(B, N, 2, generator=g) * 2 - 1
    return d


def _lattice_given(case):
    name, n, B, zd, H, L, C, act, posed = case
    assert not posed and act is nn.ReLU
    N = n * n
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)

    def steps(den, lim, *shape):             # multiples of 1/den in [-lim, lim]
        return torch.from_numpy(rs.randint(-lim * den, lim * den + 1, size=shape).astype(np.float32) / den)

    state = _fresh_state(case)               # the output layer keeps its ordinary floats
    state["coord_linear.weight"], state["coord_linear.bias"] = steps(4, 1, H, 2), steps(4, 1, H)
    if zd > 0:
        state["latent_linear.weight"] = steps(4, 1, H, zd)
    for i in range(1, L):
        state["layers.%d.weight" % (2 * i - 1)] = torch.from_numpy(rs.randint(-2, 3, size=(H, H)).astype(np.float32) / 8)
        state["layers.%d.bias" % (2 * i - 1)] = steps(8, 1, H)
    d = drawn_inputs(case)                   # dy: ordinary floats
    d["z"] = steps(2, 2, B, zd)
    d["coords"] = steps(8, 1, B, N, 2)
    return dict(d, state=state)


_GIVEN = {}


def given(case, seed=None):
    """What _run's hook takes: dict(state=, z=, dy=, coords= | theta=, dx=) of float32 CPU tensors for a lattice or pinned
    case, None for every other case (which _run draws itself)."""
    case = tuple(case)
    k = kind(case)
    if k not in ("lattice", "pinned"):
        return None
    if (case, seed) not in _GIVEN:
        if k == "lattice":
            _GIVEN[(case, seed)] = _lattice_given(case)
        else:
            _GIVEN[(case, seed)] = dict(drawn_inputs(case, PINNED_SEED[case] if seed is None else seed), state=_fresh_state(case))
    return _GIVEN[(case, seed)]


def inputs(case, seed=None):
    """The inputs of any case, in given()'s form."""
    return given(case, seed) or dict(drawn_inputs(case), state=_fresh_state(case))


def posed_grid(n):
    x0, x1 = np.meshgrid(np.linspace(-1, 1, n), np.linspace(1, -1, n))
    return torch.from_numpy(np.stack([x0.ravel(), x1.ravel()], 1).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
class _ReluOneAtZero(torch.autograd.Function):
    """relu with the derivative at exactly 0 taken as 1: mistake (b) of the sensitivity check."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * (x >= 0).to(g.dtype)


MISTAKES = ("drop_last_row", "relu_one_at_zero", "swap_columns")


def evaluate(case, dtype, seed=None, mistake=None):
    """oracle.torch_cpu_step.decoder on the CPU in `dtype` on the case's inputs, the pose applied as decoder_abi.reference
    does, autograd of sum(y * dy).  Returns (the dict _run returns: y, logits -- y again on explicit coordinates --,
    g.<parameter>, gin.<i>; the hidden layers' pre-activations, one (B * N, H) array per layer).  The logits are the last
    F.linear call's result and the pre-activations
    the arguments of the activation, both caught by standing in for the oracle's F / activation table during the call.
    mistake: one deliberate error (MISTAKES), for the sensitivity check only."""
    name, n, B, zd, H, L, C, act, posed = case
    N = n * n
    inp = inputs(case, seed)
    pp = {k: v.detach().to(dtype, copy=True).requires_grad_(True) for k, v in inp["state"].items()}
    z = inp["z"].to(dtype, copy=True).requires_grad_(zd > 0)
    dy = inp["dy"].to(dtype)
    if posed:
        th, dx = (inp[k].to(dtype, copy=True).requires_grad_(True) for k in ("theta", "dx"))
        x = posed_grid(n).to(dtype).unsqueeze(0).expand(B, N, 2)
        rot = torch.stack([torch.stack([torch.cos(th), torch.sin(th)], 1),
                           torch.stack([-torch.sin(th), torch.cos(th)], 1)], 1)
        x = (torch.bmm(x, rot) + dx.unsqueeze(1)).contiguous()
        extra = [th, dx]
    else:
        x = inp["coords"].to(dtype, copy=True).requires_grad_(True)
        extra = [x]
    if mistake == "swap_columns":
        x = x.flip(-1)
    linear_outputs, pres = [], []

    def recording_linear(*a, **k):
        linear_outputs.append(torch.nn.functional.linear(*a, **k))
        return linear_outputs[-1]

    class Functional(object):
        linear = staticmethod(recording_linear)

        def __getattr__(self, attr):
            return getattr(torch.nn.functional, attr)

    key = ACT_NAME[act]
    plain = T._ACT[key]
    if mistake == "relu_one_at_zero":
        assert act is nn.ReLU
        plain = _ReluOneAtZero.apply

    def recording_act(h):
        pres.append(h.detach().numpy().copy())
        return plain(h)

    kept_f, kept_act = T.F, T._ACT[key]
    T.F, T._ACT[key] = Functional(), recording_act
    try:
        y = T.decoder(pp, x, z, key)
    finally:
        T.F, T._ACT[key] = kept_f, kept_act
    assert len(pres) == L
    if mistake == "drop_last_row":          # the last pixel of the last image does not reach the weight-gradient sums
        part = dy.clone()
        part[-1, -1, :] = 0
        names = list(pp)
        gp = dict(zip(names, torch.autograd.grad((y * part).sum(), [pp[k] for k in names], retain_graph=True)))
    (y * dy).sum().backward()
    # _run reads the logits back only from forward_posed; forward(x, z) returns y alone and _run files it under both names
    out = {"y": y.detach().numpy(), "logits": (linear_outputs[-1].detach().view(B, N, C) if posed else y.detach()).numpy()}
    for k, q in pp.items():
        out["g." + k] = (gp[k] if mistake == "drop_last_row" else q.grad).numpy()
    for i, t in enumerate(extra + ([z] if zd > 0 else [])):
        out["gin.%d" % i] = t.grad.numpy()
    return out, pres


_REFS = {}


def _evaluated(case, dtype):
    case = tuple(case)
    if (case, dtype) not in _REFS:
        _REFS[(case, dtype)] = evaluate(case, dtype)
    return _REFS[(case, dtype)]


def reference(case, dtype):
    """The dict _run returns, computed on the CPU in `dtype`: float64 is the reference, float32 the yardstick.  Cached."""
    return _evaluated(case, dtype)[0]


def preactivations(case, dtype):
    return _evaluated(case, dtype)[1]


def margins(case, seed=None):
    """Per hidden layer (smallest |pre64|, tau_l = 64 * max |pre32 - pre64|)."""
    if seed is None:
        p32, p64 = preactivations(case, torch.float32), preactivations(case, torch.float64)
    else:
        p32, p64 = evaluate(tuple(case), torch.float32, seed)[1], evaluate(tuple(case), torch.float64, seed)[1]
    return [(float(np.abs(b).min()), MARGIN * float(np.abs(a.astype(np.float64) - b).max())) for a, b in zip(p32, p64)]


def has_margin(case, seed=None):
    """No hidden pre-activation of the float64 reference within tau_l of the kink."""
    return all(lo > tau for lo, tau in margins(case, seed))


def first_seed_with_margin(case):
    """The search that produced PINNED_SEED: the first of 11, 12, ... (16 tried) whose draw meets the margin condition."""
    for seed in range(FIRST_SEED, FIRST_SEED + SEEDS_TRIED):
        if has_margin(case, seed):
            return seed
    return None


def gradients_compared(case):
    """Whether the gradients of this case are held to float64: always, except for a rectifier on random inputs with a
    pre-activation inside the margin.  A lattice or pinned case never falls back (tests/test_decoder_sweep_cpu.py asserts
    why it need not)."""
    return kind(case) != "rectifier" or has_margin(case)


def compared(case):
    r64 = reference(case, torch.float64)
    return [k for k in r64 if k in ("y", "logits") or gradients_compared(case)]


def cap(key):
    return Y_CAP if key in ("y", "logits") else GRAD_CAP


def bounds(case):
    """{output: max(4 * e32, floor)} for every output of this case that is compared, each asserted inside its cap (y, logits
    2e-5; gradients 1e-4)."""
    r64, r32 = reference(case, torch.float64), reference(case, torch.float32)
    b = {k: max(4.0 * rel_err(r32[k], r64[k]), FLOOR) for k in compared(case)}
    for k, v in b.items():
        assert v <= cap(k), (case[0], k, v)
    return b


def check(case, runs):
    """Hold results of _run, {variant: outputs}, to the float64 reference: prints a `sweep <case> <variant> <output> err bound`
    line per compared output of every variant, then asserts that every error is inside its bound.  Returns
    {(variant, output): (error, bound)}.  No output of any case needed more than its bound on the MI355X in either GEMM mode
    (largest share: 0.86, g.layers.3.bias of tanh_h500 under SVAE_DENSE4=2), so there is no list of exceptions."""
    r64, b = reference(case, torch.float64), bounds(case)
    seen = {}
    for variant, out in runs.items():
        assert set(out) == set(r64), (case[0], variant, sorted(set(out) ^ set(r64)))
        for k, bound in b.items():
            assert out[k].shape == r64[k].shape and np.isfinite(out[k]).all(), (case[0], variant, k)
            e = rel_err(out[k], r64[k])
            print("sweep %s %s %s %.3e %.3e" % (case[0], variant, k, e, bound))
            seen[(variant, k)] = (e, bound)
    bad = {k: v for k, v in seen.items() if not v[0] <= v[1]}
    assert not bad, (case[0], bad)
    return seen
