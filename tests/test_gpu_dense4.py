"""dense4_kernel (csrc/dense4.h: four row tiles per wave, one 16-byte row-operand load per k-step) against dense_kernel on the
same inputs, in one process: SVAE_DENSE4=0 keeps the hidden-layer GEMMs on dense_kernel, =1 takes dense4_kernel wherever it is
legal (row space in whole 128-row groups, width in whole 64-column blocks, no residual).  Every variant the decoder
dispatches is covered -- plain forward, forward with the output layer's logits in the epilogue (1, 2, 3 channels), plain data
gradient (L = 3), data gradient into the coordinate layer (FIRST) with and without the rank-1 output-layer form for tanh
(LASTD 2) and sigmoid (LASTD 3), explicit coordinates and posed grids -- the dispatch is read back (svae_path_counts), the
forward activations must agree BIT FOR BIT (same k-ordered fma chain per element), everything that passes through a
differently-blocked fixed-order sum (logits, gradients) to 2e-6 of the largest entry.  The golden / oracle / full-size suites
run the default dispatch, which takes dense4_kernel at the BASELINE sizes of configs 2-5.

Every result is also held to the float64 CPU reference of the same decoder on the same inputs (tests/decoder_sweep.py: bound
max(4 * e32, 16 * 2^-24) per output, rectifier gradients only where no pre-activation sits at the kink), so that an error the
kernels share -- the coordinate layer, the output layer, the reduce and pose kernels -- cannot pass as agreement."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

import decoder_sweep as S
from helpers import rel_err

pytestmark = pytest.mark.gpu

CASES = [
    # name, n (image side), B, z, H, L, C, act, posed
    ("tanh_c1_rank1", 8, 6, 2, 64, 2, 1, nn.Tanh, True),          # CF C=1, FIRST + LASTD 2
    ("sigmoid_c1_rank1", 8, 6, 2, 64, 2, 1, nn.Sigmoid, True),    # FIRST + LASTD 3
    ("tanh_c2_stream", 8, 6, 2, 100, 2, 2, nn.Tanh, True),        # CF C=2, FIRST without LASTD (streaming out_bwd), Hp 128
    ("tanh_c3_L3", 8, 4, 3, 64, 3, 3, nn.Tanh, True),             # plain fwd, CF C=3, plain dgrad, FIRST
    ("tanh_c1_L3_rank1", 8, 4, 3, 64, 3, 1, nn.Tanh, True),       # LASTD 2 on a non-first layer
    ("relu_c1_coords", 8, 6, 2, 64, 2, 1, nn.ReLU, False),        # explicit coordinates (forward(x, z)), rectifier
    ("leaky_c2_coords", 12, 8, 0, 64, 2, 2, nn.LeakyReLU, False), # z_dim 0, 144 pixels (Npad 160: 5 tiles per image)
    ("tanh_h500", 28, 8, 2, 500, 2, 1, nn.Tanh, True),            # BASELINE width, 25 tiles per image
    ("tanh_h96_odd_tiles", 8, 6, 2, 96, 3, 2, nn.Tanh, True),     # three column tiles: NT = 2 is not legal, NT = 1 is
]


def _run(case, mode, monkeypatch, given=None):
    """One forward + backward of the decoder under SVAE_DENSE4=mode: (every output by name, svae_path_counts of the pair).
    given: dict(state=, z=, dy=, coords= | theta=, dx=) of CPU tensors to run on instead of the draws below
    (decoder_sweep.given: the lattice and pinned-seed cases); None draws them."""
    import spatial_vae.models as models
    from spatial_vae_amd import _lib
    name, n, B, zd, H, L, C, act, posed = case
    monkeypatch.setenv("SVAE_DENSE4", mode)
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    with contextlib.redirect_stdout(io.StringIO()):
        p = models.SpatialGenerator(zd, H, n_out=C, num_layers=L, activation=act).to(dev)
    N = n * n
    g = torch.Generator().manual_seed(11)
    if given is not None:
        p.load_state_dict(given["state"])
        z = given["z"].to(dev).requires_grad_(zd > 0)
        dy = given["dy"].to(dev)
    else:
        z = torch.randn(B, max(zd, 1), generator=g)[:, :zd].to(dev).requires_grad_(zd > 0)
        dy = (torch.randn(B, N, C, generator=g) / N).to(dev)
    _lib.path_counts(reset=True)
    if posed:
        x0, x1 = np.meshgrid(np.linspace(-1, 1, n), np.linspace(1, -1, n))
        grid = torch.from_numpy(np.stack([x0.ravel(), x1.ravel()], 1).astype(np.float32)).to(dev)
        if given is not None:
            theta, dx = (given[k].to(dev).requires_grad_(True) for k in ("theta", "dx"))
        else:
            theta = torch.randn(B, generator=g).to(dev).requires_grad_(True)
            dx = (0.1 * torch.randn(B, 2, generator=g)).to(dev).requires_grad_(True)
        y, logits = p.forward_posed(grid, B, theta=theta, dx=dx, z=z if zd > 0 else None, return_logits=True)
        extra = [theta, dx]
    else:
        x = (given["coords"] if given is not None else torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev).requires_grad_(True)
        y = p(x, z if zd > 0 else torch.zeros(B, 0, device=dev))
        logits = y
        extra = [x]
    y.backward(dy)
    torch.cuda.synchronize()
    counts = _lib.path_counts()
    out = {"y": y.detach().cpu().numpy(), "logits": logits.detach().cpu().numpy()}
    for k, q in p.named_parameters():
        out["g." + k] = q.grad.detach().cpu().numpy()
    for i, t in enumerate(extra + ([z] if zd > 0 else [])):
        out["gin.%d" % i] = t.grad.detach().cpu().numpy()
    return out, counts


@pytest.mark.parametrize("mode", ["1", "2"], ids=["nt1", "nt2"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_dense4_matches_dense_kernel(case, mode, monkeypatch):
    """SVAE_DENSE4=1: 32-column blocks, three waves per SIMD (the form small launches take); =2: 64-column blocks, two waves
    per SIMD (the form the BASELINE sizes of configs 2-5 take; an odd number of column tiles falls back to 1).
    MI355X against float64, largest error (bound, case) over this test and the tail-split one below: y 1.9e-7 (9.5e-7,
    tanh_h500), logits 1.2e-6 (3.1e-6, tanh_h500; closest tanh_c1_L3_rank1 on dense_kernel, 7.4e-7 of 1.1e-6), parameter
    gradients 2.6e-6 (3.0e-6, layers.3.bias of tanh_h500 under SVAE_DENSE4=2: the closest anything in the three files comes to
    its bound; 1.7e-6 on dense_kernel), input gradients 1.3e-6 (3.4e-6, dz of tanh_c3_L3)."""
    old, c_old = _run(case, "0", monkeypatch)
    new, c_new = _run(case, mode, monkeypatch)
    S.check(case, {"dense4=0": old, "dense4=" + mode: new})
    L = case[5]
    assert c_old.get("dense4", 0) == 0
    assert c_new["dense4"] == 2 * (L - 1), c_new                     # every hidden-layer GEMM, forward and data gradient
    nt2_legal = ((case[4] + 31) // 32) % 2 == 0                          # an even number of 32-column tiles
    if mode == "2" and nt2_legal:
        assert c_new["dense4_nt2"] == 2 * (L - 1), c_new                 # 64-column blocks for every one of them
    else:
        assert c_new["dense4_nt2"] == 0, c_new
    for k in old:
        e = rel_err(new[k], old[k])
        assert e < (1e-5 if case[4] >= 500 else 2e-6), (case[0], k, e)   # H = 500: sums over 6272 rows of differently-rounded logits


BITS_CASE = ("bits", 8, 6, 2, 64, 2, 3, nn.Tanh, True)


def test_dense4_forward_activations_are_bit_identical(monkeypatch):
    """The plain forward stores the same k-ordered fma chain per element: a 3-layer decoder's y can differ between the two
    kernels only through the output layer's differently-blocked partial sums, so compare an L = 2, C = 3 decoder whose logits
    come from out_fwd_kernel (SVAE_FUSE_LOGITS=0: one pass over the stored activations, identical in both runs)."""
    monkeypatch.setenv("SVAE_FUSE_LOGITS", "0")
    case = BITS_CASE
    old, _ = _run(case, "0", monkeypatch)
    runs = {"nofuse,dense4=0": old}
    for mode in ("1", "2"):
        new, c_new = _run(case, mode, monkeypatch)
        runs["nofuse,dense4=" + mode] = new
        assert c_new["dense4"] == 2
        assert c_new["dense4_nt2"] == (2 if mode == "2" else 0), (mode, c_new)
        assert np.array_equal(old["y"], new["y"]) and np.array_equal(old["logits"], new["logits"]), mode
    S.check(case, runs)


TAIL_CASES = [
    # 20 images of 64 padded rows = 1280 rows = 2.5 sets of 512 rows: the forced split leaves 1 set wide, 1.5 sets to the tail
    ("tail_tanh_c1_rank1", 8, 20, 2, 64, 2, 1, nn.Tanh, True),
    ("tail_tanh_c2_stream", 8, 20, 2, 100, 2, 2, nn.Tanh, True),
    ("tail_tanh_c3_L3", 8, 20, 3, 64, 3, 3, nn.Tanh, True),
    ("tail_relu_coords", 8, 20, 2, 64, 2, 1, nn.ReLU, False),
    ("tail_tanh_h500", 28, 8, 2, 500, 2, 1, nn.Tanh, True),           # 6400 rows, the split falls inside an image (800 rows)
] + S.LATTICE_TAIL                                                     # ReLU on lattice inputs: every gradient held to float64


@pytest.mark.parametrize("case", TAIL_CASES, ids=[c[0] for c in TAIL_CASES])
def test_split_layer_launch_matches_single_launch(case, monkeypatch):
    """A dense4_kernel<2> launch whose last round of workgroups is less than half full hands the sets of that round to a
    second launch at half the block width (launch_dense: BASELINE cfg 2 is such a launch).  The rows of the two launches then
    carry different numbers of per-column-block partials (logits, d(coords)), which the finish kernels must pick per row.
    SVAE_DENSE4_TAIL==<k> forces the split after k sets of 512 rows at test sizes; results must equal the single launch's.
    The two lattice cases (ReLU, every gradient held to float64) put the rectifier's finish kernels under the split too.
    MI355X against float64: see test_dense4_matches_dense_kernel; the lattice cases stay below 0.4 of their bounds."""
    monkeypatch.setenv("SVAE_DENSE4_TAIL", "0")
    one, c_one = _run(case, "2", monkeypatch, given=S.given(case))
    monkeypatch.setenv("SVAE_DENSE4_TAIL", "=1")
    two, c_two = _run(case, "2", monkeypatch, given=S.given(case))
    S.check(case, {"dense4=2,tail=0": one, "dense4=2,tail==1": two})
    B, n = case[2], case[1]
    rows = B * ((n * n + 31) // 32 * 32)
    assert rows > 512, "the case must span more than one set for the split to exist"
    assert c_one.get("dense4_tail", 0) == 0
    expect = 2 * (case[5] - 1) if case[6] <= 2 else 2 * (case[5] - 1) - 1      # C = 3: the logits partials have no room for a tail
    assert c_two["dense4_tail"] == expect, c_two
    # the split and the unsplit wide launch are both dense4_dual_kernel (the latter with an empty tail part)
    assert c_one["dense4_dual"] == expect and c_two["dense4_dual"] == expect, (c_one, c_two)
    assert c_one["dense4_nt2"] == 2 * (case[5] - 1) and c_two["dense4_nt2"] == 2 * (case[5] - 1), (c_one, c_two)
    for k in one:
        e = rel_err(two[k], one[k])
        assert e < (1e-5 if case[4] >= 500 else 2e-6), (case[0], k, e)
