"""The conditions under which tests/test_gpu_step_abi.py holds svae_linear_*, svae_adam_step* and the rotation's host half to
their references (tests/step_abi.py), checked without a GPU: every encoder bound inside the 5e-6 cap, the float64 references
equal to torch's own, the rectifier seeds what the search gives, the lattice cases exact and on the kink, and the comparisons
able to see six deliberate mistakes made in a float32 emulation of the kernels."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_abi as S

TORCH_ACT = {None: lambda v: v, "tanh": torch.tanh, "leakyrelu": lambda v: F.leaky_relu(v, S.LEAK), "relu": torch.relu,
             "sigmoid": torch.sigmoid}


def test_the_case_table_is_the_one_the_issue_names():
    shapes = {(c["M"], c["K"], c["N"]) for c in S.ENC_CASES}
    assert shapes == {(1, 1, 1), (3, 37, 10), (16, 16, 16), (17, 36, 20), (33, 520, 24), (20, 258, 7), (260, 44, 264), (5, 260, 262)}
    for s in S.SMALL:
        assert {c["act"] for c in S.ENC_CASES if (c["M"], c["K"], c["N"]) == s and c["kind"] == "random"} == set(S.ACTS)
    for s, rect in S.LARGE:
        acts = [c["act"] for c in S.ENC_CASES if (c["M"], c["K"], c["N"]) == s and c["kind"] in ("random", "grid")]
        assert acts == ["tanh", rect]
    assert len(S.ENC_NAMES) == len(set(S.ENC_NAMES)) == 15 + 10 + 6 + 2
    assert set(S.RECTIFIER_SEED) == {c["name"] for c in S.ENC_CASES if S.is_rectifier_on_random(c)}
    assert S.ADAM_LENGTHS == [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027, 262147]
    assert [n - 4096 * 4096 for n in S.NORM_LENGTHS] == [-3, 0, 1, 5]
    assert [S.norm_chunk(n) for n in S.NORM_LENGTHS] == [4096, 4096, 8192, 8192]
    assert [(n - 1) % S.norm_chunk(n) + 1 for n in S.NORM_LENGTHS[2:]] == [1, 5]       # the last chunk: a tail; a vector and a tail


@pytest.mark.parametrize("name", S.ENC_NAMES)
def test_every_encoder_bound_is_inside_the_cap_and_the_reference_is_torchs(name):
    """4 * e32 <= 5e-6 for out, dW, db and dx (largest: 3.5e-6, out of 5x260x262_tanh), with and without the bias; the float64
    reference written out in step_abi.layer agrees with torch autograd in float64 to 1e-12 of the largest entry."""
    c, inp = S.enc_case(name), S.enc_inputs(name)
    for bias in (True, False):
        r64, r32 = S.enc_reference(name, np.float64, bias), S.enc_reference(name, np.float32, bias)
        for k in S.ENC_OUTPUTS:
            assert r64[k].dtype == np.float64 and r32[k].dtype == np.float32 and np.isfinite(r64[k]).all(), (name, k)
            assert 4.0 * S.rel_err(r32[k], r64[k]) <= S.CAP, (name, k, S.rel_err(r32[k], r64[k]))
        assert all(0.0 < v <= S.CAP for v in S.enc_bounds(name, bias).values())
    x, w, b = (torch.from_numpy(inp[k]).double().requires_grad_(True) for k in ("x", "w", "b"))
    out = TORCH_ACT[c["act"]](F.linear(x, w, b))
    out.backward(torch.from_numpy(inp["dout"]).double())
    r64 = S.enc_reference(name)
    for k, t in (("out", out.detach()), ("dw", w.grad), ("db", b.grad), ("dx", x.grad)):
        assert S.rel_err(r64[k], t.numpy()) <= 1e-12, (name, k)


@pytest.mark.parametrize("name", sorted(S.RECTIFIER_SEED))
def test_rectifier_seeds_meet_the_margin_and_are_the_first_that_do(name):
    """No float64 pre-activation with |pre| <= 64 * max |pre32 - pre64| (tests/decoder_sweep.py's rule), so a kernel whose
    pre-activation is 64 times worse than the CPU's still takes every rectifier branch the reference takes: no case leaves a
    gradient uncompared.  The seed in the table is the first of at most 16 that qualifies."""
    lo, tau = S.enc_margin(name)
    assert lo > tau >= 0.0, (name, lo, tau)
    assert S.first_seed_with_margin(name) == S.RECTIFIER_SEED[name] < S.SEEDS_TRIED
    if S.enc_case(name)["kind"] == "grid":
        assert tau == 0.0 and S.enc_case(name)["M"] * S.enc_case(name)["N"] > 65536
    else:
        assert tau > 0.0


@pytest.mark.parametrize("name", [c["name"] for c in S.ENC_CASES if c["kind"] in ("lattice", "grid", "saturate")])
def test_dyadic_cases_are_exact_in_any_summation_order(name):
    """Every product is a multiple of the case's unit and a row's sum |x||w| + |b| stays below 2^24 units, so no partial sum in
    any order rounds: the float32 and float64 pre-activations are bit-equal.  Lattice cases: at least one pre-activation is
    exactly 0 and at least one lies on each side.  Saturation cases: both signs pass 110 and some stay of unit size."""
    c, inp = S.enc_case(name), S.enc_inputs(name)
    unit = 1.0 / 64 if c["kind"] == "lattice" else 2.0 ** -14
    p64, p32 = S.enc_reference(name)["pre"], S.enc_reference(name, np.float32)["pre"]
    assert np.array_equal(p32.astype(np.float64), p64)
    assert np.array_equal(p64 / unit, np.round(p64 / unit))
    budget = np.abs(inp["x"]).astype(np.float64) @ np.abs(inp["w"]).astype(np.float64).T + np.abs(inp["b"])
    assert budget.max() / unit < 2.0 ** 24
    if c["kind"] == "lattice":
        assert (p64 == 0).sum() >= 1 and (p64 > 0).sum() >= 1 and (p64 < 0).sum() >= 1
        assert p64[0, 0] == 0.0
        assert S.bit_equal(S.enc_exact_out32(name), S.enc_reference(name, np.float32)["out"])
    if c["kind"] == "saturate":
        assert p64.max() > S.SATURATE_SPAN and p64.min() < -S.SATURATE_SPAN and (np.abs(p64) < 2).sum() >= 1
        o32 = S.enc_out32(name)
        assert (np.abs(o32) == 1.0).sum() > 100 if c["act"] == "tanh" else ((o32 == 0.0).sum() >= 1 and (o32 == 1.0).sum() > 50)


def test_adam_reference_reproduces_torch_adam_in_float64():
    """Three steps of torch.optim.Adam on one float64 CPU tensor against adam_reference applied three times, for each beta pair
    and eps of the sweep: p, exp_avg and exp_avg_sq within 1e-12 relative.  torch gets the fp32-rounded hyper-parameters the
    entry point receives; step_size and sqrt_bc2 are handed to adam_reference as the exact doubles here (the GPU test hands it
    their fp32 roundings, adam_scalars, which is the one thing the entry point does differently from torch)."""
    n = 257
    for (b1, b2), eps in itertools.product(S.ADAM_BETAS, S.ADAM_EPS):
        lr, fb1, fb2, feps = (float(np.float32(t)) for t in (1e-3, b1, b2, eps))
        cur = {k: S.adam_inputs(n, seed=3)[k][8:].astype(np.float64) for k in "pmv"}      # the ordinary elements
        cur["m"][:], cur["v"][:] = 0.0, 0.0
        p = torch.from_numpy(cur["p"].copy()).requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr, betas=(fb1, fb2), eps=feps)
        for step in (1, 2, 3):
            g = S.adam_inputs(n, seed=10 + step)["g"][8:].astype(np.float64)
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            cur, _ = S.adam_reference(dict(cur, g=g), b1, b2, eps, lr / (1.0 - fb1 ** step), np.sqrt(1.0 - fb2 ** step))
            st = opt.state[p]
            for got, want in ((p.detach(), cur["p"]), (st["exp_avg"], cur["m"]), (st["exp_avg_sq"], cur["v"])):
                assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max(), (b1, b2, eps, step)


def test_adam_edges_are_what_the_table_says():
    inp = S.adam_inputs(1027)
    ss, bc = S.adam_scalars(**{k: S.ADAM_DEFAULT[k] for k in ("lr", "b1", "b2", "step")})
    ref, bound = S.adam_reference(inp, 0.9, 0.999, 1e-8, ss, bc)
    assert np.isinf(ref["v"][[2, 7]]).all() and (ref["p"][[2, 7]] == inp["p"][[2, 7]]).all() and (bound["v"][[2, 7]] == 0).all()
    with np.errstate(over="ignore"):
        assert np.float32(inp["g"][2]) * np.float32(inp["g"][2]) == np.inf
    assert 0 < inp["g"][3] < np.finfo(np.float32).tiny and 0 < ref["m"][6] < np.finfo(np.float32).tiny
    assert ref["p"][5] == inp["p"][5] and ref["m"][5] == 0 and ref["v"][5] == 0
    assert ref["m"][4] != inp["m"][4] and ref["v"][4] != inp["v"][4] and inp["g"][4] != 0      # n = 5's tail element moves
    assert abs(ref["p"][1] - inp["p"][1]) > 1e5                        # eps alone in the denominator
    assert inp["p"][0] == 0 and ref["p"][0] != 0
    assert np.isfinite(ref["p"]).all() and np.isfinite(ref["m"]).all()
    assert [S.adam_inputs(n)["p"].size for n in (1, 5)] == [1, 5]


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: a float32 emulation with one deliberate mistake must fail the comparison the GPU test makes
# ---------------------------------------------------------------------------------------------------------------------
def _enc_emulation(name, mistake):
    c = S.enc_case(name)
    return {k: v for k, v in S.layer(S.enc_inputs(name), c["act"], np.float32, mistake=mistake).items() if k in S.ENC_OUTPUTS}


def test_the_unmistaken_emulations_pass():
    for name in S.ENC_NAMES:
        assert not S.enc_violations(name, _enc_emulation(name, None)), name


def test_a_dropped_last_k_is_seen():
    caught = [n for n in S.ENC_NAMES if "out" in S.enc_violations(n, _enc_emulation(n, "drop_last_k"))]
    assert len(caught) >= len(S.ENC_NAMES) - 2, sorted(set(S.ENC_NAMES) - set(caught))


def test_a_bias_gradient_missing_its_last_row_is_seen():
    caught = [n for n in S.ENC_NAMES if list(S.enc_violations(n, _enc_emulation(n, "db_misses_last_row"))) == ["db"]]
    assert len(caught) >= len(S.ENC_NAMES) - 4, sorted(set(S.ENC_NAMES) - set(caught))


def test_leakyrelu_derivative_one_at_zero_is_seen():
    """Only a case with a pre-activation of exactly 0 can tell: both LeakyReLU lattice cases do, through dW, db or dx, while the
    forward value does not know."""
    for name in [c["name"] for c in S.ENC_CASES if c["kind"] == "lattice" and c["act"] == "leakyrelu"]:
        got = _enc_emulation(name, "leaky_one_at_zero")
        assert S.bit_equal(got["out"], S.enc_exact_out32(name))
        bad = S.enc_violations(name, got)
        assert bad and "out" not in bad, (name, bad)


@pytest.mark.parametrize("mistake", S.ADAM_MISTAKES)
def test_adam_mistakes_are_seen(mistake):
    """eps inside the square root (seen where v == 0 and m != 0, and wherever eps = 1e-3 matters), the two bias corrections
    swapped, the n % 4 tail left as it was: each leaves a bound at n = 1027 for every parameter set of the sweep it can
    affect, and the unmistaken emulation leaves none."""
    inp = S.adam_inputs(S.ADAM_SWEEP_N)
    seen = 0
    for step, (b1, b2), eps in itertools.product(S.ADAM_STEPS, S.ADAM_BETAS, S.ADAM_EPS):
        ss, bc = S.adam_scalars(1e-3, b1, b2, step)
        ref, bound = S.adam_reference(inp, b1, b2, eps, ss, bc)
        assert not S.adam_violations(S.adam_emulation(inp, b1, b2, eps, ss, bc), ref, bound)
        if mistake == "bias_corrections_swapped":
            wrong = S.adam_emulation(inp, b1, b2, eps, *S.adam_scalars(1e-3, b2, b1, step))
        else:
            wrong = S.adam_emulation(inp, b1, b2, eps, ss, bc, mistake)
        bad = S.adam_violations(wrong, ref, bound, " " + mistake)
        if mistake == "bias_corrections_swapped" and step == 1000000:
            continue                                         # both corrections have long been 1
        assert bad, (mistake, step, b1, b2, eps)
        seen += 1
    assert seen >= 12


def test_the_tail_mistake_needs_a_tail():
    inp = S.adam_inputs(1024)
    ss, bc = S.adam_scalars(1e-3, 0.9, 0.999, 1)
    ref, bound = S.adam_reference(inp, 0.9, 0.999, 1e-8, ss, bc)
    assert not S.adam_violations(S.adam_emulation(inp, 0.9, 0.999, 1e-8, ss, bc, "tail_not_updated"), ref, bound)
    for n in (1, 2, 3, 5, 1023, 1025, 262147):
        inp = S.adam_inputs(n)
        ref, bound = S.adam_reference(inp, 0.9, 0.999, 1e-8, ss, bc)
        assert S.adam_violations(S.adam_emulation(inp, 0.9, 0.999, 1e-8, ss, bc, "tail_not_updated"), ref, bound), n


# ---------------------------------------------------------------------------------------------------------------------
# the rotation's host half
# ---------------------------------------------------------------------------------------------------------------------
def test_rotation_matrices_send_quarter_turns_of_non_square_images_through_the_matrix():
    """ops.rotation_matrices: 90 and 270 degrees are the exact codes 1 / 3 on a square image and -1 (the general path, with
    the matrix oracle.pil_rotate.pil_matrix gives) when rows != cols -- the kernel's codes 1 and 3 index a transposed image
    and would leave a non-square one; 0 and 180 degrees stay exact either way."""
    from oracle import pil_rotate as R
    from spatial_vae_amd import ops
    off = np.array([0.0, np.pi / 2, np.pi, 3 * np.pi / 2, 2 * np.pi, np.pi / 4])
    for rows, cols in ((9, 9), (1, 1), (9, 14), (14, 9), (2, 3), (5, 40)):
        mat, quarter = ops.rotation_matrices(off, rows, cols)
        want = [0, 1, 2, 3, 0, -1] if rows == cols else [0, -1, 2, -1, 0, -1]
        assert quarter.tolist() == want, (rows, cols, quarter)
        for i in np.nonzero(quarter < 0)[0]:
            assert mat[i].tolist() == R.pil_matrix(360 * off[i] / 2 / np.pi, cols, rows)
    for shape in S.ROT_SHAPES:
        assert S.rot_offsets(shape)[:6].tolist() == off.tolist() and len(S.rot_offsets(shape)) == 12
