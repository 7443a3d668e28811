"""The conditions under which tests/test_gpu_kernel_fuzz.py, test_gpu_dense4.py and test_gpu_wgrad2.py hold the decoder kernels
to float64 (tests/decoder_sweep.py), checked without a GPU: every bound inside its cap, the lattice cases exact and on the
kink, the pinned seeds what the search gives, no case silently reduced to forward-only, and the comparison able to see three
deliberate mistakes made on the reference's side."""
import collections

import numpy as np
import pytest
import torch
import torch.nn as nn

import decoder_sweep as S
import test_gpu_dense4 as D4
import test_gpu_kernel_fuzz as FZ
import test_gpu_wgrad2 as W2
from helpers import rel_err


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            out.append(tuple(c))
    return out


# every case any of the three GPU files runs (the two files share some)
ALL = _unique(D4.CASES + [D4.BITS_CASE] + D4.TAIL_CASES + W2.CASES + [W2.FUSED_CASE] + FZ.SWEPT)
IDS = ["%s_B%d" % (c[0], c[2]) for c in ALL]          # relu_c1_coords has B = 6 in one file and 7 in the other
FUZZ00 = FZ.CASES[0]


def _violations(case, out):
    r64, b = S.reference(case, torch.float64), S.bounds(case)
    return {k: (rel_err(out[k], r64[k]), b[k]) for k in b if rel_err(out[k], r64[k]) > b[k]}


def test_the_default_sweep_and_the_tables_are_what_the_gpu_files_run():
    assert len(FZ.CASES) == 28 and FUZZ00[0] == "fuzz00_n5_B19_z5_H128_L4_C3_ReLU_coords"
    assert FZ.SWEPT == FZ.CASES + S.LATTICE + S.PINNED
    assert len(S.LATTICE) >= 8 and len(S.PINNED) >= 4
    assert len({c[0] for c in FZ.SWEPT}) == len(FZ.SWEPT)
    assert all(c in D4.TAIL_CASES for c in S.LATTICE_TAIL) and len(S.LATTICE_TAIL) == 2
    assert all(len(c) == 9 for c in ALL)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_bound_is_inside_its_cap(case):
    """bounds() asserts 4 * e32 <= 2e-5 (y, logits) / 1e-4 (gradients) for every compared output; the references are finite,
    not identically zero, shaped alike, and a smooth, lattice or pinned case compares every output.  Largest bounds with these
    seeds: y 1.2e-6, logits 5.1e-6 (fuzz24), gradients 9.0e-6 (fuzz13); printed per case."""
    r64, r32 = S.reference(case, torch.float64), S.reference(case, torch.float32)
    assert set(r64) == set(r32) and {"y", "logits"} <= set(r64)
    for k in r64:
        assert r64[k].dtype == np.float64 and r32[k].dtype == np.float32 and r64[k].shape == r32[k].shape, k
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all() and np.abs(r64[k]).max() > 0.0, k
    b = S.bounds(case)
    print("%s %s y %.2e logits %.2e gradients %.2e" % (case[0], S.kind(case), b["y"], b["logits"],
                                                        max([v for k, v in b.items() if k not in ("y", "logits")] or [0.0])))
    if S.kind(case) != "rectifier":
        assert set(b) == set(r64), sorted(set(r64) - set(b))
    else:
        assert set(b) in (set(r64), {"y", "logits"})


# the other thirteen have a pre-activation within tau of 0 and are compared on y and logits only
RECTIFIERS_WITH_MARGIN = ["fuzz04_n8_B9_z2_H32_L1_C2_ReLU_posed_B9", "fuzz06_n5_B6_z5_H200_L1_C3_LeakyReLU_posed_B6",
                          "leaky_c2_coords_B8", "leaky_c2_z0_B8"]


def test_no_class_loses_a_case_silently():
    """Cases per class over the three files, and which rectifier cases on random inputs have the margin for their gradients."""
    kinds = collections.Counter(S.kind(c) for c in ALL)
    assert kinds == {"smooth": 34, "rectifier": 17, "lattice": 9, "pinned": 5}, kinds
    for c in S.LATTICE + S.PINNED:
        assert S.gradients_compared(c) and set(S.compared(c)) == set(S.reference(c, torch.float64)), c[0]
    with_margin = sorted("%s_B%d" % (c[0], c[2]) for c in ALL if S.kind(c) == "rectifier" and S.gradients_compared(c))
    print("rectifier cases with their gradients compared:", with_margin)
    assert with_margin == RECTIFIERS_WITH_MARGIN, with_margin
    assert not S.gradients_compared(FUZZ00)


@pytest.mark.parametrize("case", S.LATTICE, ids=[c[0] for c in S.LATTICE])
def test_lattice_cases_are_exact_and_sit_on_the_kink(case):
    """Every hidden pre-activation is a multiple of the layer's lattice unit (1/32, then / 8 per hidden layer), bit-equal
    between the float32 and the float64 evaluation, and cannot round in any summation order: the largest
    sum |w| |h| + |b| of a row, in lattice units, is below 2^24.  At least one pre-activation is exactly 0 in the case and
    every layer has between 30 % and 70 % of its units on."""
    name, n, B, zd, H, L, C, act, posed = case
    p32, p64 = S.preactivations(case, torch.float32), S.preactivations(case, torch.float64)
    st = {k: v.double().numpy() for k, v in S.given(case)["state"].items()}
    assert len(p64) == L
    zeros = 0
    for l, (a, b) in enumerate(zip(p32, p64)):
        den = 32.0 * 8.0 ** l
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b), (name, l)
        assert np.array_equal(b * den, np.round(b * den)), (name, l)
        if l == 0:
            x, z = S.given(case)["coords"].double().numpy().reshape(B * n * n, 2), S.given(case)["z"].double().numpy()
            budget = np.abs(x) @ np.abs(st["coord_linear.weight"]).T + np.abs(st["coord_linear.bias"])
            if zd > 0:
                budget = budget + np.repeat(np.abs(z) @ np.abs(st["latent_linear.weight"]).T, n * n, axis=0)
        else:
            h = np.maximum(p64[l - 1], 0.0)
            budget = h @ np.abs(st["layers.%d.weight" % (2 * l - 1)]).T + np.abs(st["layers.%d.bias" % (2 * l - 1)])
        assert (np.abs(b) <= budget).all()
        print("%s layer %d: %d zeros, %.2f on, budget %.0f of 2^24 units" % (name, l, int((b == 0).sum()),
                                                                             float((b > 0).mean()), budget.max() * den))
        assert budget.max() * den < 2.0 ** 24, (name, l, budget.max() * den)
        assert 0.3 <= float((b > 0).mean()) <= 0.7, (name, l)
        zeros += int((b == 0).sum())
    assert zeros >= 1


@pytest.mark.parametrize("case", S.PINNED, ids=[c[0] for c in S.PINNED])
def test_pinned_seeds_meet_the_margin_and_are_the_first_that_do(case):
    assert case[7] is nn.LeakyReLU
    for lo, tau in S.margins(case):
        assert lo > tau > 0.0, (case[0], lo, tau)
    assert S.first_seed_with_margin(case) == S.PINNED_SEED[case]
    assert S.FIRST_SEED <= S.PINNED_SEED[case] < S.FIRST_SEED + S.SEEDS_TRIED


def test_the_pinned_cases_include_a_deep_one():
    assert any(c[5] == 4 for c in S.PINNED)


def test_fuzz00_is_the_documented_kink():
    """Its float32 CPU gradients are off by more than 1e-3 of the largest entry (g.layers.3.bias: a second-layer
    pre-activation of 1e-8 takes the other branch) while y stays inside its bound: a flip, not an error."""
    r64, r32 = S.reference(FUZZ00, torch.float64), S.reference(FUZZ00, torch.float32)
    worst = max(rel_err(r32[k], r64[k]) for k in r64 if k.startswith("g."))
    assert worst > 1e-3, worst
    assert rel_err(r32["y"], r64["y"]) <= S.bounds(FUZZ00)["y"]
    assert set(S.bounds(FUZZ00)) == {"y", "logits"} and not S.has_margin(FUZZ00)


def test_the_lattice_cases_reach_the_kernels_they_were_chosen_for():
    """dispatch() is what the GPU test asserts of svae_path_counts; here: that the table, under the fuzz file's five choices
    and the forced tail split of test_gpu_dense4.py, covers dense_kernel, dense4_kernel<1>, dense4_dual_kernel, one to three
    channels, ragged N and H, H = 500 and L = 3."""
    d = {c[0]: {m: S.dispatch(c, m) for m in ("0", "", "1", "2")} for c in S.LATTICE}
    assert all(v["0"]["dense4"] == 0 and v["0"]["dense_fp32_fwd"] > 0 for v in d.values())                  # dense_kernel
    assert all(v[m]["dense4"] == 0 for m in ("", "1", "2") for v in [d["lat_z0_seven_tiles"]])
    assert sum(v[""]["dense4"] > 0 and v[""]["dense4_nt2"] == 0 for v in d.values()) >= 6                   # dense4_kernel<1>
    assert sum(v["2"]["dense4_dual"] > 0 for v in d.values()) >= 5                                          # dual, no tail
    assert d["lat_c3_h96"]["2"]["dense4_nt2"] == 0 and d["lat_c3_h96"]["2"]["dense4"] == 2                  # odd tile count
    assert d["lat_z5_h128_n121"]["2"] == dict(d["lat_z5_h128_n121"]["2"], dense4_nt2=2, dense4_dual=1)      # C = 3
    for c in S.LATTICE_TAIL:                                                                                # forced tail
        assert c[2] * ((c[1] ** 2 + 31) // 32 * 32) > 512 and c[6] <= 2 and d[c[0]]["2"]["dense4_dual"] == 2
    assert {c[6] for c in S.LATTICE} == {1, 2, 3}
    assert any(c[1] ** 2 % 32 for c in S.LATTICE) and {96, 100, 500} <= {c[4] for c in S.LATTICE}
    assert any(c[5] == 3 for c in S.LATTICE)
    assert all(c[7] is nn.ReLU and not c[8] for c in S.LATTICE)


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: one deliberate mistake in the float32 evaluation must leave its bound
# ---------------------------------------------------------------------------------------------------------------------
WITH_GRADIENTS = [c for c in ALL if S.kind(c) != "rectifier"]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_swapped_coordinate_columns_are_seen(case):
    out, _ = S.evaluate(case, torch.float32, mistake="swap_columns")
    bad = _violations(case, out)
    assert bad and ("y" in bad or "logits" in bad), case[0]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_a_row_left_out_of_the_weight_gradients_is_seen(case):
    """The last pixel of the last image missing from the sums over rows: applicable wherever gradients are compared."""
    if not S.gradients_compared(case):
        assert S.kind(case) == "rectifier"
        return
    out, _ = S.evaluate(case, torch.float32, mistake="drop_last_row")
    bad = _violations(case, out)
    assert bad and all(k.startswith("g.") for k in bad), (case[0], bad)


@pytest.mark.parametrize("case", S.LATTICE, ids=[c[0] for c in S.LATTICE])
def test_relu_derivative_one_at_zero_is_seen(case):
    out, _ = S.evaluate(case, torch.float32, mistake="relu_one_at_zero")
    r32 = S.reference(case, torch.float32)
    assert np.array_equal(out["y"], r32["y"])          # the forward value does not know
    bad = _violations(case, out)
    assert bad and all(k.startswith("g") for k in bad), (case[0], bad)
