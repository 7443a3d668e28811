"""The yardstick and the case table of tests/test_gpu_decoder_abi.py, checked without a GPU: the float32 and float64 CPU
references of every case, the room they leave under the decoder's parity tolerances, the host-side buffer sizes, and that
each shape still reaches the plan branch it was chosen for."""
import ctypes

import numpy as np
import pytest
import torch

import decoder_abi as A
from helpers import rel_err

Y_CAP, GRAD_CAP = 2e-5, 1e-4      # what test_gpu_parity.py / test_gpu_geometry.py demand of the decoder


def test_the_table_holds_the_twelve_cases():
    assert len(A.CASES) == 12 and len(set(A.NAMES)) == 12
    assert all(len(c) == len(A.FIELDS) for c in A.CASES + A.VARIANTS)
    assert set(A.EXPECT) == set(A.BY_NAME)


@pytest.mark.parametrize("name", A.NAMES)
def test_references_are_finite_nonzero_and_leave_room_under_the_caps(name):
    """4 * e32 (e32 = rel_err of the float32 CPU reference against the float64 one) is what the GPU test allows a kernel above
    its floor; it must itself stay inside 2e-5 on y / logits and 1e-4 on every gradient, so those caps cannot be met by
    loosening.  Largest 4 * e32 over the table with these seeds: y 5.2e-7 (leaky_resid_L4), logits 4.4e-6 (z0_sigmoid_w128,
    whose largest logit is small), gradients 4.3e-6 (hidden_w0 of rank1_sigmoid_rag)."""
    r64, r32 = A.reference(name, torch.float64), A.reference(name, torch.float32)
    assert set(r64) == set(r32) == {"y", "logits"} | set(A.sink_names(name))
    for k in r64:
        assert r64[k].dtype == np.float64 and r32[k].dtype == np.float32
        assert r64[k].shape == r32[k].shape == A._shape(A.case(name), k)
        assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), k
        assert np.abs(r64[k]).max() > 0.0, "%s: the reference of %s is all zero" % (name, k)
        e4 = 4.0 * rel_err(r32[k], r64[k])
        print("%s %s 4*e32 %.3e" % (name, k, e4))
        assert e4 <= (Y_CAP if k in ("y", "logits") else GRAD_CAP), (k, e4)


def test_dy_scale_enters_the_reference_as_a_per_image_factor():
    name = "rank1_tanh"
    s = np.array([2.0, 0.0, 0.5, 1.0], np.float32)
    a, b = A.reference(name, torch.float64), A.reference(name, torch.float64, dy_scale=s)
    assert np.array_equal(a["y"], b["y"])
    for k in A.PER_IMAGE:
        if k in a:
            want = a[k] * s.reshape((-1,) + (1,) * (a[k].ndim - 1))
            assert np.allclose(b[k], want, rtol=1e-12, atol=0), k


def test_buffer_sizes_on_the_host():
    """svae_saved_bytes / svae_workspace_bytes: non-zero multiples of 256 for every case, and larger in fp16x3 mode (the
    operand fragments).  Host-only calls; the mode is restored."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    mode = L.svae_gemm_mode_get()
    try:
        for name in A.BY_NAME:
            d = A.make_desc(name)
            sizes = []
            for m in (_lib.GEMM_FP32, _lib.GEMM_FP16X3):
                assert L.svae_gemm_mode_set(m) == 0
                sv, ws = L.svae_saved_bytes(ctypes.byref(d)), L.svae_workspace_bytes(ctypes.byref(d))
                assert sv > 0 and ws > 0 and sv % 256 == 0 and ws % 256 == 0, (name, m, sv, ws)
                sizes.append((sv, ws))
            assert sizes[1][0] > sizes[0][0] and sizes[1][1] > sizes[0][1], (name, sizes)
    finally:
        assert L.svae_gemm_mode_set(mode) == 0
    assert L.svae_gemm_mode_get() == mode


@pytest.mark.parametrize("name", list(A.BY_NAME))
def test_each_case_still_reaches_its_branch(name):
    """The plan's predicates re-derived from the descriptor against the values written next to the table."""
    assert A.predicates(name) == A.EXPECT[name]


def test_the_table_covers_every_branch_it_claims():
    c, P = A.BY_NAME, {n: A.predicates(n) for n in A.BY_NAME}
    assert c["one_image_subtile"]["N"] < 32 and c["one_image_subtile"]["L"] == 1
    assert c["L1_c4_softplus"]["C"] == 4 and c["L1_c4_softplus"]["N"] % 32 != 0
    assert P["rank1_sigmoid_rag"]["rank1"] and c["rank1_sigmoid_rag"]["H"] % 32 != 0
    assert c["stream_c2_L3"]["Zd"] > 8 and c["stream_c2_L3"]["Zd"] % 8 != 0 and P["stream_c2_L3"]["Hp"] // 32 == 3
    assert c["relu_c3_coords"]["B"] % 16 == 1 and c["relu_c3_coords"]["C"] == 3
    assert c["deepest_c4"]["L"] - 1 == 7                                       # SVAE_MAX_HIDDEN
    assert c["many_images"]["B"] > 64 and c["many_images"]["B"] % 4 == 1
    assert c["z0_sigmoid_w128"]["Zd"] == 0
    assert (P["rank1_tanh_b20"]["Mp"] // 128 + 3) // 4 == 3                    # three sets: SVAE_DENSE4_TAIL==1 leaves a tail
    for n in ("rank1_tanh", "resid_tanh_w64", "z0_sigmoid_w128"):
        assert A.split_eligible(n), n
    for n in ("relu_c3_coords", "leaky_resid_L4", "stream_c2_L3", "many_images"):
        assert not A.split_eligible(n), n
    forms = {c[n]["pose"] for n in A.NAMES}
    assert forms == {"grid", "grid+theta", "grid+dx", "grid+theta+dx", "coords"}
