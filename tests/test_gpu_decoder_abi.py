"""svae_decoder_forward, svae_decoder_forward_bce and svae_decoder_backward called straight through the C ABI
(tests/decoder_abi.py) on twelve small cases, one per branch of the plan, and held to the contract of include/svae.h:

  values      every output against oracle.torch_cpu_step.decoder in float64 on the CPU;
  bounds      nothing is written outside a buffer of exactly the advertised size, every requested output is overwritten;
  scratch     the workspace carries nothing from the forward call to the backward call, and no result depends on what
              `saved` or the workspace held before;
  NULLs       any subset of the gradient sinks, dz, pg, dy_scale, saved and logits may be absent.

Bound per output: max(4 * e32, floor), e32 being helpers.rel_err of the SAME decoder evaluated in float32 on the CPU against
the float64 one (the rule of test_gpu_loss_head.py: as many terms in another grouping), never looser than the 2e-5 (y, logits)
and 1e-4 (gradients) test_gpu_parity.py asks; tests/test_decoder_abi_cpu.py holds 4 * e32 itself inside those caps.

Floor: 16 * 2^-24 = 9.5e-7 for every output, the floor of test_latent_head_against_float64, a quarter of the caps or less.
It stands for what the float32 CPU evaluation does not contain: the kernels' tanh and sigmoid on v_exp_f32 / v_rcp_f32, about
2e-7 absolute per activation (test_gpu_encoder.py), entering a gradient twice per layer through act'.  With nn.Linear's
uniform(+-1/sqrt(fan_in)) weights a layer contracts H such errors of random sign with weights of variance 1/(3 H): 0.6 of one
error comes out, so the errors do not grow with the depth or the width and a few 1e-7 of the largest entry is all there is.
No case needed more: the largest error over all tests of this file is 0.60 of its bound in fp32 mode and 0.70 in fp16x3 mode.

The file runs in the process's GEMM mode; test_the_file_passes_in_fp16x3_mode repeats it in a child under SVAE_GEMM=fp16x3
with the same bounds.  MI355X maxima are recorded in each test's docstring."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import decoder_abi as A
from decoder_abi import U
from helpers import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y_CAP, GRAD_CAP = 2e-5, 1e-4
FLOOR_Y = 16 * U
FLOOR_GRAD = 16 * U
assert FLOOR_Y <= Y_CAP / 4 and FLOOR_GRAD <= GRAD_CAP / 4

SPLIT = ("dense_split_fwd", "dense_split_dgrad", "wgrad_split")
FP32 = ("dense_fp32_fwd", "dense_fp32_dgrad", "wgrad_fp32")
SUBSET_CASES = ["rank1_tanh", "stream_c2_L3", "leaky_resid_L4", "expand_bilinear", "z0_sigmoid_w128"]
BCE_CASES = ["rank1_tanh", "relu_c3_coords", "z0_sigmoid_w128"]


def _fp16x3():
    from spatial_vae_amd import _lib
    return _lib.gemm_mode() == "fp16x3"


def _bit_equal_subsets():
    """Subsets of the sinks must reproduce the all-sinks bits wherever they run the same kernels: always, except where
    SVAE_FUSE_OUT selects the generic fused form, whose launch depends on the sinks."""
    return os.environ.get("SVAE_FUSE_OUT") is None


class Base(object):
    """The run every other test compares with: one forward call with `saved` and `logits`, one backward call with every
    applicable sink, one zero-filled workspace for both."""

    def __init__(self, name):
        self.f = A.Forward(name)
        out, self.bwd_paths, bad = self.f.backward()
        self.out = dict(self.f.out, **out)
        self.bad_guards = sorted(set(self.f.bad_guards + bad))
        self.paths = dict(self.f.paths)
        for k, v in self.bwd_paths.items():
            self.paths[k] = self.paths.get(k, 0) + v


@functools.lru_cache(maxsize=None)
def _base(name):
    return Base(name)


def _floor(key):
    return FLOOR_Y if key in ("y", "logits") else FLOOR_GRAD


def _bounds(name, dy_scale=None):
    r64, r32 = A.reference(name, torch.float64, dy_scale), A.reference(name, torch.float32, dy_scale)
    b = {k: max(4.0 * rel_err(r32[k], r64[k]), _floor(k)) for k in r64}
    for k, v in b.items():
        assert v <= (Y_CAP if k in ("y", "logits") else GRAD_CAP), (name, k, v)
    return r64, b


def _assert_values(name, out, dy_scale=None, tag=""):
    r64, bound = _bounds(name, dy_scale)
    worst = {}
    for k, got in out.items():
        if k not in r64:
            continue
        assert np.isfinite(got).all(), (name, k)
        e = rel_err(got, r64[k])
        print("abi %s%s %-10s err %.3e bound %.3e" % (name, tag, k, e, bound[k]))
        worst[k] = (e, bound[k])
    bad = {k: v for k, v in worst.items() if v[0] > v[1]}
    assert not bad, (name, tag, bad)
    return worst


def _assert_bit_equal(name, got, want, keys=None, tag=""):
    for k in (keys if keys is not None else got):
        a, b = got[k], want[k]
        same = a.view(np.uint32) == b.view(np.uint32)
        assert same.all(), "%s%s: %s differs in %d of %d entries (first at %s: %r vs %r)" % (
            name, tag, k, int((~same).sum()), same.size, np.argwhere(~same)[0].tolist(), a[~same][0], b[~same][0])


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: values, bounds of the buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMES)
def test_every_output_against_float64(name):
    """y, logits, every parameter gradient, dz, dcoords / dtheta / ddx of one forward + one backward call.
    MI355X maxima (error, bound), fp32 mode: y 1.3e-7 (9.5e-7, stream_c2_L3), logits 6.5e-7 (3.5e-6, z0_sigmoid_w128; closest
    to its bound one_image_subtile, 5.4e-7 of 1.2e-6), parameter gradients 1.0e-6 (3.4e-6, coord_b of rank1_sigmoid_rag; closest
    hidden_w1 of deepest_c4, 6.8e-7 of 1.2e-6), dz / dcoords / dtheta / ddx 5.1e-7 (2.9e-6, dtheta of rank1_sigmoid_rag; closest
    dtheta of rank1_tanh, 4.9e-7 of 1.3e-6).  fp16x3 mode: y 1.4e-7 (9.5e-7), logits 5.4e-7 (1.2e-6), parameter gradients
    4.9e-7 of 1.2e-6 (hidden_w6 of deepest_c4), per-image gradients 5.5e-7 of 9.5e-7 (dz of resid_tanh_w64)."""
    b = _base(name)
    assert set(b.out) == {"y", "logits"} | set(A.sink_names(name))
    _assert_values(name, b.out)


@pytest.mark.parametrize("name", A.NAMES)
def test_nothing_outside_the_buffers_everything_inside_overwritten(name):
    """After the calls of test 1 the 4096 bytes of 0xA5 on either side of y, logits, saved (exactly svae_saved_bytes), the
    workspace (exactly svae_workspace_bytes) and every gradient are untouched, and no output still holds the sentinel
    -12345.5 it was filled with or a non-finite value.  MI355X: holds in all twelve cases, both modes."""
    b = _base(name)
    assert not b.bad_guards, "%s: written outside %s" % (name, b.bad_guards)
    for k, v in b.out.items():
        assert A.sentinel_hits(v) == 0, "%s: %d entries of %s were never written" % (name, A.sentinel_hits(v), k)
        assert np.isfinite(v).all(), (name, k)


@pytest.mark.parametrize("name", A.NAMES)
def test_each_case_runs_the_intended_kernel_families(name):
    """svae_path_counts of the call pair.  fp32 mode: no f16 kernel anywhere, the rank-1 output-layer backward where the
    table says so and the streaming pass elsewhere, dense4 where it is legal.  fp16x3 mode: the f16 families (and
    out_bwd_split) for the eligible cases, the fp32 families and nothing else for ReLU-type activations and odd tile
    counts."""
    c, P, paths = A.case(name), A.predicates(name), _base(name).paths
    gemm = c["L"] >= 2
    if _fp16x3() and A.split_eligible(name):
        assert all(paths.get(k, 0) > 0 for k in SPLIT), paths
        assert not any(paths.get(k, 0) for k in FP32 + ("out_bwd_rank1",)), paths
        assert paths.get("out_bwd_split", 0) > 0, paths
        return
    assert not any(paths.get(k, 0) for k in SPLIT + ("out_bwd_split",)), paths
    assert all((paths.get(k, 0) > 0) == gemm for k in FP32), paths
    if os.environ.get("SVAE_FUSE_OUT") is None:
        assert (paths.get("out_bwd_rank1", 0) > 0) == P["rank1"], paths
        assert (paths.get("out_bwd_stream", 0) > 0) == (not P["rank1"]), paths
    if os.environ.get("SVAE_DENSE4") is None:
        assert (paths.get("dense4", 0) > 0) == (P["dense4"] and gemm), paths


# ---------------------------------------------------------------------------------------------------------------------
# 3: the workspace is scratch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x00], ids=["nan_filled", "zero_filled"])
@pytest.mark.parametrize("name", A.NAMES)
def test_the_workspace_carries_nothing_between_the_calls(name, fill):
    """`saved` and workspace A pre-filled with the byte (0xFF: NaN as floats), forward in A, all of A overwritten with it,
    backward in a separate workspace B filled likewise.  Every output is bit-equal to the run of test 1 (one zero-filled
    workspace for both calls; no atomics on values, fixed summation order): a difference is a read of something this call
    never wrote.  MI355X: bit-equal in all 24 runs, both modes."""
    r = A.run_abi(name, fill=fill, separate_ws=True)
    assert not r["bad_guards"], r["bad_guards"]
    _assert_bit_equal(name, r["out"], _base(name).out, tag=" fill %#x" % fill)


# ---------------------------------------------------------------------------------------------------------------------
# 4: NULL subsets of the backward outputs
# ---------------------------------------------------------------------------------------------------------------------
def _subsets(name):
    c, names = A.case(name), A.sink_names(name)
    last = c["L"] - 2
    per_image = [k for k in names if k in A.PER_IMAGE]
    params = [k for k in names if k not in A.PER_IMAGE]
    alone = "dcoords" if "dcoords" in names else ("dtheta" if "dtheta" in names else "ddx")   # stream_c2_L3 has no theta
    return {"a_pose_latent": per_image, "b_params": params, "c_out": ["out_w", "out_b"], "d_hidden_w": ["hidden_w%d" % last],
            "d_hidden_b": ["hidden_b%d" % last], "e_first_layer": [k for k in ("coord_w", "coord_b", "latent_w") if k in names],
            "f_one_pose_sink": [alone]}


SUBSET_IDS = ["a_pose_latent", "b_params", "c_out", "d_hidden_w", "d_hidden_b", "e_first_layer", "f_one_pose_sink"]


@pytest.mark.parametrize("subset", SUBSET_IDS)
@pytest.mark.parametrize("name", SUBSET_CASES)
def test_null_subsets_of_the_backward_outputs(name, subset):
    """One backward call per subset from the forward of test 1, every other sink NULL (b: dz and pg themselves NULL):
    (a) a frozen decoder, (b) parameters only, (c) the output layer, (d) the last hidden layer's weight without its bias and
    the reverse, (e) the coordinate layer, (f) one pose sink alone (dcoords on explicit coordinates, dtheta without ddx on a
    posed grid; ddx for stream_c2_L3, which has no theta).  Every requested output meets its bound of test 1 and the guards
    of everything stay intact.
    fp32 mode: the same kernels run whatever is requested (a skipped weight-gradient launch feeds nothing else), so every
    requested output is also bit-equal to the all-sinks run.
    fp16x3 mode, cases on the f16 kernels (rank1_tanh, expand_bilinear, z0_sigmoid_w128): subsets a, c, e and f leave both
    hidden_w[L-2] and hidden_b[L-2] NULL, which turns split_ob off -- the output layer's backward is then the streaming
    out_bwd_kernel ('out_bwd_stream', asserted) with a conversion pass instead of out_bwd_split_kernel, another summation
    order -- and are held to the bound only; b and d stay bit-equal.
    MI355X: bit-equal wherever demanded in both modes; closest to a bound in fp32 mode hidden_b0 of stream_c2_L3 (b), 6.0e-7
    of 1.9e-6, and dtheta of rank1_tanh (a), 4.9e-7 of 1.3e-6; in fp16x3 mode the same dtheta, 5.8e-7 of 1.3e-6."""
    b = _base(name)
    want = _subsets(name)[subset]
    out, paths, bad = b.f.backward(sinks=want, null_pg=True)
    assert not bad, bad
    assert set(out) == set(want)
    for k, v in out.items():
        assert A.sentinel_hits(v) == 0 and np.isfinite(v).all(), (name, subset, k)
    _assert_values(name, out, tag=" " + subset)
    last = A.case(name)["L"] - 2
    flips = _fp16x3() and A.split_eligible(name) and not ({"hidden_w%d" % last, "hidden_b%d" % last} & set(want))
    if flips:
        assert paths.get("out_bwd_stream", 0) > 0 and not paths.get("out_bwd_split"), paths
    elif _bit_equal_subsets():
        _assert_bit_equal(name, out, b.out, tag=" " + subset)


# ---------------------------------------------------------------------------------------------------------------------
# 5: dy_scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMES)
def test_dy_scale(name):
    """The per-image factor, which only the fused Bernoulli loss feeds elsewhere.  All ones: bit-equal to NULL (a
    multiplication by 1.0f).  Random factors in [0.25, 4): against float64 of dy * s[b], bounds as in test 1 from the float32
    evaluation of the same product.  One factor zero (the middle image): that image's dz, dtheta, ddx and dcoords are exactly
    zero and everything is finite.
    MI355X, closest to a bound: fp32 mode out_w of deepest_c4 with the zero factor, 5.8e-7 of 9.5e-7, and dz of
    resid_tanh_w64, 1.3e-6 of 2.4e-6; fp16x3 mode hidden_w6 of deepest_c4, 8.3e-7 of 1.2e-6.  All ones bit-equal, the zeroed
    image's rows exactly zero, in all twelve cases and both modes."""
    b = _base(name)
    B = A.case(name)["B"]
    ones, _, bad = b.f.backward(dy_scale=np.ones(B, np.float32))
    assert not bad, bad
    _assert_bit_equal(name, ones, b.out, tag=" dy_scale=1")
    rs = np.random.RandomState(B)
    s = rs.uniform(0.25, 4.0, size=B).astype(np.float32)
    out, _, bad = b.f.backward(dy_scale=s)
    assert not bad, bad
    _assert_values(name, out, dy_scale=s, tag=" dy_scale")
    s0 = s.copy()
    s0[B // 2] = 0.0
    out, _, bad = b.f.backward(dy_scale=s0)
    assert not bad, bad
    _assert_values(name, out, dy_scale=s0, tag=" dy_scale0")
    for k in A.PER_IMAGE:
        if k in out:
            assert (out[k][B // 2] == 0.0).all(), (name, k, out[k][B // 2])


# ---------------------------------------------------------------------------------------------------------------------
# 6: inference forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.NAMES)
def test_inference_forms_give_the_training_forms_y(name):
    """saved = NULL (the activations ping-pong through dh[0] / dh[1] of the workspace) and logits = NULL, together and
    separately, in a workspace (and `saved`) pre-filled with 0xFF: y, and logits where present, bit-equal to the training-form
    forward of test 1.  out_fwd_kernel, logits_finish_kernel and logits_finish_bce_kernel all test `logits` before the store.
    MI355X: bit-equal in all 36 runs, both modes."""
    b = _base(name)
    for saved, logits in ((False, False), (False, True), (True, False)):
        f = A.Forward(name, saved=saved, logits=logits, fill=0xFF)
        assert not f.bad_guards, f.bad_guards
        assert set(f.out) == ({"y", "logits"} if logits else {"y"})
        _assert_bit_equal(name, f.out, b.out, tag=" saved=%d logits=%d" % (saved, logits))


@pytest.mark.parametrize("name", BCE_CASES)
def test_forward_bce_without_dll_dy(name):
    """svae_decoder_forward_bce with dll_dy = NULL against the call with it: loglik, y and logits bit-equal (rank1_tanh and
    z0_sigmoid_w128 finish inside logits_finish_bce_kernel, relu_c3_coords -- three channels -- runs bce_kernel behind
    out_fwd_kernel), also with saved = NULL and logits = NULL.  y agrees with the plain forward's to 2 * 2^-24, loglik with
    float64 of the returned y to 4x the error of oracle.elbo_oracle.bce_loglik (floor 8 * 2^-24), and dll_dy entry by entry
    with -(s - t) / max((1 - s) s, 1e-12) to 8 * 2^-24.
    MI355X: bit-equal throughout; y identical to the plain forward's; loglik at most 1.3e-7 (bound 4.8e-7, relu_c3_coords),
    dll_dy at most 1.8e-7 of an entry (bound 4.8e-7), the same in fp16x3 mode."""
    from oracle import elbo_oracle as O
    b = _base(name)
    full = A.Forward(name, bce="dll", fill=0xFF)
    assert not full.bad_guards, full.bad_guards
    assert all(A.sentinel_hits(v) == 0 and np.isfinite(v).all() for v in full.out.values())
    for saved, logits in ((True, True), (False, False)):
        f = A.Forward(name, bce="nodll", saved=saved, logits=logits, fill=0xFF)
        assert not f.bad_guards, f.bad_guards
        assert "dll_dy" not in f.out
        _assert_bit_equal(name, f.out, full.out, tag=" bce saved=%d logits=%d" % (saved, logits))
    y, tgt = full.out["y"], A.inputs(name)[1]["target"]
    ref = A.bce64(y, tgt)
    o_ll, _ = O.bce_loglik(y.reshape(y.shape[0], -1), tgt.reshape(y.shape[0], -1))
    e, bound = rel_err(full.out["loglik"], ref), max(4.0 * rel_err(o_ll, ref), 8 * U)
    ey = rel_err(y, b.out["y"].astype(np.float64))
    y64, t64 = y.astype(np.float64), tgt.astype(np.float64)
    want = -(y64 - t64) / np.maximum((1.0 - y64) * y64, 1e-12)
    ed = float((np.abs(full.out["dll_dy"] - want) / np.maximum(np.abs(want), 1e-300)).max())
    print("abi %s bce loglik %.3e bound %.3e y %.3e dll %.3e" % (name, e, bound, ey, ed))
    assert e <= bound and ey <= 2 * U and ed <= 8 * U, (e, bound, ey, ed)


# ---------------------------------------------------------------------------------------------------------------------
# 7: kernel alternatives under the same contract
# ---------------------------------------------------------------------------------------------------------------------
ALTERNATIVES = [
    ("dense4_nt1", "rank1_tanh", {"SVAE_DENSE4": "1"}, ("dense4",), ("dense4_nt2",)),
    ("dense4_nt2", "rank1_tanh", {"SVAE_DENSE4": "2"}, ("dense4", "dense4_nt2", "dense4_dual"), ("dense4_tail",)),
    ("dense4_nt2_tail", "rank1_tanh_b20", {"SVAE_DENSE4": "2", "SVAE_DENSE4_TAIL": "=1"}, ("dense4_nt2", "dense4_tail"), ()),
    ("no_tail_merge", "rank1_tanh", {"SVAE_TAIL_MERGE": "0"}, ("out_bwd_rank1", "wgrad2"), ()),
    ("no_fused_logits", "rank1_tanh", {"SVAE_FUSE_LOGITS": "0"}, ("out_bwd_rank1",), ("dense4_cf",)),
]


@pytest.mark.parametrize("tag,name,env,ran,not_ran", ALTERNATIVES, ids=[a[0] for a in ALTERNATIVES])
def test_kernel_alternatives_keep_the_contract(tag, name, env, ran, not_ran, monkeypatch):
    """Tests 2 and 3 on rank1_tanh under the switches the library reads per call: SVAE_DENSE4=1 (dense4_kernel<1>), =2
    (dense4_dual_kernel, 64-column blocks), =2 with SVAE_DENSE4_TAIL==1 on the B = 20, N = 64 variant (1280 padded rows = three
    sets: one wide, two in the half-width tail), SVAE_TAIL_MERGE=0 (wgrad_reduce_kernel and first_layer_image_kernel instead of
    backward_tail_kernel) and SVAE_FUSE_LOGITS=0 (out_fwd_kernel).  Guards intact, nothing left unwritten, values inside the
    bounds of test 1, the NaN-filled separate-workspace run bit-equal to the zero-filled one under the same switch, and
    svae_path_counts names the family.  In fp16x3 mode these geometries run the f16 kernels whatever SVAE_DENSE4 says: the
    same contract is checked and the f16 families are asserted instead.
    MI355X: bit-equal and intact under all five switches; closest to a bound in fp32 mode dtheta of rank1_tanh under
    SVAE_DENSE4=1, 4.9e-7 of 1.3e-6 (largest error: dtheta of the B = 20 variant, 8.8e-7 of 2.9e-6); in fp16x3 mode dtheta of
    rank1_tanh under SVAE_FUSE_LOGITS=0, 6.1e-7 of 1.3e-6."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    same = A.run_abi(name)
    assert not same["bad_guards"], same["bad_guards"]
    for k, v in same["out"].items():
        assert A.sentinel_hits(v) == 0 and np.isfinite(v).all(), (tag, k)
    _assert_values(name, same["out"], tag=" " + tag)
    if _fp16x3():
        assert all(same["paths"].get(k, 0) > 0 for k in SPLIT), same["paths"]
    else:
        assert all(same["paths"].get(k, 0) > 0 for k in ran), (tag, same["paths"])
        assert not any(same["paths"].get(k, 0) for k in not_ran), (tag, same["paths"])
    for fill in (0xFF, 0x00):
        r = A.run_abi(name, fill=fill, separate_ws=True)
        assert not r["bad_guards"], r["bad_guards"]
        _assert_bit_equal(name, r["out"], same["out"], tag=" %s fill %#x" % (tag, fill))


# ---------------------------------------------------------------------------------------------------------------------
# 8: refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """ws_bytes one byte short, ws + 128 and saved + 128 give SVAE_E_WORKSPACE from both calls, dtheta requested with explicit
    coordinates gives SVAE_E_INVALID; svae_last_error() says why and no output buffer is touched."""
    from spatial_vae_amd import _lib
    L = _lib.lib()
    f = _base("relu_c3_coords").f
    dev = f.dev
    st = A._stream()
    d, p, pose = ctypes.byref(f.desc), ctypes.byref(f.params), ctypes.byref(f.pose)
    y = A.Guarded(f.bufs["y"].nbytes, dev).fill_float(A.SENTINEL)
    lg = A.Guarded(f.bufs["y"].nbytes, dev).fill_float(A.SENTINEL)
    saved = A.Guarded(f.saved_bytes + 256, dev).fill_byte(0)
    ws = A.Guarded(f.ws_bytes + 256, dev).fill_byte(0)
    sinks = {k: A.Guarded(4 * int(np.prod(A._shape(f.c, k))), dev).fill_float(A.SENTINEL)
             for k in ("out_w", "dz", "dcoords", "dtheta")}
    grads = _lib.Grads()
    grads.out_w = sinks["out_w"].ptr

    def refused(rc, code):
        assert rc == code, (rc, code, L.svae_last_error())
        assert L.svae_last_error().decode().strip(), "svae_last_error() is empty"

    with torch.cuda.device(dev):
        # the forward calls get buffers of their own; the backward calls the `saved` the forward of test 1 really wrote
        for off_saved, off_ws, nbytes in ((0, 0, f.ws_bytes - 1), (0, 128, f.ws_bytes), (128, 0, f.ws_bytes)):
            refused(L.svae_decoder_forward(d, p, pose, f.z, y.ptr, lg.ptr, saved.ptr + off_saved, ws.ptr + off_ws, nbytes, st),
                    _lib.E_WORKSPACE)
            pg = _lib.PoseGrads()
            pg.dcoords = sinks["dcoords"].ptr
            refused(L.svae_decoder_backward(d, p, pose, f.z, f.bufs["logits"].ptr, f.tens["dy"].data_ptr(), None,
                                            f.saved.ptr + off_saved, ctypes.byref(grads), sinks["dz"].ptr, ctypes.byref(pg),
                                            ws.ptr + off_ws, nbytes, st), _lib.E_WORKSPACE)
        pg = _lib.PoseGrads()
        pg.dtheta = sinks["dtheta"].ptr
        refused(L.svae_decoder_backward(d, p, pose, f.z, f.bufs["logits"].ptr, f.tens["dy"].data_ptr(), None, f.saved.ptr,
                                        ctypes.byref(grads), sinks["dz"].ptr, ctypes.byref(pg), f.ws.ptr, f.ws_bytes, st),
                _lib.E_INVALID)
    torch.cuda.synchronize()
    for k, buf in dict(sinks, y=y, logits=lg).items():
        a, intact = buf.read(-1)
        assert intact and A.sentinel_hits(a) == a.size, "%s was written by a refused call" % k
    for buf in (saved, ws):
        a, intact = buf.read()
        assert intact and not a.any()


# ---------------------------------------------------------------------------------------------------------------------
# 9: the same file in fp16x3 mode
# ---------------------------------------------------------------------------------------------------------------------
def test_the_file_passes_in_fp16x3_mode():
    """One fresh process (the mode is read once per process) runs this file under SVAE_GEMM=fp16x3 with the bounds unchanged:
    the mode claims fp32 accuracy.  The child deselects this test."""
    me = "tests/test_gpu_decoder_abi.py"
    env = dict(os.environ, SVAE_GEMM="fp16x3")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", me, "--deselect",
                          me + "::test_the_file_passes_in_fp16x3_mode"], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail


def test_the_child_mode_is_what_the_environment_asks():
    """Guards test 9 against a child that silently ran in fp32 mode."""
    if os.environ.get("SVAE_GEMM") == "fp16x3":
        assert _fp16x3()
