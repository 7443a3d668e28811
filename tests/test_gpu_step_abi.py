"""The entry points of the training step that are not the decoder, called straight through the C ABI (tests/step_abi.py) and
held to include/svae.h: svae_linear_forward / _backward, svae_adam_step, svae_grad_guard_norm, svae_adam_step_guarded,
svae_rotate_bicubic and svae_ctf_filter.  Raw calls through _lib.lib() on the current torch stream; every operand has exactly
its advertised size and sits between guard words inside a larger allocation (NaN around inputs, 0xA5A5A5A5 around outputs,
outputs prefilled with a NaN of their own), so a read or a write a few elements out of bounds is seen and does not fault.

  values        against float64 references written out in numpy (step_abi.layer, adam_reference, norm_reference) and the
                oracles of the rotation and the CTF bank;
  containment   no guard word changes, every element of an output is overwritten, everything is finite;
  selection     the encoder's float4 kernels run only on 16-byte-aligned operands whose contracted dimension is a multiple of
                4: the misaligned forms run the scalar kernels, agree with each other bit for bit and differ from the aligned
                result in the last bits;
  NULLs         every subset of (dweight, dbias, dx), bias, and `out` without an activation;
  refusals      leave every buffer as it was.

Encoder shapes (M, K, N), the smallest that reach each branch: (1, 1, 1) the minimum of every dimension; (3, 37, 10) the scalar
kernels with all dimensions ragged; (16, 16, 16) exact tiles; (17, 36, 20) the vector kernels with K % 16 == 4 and N % 16 == 4,
one k-group per wave or none; (33, 520, 24) vector forward with 33 k-groups, 9 per wave, a second loop trip of one group;
(20, 258, 7) scalar forward with 65 k-steps, 17 per wave, a second trip; (260, 44, 264) role W with 65 row-steps and role X
vector with 17 n-groups, 5 per wave, second trips both; (5, 260, 262) role X scalar with 66 n-steps and a vector forward with
K % 16 == 4.

The whole file (131 tests) takes about 1.5 s on the MI355X."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import step_abi as S
from step_abi import Guarded

pytestmark = pytest.mark.gpu
TOL_CTF = 2e-6          # tests/test_gpu_ctf.py's TOL: doubles inside, one fp32 rounding at the end
FWD_OFFSETS = [(4, 0), (0, 8), (12, 12)]          # (x, weight) byte offsets past a 256-byte boundary
BWD_OFFSETS = [(4, 0), (0, 8)]                    # (dout, out)
SWITCH_FWD, SWITCH_DX = (33, 520, 24), (260, 44, 264)


def _lib():
    from spatial_vae_amd import _lib as B
    return B


def _refused(r, code):
    assert r["rc"] == code, (r["rc"], code, r["err"])
    assert r["err"].strip(), "svae_last_error() is empty"


def _shape(c):
    return (c["M"], c["K"], c["N"])


# ---------------------------------------------------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd(name, off_x=0, off_w=0, bias=True):
    c = S.enc_case(name)
    r = S.linear_forward(S.enc_inputs(name), c["act"], off_x, off_w, bias=bias)
    _lib().check(r["rc"])
    return r


@functools.lru_cache(maxsize=None)
def _bwd(name, off_dout=0, off_out=0, sinks=S.SINKS):
    c = S.enc_case(name)
    r = S.linear_backward(S.enc_inputs(name), S.enc_out32(name), c["act"], sinks=sinks, off_dout=off_dout, off_out=off_out)
    _lib().check(r["rc"])
    return r


def _contained(name, r, keys, tag=""):
    assert not r["bad"], "%s%s: touched outside %s" % (name, tag, r["bad"])
    for k in keys:
        assert S.unwritten(r[k]) == 0, "%s%s: %d entries of %s were never written" % (name, tag, S.unwritten(r[k]), k)
        assert np.isfinite(r[k]).all(), (name, tag, k)


@pytest.mark.parametrize("name", S.ENC_NAMES)
def test_encoder_values_and_containment(name):
    """One forward and one backward call (all three sinks, `out` = the float64 reference's output rounded to fp32) per case,
    16-byte-aligned operands.  out, dW, db and dx within min(5e-6, max(4 e32, 16 u, 2 sqrt(Kc) u)) of the float64 reference,
    relative to its largest entry (for the `out` of tanh and sigmoid the 16 u floor is divided by max |ref|, under the same
    cap: step_abi.enc_bounds says why; it changes the bound of the two single-output cases only); no
    guard word of any buffer changed, no output element left as prefilled, everything finite although every input guard holds
    NaN.  Lattice cases: `out` equals the exact value bit for bit.  Saturation cases: `out` is exactly +-1 (tanh) or 0 / 1
    (sigmoid) wherever the float64 value rounds to that.
    MI355X maxima over every call of this file (error, share of its bound): out 8.1e-7, 0.30 (33x520x24_tanh); dW 2.4e-7, 0.16
    and db 3.8e-7, 0.15 (17x36x20_sigmoid_saturate); dx 4.0e-7, 0.16 (the same case with dout at +4 bytes).  The one output of
    1x1x1_tanh, 0.0279, is off by 3.9e-8 = 1.4e-6 of itself, past the 16 u floor and 0.28 of its bound, which is the 5e-6 cap."""
    c = S.enc_case(name)
    f, b = _fwd(name), _bwd(name)
    _contained(name, f, ["out"])
    _contained(name, b, S.SINKS)
    bad = S.enc_violations(name, dict(out=f["out"], dw=b["dw"], db=b["db"], dx=b["dx"]))
    assert not bad, (name, bad)
    if c["kind"] == "lattice":
        want = S.enc_exact_out32(name)
        same = f["out"].view(np.uint32) == want.view(np.uint32)
        assert same.all(), "%s: out differs from the exact value in %d entries" % (name, int((~same).sum()))
    if c["kind"] == "saturate":
        want = S.enc_out32(name)
        ends = (np.abs(want) == 1.0) if c["act"] == "tanh" else ((want == 0.0) | (want == 1.0))
        assert ends.sum() > 100 and (f["out"][ends] == want[ends]).all(), (name, int((f["out"][ends] != want[ends]).sum()))


FWD_ALIGN = [n for n in S.ENC_NAMES if S.enc_case(n)["K"] % 4 == 0]
BWD_ALIGN = [n for n in S.ENC_NAMES if S.enc_case(n)["N"] % 4 == 0]


@pytest.mark.parametrize("name", FWD_ALIGN)
def test_forward_alignment_forms(name):
    """Every K % 4 == 0 case again with x at +4 bytes, with weight at +8 bytes and with both at +12 bytes: each is accepted,
    contained and inside the bound of the aligned call; the three agree bit for bit (one scalar kernel, one order), and so do
    two aligned calls.  At (33, 520, 24) the aligned result differs from the misaligned one in at least one bit: the float4
    kernel contracts k in another order, which is the only evidence from outside that alignment selects the kernel.
    MI355X: they differ, in 450 of 792 entries (tanh) and 675 of 792 (LeakyReLU), and the difference is asserted; the exact cases
    (lattice, grid, saturation) coincide, as they must."""
    c = S.enc_case(name)
    base = _fwd(name)
    again = S.linear_forward(S.enc_inputs(name), c["act"])
    assert again["rc"] == 0 and S.bit_equal(again["out"], base["out"]), name
    forms = []
    for ox, ow in FWD_OFFSETS:
        r = _fwd(name, ox, ow)
        _contained(name, r, ["out"], " x+%d w+%d" % (ox, ow))
        assert not S.enc_violations(name, dict(out=r["out"]), tag=" x+%d w+%d" % (ox, ow)), (name, ox, ow)
        forms.append(r["out"])
    assert S.bit_equal(forms[0], forms[1]) and S.bit_equal(forms[0], forms[2]), name
    differ = int((forms[0].view(np.uint32) != base["out"].view(np.uint32)).sum())
    print("step_abi enc %s forward: aligned and misaligned differ in %d of %d entries" % (name, differ, base["out"].size))
    if _shape(c) == SWITCH_FWD:
        assert differ > 0, name


@pytest.mark.parametrize("name", BWD_ALIGN)
def test_backward_alignment_forms(name):
    """Every N % 4 == 0 case again with dout at +4 bytes and with out at +8 bytes: accepted, contained, inside the bounds, the
    two bit-equal to each other in dW, db and dx, and two aligned calls bit-equal.  At (260, 44, 264) the aligned dx differs
    from the misaligned one in at least one bit (role X reads n as float4 only when aligned).
    MI355X: they differ, in 9541 of 11440 entries (tanh) and 9492 of 11440 (LeakyReLU on the grid draw), and the difference is
    asserted."""
    c = S.enc_case(name)
    base = _bwd(name)
    again = S.linear_backward(S.enc_inputs(name), S.enc_out32(name), c["act"])
    assert again["rc"] == 0 and all(S.bit_equal(again[k], base[k]) for k in S.SINKS), name
    forms = []
    for od, oo in BWD_OFFSETS:
        r = _bwd(name, od, oo)
        _contained(name, r, S.SINKS, " dout+%d out+%d" % (od, oo))
        assert not S.enc_violations(name, {k: r[k] for k in S.SINKS}, tag=" dout+%d out+%d" % (od, oo)), (name, od, oo)
        forms.append(r)
    assert all(S.bit_equal(forms[0][k], forms[1][k]) for k in S.SINKS), name
    differ = int((forms[0]["dx"].view(np.uint32) != base["dx"].view(np.uint32)).sum())
    print("step_abi enc %s backward: aligned and misaligned dx differ in %d of %d entries" % (name, differ, base["dx"].size))
    if _shape(c) == SWITCH_DX:
        assert differ > 0, name


SUBSET_CASES = ["17x36x20_tanh", "17x36x20_relu", "3x37x10_tanh", "3x37x10_none", "17x36x20_leakyrelu_lattice"]
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(S.SINKS, k)]


@pytest.mark.parametrize("name", SUBSET_CASES)
def test_null_subsets_of_the_sinks(name):
    """All seven non-empty subsets of (dweight, dbias, dx): each present output is bit-equal to the all-three call's (db without
    dW runs role W and skips the store; dx alone runs with no role-W workgroup), an absent output's buffer is still all prefill
    and no guard changes.  All three NULL: SVAE_OK, nothing touched."""
    c = S.enc_case(name)
    assert len(SUBSETS) == 7
    full = _bwd(name)
    for sinks in SUBSETS:
        r = _bwd(name, sinks=sinks)
        assert not r["bad"], (name, sinks, r["bad"])
        for k in S.SINKS:
            if k in sinks:
                assert S.bit_equal(r[k], full[k]), (name, sinks, k)
            else:
                assert S.unwritten(r[k]) == r[k].size, "%s %s: absent %s was written" % (name, sinks, k)
    r = S.linear_backward(S.enc_inputs(name), S.enc_out32(name), c["act"], sinks=())
    assert r["rc"] == 0 and not r["bad"] and all(S.unwritten(r[k]) == r[k].size for k in S.SINKS), name


@pytest.mark.parametrize("name", ["17x36x20_tanh", "3x37x10_relu", "1x1x1_sigmoid", "33x520x24_leakyrelu"])
def test_forward_without_bias(name):
    """bias == NULL against the float64 reference without the bias term, same bound rule."""
    r = _fwd(name, bias=False)
    _contained(name, r, ["out"], " no bias")
    assert not S.enc_violations(name, dict(out=r["out"]), bias=False, tag=" no bias"), name


@pytest.mark.parametrize("name", ["3x37x10_none", "17x36x20_none_lattice", "16x16x16_none"])
def test_backward_without_out_when_there_is_no_activation(name):
    """out == NULL with SVAE_LINEAR_ACT_NONE: bit-equal to the call that is given `out`."""
    r = S.linear_backward(S.enc_inputs(name), S.enc_out32(name), None, out_null=True)
    assert r["rc"] == 0, r["err"]
    _contained(name, r, S.SINKS, " out NULL")
    assert all(S.bit_equal(r[k], _bwd(name)[k]) for k in S.SINKS), name


def test_encoder_refusals_touch_nothing():
    """rows, in_features or out_features < 1, an unknown activation (4, -2) and out == NULL with an activation: SVAE_E_INVALID
    with a message from both entry points, and every output buffer is still what it was prefilled with."""
    B = _lib()
    name = "3x37x10_tanh"
    inp, out32 = S.enc_inputs(name), S.enc_out32(name)
    M, K, N = 3, 37, 10
    for dims in ((0, K, N), (M, 0, N), (M, K, 0), (-1, K, N)):
        f = S.linear_forward(inp, "tanh", dims=dims)
        b = S.linear_backward(inp, out32, "tanh", dims=dims)
        for r, keys in ((f, ["out"]), (b, S.SINKS)):
            _refused(r, B.E_INVALID)
            assert not r["bad"] and all(S.unwritten(r[k]) == r[k].size for k in keys), dims
    for code in (4, -2):
        f = S.linear_forward(inp, None, act_code=code)
        b = S.linear_backward(inp, out32, None, act_code=code)
        for r, keys in ((f, ["out"]), (b, S.SINKS)):
            _refused(r, B.E_INVALID)
            assert not r["bad"] and all(S.unwritten(r[k]) == r[k].size for k in keys), code
    for act in ("tanh", "relu"):
        b = S.linear_backward(inp, out32, act, out_null=True)
        _refused(b, B.E_INVALID)
        assert not b["bad"] and all(S.unwritten(b[k]) == b[k].size for k in S.SINKS), act
    f = S.linear_forward(inp, "tanh", out_null=True)
    _refused(f, B.E_INVALID)


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def _adam_checked(inp, r, ref, bound, zero_grad, tag):
    assert r["rc"] == 0, r["err"]
    assert not r["bad"], "%s: written outside %s" % (tag, r["bad"])
    bad = S.adam_violations(r, ref, bound, tag)
    assert not bad, (tag, bad)
    if zero_grad:
        assert (r["g"].view(np.uint32) == 0).all(), "%s: grad is not all +0.0" % tag
    else:
        assert S.bit_equal(r["g"], inp["g"]), "%s: grad changed" % tag


@pytest.mark.parametrize("zero_grad", [1, 0])
@pytest.mark.parametrize("n", S.ADAM_LENGTHS)
def test_adam_lengths(n, zero_grad):
    """svae_adam_step at the default hyper-parameters, step 1, over lengths that are a scalar tail alone (1, 2, 3), one vector
    (4), a vector and a tail (5), either side of the 1024-element block (1023 .. 1027) and many blocks with a tail (262147);
    the first elements are step_abi.ADAM_EDGES.  Per element against float64: m within 4u (|b1 m| + |(1 - b1) g|), v within
    4u (|b2 v| + |(1 - b2) g^2|), p within 2 spacing(p) + 16u |update| (each plus 2^-149, the fp32 spacing below the normal
    range); the overflow elements give v = +inf and leave p alone.  zero_grad = 1 leaves grad all +0.0, tail included;
    zero_grad = 0 leaves it bit-identical.  Guards of all four buffers (16-byte-aligned start, end wherever n puts it) intact.
    MI355X maxima (share of the bound): p 0.25 (n = 1023), m 0.46 and v 0.52 (n = 262147).  The one widening of the issue's
    formulas is the 2^-149 on m and v, the rounding of a stored moment onto the denormal grid (step_abi.adam_reference)."""
    D = S.ADAM_DEFAULT
    inp = S.adam_inputs(n)
    ss, bc = S.adam_scalars(D["lr"], D["b1"], D["b2"], D["step"])
    ref, bound = S.adam_reference(inp, D["b1"], D["b2"], D["eps"], ss, bc)
    r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], D["step"], zero_grad)
    _adam_checked(inp, r, ref, bound, zero_grad, " n=%d zero_grad=%d" % (n, zero_grad))


@pytest.mark.parametrize("step", S.ADAM_STEPS)
def test_adam_parameter_sweep(step):
    """n = 1027 with step in {1, 2, 1000000} x betas in {(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)} x eps in {1e-8, 1e-3}: the same
    bounds.  MI355X maxima (share of the bound): p 0.25, m 0.25, v 0.36."""
    inp = S.adam_inputs(S.ADAM_SWEEP_N)
    for (b1, b2), eps in itertools.product(S.ADAM_BETAS, S.ADAM_EPS):
        ss, bc = S.adam_scalars(1e-3, b1, b2, step)
        ref, bound = S.adam_reference(inp, b1, b2, eps, ss, bc)
        r = S.adam_call(inp, 1e-3, b1, b2, eps, step, 1)
        _adam_checked(inp, r, ref, bound, 1, " step=%d betas=(%g, %g) eps=%g" % (step, b1, b2, eps))


@pytest.mark.parametrize("n", [5, 1027])
def test_adam_guarded_with_control_records_written_by_the_test(n):
    """svae_adam_step_guarded reading records built on the host, which svae_grad_guard_norm would not produce:
    apply = 1, coef = 1 with step 7's step_size and sqrt_bc2: bit-equal to svae_adam_step(step = 7);
    coef = 0.25: the float64 reference on fp32(0.25 g), the bounds of test_adam_lengths;
    apply = 0, zero_grad = 0: all four buffers bit-identical;  apply = 0, zero_grad = 1: only grad changes, to +0.0.
    MI355X: bit-equal and bit-identical where demanded; coef = 0.25 at most p 0.25, m 0.25, v 0.28 of the bounds."""
    D = S.ADAM_DEFAULT
    inp = S.adam_inputs(n)
    ss, bc = S.adam_scalars(D["lr"], D["b1"], D["b2"], 7)
    plain = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], 7, 1)
    assert plain["rc"] == 0 and not plain["bad"]
    r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], 0, 1, control=S.control_bytes(1, 1.0, ss, bc))
    assert r["rc"] == 0 and not r["bad"], (r["err"], r["bad"])
    assert all(S.bit_equal(r[k], plain[k]) for k in "pgmv"), n
    ref, bound = S.adam_reference(inp, D["b1"], D["b2"], D["eps"], ss, bc, coef=0.25)
    r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], 0, 0, control=S.control_bytes(1, 0.25, ss, bc))
    _adam_checked(inp, r, ref, bound, 0, " guarded n=%d coef=0.25" % n)
    r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], 0, 0, control=S.control_bytes(0, 0.25, ss, bc))
    assert r["rc"] == 0 and not r["bad"] and all(S.bit_equal(r[k], inp[k]) for k in "pgmv"), n
    r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], 0, 1, control=S.control_bytes(0, 0.25, ss, bc))
    assert r["rc"] == 0 and not r["bad"] and all(S.bit_equal(r[k], inp[k]) for k in "pmv"), n
    assert (r["g"].view(np.uint32) == 0).all(), n


def test_adam_refusals_write_nothing():
    """A parameter pointer at +4 bytes, n = 0, step = 0 and (guarded) a NULL control: SVAE_E_INVALID, all four buffers as they
    were."""
    B = _lib()
    D = S.ADAM_DEFAULT
    inp = S.adam_inputs(1027)
    ss, bc = S.adam_scalars(D["lr"], D["b1"], D["b2"], 1)
    ok = S.control_bytes(1, 1.0, ss, bc)
    calls = [dict(step=1, off_p=4), dict(step=1, n=0), dict(step=0), dict(step=1, control=ok, off_p=4), dict(step=1, control=ok, n=0),
             dict(step=1, control="null")]
    for kw in calls:
        r = S.adam_call(inp, D["lr"], D["b1"], D["b2"], D["eps"], kw.pop("step"), 1, **kw)
        _refused(r, B.E_INVALID)
        assert not r["bad"] and all(S.bit_equal(r[k], inp[k]) for k in "pgmv"), kw


# ---------------------------------------------------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------------------------------------------------
def _norm_call(g, n, max_norm=float("inf"), ws=None, ws_bytes=None, control=None):
    B = _lib()
    L = B.lib()
    need = L.svae_grad_guard_workspace_bytes(n)
    ws = Guarded(need // 4) if ws is None else ws
    control = Guarded(18, 0, "out", np.zeros(72, np.uint8)) if control is None else control
    with torch.cuda.device(S.dev()):
        rc = L.svae_grad_guard_norm(g, n, max_norm, 1e-3, 0.9, 0.999, control.ptr, ws.ptr, need if ws_bytes is None else ws_bytes,
                                    S.stream())
    torch.cuda.synchronize()
    raw, ch_c = control.read(np.uint8)
    rec = B.GuardControl()
    ctypes.memmove(ctypes.byref(rec), raw.tobytes(), ctypes.sizeof(rec))
    ch_w = ws.read()[1]
    return dict(rc=rc, rec=rec, raw=raw, bad=(["control"] if ch_c else []) + (["ws"] if ch_w else []),
                err=L.svae_last_error().decode() if rc else "")


@pytest.mark.parametrize("n", S.NORM_LENGTHS)
def test_norm_where_the_chunk_doubles(n):
    """n = 4096^2 - 3 and 4096^2 keep chunks of 4096 floats (4096 of them, 16 per lane of the control kernel); 4096^2 + 1 and + 5
    double the chunk to 8192, run grad_sumsq_kernel's four-in-flight loop a second trip and end in a chunk of 1 element (a scalar
    tail alone) or 5 (one vector and a scalar).  svae_grad_guard_workspace_bytes is ceil(n / chunk) * 8; total within 4 fp32
    spacings of the float64 norm of the host copy (the bar of test_norm_matches_float64_and_is_reproducible); two calls
    bit-equal; the guards of a workspace of exactly the advertised bytes (prefilled with NaN) and of the control record intact.
    The floats behind grad[n - 1] are NaN: a lane reading past the end would make the norm NaN.
    MI355X: at most 0.21 spacings (n = 4096^2 + 1); each case takes 0.05 s."""
    L = _lib().lib()
    chunk = S.norm_chunk(n)
    assert chunk == (4096 if n <= S.NORM_BASE else 8192)
    need = L.svae_grad_guard_workspace_bytes(n)
    assert need == -(-n // chunk) * 8
    gen = torch.Generator(device=S.dev()).manual_seed(n % 1000)
    g = torch.randn(n + 1024, generator=gen, device=S.dev())
    g[n:] = float("nan")
    assert g.data_ptr() % 16 == 0
    want = S.norm_reference(g[:n].cpu().numpy())
    a = _norm_call(g.data_ptr(), n)
    b = _norm_call(g.data_ptr(), n)
    for r in (a, b):
        assert r["rc"] == 0, r["err"]
        assert not r["bad"], r["bad"]
    spacings = abs(float(a["rec"].total) - want) / float(np.spacing(np.float32(want)))
    print("step_abi norm n=%d chunk %d: total %.9g float64 %.17g, %.2f spacings" % (n, chunk, a["rec"].total, want, spacings))
    assert spacings <= 4.0
    assert a["rec"].finite == 1 and a["rec"].apply == 1 and a["rec"].t == 1 and a["rec"].coef == 1.0
    assert np.array_equal(a["raw"], b["raw"])


def test_norm_refusals_leave_the_control_record():
    """ws_bytes one short and ws at +16 bytes (not 256-byte aligned): SVAE_E_WORKSPACE; grad at +4 bytes and max_norm = 0:
    SVAE_E_INVALID.  The control record (prefilled with a pattern) and its guards are untouched."""
    B = _lib()
    n = 4099
    need = B.lib().svae_grad_guard_workspace_bytes(n)
    assert need == 16
    g = torch.ones(n + 4, device=S.dev())
    pattern = np.arange(72, dtype=np.uint8)
    cases = [(dict(ws_bytes=need - 1), B.E_WORKSPACE), (dict(ws=Guarded(need // 4, 16)), B.E_WORKSPACE),
             (dict(max_norm=0.0), B.E_INVALID)]
    for kw, code in cases:
        r = _norm_call(g.data_ptr(), n, control=Guarded(18, 0, "out", pattern), **kw)
        _refused(r, code)
        assert not r["bad"] and np.array_equal(r["raw"], pattern), kw
    r = _norm_call(g.data_ptr() + 4, n, control=Guarded(18, 0, "out", pattern))
    _refused(r, B.E_INVALID)
    assert not r["bad"] and np.array_equal(r["raw"], pattern)


# ---------------------------------------------------------------------------------------------------------------------
# rotation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", S.ROT_SHAPES, ids=["x".join(map(str, s)) for s in S.ROT_SHAPES])
def test_rotation_of_non_square_and_tiny_images_equals_the_oracle(shape, u8):
    """ops.rotate_augment against oracle.pil_rotate image by image, bit for bit: rows != cols in both orientations, one to four
    channels, images smaller than the 4 x 4 bicubic window (1 x 1, 2 x 3, 3 x 2) and a 5 x 40 strip; 12 angles: 0, pi/2, pi,
    3 pi/2, 2 pi, pi/4 and six random ones.  On a non-square image the quarter turns at 90 and 270 degrees go through the
    matrix (tests/test_step_abi_cpu.py pins that choice of the host).  MI355X: equal in all twelve runs."""
    from spatial_vae_amd import ops
    rows, cols, C = shape
    y, off = S.rot_images(shape, u8), S.rot_offsets(shape)
    want = S.rot_oracle(y, off, shape, u8)
    got = ops.rotate_augment(torch.from_numpy(y).to(S.dev()), off, rows, cols, quantize_u8=u8).cpu().numpy()
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), "%s: %d of %d samples differ, first in image %d" % (shape, int((~same).sum()), same.size, np.argwhere(~same)[0][0])


def _rotate_raw(y, matrix, quarter, B, rows, cols, C, u8, alias=False, null_matrix=False):
    L = _lib().lib()
    src = Guarded(y.size, 0, "in", y)
    dst = Guarded(y.size)
    mat = Guarded(matrix.size * 2, 0, "in", matrix)
    q = Guarded(quarter.size, 0, "in", quarter)
    with torch.cuda.device(S.dev()):
        rc = L.svae_rotate_bicubic(src.ptr, src.ptr if alias else dst.ptr, None if null_matrix else mat.ptr, q.ptr, B, rows, cols, C,
                                   1 if u8 else 0, S.stream())
    torch.cuda.synchronize()
    out, ch = dst.read(np.float32, y.shape)
    bad = (["y_rot"] if ch else []) + [nm for nm, b in (("y", src), ("matrix", mat), ("quarter", q)) if b.read()[1]]
    return dict(rc=rc, out=out, src=src.read(np.float32, y.shape)[0], bad=bad, err=L.svae_last_error().decode() if rc else "")


def test_rotation_raw_call_is_contained_and_refusals_touch_nothing():
    """One raw call on a 9 x 14 single-channel batch with quarter codes [-1, 0, 2] (codes 1 and 3 require a square image and are
    never sent otherwise): equal to the oracle, guards of y_rot and of the inputs unchanged, every element written.
    y == y_rot, a zero dimension and a NULL matrix: SVAE_E_INVALID and the output (and the aliased input) untouched."""
    from spatial_vae_amd import ops
    B = _lib()
    shape = (9, 14, 1)
    rows, cols, C = shape
    y = S.rot_images(shape, False)[:3]
    off = np.array([0.7, 0.0, np.pi])
    matrix, quarter = ops.rotation_matrices(off, rows, cols)
    assert quarter.tolist() == [-1, 0, 2]
    r = _rotate_raw(y, matrix, quarter, 3, rows, cols, C, False)
    assert r["rc"] == 0, r["err"]
    assert not r["bad"] and S.unwritten(r["out"]) == 0, r["bad"]
    assert S.bit_equal(r["out"], S.rot_oracle(y, off, shape, False))
    for kw, dims in ((dict(alias=True), (3, rows, cols, C)), (dict(), (3, 0, cols, C)), (dict(), (3, rows, 0, C)),
                     (dict(), (0, rows, cols, C)), (dict(), (3, rows, cols, 0)), (dict(null_matrix=True), (3, rows, cols, C))):
        r = _rotate_raw(y, matrix, quarter, *dims, False, **kw)
        _refused(r, B.E_INVALID)
        assert not r["bad"] and S.unwritten(r["out"]) == r["out"].size and S.bit_equal(r["src"], y), (kw, dims)


# ---------------------------------------------------------------------------------------------------------------------
# CTF bank
# ---------------------------------------------------------------------------------------------------------------------
def _ctf_oracle(tab, n, m, scale):
    from oracle import ctf_oracle as C
    return C.ctf_filter({k: tab[:, i] for i, k in enumerate(C.COLUMNS)}, n, m, scale=scale)


def _ctf_raw(tab, n, m, scale, ws_bits):
    L = _lib().lib()
    P = tab.shape[0]
    need = L.svae_ctf_filter_workspace_bytes(P, n, m)
    params = Guarded(tab.size * 2, 0, "in", tab)
    filters = Guarded(P * n * m)
    ws = Guarded(need // 4).fill_bits(ws_bits)
    with torch.cuda.device(S.dev()):
        rc = L.svae_ctf_filter(params.ptr, filters.ptr, P, n, m, scale, ws.ptr, need, S.stream())
    torch.cuda.synchronize()
    out, ch = filters.read(np.float32, (P, n, m))
    bad = (["filters"] if ch else []) + (["ws"] if ws.read()[1] else []) + (["params"] if params.read()[1] else [])
    return dict(rc=rc, out=out, bad=bad, need=need, err=L.svae_last_error().decode() if rc else "")


@pytest.mark.parametrize("n,m", S.CTF_SMALL)
def test_ctf_bank_below_nine_by_nine(n, m):
    """(1, 1), (1, 5), (2, 2) and (3, 8) filters of three particles against oracle.ctf_oracle.ctf_filter at the 2e-6 of
    tests/test_gpu_ctf.py, through a raw guarded call.  MI355X: every tap equal to the oracle's."""
    tab = S.ctf_table(S.CTF_COUNT, 10 * n + m)
    want = _ctf_oracle(tab, n, m, 1.5)
    r = _ctf_raw(tab, n, m, 1.5, S.NAN_BITS)
    assert r["rc"] == 0, r["err"]
    assert not r["bad"] and S.unwritten(r["out"]) == 0 and np.isfinite(r["out"]).all(), r["bad"]
    e = S.rel_err(r["out"], want)
    print("step_abi ctf %dx%d err %.3e of %.1e" % (n, m, e, TOL_CTF))
    assert e < TOL_CTF


@pytest.mark.parametrize("n,m", S.CTF_GUARDED)
def test_ctf_bank_is_contained_and_its_workspace_is_scratch(n, m):
    """39 x 39 and 81 x 81 (the planes in LDS, workspace size 0: 24 n m + 16 (n + m) bytes still fit the 160 KiB at 81, the
    largest square that does) and 82 x 82 (the first with the planes in a workspace, of exactly
    svae_ctf_filter_workspace_bytes): the guards of `filters` and of `ws` are unchanged, every tap is written, the values agree
    with the oracle to 2e-6, and the result with `ws` prefilled with NaN is bit-equal to the result with `ws` zeroed.
    MI355X: holds at all three sizes."""
    tab = S.ctf_table(S.CTF_COUNT, 10 * n + m)
    a, b = _ctf_raw(tab, n, m, 1.5, S.NAN_BITS), _ctf_raw(tab, n, m, 1.5, 0)
    assert (a["need"] == 0) == (24 * n * m + 16 * (n + m) <= 160 * 1024) == (n < 82)
    assert a["need"] in (0, S.CTF_COUNT * 3 * 8 * n * m)
    for r in (a, b):
        assert r["rc"] == 0, r["err"]
        assert not r["bad"] and S.unwritten(r["out"]) == 0 and np.isfinite(r["out"]).all(), r["bad"]
    assert S.bit_equal(a["out"], b["out"])
    e = S.rel_err(a["out"], _ctf_oracle(tab, n, m, 1.5))
    print("step_abi ctf %dx%d err %.3e of %.1e, workspace %d bytes" % (n, m, e, TOL_CTF, a["need"]))
    assert e < TOL_CTF
