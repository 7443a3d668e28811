"""dtheta / ddx of svae_decoder_backward when d(coords) itself is not requested: the data-gradient GEMM's FIRST epilogue then
leaves out the per-row d(coords) partials, and the role-0 blocks of the per-image launch form both pose gradients from the
per-image sums (G0, G1, S) -- tests/test_pose_identity_cpu.py has the algebra.  Driven through the C ABI with the guarded
buffers of tests/decoder_abi.py and held to float64 (oracle.torch_cpu_step.decoder) with the bound of
tests/test_gpu_decoder_abi.py for the pose sinks: max(4 * e32, 16 * 2^-24), e32 the error of the same decoder in float32 on
the CPU, never above 1e-4.

Per case ONE forward call and three backward calls from it: "old" requests dcoords besides dtheta / ddx (a grid pose with
dcoords: the epilogue with the per-row partials, the role-1 blocks), "new" twice without dcoords.  Checked:
  * dtheta, ddx of both routes against float64, and against each other within the same bound;
  * every other output (parameter gradients, dz) bit-equal between the routes: the epilogue form without d(coords) and the
    folded dW_o / db_o reduction change nothing else;
  * the two new-route calls bit-equal (fixed summation order, no atomics);
  * all guard bytes intact, nothing left at the sentinel.

Cases: the smallest shapes at which each route can go wrong.  n = 28 (784 rows pad to 800: 25 tiles per image), H = 500 (pads to
512), B = 4: Mp = 3200 = 25 row groups, dense4_kernel<1>; B = 3: Mp = 2400 is not whole row groups, dense_kernel's FIRST epilogue
(it still writes the partials, nobody reads them); n = 8, B = 20, H = 64 with SVAE_DENSE4=2 and SVAE_DENSE4_TAIL==1: both block
widths in one dense4_dual_kernel launch; at that shape the sigmoid (LASTD 3) and two-channel (LASTD 0, streamed output
backward) forms, three layers, rotate only, translate only, no latent, the bilinear table, the default dispatch
(dense4_kernel<1>) of the three LASTD forms, and the two unbounded activations (each its own instance of the epilogue).  One case is repeated in a child process in fp16x3 mode.

MI355X maxima: in the docstring of test_pose_gradients_from_sums."""
import ctypes
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import rel_err

# a private instance of tests/decoder_abi.py: its case table is looked up by name (inputs and references are seeded by the
# name), and the cases added below must not show up in the table the other test files check
_spec = importlib.util.spec_from_file_location("decoder_abi_pose_from_sums",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "decoder_abi.py"))
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)
U = A.U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_CAP = 1e-4
FLOOR_GRAD = 16 * U

DUAL = {"SVAE_DENSE4": "2", "SVAE_DENSE4_TAIL": "=1"}
#        name                N    B   H    L  C  Zd in act        flags          pose              environment
TABLE = [("pfs_n28_b4", 784, 4, 500, 2, 1, 2, 2, "tanh", (), "grid+theta+dx", {}),
         ("pfs_n28_b3", 784, 3, 500, 2, 1, 2, 2, "tanh", (), "grid+theta+dx", {}),
         ("pfs_dual_tanh", 64, 20, 64, 2, 1, 2, 2, "tanh", (), "grid+theta+dx", DUAL),
         ("pfs_dual_sigmoid", 64, 20, 64, 2, 1, 2, 2, "sigmoid", (), "grid+theta+dx", DUAL),
         ("pfs_dual_c2", 64, 20, 64, 2, 2, 2, 2, "tanh", (), "grid+theta+dx", DUAL),
         ("pfs_dual_L3", 64, 20, 64, 3, 1, 2, 2, "tanh", (), "grid+theta+dx", DUAL),
         ("pfs_dual_rotate", 64, 20, 64, 2, 1, 2, 2, "tanh", (), "grid+theta", DUAL),
         ("pfs_dual_translate", 64, 20, 64, 2, 1, 2, 2, "tanh", (), "grid+dx", DUAL),
         ("pfs_dual_z0", 64, 20, 64, 2, 1, 0, 2, "tanh", (), "grid+theta+dx", DUAL),
         ("pfs_dual_bilinear", 64, 20, 64, 2, 1, 2, 2, "tanh", ("bilinear",), "grid+theta+dx", DUAL),
         ("pfs_nt1_tanh", 64, 20, 64, 2, 1, 2, 2, "tanh", (), "grid+theta+dx", {}),
         ("pfs_nt1_sigmoid", 64, 20, 64, 2, 1, 2, 2, "sigmoid", (), "grid+theta+dx", {}),
         ("pfs_nt1_c2", 64, 20, 64, 2, 2, 2, 2, "tanh", (), "grid+theta+dx", {}),
         ("pfs_nt1_relu", 64, 20, 64, 2, 1, 2, 2, "relu", (), "grid+theta+dx", {}),
         ("pfs_dual_leaky", 64, 20, 64, 2, 1, 2, 2, "leakyrelu", (), "grid+theta+dx", DUAL)]
ENV = {t[0]: t[-1] for t in TABLE}
for _t in TABLE:
    assert _t[0] not in A.BY_NAME
    A.BY_NAME[_t[0]] = dict(zip(A.FIELDS, _t[:-1]))
NAMES = [t[0] for t in TABLE]
FP16X3_CASE = "pfs_dual_tanh"


def _backward(f, sinks):
    """Forward.backward of tests/decoder_abi.py, but `sinks` may hold dcoords although the pose is a grid."""
    c, dev, lib = f.c, f.dev, f._lib
    bufs = {nm: A.Guarded(4 * int(np.prod(A._shape(c, nm))), dev).fill_float(A.SENTINEL) for nm in sinks}
    grads = f._param_struct(lib.Grads(), {k: b.ptr for k, b in bufs.items() if k not in A.PER_IMAGE})
    pg = lib.PoseGrads()
    for k in A.POSE_SINKS:
        setattr(pg, k, bufs[k].ptr if k in bufs else None)
    lib.path_counts(reset=True)
    with torch.cuda.device(dev):
        rc = f.L.svae_decoder_backward(ctypes.byref(f.desc), ctypes.byref(f.params), ctypes.byref(f.pose), f.z,
                                       f.bufs["logits"].ptr, f.tens["dy"].data_ptr(), None, f.saved.ptr, ctypes.byref(grads),
                                       bufs["dz"].ptr if "dz" in bufs else None, ctypes.byref(pg), f.ws.ptr, f.ws_bytes,
                                       A._stream())
    lib.check(rc)
    torch.cuda.synchronize()
    paths = {k: v for k, v in lib.path_counts(reset=True).items() if v}
    out, bad = A._collect(c, bufs)
    bad += A._guards_only(dict(ws=f.ws, saved=f.saved, logits=f.bufs["logits"], y=f.bufs["y"]))
    return out, paths, bad


class Runs(object):
    def __init__(self, name):
        keep = {k: os.environ.get(k) for k in DUAL}
        try:
            for k in DUAL:
                os.environ.pop(k, None)
            os.environ.update(ENV[name])              # read per call by the library
            self.f = A.Forward(name)
            sinks = A.sink_names(name)
            self.old, self.old_paths, self.old_bad = _backward(self.f, sinks + ["dcoords"])
            self.new, self.new_paths, self.new_bad = _backward(self.f, sinks)
            self.again, _, self.again_bad = _backward(self.f, sinks)
        finally:
            for k, v in keep.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _runs(name):
    return Runs(name)


def _bounds(name):
    r64, r32 = A.reference(name, torch.float64), A.reference(name, torch.float32)
    b = {k: max(4.0 * rel_err(r32[k], r64[k]), FLOOR_GRAD) for k in ("dtheta", "ddx") if k in r64}
    for k, v in b.items():
        assert v <= GRAD_CAP, (name, k, v)
    return r64, b


def _fp16x3():
    from spatial_vae_amd import _lib
    return _lib.gemm_mode() == "fp16x3"


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_run_the_intended_kernels(name):
    """fp32 mode: the first two cases take dense4 / dense_kernel as the module docstring says, the SVAE_DENSE4=2 cases the dual
    launch with a half-width tail, the rest dense4 without it.  (fp16x3 mode: the split data gradient.)"""
    r = _runs(name)
    for p in (r.old_paths, r.new_paths):
        if _fp16x3():
            assert p.get("dense_split_dgrad", 0) >= 1, p
            continue
        assert p.get("dense_fp32_dgrad", 0) == A.case(name)["L"] - 1, p
        if name == "pfs_n28_b3":
            assert p.get("dense4", 0) == 0, p
        elif ENV[name]:
            assert p.get("dense4_dual", 0) >= 1 and p.get("dense4_tail", 0) >= 1, p
        else:
            assert p.get("dense4", 0) >= 1 and p.get("dense4_dual", 0) == 0, p


@pytest.mark.parametrize("name", NAMES)
def test_pose_gradients_from_sums(name):
    """dtheta, ddx of the route without d(coords) (and of the one with it) against float64, and against each other.
    MI355X, fp32 mode, largest error over the fifteen cases: new route dtheta 5.9e-7 (bound 1.6e-6, pfs_n28_b4), ddx 6.4e-7
    (bound 1.7e-6, pfs_n28_b3); old route ddx 6.0e-7 (bound 2.2e-6, pfs_nt1_c2); every case inside its bound, none above 0.4
    of it.  fp16x3 mode (pfs_dual_tanh): passes with the same bounds."""
    r = _runs(name)
    r64, bound = _bounds(name)
    assert set(bound) == {k for k in ("dtheta", "ddx") if k in A.sink_names(name)} and bound
    bad = {}
    for k in bound:
        for tag, got in (("old", r.old[k]), ("new", r.new[k])):
            assert np.isfinite(got).all() and A.sentinel_hits(got) == 0, (name, k, tag)
            e = rel_err(got, r64[k])
            print("pfs %s %-6s %s err %.3e bound %.3e" % (name, k, tag, e, bound[k]))
            if e > bound[k]:
                bad[(k, tag)] = (e, bound[k])
        e = rel_err(r.new[k], r.old[k])
        print("pfs %s %-6s new-old %.3e bound %.3e" % (name, k, e, bound[k]))
        if e > bound[k]:
            bad[(k, "new-old")] = (e, bound[k])
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", NAMES)
def test_everything_else_is_bit_equal_and_nothing_is_overrun(name):
    """Parameter gradients and dz of the two routes are np.array_equal (the same kernels but for the d(coords) part of the
    epilogue), the old route's dcoords is finite and fully written, two calls of the new route are bit-equal in every output, and no guard byte of any buffer changed in any of the three calls."""
    r = _runs(name)
    assert not r.f.bad_guards and not r.old_bad and not r.new_bad and not r.again_bad, (r.f.bad_guards, r.old_bad, r.new_bad,
                                                                                         r.again_bad)
    assert set(r.new) == set(A.sink_names(name)) and set(r.old) == set(r.new) | {"dcoords"}
    assert np.isfinite(r.old["dcoords"]).all() and A.sentinel_hits(r.old["dcoords"]) == 0
    for k, v in r.new.items():
        assert A.sentinel_hits(v) == 0, (name, k)
        assert np.array_equal(v.view(np.uint32), r.again[k].view(np.uint32)), (name, k, "two runs of the new route differ")
        if k not in ("dtheta", "ddx"):
            assert np.array_equal(v.view(np.uint32), r.old[k].view(np.uint32)), (name, k, "differs between the routes")


def test_one_case_in_fp16x3_mode():
    """The fp16x3 kernel's FIRST epilogue (two row halves per tile, split.h) feeds the same role-0 code: one fresh process
    (the mode is read once per process) runs this file's three tests of one case under SVAE_GEMM=fp16x3, bounds unchanged
    (-k selects by the case's name, so the child does not run this test again)."""
    me = "tests/test_gpu_pose_from_sums.py"
    env = dict(os.environ, SVAE_GEMM="fp16x3")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", me, "-k",
                          FP16X3_CASE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    print("\n".join(l for l in out.stdout.splitlines() if l.startswith("pfs ")))
    assert out.returncode == 0, tail
    assert "3 passed" in out.stdout and "failed" not in out.stdout, tail
