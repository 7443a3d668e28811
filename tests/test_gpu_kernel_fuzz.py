"""Seeded shape sweep over the kernel alternatives: every case runs the decoder forward + backward five times in one
process -- the r01/r02 kernels (SVAE_DENSE4=0, SVAE_WGRAD2=0), the defaults (dense4_kernel / dense4_dual_kernel where the
plan takes them, wgrad2_kernel, the merged tail launch), the defaults with the tail launch split, and dense4_kernel forced at
either block width -- and compares all outputs.  The ISA
check of the hand-issued loads (tools/check_asm_loads.py) is static; this is its dynamic counterpart: shapes nobody picked by
hand (ragged tile counts, 1-3 octet row ranges per split, every activation, 1-4 layers, 1-3 channels, posed / explicit
coordinates, z_dim 0) must give the same numbers whichever kernels run.

The same numbers are not yet the right ones: every choice shares prepare_kernel, the coordinate layer, out_fwd / logits_finish,
out_bwd, the reduce kernels, first_layer_image_kernel / backward_tail_kernel and the pose gradients.  So all five results of a
case are also held to the float64 CPU reference of the same decoder on the same inputs (tests/decoder_sweep.py): per output
max(4 * e32, 16 * 2^-24), e32 the float32 CPU evaluation's own error, inside 2e-5 (y, logits) and 1e-4 (gradients).  A
rectifier's gradients are compared only where no hidden pre-activation of the reference sits within rounding of the kink; the
lattice cases (ReLU on dyadic inputs: every pre-activation exact in fp32, many exactly 0) and the pinned-seed LeakyReLU cases
of decoder_sweep.py are built so that they always are, run here through the same five choices, and have their dispatch asserted.

The file runs in the process's GEMM mode.  test_the_file_passes_in_fp16x3_mode repeats it in a child under SVAE_GEMM=fp16x3
with the same bounds; there the split-eligible cases must take the f16 kernels (which ignore SVAE_DENSE4 / SVAE_WGRAD2: the
variants coincide) and every other case the fp32 kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch.nn as nn

import decoder_sweep as S
from helpers import rel_err
from test_gpu_dense4 import _run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ME = "tests/test_gpu_kernel_fuzz.py"


def _cases(count, seed, big=False):
    rs = np.random.RandomState(seed)
    acts = [nn.Tanh, nn.Tanh, nn.Sigmoid, nn.ReLU, nn.LeakyReLU]
    out = []
    for i in range(count):
        n = int(rs.choice([5, 8, 11, 12, 16, 20, 28]))
        B = int(rs.randint(1, 24))
        zd = int(rs.choice([0, 1, 2, 5]))
        H = int(rs.choice([24, 32, 64, 96, 100, 128, 200, 500]))
        if H >= 200:
            B = min(B, 6)
        L = int(rs.randint(1, 5))
        if big:      # one-off soak at sizes where the wide / dual launches and long register-ring trips are what runs
            n = int(rs.choice([28, 32, 40]))
            B = int(rs.randint(24, 200))
            H = int(rs.choice([200, 256, 500, 512]))
            L = int(rs.randint(2, 4))
        C = int(rs.randint(1, 4))
        act = acts[int(rs.randint(len(acts)))]
        posed = bool(rs.randint(2))
        out.append(("fuzz%02d_n%d_B%d_z%d_H%d_L%d_C%d_%s_%s" % (i, n, B, zd, H, L, C, act.__name__, "posed" if posed else "coords"),
                    n, B, zd, H, L, C, act, posed))
    return out


# SVAE_FUZZ_COUNT widens the sweep for a one-off soak run (profiles/r03_kernel_fuzz_soak.txt: 400 geometries)
CASES = _cases(int(os.environ.get("SVAE_FUZZ_COUNT", "28")), 20261005, big=os.environ.get("SVAE_FUZZ_BIG") == "1")
SWEPT = CASES + S.LATTICE + S.PINNED


def _mode():
    from spatial_vae_amd import _lib
    return _lib.gemm_mode()


@pytest.mark.parametrize("case", SWEPT, ids=[c[0] for c in SWEPT])
def test_every_kernel_choice_gives_the_same_numbers(case, monkeypatch):
    """MI355X, fp32 mode, against float64 over all five choices: 52 of the 64 cases of the three files have their gradients
    compared (every smooth, lattice and pinned one).  Largest error (bound, case) -- the 28 random geometries: y 1.9e-7 (9.5e-7,
    fuzz14), logits 1.1e-6 (2.7e-6, fuzz23; closest fuzz10, 1.1e-6 of 2.4e-6), parameter gradients 1.8e-6 (3.9e-6, coord_linear.bias
    of fuzz13; closest the same of fuzz10, 1.0e-6 of 2.2e-6), input gradients 9.8e-7 (6.1e-6, dz of fuzz24; closest its ddx,
    6.8e-7 of 1.1e-6).  Lattice cases: y and logits 1.2e-7 (9.5e-7), parameter gradients 5.9e-7 (5.1e-6, coord_linear.weight of
    lat_h500; closest layers.3.bias of lat_c2_h100_n25, 3.7e-7 of 9.5e-7), input gradients 7.3e-7 (3.2e-6, dz of lat_h500).
    Pinned LeakyReLU cases: y 1.1e-7, logits 3.1e-7 (1.2e-6), gradients 4.7e-7 (1.3e-6, coord_linear.weight of
    pin_leaky_c3_h96).  Each case takes 0.15 s or less."""
    given, L, mode = S.given(case), case[5], _mode()
    split = mode == "fp16x3" and S.split_eligible(case)
    pinned_paths = S.kind(case) in ("lattice", "pinned") and mode == "fp32"

    def dispatched(counts, d4):
        took = all(counts.get(k, 0) > 0 for k in S.SPLIT_PATHS)
        assert took == split and (split or not any(counts.get(k, 0) for k in S.SPLIT_PATHS)), (case[0], d4, counts)
        if pinned_paths:
            want = S.dispatch(case, d4)
            assert {k: counts.get(k, 0) for k in want} == want, (case[0], d4, counts)
        return took

    monkeypatch.setenv("SVAE_WGRAD2", "0")
    monkeypatch.setenv("SVAE_TAIL_MERGE", "0")
    old, c_old = _run(case, "0", monkeypatch, given=given)
    assert c_old.get("dense4", 0) == 0 and c_old.get("wgrad2", 0) == 0
    print("sweep-paths %s %s %s" % (case[0], mode, "split" if dispatched(c_old, "0") else "fp32"))
    monkeypatch.delenv("SVAE_WGRAD2")
    monkeypatch.delenv("SVAE_TAIL_MERGE")
    monkeypatch.delenv("SVAE_DENSE4", raising=False)
    runs = {}
    # (SVAE_DENSE4, SVAE_TAIL_MERGE): the default dispatch with and without the merged tail launch, then dense4_kernel forced
    # at either block width wherever it is legal (small shapes take dense_kernel by default)
    for d4, merge in (("", "1"), ("", "0"), ("1", "1"), ("2", "1")):
        monkeypatch.setenv("SVAE_TAIL_MERGE", merge)
        os.environ.pop("SVAE_DENSE4", None)
        new, c_new = _run_default(case, monkeypatch, given) if d4 == "" else _run(case, d4, monkeypatch, given=given)
        runs[(d4, merge)] = new
        if L >= 2:
            assert c_new.get("wgrad_split" if split else "wgrad2", 0) == L - 1, c_new
        dispatched(c_new, d4)
        tol = 1e-5      # blocked fp32 sums over up to 12 k rows in different orders (the goldens allow 2e-5)
        for k in old:
            assert rel_err(new[k], old[k]) < tol, (case[0], d4, merge, k, rel_err(new[k], old[k]))
    for k in runs[("", "1")]:   # where the split-K reduction runs does not change a bit
        assert np.array_equal(runs[("", "1")][k], runs[("", "0")][k]), (case[0], k)
    swept = {"r01": old}
    swept.update({"dense4=%s,merge=%s" % (d4 or "default", merge): v for (d4, merge), v in runs.items()})
    S.check(case, swept)


def _run_default(case, monkeypatch, given=None):
    """_run sets SVAE_DENSE4 to a mode; the default dispatch is the unset variable."""
    import test_gpu_dense4 as t

    class _NoDense4(object):
        def setenv(self, k, v):
            if k != "SVAE_DENSE4":
                monkeypatch.setenv(k, v)

    return t._run(case, "", _NoDense4(), given=given)


def test_the_file_passes_in_fp16x3_mode():
    """One fresh process (the mode is read once per process) runs this file under SVAE_GEMM=fp16x3 with the bounds unchanged:
    the mode claims fp32 accuracy.  The child deselects this test.  Its `sweep-paths` lines (one per case, printed after the
    case's dispatch was asserted in the child) must name the f16 kernels for exactly the split-eligible cases -- bounded
    activation, an even count of 32-column tiles, L >= 2 -- and the mode the environment asked for: a child that fell back to
    the fp32 kernels everywhere would pass every comparison.
    MI355X: 7 of the 42 cases take the f16 kernels (fuzz02, 08, 10, 13, 23, 25, 26).  Largest error of those against float64
    (bound, case): y 1.6e-7 (9.5e-7, fuzz08), logits 1.3e-6 (2.7e-6, fuzz23), gradients 1.6e-6 (3.9e-6, coord_linear.bias of
    fuzz13; closest the same of fuzz26, 4.2e-7 of 9.5e-7).  The other 35 repeat the fp32 kernels' figures; the child takes 4 s."""
    env = dict(os.environ, SVAE_GEMM="fp16x3")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", ME, "--deselect",
                          ME + "::test_the_file_passes_in_fp16x3_mode"], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    tail = out.stdout[-3000:] + out.stderr[-1500:]
    assert out.returncode == 0, tail
    assert " passed" in out.stdout and "failed" not in out.stdout, tail
    seen = {m[0]: (m[1], m[2]) for m in re.findall(r"sweep-paths (\S+) (\S+) (\S+)", out.stdout)}
    assert set(seen) == {c[0] for c in SWEPT}, sorted(set(seen) ^ {c[0] for c in SWEPT})
    assert all(v[0] == "fp16x3" for v in seen.values()), seen
    eligible = {c[0] for c in SWEPT if S.split_eligible(c)}
    assert len(eligible) >= 7 or len(CASES) != 28, eligible      # the default sweep has seven
    assert {k for k, v in seen.items() if v[1] == "split"} == eligible, seen
