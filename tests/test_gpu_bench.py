"""bench.py as the driver invokes it: a plain `python bench.py --gpus N` must start its own ranks and print ONE JSON line.
On a 1-GPU box the two ranks share cuda:0 (SVAE_SHARE_GPU=1, gloo transport): a functional rehearsal of the launch path and
of the weak / strong sharding, not a scaling measurement."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(extra, share=False):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_GEMM")}
    if share:
        env["SVAE_SHARE_GPU"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_two_ranks_from_a_plain_invocation(scaling):
    d = _bench(["--gpus", "2", "--config", "1", "--steps", "3", "--warmup", "2", "--scaling", scaling, "--full",
                "--no-cpu-baseline", "--no-secondary"], share=True)
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["steps"] == 3 and d["value"] > 0
    assert d["config"]["global_batch"] == (128 if scaling == "weak" else 64)
    assert d["config"]["per_gpu_batch"] == (64 if scaling == "weak" else 32)
    ar = d["allreduce"]
    assert len(ar["buckets_bytes"]) == 1 and sum(ar["buckets_bytes"]) == ar["bytes_per_step"]   # small encoder: one all-reduce
    # cfg 1 has 899,507 parameters; 12 tensors, each aligned to 64 floats in the flat buffer, + 3 metrics
    assert 4 * (899507 + 3) <= ar["bytes_per_step"] <= 4 * (899507 + 3 + 13 * 64)
    assert d["cpu_baseline"] is None and d["roofline"]["kernel"] in ("dense_fwd", "dense_dgrad", "wgrad")
    # the record itself shows that both ranks joined the collectives (here both on cuda:0: the shared-GPU rehearsal)
    assert ar["world"] == 2 and sorted(r for r, _ in ar["ranks_devices"]) == [0, 1]


def test_single_gpu_line_carries_roofline_and_cpu_baseline():
    d = _bench(["--config", "1", "--steps", "5", "--warmup", "2", "--full", "--cpu-seconds", "2", "--no-secondary",
                "--sustained", "1.5"])
    s = d["sustained"]          # >= 1.5 s of back-to-back steps after the timed window
    # (a 5-step window at 0.9 ms per step is mostly the pipeline filling behind the synchronisation: the sustained rate is up
    # to twice that line's value; the bound only catches a wrong unit or a wrong step count)
    assert s["seconds"] >= 1.5 and s["steps"] >= 100 and 0.5 * d["value"] < s["value"] < 3.0 * d["value"]
    assert set(s["gemm_kernels_avg_ms"]) == {"dense_fwd", "dense_dgrad", "wgrad"} and 0.05 < s["roofline_frac"] < 1.0
    assert d["n_gpus"] == 1 and d["dtype"] == "f32" and d["unit"] == "images/s" and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["peak"] == 157.3 and 0.05 < r["frac"] < 1.0
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["one_thread"]["value"] > 0
    assert "median" in c["sample"] and "2 warm-up" in c["sample"]


def test_plain_line_times_the_steps_and_dumps_repeat(tmp_path):
    """A plain run carries the headline only (the extras are --full's) and times exactly --steps steps; --dump-outputs writes
    the last timed step's metrics, y_hat and updated parameters, identical from run to run with the same arguments."""
    import numpy as np
    dumps = []
    for k in range(2):
        out = tmp_path / str(k)
        d = _bench(["--config", "1", "--steps", "4", "--warmup", "2", "--dump-outputs", str(out)])
        assert d["steps"] == 4 and d["warmup"] == 2 and d["dtype"] == "f32" and d["unit"] == "images/s"
        assert abs(d["value"] * d["ms_per_step"] / 1e3 - 64) < 0.1                   # batch 64 per step
        assert d["roofline"] is None and d["cpu_baseline"] is None and "sustained" not in d and "fp16x3_mode" not in d
        dumps.append({f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))})
    a, b = dumps
    assert {"elbo", "log_p_x_g_z", "kl_div", "y_hat", "p_net.layers.1.weight", "q_net.layers.0.weight"} <= set(a) == set(b)
    assert a["y_hat"].shape == (64, 784) and np.isfinite(a["elbo"]).all()
    for name in a:
        assert a[name].dtype == np.float32 and np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("config,batch,kernel_min_frac", [(3, 512, 0.5), (4, 128, 0.6), (5, 256, 0.5)])
def test_every_baseline_config_has_a_bench_line(config, batch, kernel_min_frac):
    """`bench.py --config N` runs BASELINE configs 3 (fit-noise particles), 4 (galaxy RGB, three hidden layers, the 271 M
    parameter encoder that stays with the vendor GEMM) and 5 (particles with CTF filters built on the device) at their full
    sizes and reports the dominant GEMM against the fp32-MFMA peak."""
    d = _bench(["--config", str(config), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-secondary",
                "--sustained", "0"])
    assert d["config"]["baseline_config"] == config and d["config"]["global_batch"] == batch
    assert d["value"] > 0 and d["dtype"] == "f32"
    r = d["roofline"]
    assert r["kernel"] in ("dense_fwd", "dense_dgrad", "wgrad") and kernel_min_frac < r["frac"] < 1.0
    assert set(r["gemm_kernels_frac"]) == {"dense_fwd", "dense_dgrad", "wgrad"}


def test_gemm_kernel_times_ride_on_the_launches():
    """svae_profile_enable(1): the three GEMM launches carry their own start/stop events (no record packets between the
    kernels); every launch must come back from svae_profile_read with a plausible duration, pools must recycle."""
    import contextlib
    import io

    import numpy as np
    import torch
    import torch.nn as nn

    import spatial_vae.models as models
    from spatial_vae_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        p = models.SpatialGenerator(2, 128, num_layers=3, activation=nn.Tanh).to(dev)
    n, B = 16, 8
    x0, x1 = np.meshgrid(np.linspace(-1, 1, n), np.linspace(1, -1, n))
    grid = torch.from_numpy(np.stack([x0.ravel(), x1.ravel()], 1).astype(np.float32)).to(dev)
    theta = torch.zeros(B, device=dev, requires_grad=True)
    z = torch.randn(B, 2, device=dev, requires_grad=True)
    _lib.profile_enable(1)
    _lib.profile_read()
    try:
        for rounds in (1, 3):
            for _ in range(rounds):
                y = p.forward_posed(grid, B, theta=theta, dx=None, z=z)
                y.sum().backward()
            torch.cuda.synchronize()
            prof = _lib.profile_read()
            assert set(prof) == {"dense_fwd", "dense_dgrad", "wgrad"}, prof
            for k, (ms, launches) in prof.items():
                assert launches == 2 * rounds, (k, launches)          # L = 3: two hidden-layer GEMMs of each role per pass
                assert 0.0 < ms / launches < 5.0, (k, ms, launches)   # a real kernel duration: not 0, not garbage
    finally:
        _lib.profile_enable(0)
        _lib.profile_read()
