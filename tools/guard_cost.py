#!/usr/bin/env python
"""What the gradient guard costs per training step.

    python tools/guard_cost.py [--out profiles/r06_grad_guard.json] [--blocks 3] [--block-steps 200] [--warmup 30]
                               [--bench-line JSON --parent-bench-line JSON --parent-commit SHA]

Builds the bench's workload from bench.py itself (CONFIGS, build_nets, synthetic_targets, LR, DX_SCALE, coord_grid), the way
tests/test_gpu_bench_step.py does, at BASELINE cfg 2 (its own batch) and cfg 4 (B = 8), once as the plain dp.TrainStep and
once with clip_grad_norm set (a threshold of half the first gradient's norm; the guard's work does not depend on whether a
step clips: the gradient is multiplied by coef either way).  After the warm-up (the first ~12 steps run slow:
profiles/r03_clock_ramp.txt) the two arms are timed in ALTERNATING blocks, wall clock
around a synchronised block, so that clock drift hits both alike.  A last short run of each arm under svae_profile_enable(2)
gives the device time of the guard's own kernels (grad_norm: the two norm launches; adam_guarded against adam).  The two
bench lines of `bench.py --steps 30 --warmup 5` on this commit and on its parent, measured on the same machine, are stored
alongside when given."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def workload(cfg, B, dev, **guard):
    import bench
    from spatial_vae_amd import dp, elbo as E
    fn = {"mnist": E.eval_minibatch_mnist, "galaxy": E.eval_minibatch_galaxy, "particles": E.eval_minibatch_particles}[cfg["script"]]
    torch.manual_seed(0)
    p_net, q_net = bench.build_nets(cfg)
    p_net.to(dev)
    q_net.to(dev)
    step = dp.TrainStep(p_net, q_net, fn, lr=bench.LR, rotate=cfg["rotate"], translate=cfg["translate"], dx_scale=bench.DX_SCALE,
                        theta_prior=cfg["theta_prior"], **guard)
    rs = np.random.RandomState(1000)
    y = torch.from_numpy(bench.synthetic_targets(cfg, rs, B)).to(dev)
    r = torch.from_numpy(rs.normal(size=(B, bench.inf_dim(cfg))).astype(np.float32)).to(dev)
    x = torch.from_numpy(bench.coord_grid(cfg["n"], cfg["n"])).to(dev)
    return step, x, y, r


def first_norm(cfg, B, dev):
    """The first step's gradient norm, from a plain step whose optimiser call is replaced by a copy of the gradient."""
    step, x, y, r = workload(cfg, B, dev)
    kept = {}
    step.optim.step = lambda: kept.setdefault("g", step.grads.flat.detach().clone())
    step(x, y, noise=r)
    return float(torch.linalg.vector_norm(kept["g"].double()))


def block(step, x, y, r, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, y, noise=r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(k, B, dev, args):
    import bench
    from spatial_vae_amd import _lib
    cfg = dict(bench.CONFIGS[k])
    B = B or cfg["B"]
    norm = first_norm(cfg, B, dev)
    torch.cuda.empty_cache()
    arms = {"plain": workload(cfg, B, dev), "guarded": workload(cfg, B, dev, clip_grad_norm=0.5 * norm)}
    for arm in arms.values():
        block(*arm, args.warmup)
    ms = {name: [] for name in arms}
    for _ in range(args.blocks):
        for name, arm in arms.items():
            ms[name].append(block(*arm, args.block_steps))
    kernels = {}
    for name, arm in arms.items():
        _lib.profile_enable(2)
        _lib.profile_read()
        block(*arm, args.profile_steps)
        prof = _lib.profile_read()
        _lib.profile_enable(0)
        kernels[name] = {kind: {"us_per_launch": 1e3 * t / c, "launches_per_step": c / args.profile_steps}
                         for kind, (t, c) in prof.items() if kind in ("adam", "adam_guarded", "grad_norm")}
    stats = arms["guarded"][0].guard_stats()
    n = arms["plain"][0].grads.n
    med = {name: float(np.median(v)) for name, v in ms.items()}
    return {"config": k, "batch": B, "flat_gradient_floats": n, "flat_gradient_MB": round(n * 4 / 1e6, 2),
            "first_gradient_norm": norm, "threshold": 0.5 * norm, "guard_stats": stats,
            "ms_per_step_blocks": ms, "ms_per_step_median": med, "guard_ms_per_step": med["guarded"] - med["plain"],
            "kernels": kernels}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_grad_guard.json"))
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block-steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--bench-line", default=None, help="file holding bench.py's JSON line on this commit")
    ap.add_argument("--parent-bench-line", default=None, help="file holding bench.py's JSON line on the parent commit")
    ap.add_argument("--parent-commit", default=None)
    args = ap.parse_args()
    if args.block_steps < 200 or args.warmup < 30:
        raise SystemExit("blocks of >= 200 steps after >= 30 warm-up steps (profiles/r03_clock_ramp.txt)")
    dev = torch.device("cuda:0")
    out = {"box": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "blocks": args.blocks, "block_steps": args.block_steps, "warmup": args.warmup,
           "method": "wall clock around synchronised blocks, arms alternating; kernels: svae_profile_enable(2) event pairs"}
    try:
        out["commit"] = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        out["commit"] = None
    out["commit"] = os.environ.get("SVAE_COMMIT", out["commit"])
    out["cfg2"] = measure(2, None, dev, args)
    torch.cuda.empty_cache()
    out["cfg4_B8"] = measure(4, 8, dev, args)
    for key, path in (("bench_line", args.bench_line), ("bench_line_parent", args.parent_bench_line)):
        if path:
            with open(path) as f:
                lines = [l for l in f.read().splitlines() if l.startswith("{")]
            out[key] = json.loads(lines[-1])
    if args.parent_commit:
        out["parent_commit"] = args.parent_commit
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({k: {"ms": v["ms_per_step_median"], "guard_ms": v["guard_ms_per_step"], "kernels": v["kernels"]}
                      for k, v in out.items() if k.startswith("cfg")}))


if __name__ == "__main__":
    main()
