#!/usr/bin/env python
"""What a K-sample importance-weighted training step costs against the plain step with the same decoder work
(DESIGN.md section 7).

    python tools/iw_cost.py [--out profiles/r07_iw_samples.json] [--blocks 3] [--block-steps 200] [--warmup 30]
                            [--bench-line JSON --parent-bench-line JSON --parent-commit SHA]

Builds the bench's workload from bench.py itself (CONFIGS, build_nets, synthetic_targets, LR, DX_SCALE, coord_grid), the way
tools/guard_cost.py does, at BASELINE cfg 2: the plain dp.TrainStep at B = 256, and dp.TrainStep(num_samples=K) at
(B, K) = (64, 4) and (32, 8) -- 256 decoder rows each.  After the warm-up the arms are timed in ALTERNATING blocks, wall clock
around a synchronised block, so that clock drift hits all alike; medians of the blocks are reported.  A last short run of each
arm under svae_profile_enable(2) gives the launches per step and device time of each kernel kind.  The two bench lines of
`bench.py --steps 30 --warmup 5` on this commit and on its parent, measured on the same machine, are stored alongside when
given."""
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

ARMS = (("plain_B256", 256, 1), ("iw_B64_K4", 64, 4), ("iw_B32_K8", 32, 8))


def workload(cfg, B, K, dev):
    import bench
    from spatial_vae_amd import dp, elbo as E
    fn = {"mnist": E.eval_minibatch_mnist, "galaxy": E.eval_minibatch_galaxy, "particles": E.eval_minibatch_particles}[cfg["script"]]
    torch.manual_seed(0)
    p_net, q_net = bench.build_nets(cfg)
    p_net.to(dev)
    q_net.to(dev)
    extra = {"num_samples": K} if K > 1 else {}
    step = dp.TrainStep(p_net, q_net, fn, lr=bench.LR, rotate=cfg["rotate"], translate=cfg["translate"], dx_scale=bench.DX_SCALE,
                        theta_prior=cfg["theta_prior"], **extra)
    rs = np.random.RandomState(1000)
    y = torch.from_numpy(bench.synthetic_targets(cfg, rs, B)).to(dev)
    r = torch.from_numpy(rs.normal(size=(B * K, bench.inf_dim(cfg))).astype(np.float32)).to(dev)
    x = torch.from_numpy(bench.coord_grid(cfg["n"], cfg["n"])).to(dev)
    return step, x, y, r


def block(step, x, y, r, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, y, noise=r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def measure(k, dev, args):
    import bench
    from spatial_vae_amd import _lib
    cfg = dict(bench.CONFIGS[k])
    arms = {name: workload(cfg, B, K, dev) for name, B, K in ARMS}
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
                         for kind, (t, c) in prof.items()}
    med = {name: float(np.median(v)) for name, v in ms.items()}
    return {"config": k, "arms": {name: {"batch": B, "num_samples": K, "decoder_rows": B * K} for name, B, K in ARMS},
            "ms_per_step_blocks": ms, "ms_per_step_median": med,
            "iw_minus_plain_ms": {name: med[name] - med["plain_B256"] for name in med if name != "plain_B256"},
            "kernels": kernels}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_iw_samples.json"))
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
    out["cfg2"] = measure(2, dev, args)
    for key, path in (("bench_line", args.bench_line), ("bench_line_parent", args.parent_bench_line)):
        if path:
            with open(path) as f:
                lines = [l for l in f.read().splitlines() if l.startswith("{")]
            out[key] = json.loads(lines[-1])
    if args.parent_commit:
        out["parent_commit"] = args.parent_commit
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps({"ms": out["cfg2"]["ms_per_step_median"], "iw_minus_plain_ms": out["cfg2"]["iw_minus_plain_ms"]}))


if __name__ == "__main__":
    main()
