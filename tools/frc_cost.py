#!/usr/bin/env python3
"""Per-launch times of the two ring-correlation kernels (include/svae_frc.h) under svae_profile_enable(2), at config 5's
40 x 40 box with 20 planes (the LDS form) and at a 256 x 256 box with 8 planes (the workspace form): one JSON object on stdout
and, with --out, in that file (profiles/frc_cost.json is this script's output).  The two launches share the `augment` profile
kind, so each is timed in a window of its own: warm-up launches, a read that clears the counters, then `--launches` launches.

  python tools/frc_cost.py --out profiles/frc_cost.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402
from spatial_vae_amd import elbo as E  # noqa: E402

SHAPES = [{"n": 40, "m": 40, "planes": 20}, {"n": 256, "m": 256, "planes": 8}]


def timed(fn, launches, warmup=3):
    """ms per launch of fn() from the library's own event pairs."""
    for _ in range(warmup):
        fn()
    _lib.profile_read()
    for _ in range(launches):
        fn()
    ms, count = _lib.profile_read()["augment"]
    assert count == launches, (count, launches)
    return ms / count


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=20)
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    rows = []
    for s in SHAPES:
        n, m, P = s["n"], s["m"], s["planes"]
        gen = torch.Generator().manual_seed(n)
        signal = torch.randn(P, n, m, generator=gen, dtype=torch.float64)
        a = (signal + 0.35 * torch.randn(P, n, m, generator=gen, dtype=torch.float64)).to(dev)
        b = (signal + 0.35 * torch.randn(P, n, m, generator=gen, dtype=torch.float64)).to(dev)
        radius = max(min(n, m) / 2.0 - 3.0, 1.0)
        weight = E.frc_weight(ops.frc(a, b, n, m, radius, 3.0)[1])
        row = dict(s, form="lds" if _lib.lib().svae_frc_workspace_bytes(P, n, m) == 0 else "workspace")
        row["frc_ms"] = timed(lambda: ops.frc(a, b, n, m, radius, 3.0), args.launches)
        row["frc_filter_ms"] = timed(lambda: ops.frc_filter(a, weight, n, m), args.launches)
        rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    _lib.profile_enable(0)
    result = {"what": "ms per launch, HIP events around each launch (svae_profile_enable(2), kind augment)", "launches": args.launches,
              "device": torch.cuda.get_device_name(0), "command": "python tools/frc_cost.py", "shapes": rows}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
