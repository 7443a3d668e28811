#!/usr/bin/env python3
"""Per-launch time of the pose search (include/svae_refine.h) under svae_profile_enable(2), at config 5's 40 x 40 box with a
minibatch of 100 images (the LDS form) and at a 256 x 256 box with 16 images (the workspace form), both at infer.py's default
search (5 angles on each side, shifts up to 2 pixels: 11 x 25 = 275 candidates per image) and both interpolations: one JSON
object on stdout and, with --out, in that file (profiles/refine_cost.json is this script's output).  The launch is filed under
the `augment` profile kind; it is timed in a window of its own: warm-up launches, a read that clears the counters, then
`--launches` launches.  No threshold is attached.

  python tools/refine_cost.py --out profiles/refine_cost.json
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402
from spatial_vae_amd import elbo as E  # noqa: E402

SHAPES = [{"rows": 40, "cols": 40, "images": 100}, {"rows": 256, "cols": 256, "images": 16}]
ANGLES, STEP_DEG, SHIFT, CLASSES = 5, 2.0, 2, 4


def timed(fn, launches, warmup=2):
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
    p.add_argument("--launches", type=int, default=10)
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    rows = []
    for s in SHAPES:
        n, m, B = s["rows"], s["cols"], s["images"]
        gen = torch.Generator().manual_seed(n)
        y = torch.randn(B, n * m, 1, generator=gen).to(dev)
        ref = torch.randn(CLASSES, n * m, 1, generator=gen, dtype=torch.float64).to(dev)
        weight = torch.from_numpy(E.refine_mask(n, m, SHIFT).reshape(-1)).to(dev)
        index = (torch.arange(B, dtype=torch.int32) % CLASSES).to(dev)
        pose = torch.cat([torch.rand(B, 1, generator=gen) * 6 - 3, torch.rand(B, 2, generator=gen) * 0.2 - 0.1], 1).to(dev)
        row = dict(s, angles=ANGLES, step_deg=STEP_DEG, shift=SHIFT, candidates=(2 * ANGLES + 1) * (2 * SHIFT + 1) ** 2,
                   form="lds" if _lib.lib().svae_pose_search_workspace_bytes(B, n, m, 1, ANGLES, SHIFT) == 0 else "workspace")
        for interp in ("bicubic", "bilinear"):
            row["pose_search_%s_ms" % interp] = timed(
                lambda: ops.pose_search(y, ref, weight, index, pose, n, m, ANGLES, math.radians(STEP_DEG), SHIFT, interp), args.launches)
        rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    _lib.profile_enable(0)
    result = {"what": "ms per launch, HIP events around each launch (svae_profile_enable(2), kind augment)", "launches": args.launches,
              "device": torch.cuda.get_device_name(0), "command": "python tools/refine_cost.py", "shapes": rows}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
