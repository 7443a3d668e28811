#!/usr/bin/env python3
"""Per-launch time of the multi-reference alignment (include/svae_classify.h) under svae_profile_enable(2), at
tools/refine_cost.py's two shapes (40 x 40 with 100 images: the LDS form; 256 x 256 with 16 images: the workspace form) and its
search (5 angles on each side, shifts up to 2 pixels, bicubic), with M = 1, 8 and 64 candidates per image; beside each the time
of the M separate svae_pose_search launches that score the same images against the same references: one JSON object on stdout
and, with --out, in that file (profiles/classify_cost.json is this script's output).  Both are filed under the `augment`
profile kind (one event pair per call: svae_pose_classify's pair spans its norms launch too); each is timed in a window of its
own: warm-up calls, a read that clears the counters, then `--launches` calls.  No threshold is attached.

  python tools/classify_cost.py --out profiles/classify_cost.json
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
ANGLES, STEP_DEG, SHIFT, INTERP = 5, 2.0, 2, "bicubic"
CANDIDATES = (1, 8, 64)


def timed(fn, launches, per_call=1, warmup=2):
    """ms per call of fn() from the library's own event pairs; fn() makes `per_call` launches of the kind."""
    for _ in range(warmup):
        fn()
    _lib.profile_read()
    for _ in range(launches):
        fn()
    ms, count = _lib.profile_read()["augment"]
    assert count == launches * per_call, (count, launches, per_call)
    return ms / launches


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=10)
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    rows = []
    step = math.radians(STEP_DEG)
    for s in SHAPES:
        n, m, B = s["rows"], s["cols"], s["images"]
        gen = torch.Generator().manual_seed(n)
        y = torch.randn(B, n * m, 1, generator=gen).to(dev)
        refs = torch.randn(max(CANDIDATES), n * m, 1, generator=gen, dtype=torch.float64).to(dev)
        weight = torch.from_numpy(E.refine_mask(n, m, SHIFT).reshape(-1)).to(dev)
        pose = torch.cat([torch.rand(B, 1, generator=gen) * 6 - 3, torch.rand(B, 2, generator=gen) * 0.2 - 0.1], 1).to(dev)
        for M in CANDIDATES:
            ref = refs[:M].contiguous()
            cand = torch.arange(M, dtype=torch.int32, device=dev).unsqueeze(0).expand(B, M).contiguous()
            columns = [cand[:, j].contiguous() for j in range(M)]
            need = _lib.lib().svae_pose_classify_workspace_bytes(B, M, M, n, m, 1)
            row = dict(s, angles=ANGLES, step_deg=STEP_DEG, shift=SHIFT, interp=INTERP, M=M,
                       form="lds" if need == 8 * ((M + 31) // 32 * 32) else "workspace")

            def searches():
                for index in columns:
                    ops.pose_search(y, ref, weight, index, pose, n, m, ANGLES, step, SHIFT, INTERP)

            row["pose_classify_ms"] = timed(lambda: ops.pose_classify(y, ref, weight, cand, pose, n, m, ANGLES, step, SHIFT, INTERP),
                                            args.launches)
            row["M_pose_searches_ms"] = timed(searches, args.launches, per_call=M)
            row["ratio"] = row["pose_classify_ms"] / row["M_pose_searches_ms"]
            rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    _lib.profile_enable(0)
    result = {"what": "ms per call, HIP events around each call (svae_profile_enable(2), kind augment); M_pose_searches_ms is the sum "
                      "over the M launches", "launches": args.launches, "device": torch.cuda.get_device_name(0),
              "command": "python tools/classify_cost.py", "shapes": rows}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
