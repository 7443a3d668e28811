#!/usr/bin/env python3
"""Per-call time of the maximum-likelihood class averaging (include/svae_expect.h) under svae_profile_enable(2), at
tools/classify_cost.py's LDS shape (40 x 40 x 1 with 100 images) and its search (5 angles on each side, shifts up to 2 pixels,
bicubic), with M = 1, 4 and 8 slots per image: svae_pose_expect (its event pair spans the prologue too), svae_expect_sums_update
into M classes, and in the same run svae_pose_classify on the same images, references and slots, with the ratio of the two soft
calls to it: one JSON object on stdout and, with --out, in that file (profiles/expect_cost.json is this script's output).  All
three are filed under the `augment` profile kind, one event pair per call; each is timed in windows of its own: warm-up calls, a
read that clears the counters, then `--launches` calls, and that `--repeats` times: the figure is the median of the windows'
means, and the least and largest window are kept beside it.  No threshold is attached.

  python tools/expect_cost.py --out profiles/expect_cost.json
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402
from spatial_vae_amd import elbo as E  # noqa: E402

SHAPE = {"rows": 40, "cols": 40, "images": 100}
ANGLES, STEP_DEG, SHIFT, INTERP = 5, 2.0, 2, "bicubic"
SLOTS = (1, 4, 8)
INV_SIGMA2 = 0.05       # with unit-variance images and references the posterior is neither flat nor one-hot: each row records it


def timed(fn, launches, repeats, warmup=2):
    """(median, least, largest) over `repeats` windows of the mean ms per call of fn(), from the library's own event pairs."""
    for _ in range(warmup):
        fn()
    means = []
    for _ in range(repeats):
        _lib.profile_read()
        for _ in range(launches):
            fn()
        ms, count = _lib.profile_read()["augment"]
        assert count == launches, (count, launches)
        means.append(ms / launches)
    return statistics.median(means), min(means), max(means)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--launches", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    n, m, B = SHAPE["rows"], SHAPE["cols"], SHAPE["images"]
    step = math.radians(STEP_DEG)
    gen = torch.Generator().manual_seed(n)
    y = torch.randn(B, n * m, 1, generator=gen).to(dev)
    refs = torch.randn(max(SLOTS), n * m, 1, generator=gen, dtype=torch.float64).to(dev)
    weight = torch.from_numpy(E.refine_mask(n, m, SHIFT).reshape(-1)).to(dev)
    pose = torch.cat([torch.rand(B, 1, generator=gen) * 6 - 3, torch.rand(B, 2, generator=gen) * 0.2 - 0.1], 1).to(dev)
    rows = []
    for M in SLOTS:
        ref = refs[:M].contiguous()
        cand = torch.arange(M, dtype=torch.int32, device=dev).unsqueeze(0).expand(B, M).contiguous()
        need = _lib.lib().svae_pose_expect_workspace_bytes(B, M, M, n, m, 1, ANGLES, SHIFT)
        row = dict(SHAPE, angles=ANGLES, step_deg=STEP_DEG, shift=SHIFT, interp=INTERP, M=M, inv_sigma2=INV_SIGMA2,
                   form="lds" if need == 8 * ((M + 31) // 32 * 32) else "workspace")

        def expect():
            return ops.pose_expect(y, ref, weight, None, cand, pose, n, m, ANGLES, step, SHIFT, INV_SIGMA2, INTERP)

        spread = expect()
        sums = ops.ClassSums(M, n * m, 1, dev)
        row["largest_posterior_median"] = float(spread.class_post.max(1).values.median().item())
        for key, fn in (("pose_expect_ms", expect), ("expect_sums_update_ms", lambda: sums.update_soft(spread, cand)),
                        ("pose_classify_ms", lambda: ops.pose_classify(y, ref, weight, cand, pose, n, m, ANGLES, step, SHIFT, INTERP))):
            row[key], row[key + "_min"], row[key + "_max"] = timed(fn, args.launches, args.repeats)
        row["ratio"] = (row["pose_expect_ms"] + row["expect_sums_update_ms"]) / row["pose_classify_ms"]
        rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    _lib.profile_enable(0)
    result = {"what": "ms per call, HIP events around each call (svae_profile_enable(2), kind augment): the median over `repeats` "
                      "windows of `launches` calls, with the least and the largest window; ratio = (pose_expect_ms + "
                      "expect_sums_update_ms) / pose_classify_ms", "launches": args.launches, "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0), "command": "python tools/expect_cost.py", "shapes": rows}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
