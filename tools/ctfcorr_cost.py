#!/usr/bin/env python3
"""Per-launch times of the three CTF-correction kernels (include/svae_ctfcorr.h) under svae_profile_enable(2), at config 5's
40 x 40 box (100 images) and at a 256 x 256 box (16 images), the size real cryo-EM data takes: one JSON object on stdout and,
with --out, in that file (profiles/ctfcorr_cost.json is this script's output).  The three launches share the `augment` profile
kind, so each is timed in a window of its own: warm-up launches, a read that clears the counters, then `--launches` launches.

  python tools/ctfcorr_cost.py --out profiles/ctfcorr_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402

SHAPES = [{"n": 40, "m": 40, "images": 100, "classes": 10}, {"n": 256, "m": 256, "images": 16, "classes": 4}]


def table(P, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(0.8, 3.5, P), np.full(P, 2.7), rs.choice([200.0, 300.0], P), rs.uniform(1.0, 2.5, P),
                     rs.uniform(0, 200, P), rs.uniform(5, 15, P), np.zeros(P), rs.uniform(0, 180, P)], 1)


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
        n, m, B, K = s["n"], s["m"], s["images"], s["classes"]
        gen = torch.Generator().manual_seed(n)
        y = torch.randn(B, n * m, generator=gen).to(dev)
        tab = torch.from_numpy(table(B, n)).to(dev)
        label = (torch.arange(B) % K).to(torch.int32).to(dev)
        power = ops.CtfPower(K, n, m, dev)
        total = torch.randn(K, n * m, 1, generator=gen, dtype=torch.float64).to(dev)
        den = torch.rand(K, n, m, generator=gen, dtype=torch.float64).to(dev) + 0.5
        row = dict(s, form="lds" if _lib.lib().svae_ctf_apply_workspace_bytes(B, n, m) == 0 else "workspace")
        row["ctf_apply_flip_ms"] = timed(lambda: ops.ctf_apply(y, tab, n, m, 1.0, "flip"), args.launches)
        row["ctf_apply_multiply_ms"] = timed(lambda: ops.ctf_apply(y, tab, n, m, 1.0, "multiply"), args.launches)
        row["ctf_power_update_ms"] = timed(lambda: power.update(tab, label), args.launches)
        row["wiener_finish_ms"] = timed(lambda: ops.wiener_finish(total, den, 1.0, n, m), args.launches)
        rows.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()})
    _lib.profile_enable(0)
    result = {"what": "ms per launch, HIP events around each launch (svae_profile_enable(2), kind augment)", "launches": args.launches,
              "device": torch.cuda.get_device_name(0), "command": "python tools/ctfcorr_cost.py", "shapes": rows}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
