#!/usr/bin/env python3
"""Device time of the three PCA calls (include/svae_pca.h) at three shapes -- N = 100 000 points with D = 8 in one group, the
same in 50 groups, and D = 64 in one group -- from the library's own event pairs (svae_profile_enable(2): one pair around each
call's launches, filed under `augment`): per call one warm-up, then the mean of five.  One JSON object on stdout and, with
--out, in that file (profiles/pca_cost.json is this script's output).  --bench / --bench_parent take files holding the JSON
lines of `bench.py --gpus 1 --steps 30 --warmup 5` from this commit and from its parent, and are copied into the object: the
default training path launches nothing new, and the runs show it.

  python tools/pca_cost.py --bench this.json --bench_parent parent.json --out profiles/pca_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402

SHAPES = [(100000, 8, 1), (100000, 8, 50), (100000, 64, 1)]
LAUNCHES = {"svae_pca_moments": 4, "svae_pca_eigen": 1, "svae_pca_project": 1}
REPEATS = 5


def bench_lines(path):
    """Every line of `path` that parses as a JSON object, in order."""
    with open(path) as f:
        return [json.loads(l) for l in f.read().splitlines() if l.startswith("{")]


def timed(call):
    """ms per call from the `augment` event pairs: one warm-up, then REPEATS calls."""
    call()
    torch.cuda.synchronize()
    _lib.profile_read()
    for _ in range(REPEATS):
        call()
    ms, count = _lib.profile_read()["augment"]
    assert count == REPEATS, count
    return ms / count


def shape_cost(N, D, G, dev):
    rs = np.random.RandomState(0)
    group = rs.randint(0, G, size=N).astype(np.int32)
    x = (rs.randn(N, D) * np.linspace(1.0, 3.0, D) + group[:, None]).astype(np.float32)
    x, group = torch.from_numpy(x).to(dev), (torch.from_numpy(group).to(dev) if G > 1 else None)
    fit = ops.LatentPCA(D, dev).fit(x, group, G)            # allocates the outputs and the workspace the timed calls reuse
    ws = ops._buf(dev, _lib.lib().svae_pca_workspace_bytes(N, D, G), "pca")
    calls = {"svae_pca_moments": lambda: ops._call("svae_pca_moments", dev, x, N, D, G, group, fit.count, fit.mean, fit.cov, ws, ws.numel()),
             "svae_pca_eigen": lambda: ops._call("svae_pca_eigen", dev, fit.cov, D, G, fit.eigenvalues, fit.components, fit.sweeps,
                                                 fit.off_norm),
             "svae_pca_project": lambda: ops._call("svae_pca_project", dev, x, N, D, G, D, group, fit.count, fit.mean, fit.components,
                                                   fit.proj)}
    out = {"N": N, "D": D, "G": G, "sweeps_max": int(fit.sweeps.max().item())}
    for name, call in calls.items():
        ms = timed(call)
        out[name] = {"ms_per_call": round(ms, 4), "launches": LAUNCHES[name], "ms_per_launch": round(ms / LAUNCHES[name], 4)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bench")
    p.add_argument("--bench_parent")
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    result = {"what": "device ms of each PCA call from the library's event pairs around its launches (profile level 2), one warm-up "
                      "call and the mean of %d; ms_per_launch divides by the call's launches" % REPEATS,
              "device": torch.cuda.get_device_name(0), "command": "python tools/pca_cost.py",
              "shapes": [shape_cost(N, D, G, dev) for N, D, G in SHAPES]}
    _lib.profile_enable(0)
    if args.bench:
        result["bench_this_commit"] = bench_lines(args.bench)
    if args.bench_parent:
        result["bench_parent_commit"] = bench_lines(args.bench_parent)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
