#!/usr/bin/env python3
"""Wall time of ops.GaussianMixture.fit (include/svae_gmm.h) at N = 100 000 points, D = 8, k = 50, 50 iterations, started from
a 10-step ops.KMeans fit that is not timed: one warm-up fit, then the median of three, each timed from the first enqueue to a
device synchronisation.  tol = 0 and the planted blobs overlap, so that the fit is not frozen early and every step does its
work.  One JSON object on stdout and, with --out, in that file (profiles/gmm_cost.json is this script's output).  --bench /
--bench_parent take files holding the JSON line of `bench.py --gpus 1 --steps 30 --warmup 5` from this commit and from its
parent, and are copied into the object: the default training path launches nothing new, and the pair shows it.

  python tools/gmm_cost.py --bench this.json --bench_parent parent.json --out profiles/gmm_cost.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import ops  # noqa: E402

N, D, K, ITERS = 100000, 8, 50, 50


def bench_line(path):
    """The last line of `path` that parses as a JSON object."""
    with open(path) as f:
        lines = [l for l in f.read().splitlines() if l.startswith("{")]
    return json.loads(lines[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bench")
    p.add_argument("--bench_parent")
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(0)
    planted = rs.randn(K, D) * 0.6
    x = torch.from_numpy((planted[rs.randint(0, K, size=N)] + 0.35 * rs.randn(N, D)).astype(np.float32)).to(dev)
    start = ops.KMeans(K, D, dev).fit(x, 10, rs.rand(K))
    gm = ops.GaussianMixture(K, D, dev)

    def fit():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gm.fit(x, start.label, start.centres, ITERS, reg=1e-6, tol=0.0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    fit()
    runs = [fit() for _ in range(3)]
    rec = ops.GaussianMixture.read_record(runs[-1][1].record)
    result = {"what": "ms per ops.GaussianMixture.fit: init (three launches), `iterations` update steps of four launches and one "
                      "labelling step of three, a device-to-device copy of the loglik after each; wall clock around enqueue + "
                      "synchronise, one warm-up fit, median of three",
              "device": torch.cuda.get_device_name(0), "command": "python tools/gmm_cost.py", "N": N, "D": D, "k": K,
              "iterations": ITERS, "fit_ms": [round(r[0], 3) for r in runs], "fit_ms_median": round(float(np.median([r[0] for r in runs])), 3),
              "iterations_applied": rec["iterations"], "converged_at": rec["converged_at"], "dead": rec["dead"], "loglik": rec["loglik"]}
    if args.bench:
        result["bench_this_commit"] = bench_line(args.bench)
    if args.bench_parent:
        result["bench_parent_commit"] = bench_line(args.bench_parent)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
