#!/usr/bin/env python3
"""Device time of the six eigenimage calls (include/svae_eigen.h) at two shapes -- 40 x 40 boxes with 100 images in 10 classes,
and 256 x 256 boxes with 16 images in 4 classes, R = 16 columns and P = 8 components in both -- from the library's own event
pairs (svae_profile_enable(2): one pair around each call's launch, filed under `augment`): per call one warm-up, then the mean
of five.  One JSON object on stdout and, with --out, in that file (profiles/eigen_cost.json is this script's output).  --bench /
--bench_parent take files holding the JSON lines of `bench.py --gpus 1 --steps 30 --warmup 5` from this commit and from its
parent, and are copied into the object: the default training path launches nothing new, and the runs show it.

  python tools/eigen_cost.py --bench this.json --bench_parent parent.json --out profiles/eigen_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402

SHAPES = [(40, 40, 100, 10, 16, 8), (256, 256, 16, 4, 16, 8)]     # rows, cols, images, classes, R, P
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


def shape_cost(rows, cols, B, K, R, P, dev):
    rs = np.random.RandomState(0)
    N, C = rows * cols, 1
    label = torch.from_numpy((np.arange(B) % K).astype(np.int32)).to(dev)
    aligned = torch.from_numpy(rs.randn(B, N, C).astype(np.float32)).to(dev)
    cover = torch.ones(B, N, dtype=torch.uint8, device=dev)
    sums = ops.ClassSums(K, N, C, dev)
    sums.update(aligned, cover, label)
    mean = (sums.sum / sums.count.unsqueeze(2)).contiguous()
    eig = ops.EigenImages(K, N, C, R, dev)
    start = torch.from_numpy(rs.randn(K, N * C, R)).to(dev)
    eig.start(start)
    eig.begin_pass()
    eig.update(aligned, cover, label, mean)
    fit = eig.finish(P)                                        # every buffer the timed calls reuse now holds real values
    f64 = dict(dtype=torch.float64, device=dev)
    T, G, W, rot = eig._rows[0], torch.empty(K, R, R, **f64), torch.empty(K, R, R, **f64), torch.empty(K, P, R, **f64)
    sweeps, off = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, **f64)
    Q1, coords = torch.empty_like(eig.Q), torch.empty(B, P, **f64)
    ops._call("svae_eig_gram", dev, eig.Q, eig.Y, eig.members, K, N * C, R, G)
    ops._call("svae_pca_eigen", dev, G, R, K, fit.eigenvalues, W, sweeps, off)
    calls = {
        "svae_eig_project": lambda: ops._call("svae_eig_project", dev, aligned, cover, label, mean, eig.Q, B, N, C, K, R, T),
        "svae_eig_accumulate": lambda: ops._call("svae_eig_accumulate", dev, aligned, cover, label, mean, T, B, N, C, K, R, eig.Y, eig.ssq),
        "svae_eig_orthonormalise": lambda: ops._call("svae_eig_orthonormalise", dev, eig.Y, K, N * C, R, Q1),
        "svae_eig_gram": lambda: ops._call("svae_eig_gram", dev, eig.Q, eig.Y, eig.members, K, N * C, R, G),
        "svae_eig_rotate": lambda: ops._call("svae_eig_rotate", dev, eig.Q, eig.Y, W, fit.eigenvalues, eig.members, K, N * C, R, P,
                                             fit.eigenimages, fit.residual, rot),
        "svae_eig_coords": lambda: ops._call("svae_eig_coords", dev, T, label, rot, B, K, R, P, coords)}
    out = {"rows": rows, "cols": cols, "images": B, "classes": K, "R": R, "P": P}
    for name, call in calls.items():
        out[name] = {"ms_per_launch": round(timed(call), 4), "launches": 1}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bench")
    p.add_argument("--bench_parent")
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    result = {"what": "device ms of each eigenimage call from the library's event pairs around its launch (profile level 2), one "
                      "warm-up call and the mean of %d; every call is one launch; a pass makes project and accumulate once per "
                      "minibatch and orthonormalise once" % REPEATS,
              "device": torch.cuda.get_device_name(0), "command": "python tools/eigen_cost.py",
              "shapes": [shape_cost(*shape, dev) for shape in SHAPES]}
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
