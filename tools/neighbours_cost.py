#!/usr/bin/env python3
"""Device time of the two neighbour calls (include/svae_neighbours.h) at two sizes -- 10 000 images with D = 2 and K = 32, and
100 000 images with D = 8 and K = 100 -- from the library's own event pairs (svae_profile_enable(2): one pair around each
call's launch, filed under `augment`): per call one warm-up, then the mean of three.  svae_nbr_search is timed as neighbours.py
makes it: one block of QUERY_BLOCK queries against all candidates, from empty lists (refilled before every call, outside the
event pair); the whole set takes `launches_per_split` such launches.  svae_nbr_average is timed for one minibatch of 1000
images over the lists the search found (the image itself first, uniform weights), at 784 and at 4096 pixels of one channel.
With each number goes what it implies: the pairs compared, or the bytes of neighbour rows gathered.  No threshold is attached
to any of them.  One JSON object on stdout and, with --out, in that file (profiles/neighbours_cost.json is this script's
output).  --bench / --bench_parent take files holding the JSON lines of `bench.py --gpus 1 --steps 30 --warmup 5` from this
commit and from its parent, and are copied into the object: the default training path launches nothing new.

  python tools/neighbours_cost.py --bench this.json --bench_parent parent.json --out profiles/neighbours_cost.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spatial_vae_amd import _lib, ops  # noqa: E402
from spatial_vae_amd.neighbours import QUERY_BLOCK  # noqa: E402

SETS = [(10000, 2, 32), (100000, 8, 100)]       # images, D, K
PIXELS = (784, 4096)
MINIBATCH = 1000
REPEATS = 3


def bench_lines(path):
    """Every line of `path` that parses as a JSON object, in order."""
    with open(path) as f:
        return [json.loads(l) for l in f.read().splitlines() if l.startswith("{")]


def timed(call, before=lambda: None):
    """ms per call from the `augment` event pairs: one warm-up, then REPEATS calls; `before` runs ahead of each, untimed."""
    before()
    call()
    torch.cuda.synchronize()
    _lib.profile_read()
    for _ in range(REPEATS):
        before()
        call()
    ms, count = _lib.profile_read()["augment"]
    assert count == REPEATS, count
    return ms / count


def set_cost(images, D, K, dev):
    rs = np.random.RandomState(0)
    z = torch.from_numpy(rs.randn(images, D)).to(dev)
    block = min(QUERY_BLOCK, images)
    probe = ops.NeighbourSearch(block, K, dev)

    def refill():
        probe.d2.fill_(float("inf"))
        probe.index.fill_(-1)

    ms = timed(lambda: probe.update(z[:block], 0, z, 0), refill)
    launches = -(-images // block)
    out = {"images": images, "D": D, "K": K,
           "svae_nbr_search": {"ms_per_launch": round(ms, 4), "queries": block, "candidates": images, "pairs": block * images,
                               "launches_per_split": launches, "pairs_per_split": images * images}}
    search = ops.NeighbourSearch(images, K, dev)
    for lo in range(0, images, block):
        search.update(z[lo:lo + block], lo, z, 0)
    index = torch.cat([torch.arange(images, dtype=torch.int64, device=dev).unsqueeze(1), search.index], 1)[:MINIBATCH].contiguous()
    assert int((index >= 0).sum()) == index.numel()
    for N in PIXELS:
        stack = torch.randn(images, N, 1, device=dev)
        cover = torch.ones(images, N, dtype=torch.uint8, device=dev)
        ms = timed(lambda: ops.neighbour_average(stack, cover, index, None, support=True))
        out["svae_nbr_average_%d_pixels" % N] = {"ms_per_launch": round(ms, 4), "images_averaged": MINIBATCH, "T": K + 1,
                                                 "bytes_gathered": MINIBATCH * (K + 1) * N * 5,
                                                 "launches_per_split": -(-images // MINIBATCH)}
        del stack, cover
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bench")
    p.add_argument("--bench_parent")
    p.add_argument("--out")
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    _lib.profile_enable(2)
    result = {"what": "device ms of each neighbour call from the library's event pairs around its launch (profile level 2), one "
                      "warm-up call and the mean of %d; every call is one launch.  svae_nbr_search: one block of queries against "
                      "all candidates from empty lists, `pairs` distances of D coordinates each.  svae_nbr_average: %d images of "
                      "T slots each, `bytes_gathered` = images x T x pixels x (4 bytes of the float + 1 of cover).  No threshold "
                      "is attached to these numbers" % (REPEATS, MINIBATCH),
              "device": torch.cuda.get_device_name(0), "command": "python tools/neighbours_cost.py",
              "sets": [set_cost(*s, dev) for s in SETS]}
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
