"""Child process of tests/test_gpu_grad_guard.py: dp.TrainStep with the real HIP decoder and clip_grad_norm set, as ONE rank
or as two ranks sharing cuda:0 (SVAE_SHARE_GPU=1, gloo), over the same global minibatches (sizes 8, 8 split 5+3, 1 with an
EMPTY shard, 6).

The one-rank run measures the first minibatch's gradient norm with a plain backward on copies of its modules, takes HALF of it
as the threshold (that step certainly clips) and writes threshold, final parameters and guard statistics to SVAE_GUARD_REF;
the two-rank run reads the threshold from there, checks its replicas bit for bit and its parameters against the one-rank
run's, and prints one `rank <r> stats <json>` line per rank."""
import contextlib
import copy
import io
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn as nn  # noqa: E402


def main():
    import spatial_vae.models as models
    from spatial_vae_amd import cli, dp, elbo as E, ops
    ref_path = os.environ["SVAE_GUARD_REF"]
    rank, world, local = dp.init_process_group(device_is_gpu=True)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    n = m = 12
    torch.manual_seed(100 + rank)                       # every rank initialises differently; rank 0's weights must win
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(2, 64, num_layers=2, activation=nn.Tanh).to(dev)
        q_net = models.InferenceNetwork(n * m, 5, 32, num_layers=2, activation=nn.Tanh).to(dev)
    x = cli.coord_grid(n, m).to(dev)
    rs = np.random.RandomState(7)
    sizes = [8, 8, 1, 6]
    ys = [torch.from_numpy(rs.uniform(size=(b, n * m)).astype(np.float32)).to(dev) for b in sizes]
    ns = [torch.from_numpy(rs.normal(size=(b, 5)).astype(np.float32)).to(dev) for b in sizes]
    kw = dict(rotate=True, translate=True, dx_scale=0.1, theta_prior=math.pi / 4)
    if world == 1:
        p2, q2 = copy.deepcopy(p_net), copy.deepcopy(q_net)
        (-E.eval_minibatch_mnist(x, ys[0], p2, q2, noise=ns[0], **kw)[0]).backward()
        first = float(torch.linalg.vector_norm(torch.cat([p.grad.reshape(-1).double() for p in
                                                          list(p2.parameters()) + list(q2.parameters())])))
        max_norm = 0.5 * first
    else:
        max_norm = float(torch.load(ref_path, weights_only=True)["max_norm"])
    step = dp.TrainStep(p_net, q_net, E.eval_minibatch_mnist, lr=1e-2, clip_grad_norm=max_norm, **kw)
    assert isinstance(step.optim, ops.FlatAdam) and step.optim.guarded and step.aliased()

    def bounds(i, b):
        if world == 2 and i == 1:                       # a deliberately ragged 5 + 3 split of the second batch
            return (0, 5) if rank == 0 else (5, 8)
        return dp.shard_bounds(b, rank, world)

    for i, (y, r) in enumerate(zip(ys, ns)):
        lo, hi = bounds(i, y.size(0))
        step(x, y[lo:hi], weight=(hi - lo) / y.size(0), global_batch=y.size(0), noise=r[lo:hi])
    stats = step.guard_stats()                          # synchronises
    flat = step.grads.flat_param.detach().cpu()
    assert step.aliased() and int(step.optim.state[step.master]["step"]) == len(sizes)
    assert float(step.grads.flat.abs().max()) == 0.0
    if world == 1:
        torch.save({"flat": flat, "max_norm": max_norm, "first_norm": first}, ref_path)
    else:
        ref = torch.load(ref_path, weights_only=True)
        both = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1]), "replicas diverged"
        perr = (flat - ref["flat"]).abs().max().item() / ref["flat"].abs().max().item()
        print("rank", rank, "param err %.3e" % perr)
        assert perr < 2e-6, perr
    print("rank", rank, "stats", json.dumps(dict(stats, threshold=max_norm)))
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
