"""--resume on the MI355X: a run stopped after epoch 2 and continued in a NEW process is the uninterrupted run, bit for bit
(every reduction is fixed-order; section 7: what a state file holds).  Every command-line run is a fresh
child process, one at a time, each under its own time limit; a test stops at the first child that does not exit 0.
The CPU half of the contract (file format, refusals, flags, the loader on the gloo path) is tests/test_checkpoint_cpu.py."""
import contextlib
import glob
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIMIT = 300                                                          # seconds per child process


def _env(**extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_SHARE_GPU", "SVAE_DP_SOLO", "SVAE_DP_BUCKETS", "SVAE_DP_LOWRANK"):
        env.pop(k, None)
    env.update(extra)
    return env


def _cli(script, args, cwd, ranks=1):
    if ranks == 1:
        cmd, env = [sys.executable, os.path.join(ROOT, script)] + args, _env()
    else:
        code = ("import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
                "sys.exit(dp.launch_ranks(%d, [%r] + %r, timeout=%d))" % (ROOT, ranks, os.path.join(ROOT, script), args, LIMIT - 30))
        cmd, env = [sys.executable, "-c", code], _env(SVAE_SHARE_GPU="1")
    out = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    return [l for l in out.stdout.splitlines() if "\t" in l]


def _sd(path):
    return torch.load(path, weights_only=False).state_dict()         # a file a child of this test just wrote


def _assert_same_state_files(a, b):
    """Parameters, both moments, the step count and the two generator states of two state files, exactly."""
    a, b = torch.load(a, weights_only=True), torch.load(b, weights_only=True)
    assert a["completed"] == b["completed"] and a["train_step"]["step"] == b["train_step"]["step"] > 0
    for group in ("p_net", "q_net"):
        assert sorted(a["train_step"][group]) == sorted(b["train_step"][group])
        for k, v in a["train_step"][group].items():
            assert torch.equal(v, b["train_step"][group][k]), (group, k)
            for m in ("exp_avg", "exp_avg_sq"):
                if k in a["train_step"][m][group]:
                    assert torch.equal(a["train_step"][m][group][k], b["train_step"][m][group][k]), (m, group, k)
    assert sorted(a["rng"]) == sorted(b["rng"])
    for k, v in a["rng"].items():
        assert torch.equal(v, b["rng"][k]) if torch.is_tensor(v) else v == b["rng"][k], k
    assert a["lines"] == b["lines"]


_SMALL = ["--p_hidden_dim", "32", "--q_hidden_dim", "32", "--progress_every", "0", "--save_interval", "2", "--checkpoint_interval", "2",
          "--num_epochs", "4", "-l", "1e-3"]
CASES = {
    # 200 = 3 x 64 + 8 and 100 = 3 x 32 + 4: a ragged last minibatch; --save_interval 2 puts an image dump (and its draws) on
    # both sides of the stop
    "mnist": ("train_mnist.py", ["--synthetic", "200", "--seed", "5", "--minibatch_size", "64"] + _SMALL),
    # the z_scale switch (epoch index 3) and the np.random augmentation angles of epochs 3 and 4 fall on the resumed side
    "galaxy_augment_zdelay": ("train_galaxy.py", ["x", "y", "--synthetic", "100", "--seed", "6", "--minibatch_size", "32", "-z", "3",
                                                  "--augment_rotation", "--z_delay", "3"] + _SMALL),
    "particles_fit_noise": ("train_particles.py", ["x", "y", "--synthetic", "100", "--seed", "7", "--minibatch-size", "32", "--fit-noise"]
                            + [a if not a.startswith("--") else a.replace("_", "-") for a in _SMALL]),
    "mnist_vanilla": ("train_mnist.py", ["--synthetic", "200", "--seed", "8", "--minibatch_size", "64", "--vanilla"] + _SMALL),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_resumed_run_is_the_uninterrupted_run(tmp_path, case):
    """Run A goes through its 4 epochs; run B starts from A's epoch-2 state file with the same arguments under another prefix.
    B's rows for epochs 3 and 4 are A's strings, train.txt / val.txt are identical files, the final .sav state-dicts and the
    final state files (parameters, moments, step count, generator states) are equal exactly."""
    script, args = CASES[case]
    particles = script == "train_particles.py"
    flag = "--save-prefix" if particles else "--save_prefix"
    cwd = str(tmp_path)
    a = _cli(script, args + [flag, "a"], cwd)
    base = (lambda p: str(tmp_path / p)) if particles else (lambda p: str(tmp_path / ("outputs_" + p) / "trained" / p))
    assert os.path.exists(base("a") + "_state_epoch2.ckpt") and os.path.exists(base("a") + "_state_epoch4.ckpt")
    assert not glob.glob(base("a") + "_state_epoch*.tmp*")
    b = _cli(script, args + [flag, "b", "--resume", base("a") + "_state_epoch2.ckpt"], cwd)
    assert len(a) == 1 + 8 and len(b) == 1 + 4 and a[0] == b[0]
    assert a[5:] == b[1:], (a[5:], b[1:])                            # the same STRINGS
    assert not os.path.exists(base("b") + "_state_epoch2.ckpt")      # B wrote epoch 4's only
    if not particles:
        for f in ("train.txt", "val.txt"):
            fa, fb = (tmp_path / "outputs_a" / f).read_bytes(), (tmp_path / "outputs_b" / f).read_bytes()
            assert fa == fb and len(fa.splitlines()) == 5, f
    for tag in ("generator", "inference"):
        sa, sb = _sd(base("a") + "_%s_epoch4.sav" % tag), _sd(base("b") + "_%s_epoch4.sav" % tag)
        assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), tag
    _assert_same_state_files(base("a") + "_state_epoch4.ckpt", base("b") + "_state_epoch4.ckpt")
    two, four = torch.load(base("a") + "_state_epoch2.ckpt", weights_only=True), torch.load(base("a") + "_state_epoch4.ckpt", weights_only=True)
    assert four["train_step"]["step"] == 2 * two["train_step"]["step"] == 16          # 4 minibatches per epoch
    assert any(not torch.equal(v, four["train_step"]["p_net"][k]) for k, v in two["train_step"]["p_net"].items())


def test_resume_is_refused_before_training_when_the_run_differs(tmp_path):
    script, args = CASES["mnist"]
    short = [a if a != "4" else "2" for a in args]                   # two epochs are enough to have a state file
    _cli(script, short + ["--save_prefix", "a"], str(tmp_path))
    ck = str(tmp_path / "outputs_a" / "trained" / "a_state_epoch2.ckpt")
    for extra, word in ((["--num_epochs", "2"], "num_epochs"), (["--num_epochs", "4", "-z", "3"], "z_dim"),
                        (["--num_epochs", "4", "--synthetic", "240"], "synthetic")):
        out = subprocess.run([sys.executable, os.path.join(ROOT, script)] + short + ["--save_prefix", "b", "--resume", ck] + extra,
                             cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=LIMIT)
        assert out.returncode == 1 and "--resume" in out.stderr and word in out.stderr, out.stderr[-2000:]
        assert "Traceback" not in out.stderr
    data = open(ck, "rb").read()
    with open(str(tmp_path / "cut.ckpt"), "wb") as f:
        f.write(data[:len(data) // 2])
    out = subprocess.run([sys.executable, os.path.join(ROOT, script)] + short + ["--save_prefix", "b", "--num_epochs", "4", "--resume",
                                                                                   str(tmp_path / "cut.ckpt")],
                         cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 1 and "cannot read the state file" in out.stderr and "Traceback" not in out.stderr


# ---- 8. the loader keeps the modules inside the flat buffers ----------------------------------------------------------------
def _gpu_step(seed, dev):
    import spatial_vae.models as models
    from spatial_vae_amd import dp, elbo as E
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(2, 32, num_layers=2, activation=nn.Tanh).to(dev)
        q_net = models.InferenceNetwork(100, 5, 16, num_layers=2, activation=nn.Tanh).to(dev)
    return dp.TrainStep(p_net, q_net, E.eval_minibatch_mnist, lr=1e-2, rotate=True, translate=True, dx_scale=0.1,
                        theta_prior=math.pi / 4)


def test_loaded_state_lives_in_the_flat_buffers_and_training_moves_it():
    from spatial_vae_amd import cli, ops
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    x = cli.coord_grid(10, 10).to(dev)
    ys = [torch.from_numpy(rs.uniform(size=(16, 100)).astype(np.float32)).to(dev) for _ in range(5)]
    ns = [torch.from_numpy(rs.normal(size=(16, 5)).astype(np.float32)).to(dev) for _ in range(5)]
    a = _gpu_step(3, dev)
    assert isinstance(a.optim, ops.FlatAdam)
    for y, r in zip(ys[:3], ns[:3]):
        a(x, y, noise=r)
    state = a.state_dict()
    assert all(not t.is_cuda for t in state["p_net"].values()) and state["step"] == 3
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    state = torch.load(buf, weights_only=True)
    for y, r in zip(ys[3:], ns[3:]):
        a(x, y, noise=r)

    b = _gpu_step(4, dev)                                            # other weights, FlatAdam without state yet
    assert not b.optim.state.get(b.master)
    pad = torch.ones(b.grads.n, dtype=torch.bool, device=dev)
    for p, off in zip(b.grads.params, b.grads.offsets):
        pad[off:off + p.numel()] = False
    ptrs = [p.data_ptr() for p in b.grads.params]
    sinks = {k: v.data_ptr() for k, v in b.p_net._grad_sinks.items() if torch.is_tensor(v)}
    b.load_state_dict(state)
    assert b.aliased() and b.master.grad is b.grads.flat and [p.data_ptr() for p in b.grads.params] == ptrs
    assert {k: v.data_ptr() for k, v in b.p_net._grad_sinks.items() if torch.is_tensor(v)} == sinks
    lo, hi = b.grads.flat.data_ptr(), b.grads.flat.data_ptr() + 4 * b.grads.n
    assert all(lo <= p < hi for p in sinks.values())
    st = b.optim.state[b.master]
    assert st["step"] == 3 and float(b.grads.flat_param[pad].abs().max()) == 0.0 and float(st["exp_avg"][pad].abs().max()) == 0.0
    assert torch.equal(b.p_net.coord_linear.weight.detach().cpu(), state["p_net"]["coord_linear.weight"])
    before = b.p_net.coord_linear.weight.detach().clone()
    b(x, ys[3], noise=ns[3])
    assert not torch.equal(before, b.p_net.coord_linear.weight.detach()), "the optimiser stepped memory the module does not read"
    b(x, ys[4], noise=ns[4])
    torch.cuda.synchronize()
    sa = a.optim.state[a.master]
    assert torch.equal(a.grads.flat_param, b.grads.flat_param) and sa["step"] == st["step"] == 5
    assert torch.equal(sa["exp_avg"], st["exp_avg"]) and torch.equal(sa["exp_avg_sq"], st["exp_avg_sq"])


# ---- 9. two ranks sharing cuda:0 --------------------------------------------------------------------------------------------
_WORKER = r'''
import contextlib, io, math, os, sys
sys.path.insert(0, os.environ["SVAE_ROOT"])
import numpy as np, torch, torch.nn as nn, torch.distributed as dist
import spatial_vae.models as models
from spatial_vae_amd import dp, elbo as E, cli

mode, tmp = os.environ["SVAE_MODE"], os.environ["SVAE_TMP"]          # through | resume
rank, world, local = dp.init_process_group(device_is_gpu=True)
dev = torch.device("cuda", local)
torch.cuda.set_device(dev)
n = m = 12
# a resumed rank starts from weights of its OWN (and rank 1 from other ones than rank 0): only the load may make them equal
torch.manual_seed((100 if mode == "through" else 500) + rank)
with contextlib.redirect_stdout(io.StringIO()):
    p_net = models.SpatialGenerator(2, 64, num_layers=2, activation=nn.Tanh).to(dev)
    q_net = models.InferenceNetwork(n * m, 5, 32, num_layers=2, activation=nn.Tanh).to(dev)
step = dp.TrainStep(p_net, q_net, E.eval_minibatch_mnist, lr=1e-2, rotate=True, translate=True, dx_scale=0.1,
                    theta_prior=math.pi / 4)
x = cli.coord_grid(n, m).to(dev)
rs = np.random.RandomState(7)
sizes = [8, 7, 1, 6, 8, 5, 1, 6]                    # ragged and EMPTY shards on both sides of the stop after step 4
ys = [torch.from_numpy(rs.uniform(size=(b, n * m)).astype(np.float32)).to(dev) for b in sizes]
ns = [torch.from_numpy(rs.normal(size=(b, 5)).astype(np.float32)).to(dev) for b in sizes]

def run(lo_i, hi_i):
    for y, r in zip(ys[lo_i:hi_i], ns[lo_i:hi_i]):
        lo, hi = dp.shard_bounds(y.size(0), rank, world)
        step(x, y[lo:hi], weight=(hi - lo) / y.size(0), global_batch=y.size(0), noise=r[lo:hi])

def gathered(t):
    both = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(both, t)
    return both

name = os.environ["SVAE_FROM"]
if mode == "through":
    run(0, 4)
    if rank == 0:
        torch.save(step.state_dict(), os.path.join(tmp, "state_w%d.pt" % world))
    run(4, 8)
    torch.cuda.synchronize()
    if rank == 0:
        torch.save({"flat": step.grads.flat_param.detach().cpu(), "exp_avg": step.optim.state[step.master]["exp_avg"].cpu(),
                    "exp_avg_sq": step.optim.state[step.master]["exp_avg_sq"].cpu()}, os.path.join(tmp, "final_w%d.pt" % world))
    print("rank", rank, "through ok")
else:
    before = step.grads.flat_param.detach().clone()
    step.load_state_dict(torch.load(os.path.join(tmp, "state_%s.pt" % name), weights_only=True))
    st = step.optim.state[step.master]
    assert step.aliased() and st["step"] == 4 and not torch.equal(before, step.grads.flat_param)
    if world > 1:
        for t in (step.grads.flat_param, st["exp_avg"], st["exp_avg_sq"]):
            both = gathered(t)
            assert torch.equal(both[0], both[1]), "replicas differ after the load"
    run(4, 8)
    torch.cuda.synchronize()
    ref = torch.load(os.path.join(tmp, "final_%s.pt" % name), weights_only=True)
    flat = step.grads.flat_param.detach().cpu()
    if world > 1:
        both = gathered(step.grads.flat_param)
        assert torch.equal(both[0], both[1]), "replicas diverged"
    perr = (flat - ref["flat"]).abs().max().item() / ref["flat"].abs().max().item()
    print("rank", rank, "resume from", name, "under", world, "param err %.3e" % perr)
    if name == "w%d" % world:                       # the same world size: bit for bit, moments included
        assert torch.equal(flat, ref["flat"]), perr
        assert torch.equal(st["exp_avg"].cpu(), ref["exp_avg"]) and torch.equal(st["exp_avg_sq"].cpu(), ref["exp_avg_sq"])
    else:                                           # another world size: another summation order (tests/test_gpu_dp.py's figure)
        assert perr < 2e-6, perr
if dist.is_initialized():
    dist.destroy_process_group()
'''


def _worker(tmp_path, mode, source, ranks):
    script = tmp_path / "resume_worker.py"
    script.write_text(_WORKER)
    env = _env(SVAE_ROOT=ROOT, SVAE_MODE=mode, SVAE_TMP=str(tmp_path), SVAE_FROM=source)
    if ranks == 1:
        cmd = [sys.executable, str(script)]
    else:
        env["SVAE_SHARE_GPU"] = "1"
        cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
               "sys.exit(dp.launch_ranks(%d, [%r], timeout=%d))" % (ROOT, ranks, str(script), LIMIT - 30)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=LIMIT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert len([l for l in out.stdout.splitlines() if l.startswith("rank")]) == ranks
    return out.stdout


def test_two_ranks_resume_exactly_and_one_rank_state_resumes_under_two(tmp_path):
    """TrainStep under two ranks sharing cuda:0 (gloo): an 8-step run stopped after step 4 and resumed by two NEW ranks that were
    initialised differently (from each other and from the stored run) is bit-equal to the uninterrupted two-rank run, and the
    replicas are bit-equal right after the load.  The one-rank run's state resumed under two ranks stays within 2e-6 of the
    one-rank continuation."""
    _worker(tmp_path, "through", "-", 2)
    _worker(tmp_path, "resume", "w2", 2)
    _worker(tmp_path, "through", "-", 1)
    _worker(tmp_path, "resume", "w1", 1)                              # one rank continues itself bit for bit
    _worker(tmp_path, "resume", "w1", 2)


def test_command_line_under_two_ranks_resumes_exactly(tmp_path):
    """train_mnist.py under two ranks sharing cuda:0: every rank opens the state file, rank 0 alone writes; the resumed two-rank
    run prints the uninterrupted two-rank run's rows and ends in the same parameters, moments and generator states."""
    script, args = CASES["mnist"]
    a = _cli(script, args + ["--save_prefix", "a"], str(tmp_path), ranks=2)
    base = lambda p: str(tmp_path / ("outputs_" + p) / "trained" / p)  # noqa: E731
    b = _cli(script, args + ["--save_prefix", "b", "--resume", base("a") + "_state_epoch2.ckpt"], str(tmp_path), ranks=2)
    assert len(a) == 9 and a[5:] == b[1:], (a[5:], b[1:])
    assert (tmp_path / "outputs_a" / "train.txt").read_bytes() == (tmp_path / "outputs_b" / "train.txt").read_bytes()
    _assert_same_state_files(base("a") + "_state_epoch4.ckpt", base("b") + "_state_epoch4.ckpt")
    assert torch.load(base("b") + "_state_epoch4.ckpt", weights_only=True)["world"] == 2


# ---- 10. the reference's own .sav files on the GPU --------------------------------------------------------------------------
GENERATORS = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "sav_*.sav"))
                    if not os.path.basename(f).startswith("sav_inf_"))


@pytest.mark.parametrize("name", GENERATORS)
def test_reference_written_generator_runs_on_the_gpu_and_saves_back(tmp_path, name):
    from spatial_vae_amd import cli
    assert len(GENERATORS) == 7
    with np.load(os.path.join(GOLDEN, "sav_%s.npz" % name), allow_pickle=False) as f:
        fx = {k: f[k] for k in f.files}
    dev = torch.device("cuda:0")
    p_net = torch.load(os.path.join(GOLDEN, "sav_%s.sav" % name), weights_only=False).to(dev)        # committed data
    q_net = torch.load(os.path.join(GOLDEN, "sav_inf_plain.sav"), weights_only=False).to(dev)        # committed data
    with torch.no_grad():
        y = p_net(torch.from_numpy(fx["x"]).to(dev), torch.from_numpy(fx["z"]).to(dev))
    err = rel_err(y.cpu().numpy(), fx["y_hat"])
    print("%s: y_hat rel err %.3e" % (name, err))
    assert y.shape == fx["y_hat"].shape and err < 2e-5, err
    cli.save_models(str(tmp_path / "back"), "1", p_net, q_net, dev)
    sd = _sd(str(tmp_path / "back_generator_epoch1.sav"))
    assert sorted(sd) == sorted(k[3:] for k in fx if k.startswith("sd."))
    for k, v in sd.items():
        assert not v.is_cuda and torch.equal(v, torch.from_numpy(fx["sd." + k])), k
    ctor = json.loads(str(fx["ctor"]))
    assert type(p_net).__name__ == ctor["cls"]
