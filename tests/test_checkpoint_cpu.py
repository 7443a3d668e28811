"""Checkpoints without a GPU: whole-module `.sav` interchange with the reference (fixtures written by the reference:
tests/golden/gen_sav_golden.py), dp.TrainStep.state_dict / load_state_dict on the CPU path (torch.optim.Adam on the flat
master), the checkpoint file of the command lines, its refusals and the new flags.  The same contract on the MI355X, end to
end and bit for bit, is tests/test_gpu_resume.py."""
import argparse
import contextlib
import glob
import io
import json
import os
import pickletools
import subprocess
import sys
import zipfile

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACT = {"tanh": nn.Tanh, "leakyrelu": nn.LeakyReLU, "relu": nn.ReLU, "sigmoid": nn.Sigmoid}
FIXTURES = sorted(os.path.basename(f)[4:-4] for f in glob.glob(os.path.join(GOLDEN, "sav_*.sav")))


def _fixture(name):
    with np.load(os.path.join(GOLDEN, "sav_%s.npz" % name), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _construct(ctor):
    import spatial_vae_amd.models as M
    kw = dict(ctor["kwargs"], activation=ACT[ctor["kwargs"]["activation"]])
    with contextlib.redirect_stdout(io.StringIO()):
        return getattr(M, ctor["cls"])(*ctor["args"], **kw)


def _pickle_of(path):
    with zipfile.ZipFile(path) as z:
        return z.read([n for n in z.namelist() if n.endswith("/data.pkl")][0])


def _strings(pkl):
    out = []
    for _, arg, _ in pickletools.genops(pkl):
        if isinstance(arg, bytes):
            arg = arg.decode("latin-1")
        if isinstance(arg, str):
            out.append(arg)
    return out


def test_fixture_set_is_complete():
    assert FIXTURES == sorted(["gen_tanh_L2", "gen_leaky_resid_bilinear_expand_L3", "gen_z0", "gen_softplus_nout2", "gen_relu",
                               "gen_sigmoid", "inf_plain", "inf_resid", "vanilla"])


# ---- 1. what a module saved here looks like ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gen_leaky_resid_bilinear_expand_L3", "inf_resid", "vanilla", "gen_z0"])
def test_saved_module_carries_the_reference_class_path_and_attribute_set(tmp_path, name):
    """All four classes (ResidLinear rides inside the resid variants): the pickle names spatial_vae.models, never
    spatial_vae_amd, and the pickled __dict__ has exactly the keys the reference's has (no _spec, no _grad_sinks)."""
    fx = _fixture(name)
    net = _construct(json.loads(str(fx["ctor"])))
    net._grad_sinks = {"x": torch.zeros(1)}                 # what dp.TrainStep hangs on a module
    path = str(tmp_path / "m.sav")
    torch.save(net, path)
    strings = _strings(_pickle_of(path))
    assert any(s.startswith("spatial_vae.models") for s in strings)
    assert not any("spatial_vae_amd" in s for s in strings), [s for s in strings if "spatial_vae_amd" in s]
    assert "_spec" not in strings and "_grad_sinks" not in strings
    assert sorted(net.__getstate__()) == sorted(str(k) for k in fx["dict_keys"])
    if "resid" in name:
        assert "ResidLinear" in strings or "spatial_vae.models ResidLinear" in strings
    assert "_grad_sinks" in net.__dict__                    # saving does not strip the live module
    back = torch.load(path, weights_only=False)             # a file this test just wrote
    assert type(back) is type(net) and not hasattr(back, "_grad_sinks")
    assert getattr(back, "_spec", None) == getattr(net, "_spec", None)


def test_class_objects_are_shared_between_the_two_import_paths():
    import spatial_vae.models as A
    import spatial_vae_amd.models as B
    for n in ("ResidLinear", "InferenceNetwork", "SpatialGenerator", "VanillaGenerator"):
        assert getattr(A, n) is getattr(B, n) and getattr(A, n).__module__ == "spatial_vae.models"


# ---- 2. what the reference wrote loads here ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_written_module_loads(name):
    import spatial_vae_amd.models as M
    fx = _fixture(name)
    ctor = json.loads(str(fx["ctor"]))
    net = torch.load(os.path.join(GOLDEN, "sav_%s.sav" % name), weights_only=False)      # committed data, written by the reference
    assert isinstance(net, getattr(M, ctor["cls"]))
    sd = net.state_dict()
    assert sorted(sd) == sorted(k[3:] for k in fx if k.startswith("sd."))
    for k, v in sd.items():
        assert torch.equal(v, torch.from_numpy(fx["sd." + k])), k
    fresh = _construct(ctor)
    if ctor["cls"] == "SpatialGenerator":
        assert net._spec == fresh._spec
    assert sorted(net.__getstate__()) == sorted(str(k) for k in fx["dict_keys"]) == sorted(fresh.__getstate__())
    if ctor["cls"] == "VanillaGenerator":                   # ordinary torch: the reference's output, on the CPU
        with torch.no_grad():
            y = net(torch.from_numpy(fx["x"]), torch.from_numpy(fx["z"]))
        assert torch.equal(y, torch.from_numpy(fx["y_hat"]))


def test_module_pickled_by_an_earlier_build_still_loads(tmp_path):
    """Earlier builds pickled under spatial_vae_amd.models and with _spec inside."""
    import spatial_vae_amd.models as M
    net = _construct({"cls": "SpatialGenerator", "args": [2, 8], "kwargs": {"num_layers": 3, "activation": "tanh", "resid": True}})
    classes = (M.ResidLinear, M.SpatialGenerator)
    keep = M._ReferencePickle.__getstate__
    try:
        for c in classes:
            c.__module__ = "spatial_vae_amd.models"
        M._ReferencePickle.__getstate__ = lambda self: dict(self.__dict__)
        path = str(tmp_path / "old.sav")
        torch.save(net, path)
    finally:
        M._ReferencePickle.__getstate__ = keep
        for c in classes:
            c.__module__ = "spatial_vae.models"
    strings = _strings(_pickle_of(path))
    assert any(s.startswith("spatial_vae_amd.models") for s in strings) and "_spec" in strings
    back = torch.load(path, weights_only=False)             # a file this test just wrote
    assert type(back) is M.SpatialGenerator and back._spec == net._spec
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), net.state_dict().values()))


def test_unsupported_activation_or_slope_is_refused_at_load(tmp_path):
    import spatial_vae_amd.models as M
    net = _construct({"cls": "SpatialGenerator", "args": [2, 8], "kwargs": {"num_layers": 2, "activation": "leakyrelu"}})
    net.layers[0].negative_slope = 0.2
    torch.save(net, str(tmp_path / "slope.sav"))
    with pytest.raises(NotImplementedError, match="LeakyReLU slope"):
        torch.load(str(tmp_path / "slope.sav"), weights_only=False)
    net = _construct({"cls": "SpatialGenerator", "args": [2, 8], "kwargs": {"num_layers": 2, "activation": "tanh"}})
    net.layers[0] = nn.ELU()
    torch.save(net, str(tmp_path / "elu.sav"))
    with pytest.raises(NotImplementedError, match="supports activations"):
        torch.load(str(tmp_path / "elu.sav"), weights_only=False)
    assert M.SpatialGenerator.__module__ == "spatial_vae.models"


# ---- 3. TrainStep.state_dict / load_state_dict on the CPU path --------------------------------------------------------------
def _toy_elbo(x, y, p_net, q_net, noise=None):
    q = q_net(y)
    mu, logstd = q[:, :2], q[:, 2:]
    z = mu + logstd.exp() * noise
    y_hat = p_net(z)
    log_p = -((y_hat - y) ** 2).sum(1).mean()
    kl = (-logstd + 0.5 * logstd.exp() ** 2 + 0.5 * mu ** 2 - 0.5).sum(1).mean()
    return log_p - kl, log_p, kl


def _toy_nets(seed):
    torch.manual_seed(seed)
    return (nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 5)),
            nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 4)))


def _padding_mask(step):
    pad = torch.ones(step.grads.n, dtype=torch.bool)
    for p, off in zip(step.grads.params, step.grads.offsets):
        pad[off:off + p.numel()] = False
    return pad


def test_trainstep_state_round_trip_is_exact_on_cpu():
    from spatial_vae_amd import dp
    gen = torch.Generator().manual_seed(5)
    ys = [torch.randn(b, 5, generator=gen) for b in (8, 5, 7, 6, 3)]
    rs = [torch.randn(b, 2, generator=gen) for b in (8, 5, 7, 6, 3)]
    a = dp.TrainStep(*_toy_nets(1), _toy_elbo, lr=1e-2)
    for y, r in zip(ys[:3], rs[:3]):
        a(None, y, noise=r)
    rng_before = torch.get_rng_state()
    state = a.state_dict()
    assert torch.equal(rng_before, torch.get_rng_state())            # taking the state draws nothing
    assert state["step"] == 3 and state["lr"] == 1e-2 and state["betas"] == [0.9, 0.999]
    assert set(state["p_net"]) == {"0.weight", "0.bias", "2.weight", "2.bias"} == set(state["exp_avg"]["p_net"])
    frozen = torch.load(_saved(state), weights_only=True)            # what a file would hold: survives the steps below
    for y, r in zip(ys[3:], rs[3:]):
        a(None, y, noise=r)

    b = dp.TrainStep(*_toy_nets(2), _toy_elbo, lr=1e-2)              # differently initialised, no step run yet
    assert not torch.equal(a.grads.flat_param, b.grads.flat_param) and not b.optim.state.get(b.master)
    pad = _padding_mask(b)
    b.grads.flat_param[pad] = 7.0                                    # mark the padding: the load must not write there
    ptrs = [p.data_ptr() for p in b.grads.params]
    b.load_state_dict(frozen)
    assert b.aliased() and b.master.grad is b.grads.flat and [p.data_ptr() for p in b.grads.params] == ptrs
    assert bool((b.grads.flat_param[pad] == 7.0).all())
    st = b.optim.state[b.master]
    assert float(st["step"]) == 3.0 and bool((st["exp_avg"][pad] == 0).all()) and bool((st["exp_avg_sq"][pad] == 0).all())
    b.grads.flat_param[pad] = 0.0
    for y, r in zip(ys[3:], rs[3:]):
        b(None, y, noise=r)
    sa, sb = a.optim.state[a.master], b.optim.state[b.master]
    assert torch.equal(a.grads.flat_param, b.grads.flat_param)
    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert float(sa["step"]) == float(sb["step"]) == 5.0


def _saved(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return buf


def test_trainstep_load_names_the_offending_tensor():
    from spatial_vae_amd import dp
    a = dp.TrainStep(*_toy_nets(1), _toy_elbo, lr=1e-2)
    good = a.state_dict()
    bad = torch.load(_saved(good), weights_only=True)
    bad["q_net"]["2.weight"] = torch.zeros(3, 8)
    with pytest.raises(ValueError, match=r"q_net\.2\.weight"):
        a.load_state_dict(bad)
    bad = torch.load(_saved(good), weights_only=True)
    bad["p_net"]["0.bias"] = bad["p_net"]["0.bias"].double()
    with pytest.raises(ValueError, match=r"p_net\.0\.bias"):
        a.load_state_dict(bad)
    bad = torch.load(_saved(good), weights_only=True)
    bad["p_net"]["9.weight"] = bad["p_net"].pop("0.weight")
    with pytest.raises(KeyError, match=r"0\.weight.*9\.weight"):
        a.load_state_dict(bad)
    bad = torch.load(_saved(good), weights_only=True)
    del bad["exp_avg_sq"]["q_net"]["0.bias"]
    with pytest.raises(KeyError, match=r"q_net\.0\.bias.*exp_avg_sq"):
        a.load_state_dict(bad)
    bad = dict(good, version=99)
    with pytest.raises(ValueError, match="version"):
        a.load_state_dict(bad)
    assert a.aliased()


_DP_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["SVAE_ROOT"])
import torch, torch.nn as nn, torch.distributed as dist
from spatial_vae_amd import dp
sys.path.insert(0, os.path.join(os.environ["SVAE_ROOT"], "tests"))
from test_checkpoint_cpu import _toy_elbo, _toy_nets

rank, world, _ = dp.init_process_group(device_is_gpu=False)
step = dp.TrainStep(*_toy_nets(50 + rank), _toy_elbo, lr=1e-2)
state = torch.load(os.environ["SVAE_STATE"], weights_only=True)
if rank == 1:                                       # this rank "read something else": every tensor perturbed, another step count
    for group in (state["p_net"], state["q_net"], state["exp_avg"]["p_net"], state["exp_avg"]["q_net"],
                  state["exp_avg_sq"]["p_net"], state["exp_avg_sq"]["q_net"]):
        for k in group:
            group[k] = group[k] + 1.0
    state["step"] = 11
step.load_state_dict(state)
assert step.aliased()
st = step.optim.state[step.master]
for t in (step.grads.flat_param, st["exp_avg"], st["exp_avg_sq"]):
    both = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(both, t)
    assert torch.equal(both[0], both[1]), "replicas differ after the load"
assert float(st["step"]) == 3.0, st["step"]
good = torch.load(os.environ["SVAE_STATE"], weights_only=True)
mine = step.state_dict()
for key in ("p_net", "q_net"):
    for k, v in good[key].items():
        assert torch.equal(mine[key][k], v), (key, k)
        assert torch.equal(mine["exp_avg"][key][k], good["exp_avg"][key][k])
        assert torch.equal(mine["exp_avg_sq"][key][k], good["exp_avg_sq"][key][k])
gen = torch.Generator().manual_seed(9)              # and the replicas stay bit-equal through a further (sharded) step
y, r = torch.randn(6, 5, generator=gen), torch.randn(6, 2, generator=gen)
lo, hi = dp.shard_bounds(6, rank, world)
step(None, y[lo:hi], weight=(hi - lo) / 6, noise=r[lo:hi])
both = [torch.empty_like(step.grads.flat_param) for _ in range(world)]
dist.all_gather(both, step.grads.flat_param)
assert torch.equal(both[0], both[1])
print("rank", rank, "state ok")
dist.destroy_process_group()
'''


def test_two_gloo_ranks_are_bit_equal_after_loading_different_states(tmp_path):
    from spatial_vae_amd import dp
    gen = torch.Generator().manual_seed(5)
    a = dp.TrainStep(*_toy_nets(1), _toy_elbo, lr=1e-2)
    for b in (8, 5, 7):
        a(None, torch.randn(b, 5, generator=gen), noise=torch.randn(b, 2, generator=gen))
    torch.save(a.state_dict(), str(tmp_path / "state.pt"))
    script = tmp_path / "state_worker.py"
    script.write_text(_DP_WORKER)
    env = dict(os.environ, SVAE_ROOT=ROOT, SVAE_STATE=str(tmp_path / "state.pt"), OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    code = ("import sys; sys.path.insert(0, %r); from spatial_vae_amd import dp; "
            "sys.exit(dp.launch_ranks(2, [%r]))" % (ROOT, str(script)))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.count("state ok") == 2


# ---- 4. the checkpoint file -------------------------------------------------------------------------------------------------
def _args(**over):
    base = dict(z_dim=2, p_hidden_dim=32, q_hidden_dim=32, num_layers=2, activation="tanh", vanilla=False, no_rotate=False,
                no_translate=False, dx_scale=0.1, theta_prior=np.pi / 4, learning_rate=1e-4, minibatch_size=64, save_prefix="a",
                save_interval=10, num_epochs=4, device=-2, synthetic=200, progress_every=0, seed=3, gemm=None, resume=None,
                checkpoint_interval=2, z_delay=0, augment_rotation=False, fit_noise=False, mask=False, ctf_train=None)
    base.update(over)
    return argparse.Namespace(**base)


def _fingerprint(scale=1.0):
    from spatial_vae_amd import cli
    g = torch.Generator().manual_seed(0)
    return cli.dataset_fingerprint(torch.rand(20, 16, generator=g) * scale, torch.rand(5, 16, generator=g))


def _one_step():
    from spatial_vae_amd import dp
    step = dp.TrainStep(*_toy_nets(1), _toy_elbo, lr=1e-4)           # (seeds torch: build it before looking at generator states)
    step(None, torch.ones(4, 5), noise=torch.ones(4, 2))
    return step


def _write(path, completed=2, args=None, fingerprint=None, step=None):
    from spatial_vae_amd import cli
    step = step or _one_step()
    lines = dict(train_lines=["h", "0\t1.0\t2.0\t3.0"], val_lines=["h", "0\t1.5\t2.5\t3.5"], rows=[])
    cli.write_checkpoint(str(path), step.state_dict(), completed, args or _args(), 1, fingerprint or _fingerprint(), lines)
    return step


def test_checkpoint_file_round_trip_and_generator_states(tmp_path):
    from spatial_vae_amd import cli
    step = _one_step()
    fingerprint = _fingerprint()
    torch.manual_seed(17)
    np.random.seed(17)
    torch.randn(5), np.random.rand(3), np.random.normal()            # somewhere inside both streams, a cached gaussian pending
    before = cli.rng_state()
    path = tmp_path / "a_state_epoch2.ckpt"
    _write(path, step=step, fingerprint=fingerprint)
    after = cli.rng_state()
    assert torch.equal(before["torch"], after["torch"]) and torch.equal(before["numpy_keys"], after["numpy_keys"])
    assert {k: v for k, v in before.items() if not torch.is_tensor(v)} == {k: v for k, v in after.items() if not torch.is_tensor(v)}
    assert os.listdir(tmp_path) == ["a_state_epoch2.ckpt"]           # the temporary name is gone
    went_on = (torch.randn(4), np.random.rand(2), np.random.randint(0, 1000, 5), np.random.normal(size=3))
    torch.manual_seed(99)
    np.random.seed(99)
    ck = torch.load(str(path), weights_only=True)                    # the weights-only unpickler reads the whole file
    assert set(ck) == set(cli.read_checkpoint(str(path)))
    ck = cli.read_checkpoint(str(path))
    assert ck["version"] == cli.CHECKPOINT_VERSION and ck["completed"] == 2 and ck["world"] == 1
    assert ck["args"]["theta_prior"] == np.pi / 4 and ck["args"]["gemm"] is None and ck["args"]["vanilla"] is False
    assert ck["lines"]["train_lines"] == ["h", "0\t1.0\t2.0\t3.0"]
    assert ck["fingerprint"]["train_shape"] == [20, 16] and ck["fingerprint"]["sums"].dtype == torch.float64
    mine = step.state_dict()
    assert ck["train_step"]["step"] == 1
    for key in ("p_net", "q_net"):
        for k, v in mine[key].items():
            assert torch.equal(ck["train_step"][key][k], v)
            assert torch.equal(ck["train_step"]["exp_avg_sq"][key][k], mine["exp_avg_sq"][key][k])
    cli.set_rng_state(ck["rng"])
    resumed = (torch.randn(4), np.random.rand(2), np.random.randint(0, 1000, 5), np.random.normal(size=3))
    assert torch.equal(went_on[0], resumed[0])
    assert all(np.array_equal(a, b) for a, b in zip(went_on[1:], resumed[1:]))


def test_interrupted_write_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    from spatial_vae_amd import cli
    path = tmp_path / "a_state_epoch2.ckpt"
    _write(path)
    good = path.read_bytes()

    def failing_save(obj, f, *a, **k):
        with open(f, "wb") as fh:
            fh.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", failing_save)
    with pytest.raises(OSError, match="disk full"):
        _write(path, completed=4)
    with pytest.raises(OSError, match="disk full"):
        _write(tmp_path / "a_state_epoch4.ckpt", completed=4)
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["a_state_epoch2.ckpt"] and path.read_bytes() == good
    assert cli.read_checkpoint(str(path))["completed"] == 2


_FLOW_WORKER = r'''
import sys, os, io, contextlib
sys.path.insert(0, os.environ["SVAE_ROOT"])
import numpy as np, torch, torch.nn as nn
from spatial_vae_amd import cli, dp, elbo as E
import train_mnist

def toy(x, y, p_net, q_net, rotate=None, translate=None, dx_scale=None, theta_prior=None, noise=None):
    q = q_net(y); mu, ls = q[:, :2], q[:, 2:]
    z = mu + ls.exp() * noise
    yh = torch.sigmoid(p_net(z))
    log_p = -((yh - y) ** 2).sum(1).mean()
    kl = (-ls + 0.5 * ls.exp() ** 2 + 0.5 * mu ** 2 - 0.5).sum(1).mean()
    return log_p - kl, log_p, kl, yh
E.eval_minibatch_mnist = toy
cli.pick_device = lambda d, world=1, local=0: torch.device("cpu")

def build(args, device):
    tr = cli.synthetic_images("mnist", args.synthetic, 28, 28, 1, 0)
    te = cli.synthetic_images("mnist", args.synthetic // 4, 28, 28, 1, 1)
    y_train = torch.from_numpy(tr).float().div(255).view(-1, 784); y_test = torch.from_numpy(te).float().div(255).view(-1, 784)
    p = nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 784))
    q = nn.Sequential(nn.Linear(784, 8), nn.Tanh(), nn.Linear(8, 4)); q.latent_dim = 2
    return dict(y_train=y_train, y_test=y_test, n=28, m=28, p_net=p, q_net=q, rotate=False, translate=False, table=["Epoch", "ELBO", "BCE loss", "KL"])

def run(extra):
    args = train_mnist.mnist_arguments(["--synthetic", "200", "--seed", "5", "--minibatch_size", "64", "--num_epochs", "4", "--progress_every", "0",
                                        "--save_interval", "100", "--checkpoint_interval", "2", "-l", "1e-2"] + extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.train_main("mnist", args, build)
    return [l for l in buf.getvalue().splitlines() if "\t" in l]

a = run(["--save_prefix", "a"])
b = run(["--save_prefix", "b", "--resume", "outputs_a/trained/a_state_epoch2.ckpt"])
print(a); print(b)
assert a[5:] == b[1:] and len(b) == 5
assert open("outputs_a/train.txt").read() == open("outputs_b/train.txt").read()
fa, fb = (torch.load("outputs_%s/trained/%s_state_epoch4.ckpt" % (p, p), weights_only=True) for p in "ab")
for g in ("p_net", "q_net"):
    for k in fa["train_step"][g]:
        assert torch.equal(fa["train_step"][g][k], fb["train_step"][g][k])
        assert torch.equal(fa["train_step"]["exp_avg_sq"][g][k], fb["train_step"]["exp_avg_sq"][g][k])
assert torch.equal(fa["rng"]["torch"], fb["rng"]["torch"]) and torch.equal(fa["rng"]["numpy_keys"], fb["rng"]["numpy_keys"])
assert fa["train_step"]["step"] == fb["train_step"]["step"] == 16
print(sorted(os.listdir("outputs_b/trained")))
for bad in (["--num_epochs", "2"], ["-z", "3"]):
    try:
        run(["--save_prefix", "c", "--resume", "outputs_a/trained/a_state_epoch2.ckpt"] + bad); raise AssertionError
    except SystemExit as e:
        print("refused:", e)
print("FLOW OK")
'''


def test_train_main_resumes_bit_for_bit_with_a_toy_elbo_on_cpu(tmp_path):
    """The whole loop of cli.train_main -- plans, draws, rows, files, state files, the resume path -- in a child process with
    the device pick and the ELBO replaced by CPU stand-ins (the decoder has no CPU form): run A goes through 4 epochs, run B
    resumes A's epoch-2 state file; rows, train.txt, parameters, moments, step count and generator states are equal exactly
    and the refusals end the command line.  The real command lines on the MI355X: tests/test_gpu_resume.py."""
    script = tmp_path / "flow_worker.py"
    script.write_text(_FLOW_WORKER)
    env = dict(os.environ, SVAE_ROOT=ROOT, OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "SVAE_SHARE_GPU", "SVAE_DP_SOLO"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(script)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FLOW OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
_TRAJECTORY_ARGS = dict(z_dim=3, p_hidden_dim=64, q_hidden_dim=16, num_layers=3, activation="relu", vanilla=True, no_rotate=True,
                        no_translate=True, dx_scale=0.2, theta_prior=1.0, learning_rate=1e-3, minibatch_size=32, z_delay=1,
                        augment_rotation=True, fit_noise=True, mask=True, ctf_train="ctf.txt", gemm="fp16x3", seed=4, synthetic=100,
                        save_interval=2)


@pytest.mark.parametrize("field", sorted(_TRAJECTORY_ARGS))
def test_resume_refuses_an_argument_that_changes_the_run(tmp_path, field):
    from spatial_vae_amd import cli
    path = tmp_path / "s.ckpt"
    _write(path)
    ck = cli.read_checkpoint(str(path))
    cli.check_resume_args(ck, _args(), "mnist")                                          # the same arguments pass
    cli.check_resume_args(ck, _args(num_epochs=9, save_prefix="b", device=0, resume=str(path), checkpoint_interval=0,
                                    progress_every=5), "mnist")                          # and so do the free ones
    with pytest.raises(cli.CheckpointError, match=r"\b%s\b" % field):
        cli.check_resume_args(ck, _args(**{field: _TRAJECTORY_ARGS[field]}), "mnist")


def test_resume_refusals_of_version_fingerprint_and_finished_runs(tmp_path):
    from spatial_vae_amd import cli
    path = tmp_path / "s.ckpt"
    _write(path, completed=4)
    ck = cli.read_checkpoint(str(path))
    with pytest.raises(cli.CheckpointError, match="completed.*num_epochs"):
        cli.check_resume_args(ck, _args(), "mnist")
    with pytest.raises(cli.CheckpointError, match="completed.*num_epochs"):
        cli.check_resume_args(ck, _args(num_epochs=3), "mnist")
    cli.check_resume_args(ck, _args(num_epochs=5), "mnist")                              # extending the run is allowed
    cli.check_resume_args(ck, _args(num_epochs=5, save_interval=3), "particles")         # particles: the interval draws nothing
    cli.check_resume_fingerprint(ck, _fingerprint())
    with pytest.raises(cli.CheckpointError, match="fingerprint.*sums"):
        cli.check_resume_fingerprint(ck, _fingerprint(scale=1.0 + 1e-6))
    other = _fingerprint()
    other["train_shape"] = [19, 16]
    with pytest.raises(cli.CheckpointError, match="fingerprint.*train_shape"):
        cli.check_resume_fingerprint(ck, other)
    payload = torch.load(str(path), weights_only=True)
    payload["version"] = 99
    torch.save(payload, str(tmp_path / "v.ckpt"))
    with pytest.raises(cli.CheckpointError, match="version 99"):
        cli.read_checkpoint(str(tmp_path / "v.ckpt"))


def test_unreadable_state_files_give_one_clean_error(tmp_path):
    from spatial_vae_amd import cli
    path = tmp_path / "s.ckpt"
    _write(path)
    data = path.read_bytes()
    for name, content in (("cut.ckpt", data[:len(data) // 2]), ("tail.ckpt", data[:-40]), ("empty.ckpt", b""), ("text.ckpt", b"hello\n")):
        (tmp_path / name).write_bytes(content)
        with pytest.raises(cli.CheckpointError, match="cannot read the state file") as e:
            cli.read_checkpoint(str(tmp_path / name))
        assert e.value.__suppress_context__ and name in str(e.value)
    with pytest.raises(cli.CheckpointError, match="cannot read the state file"):
        cli.read_checkpoint(str(tmp_path / "missing.ckpt"))
    torch.save({"a": 1}, str(tmp_path / "other.ckpt"))
    with pytest.raises(cli.CheckpointError, match="not a training state file"):
        cli.read_checkpoint(str(tmp_path / "other.ckpt"))
    # the command line ends with the message (exit status 1), before it needs a GPU for anything but the device pick
    assert issubclass(cli.CheckpointError, SystemExit)


# ---- 6. the flags -----------------------------------------------------------------------------------------------------------
def test_the_three_parsers_take_the_flags_in_their_own_spelling():
    sys.path.insert(0, ROOT)
    import train_galaxy
    import train_mnist
    import train_particles
    a = train_mnist.mnist_arguments([])
    assert a.resume is None and a.checkpoint_interval == 0
    a = train_mnist.mnist_arguments(["--resume", "x.ckpt", "--checkpoint_interval", "5"])
    assert a.resume == "x.ckpt" and a.checkpoint_interval == 5
    a = train_galaxy.galaxy_arguments(["tr", "te"])
    assert a.resume is None and a.checkpoint_interval == 0
    a = train_galaxy.galaxy_arguments(["tr", "te", "--resume", "x.ckpt", "--checkpoint_interval", "5"])
    assert a.resume == "x.ckpt" and a.checkpoint_interval == 5
    a = train_particles.particle_arguments(["tr", "te"])
    assert a.resume is None and a.checkpoint_interval == 0
    a = train_particles.particle_arguments(["tr", "te", "--resume", "x.ckpt", "--checkpoint-interval", "5"])
    assert a.resume == "x.ckpt" and a.checkpoint_interval == 5
    with pytest.raises(SystemExit):
        train_particles.particle_arguments(["tr", "te", "--checkpoint_interval", "5"])
