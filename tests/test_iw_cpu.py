"""The host side of the K-sample importance-weighted bound (--num_samples / --eval_num_samples), without a GPU: the three
parsers, the noise plans, the resume check, and the refusals of everything that has no HIP device under it."""
import argparse
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parsers():
    sys.path.insert(0, ROOT)
    import train_galaxy
    import train_mnist
    import train_particles
    return train_mnist.mnist_arguments, train_galaxy.galaxy_arguments, train_particles.particle_arguments


def test_the_three_parsers_take_the_sample_counts_in_their_own_spelling():
    mnist, galaxy, particles = _parsers()
    for a in (mnist([]), galaxy(["tr", "te"]), particles(["tr", "te"])):
        assert a.num_samples == 1 and a.eval_num_samples == 1
    a = mnist(["--num_samples", "3", "--eval_num_samples", "5"])
    assert (a.num_samples, a.eval_num_samples) == (3, 5)
    a = galaxy(["tr", "te", "--num_samples", "4"])
    assert (a.num_samples, a.eval_num_samples) == (4, 4)             # validation follows training unless told otherwise
    a = galaxy(["tr", "te", "--eval_num_samples", "64"])
    assert (a.num_samples, a.eval_num_samples) == (1, 64)
    a = particles(["tr", "te", "--num-samples", "2", "--eval-num-samples", "1024"])
    assert (a.num_samples, a.eval_num_samples) == (2, 1024)
    for bad in (["--num_samples", "0"], ["--eval_num_samples", "1025"], ["--num-samples", "2"]):
        with pytest.raises(SystemExit):
            mnist(bad)
    with pytest.raises(SystemExit):
        particles(["tr", "te", "--num_samples", "2"])


def _parent_train_plan(cli, N, bs, inf_dim):
    """train_pass_plan as it was before the sample counts: the loader's draws, then one (b, inf_dim) draw per minibatch."""
    perm = cli.loader_order(N, True)
    batches = [perm[i:i + bs] for i in range(0, N, bs)]
    return batches, [torch.empty(b.numel(), inf_dim).normal_() for b in batches]


def _parent_eval_plan(cli, ntest, bs, inf_dim, shapes):
    order = cli.loader_order(ntest, False)
    tb = [order[i:i + bs] for i in range(0, ntest, bs)]
    noise, shown = [], []
    for i, b in enumerate(tb):
        noise.append(torch.empty(b.numel(), inf_dim).normal_())
        if i == 0:
            shown = [torch.empty(*s).normal_() for s in shapes(b.numel())]
    return tb, noise, shown


@pytest.mark.parametrize("K", [1, 3])
def test_the_pass_plans_draw_one_b_times_K_block_per_minibatch(K):
    """(b*K, inf_dim) per minibatch, the ragged last one included; with K = 1 the draws and the state torch's generator is
    left in equal those of the plan without the option, for the training pass and for an evaluation pass that dumps images.
    Display draws keep their single-sample shapes for any K."""
    from spatial_vae_amd import cli
    cpu = torch.device("cpu")
    N, bs, inf_dim = 23, 5, 7
    shapes = cli.display_draw_shapes("galaxy", inf_dim, 4)
    torch.manual_seed(11)
    batches, noise = cli.train_pass_plan(N, bs, inf_dim, cpu, num_samples=K)
    tb, enoise, shown = cli.eval_pass_plan(N, bs, inf_dim, cpu, None, shapes, num_samples=K)
    state = torch.get_rng_state()
    assert [tuple(r.shape) for r in noise] == [(b.numel() * K, inf_dim) for b in batches]
    assert [b.numel() for b in batches] == [5, 5, 5, 5, 3]
    assert [tuple(r.shape) for r in enoise] == [(b.numel() * K, inf_dim) for b in tb]
    assert [tuple(t.shape) for t in shown] == [(5, inf_dim), (5, 4)]
    torch.manual_seed(11)
    p_batches, p_noise = _parent_train_plan(cli, N, bs, inf_dim)
    p_tb, p_enoise, p_shown = _parent_eval_plan(cli, N, bs, inf_dim, shapes)
    p_state = torch.get_rng_state()
    assert all(torch.equal(a, b) for a, b in zip(batches, p_batches))              # the order does not depend on K
    if K == 1:
        assert torch.equal(state, p_state)
        for got, want in ((noise, p_noise), (enoise, p_enoise), (shown, p_shown)):
            assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
        torch.manual_seed(11)
        cli.train_pass_plan(N, bs, inf_dim, cpu)                                  # the keyword left out: the same again
        cli.eval_pass_plan(N, bs, inf_dim, cpu, None, shapes)
        assert torch.equal(torch.get_rng_state(), p_state)
    else:
        assert not torch.equal(state, p_state)


def _args(**over):
    base = dict(z_dim=2, learning_rate=1e-4, minibatch_size=64, save_prefix="a", num_epochs=4, seed=3, resume=None,
                checkpoint_interval=2, clip_grad_norm=None, skip_nonfinite=False, num_samples=1, eval_num_samples=1)
    base.update(over)
    return argparse.Namespace(**base)


def test_resume_reads_a_file_without_the_sample_counts_as_one_and_refuses_another_value():
    from spatial_vae_amd import cli
    old = {k: v for k, v in cli.plain_args(_args()).items() if k not in ("num_samples", "eval_num_samples")}
    ck = {"args": old, "completed": 2}
    cli.check_resume_args(ck, _args(), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"argument num_samples is 4 now .* written with 1"):
        cli.check_resume_args(ck, _args(num_samples=4), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\beval_num_samples\b"):
        cli.check_resume_args(ck, _args(eval_num_samples=16), "mnist")
    ck = {"args": cli.plain_args(_args(num_samples=3, eval_num_samples=5)), "completed": 2}
    cli.check_resume_args(ck, _args(num_samples=3, eval_num_samples=5), "particles")
    with pytest.raises(cli.CheckpointError, match=r"\bnum_samples\b"):
        cli.check_resume_args(ck, _args(num_samples=1, eval_num_samples=5), "mnist")
    with pytest.raises(cli.CheckpointError, match=r"\beval_num_samples\b"):
        cli.check_resume_args(ck, _args(num_samples=3, eval_num_samples=3), "mnist")


def test_cpu_tensors_refuse_more_than_one_sample():
    """ops.latent_head_iw / ops.iw_head and eval_minibatch_mnist(num_samples=2) on CPU tensors raise, like everything else in
    ops.py: there is no torch restatement to fall back to."""
    from spatial_vae_amd import elbo as E, models, ops
    q_out, r = torch.zeros(2, 6), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.latent_head_iw(q_out, r, 2, True, True, True, 0.1, 1.0, 3.14)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.iw_head(torch.zeros(4), torch.zeros(4), 2)
    p_net = models.SpatialGenerator(2, 8, num_layers=2)
    q_net = models.InferenceNetwork(16, 5, 8, num_layers=1)
    x = torch.zeros(16, 2)
    y = torch.rand(3, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        E.eval_minibatch_mnist(x, y, p_net, q_net, noise=torch.zeros(6, 5), num_samples=2)
    with pytest.raises(RuntimeError, match="num_samples"):
        E.eval_minibatch_mnist(x, y, p_net, q_net, num_samples=0)


def test_the_torch_only_step_refuses_more_than_one_sample():
    from spatial_vae_amd import dp

    def toy(x, y, p_net, q_net, noise=None, num_samples=1):
        raise AssertionError("the step must refuse before it evaluates anything")

    def nets():
        return nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 5)), nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 4))

    torch.manual_seed(1)
    step = dp.TrainStep(*nets(), toy, lr=1e-2)
    before = step.grads.flat_param.clone()
    with pytest.raises(RuntimeError, match=r"num_samples > 1"):
        step(None, torch.zeros(4, 5), noise=torch.zeros(8, 2), num_samples=2)
    step2 = dp.TrainStep(*nets(), toy, lr=1e-2, num_samples=4)
    with pytest.raises(RuntimeError, match=r"num_samples > 1"):
        step2(None, torch.zeros(4, 5), noise=torch.zeros(16, 2))
    assert torch.equal(step.grads.flat_param, before)
