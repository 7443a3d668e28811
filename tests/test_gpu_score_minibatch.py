"""elbo.score_minibatch (encode once, stream the K samples through the decoder in chunks) against the eval_minibatch_*
functions with num_samples = K on the same noise: same bound, same log p(x|z), same Monte-Carlo KL to 2e-5 relative (the
project's parity bar for the HIP path), whatever the chunk size.  Small networks built here."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases

pytestmark = pytest.mark.gpu
TOL = 2e-5
B, SIDE, K = 5, 6, 12
N = SIDE * SIDE
CHUNKS = (12, 5, 1)

#          script       n_out softplus  ctf    mask   vanilla  z_scale theta_prior
NETS = {"mnist": ("mnist", 1, False, False, False, False, 1.0, math.pi / 4),
        "galaxy": ("galaxy", 3, False, False, False, False, 0.5, math.pi),
        "particles_ctf_mask": ("particles", 1, False, True, True, False, 1.0, 0.5),
        "particles_fit_noise_softplus_mask": ("particles", 2, True, False, True, False, 1.0, 0.5),
        "mnist_vanilla": ("mnist", 1, False, False, False, True, 1.0, math.pi)}


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


@pytest.mark.parametrize("name", sorted(NETS))
def test_score_minibatch_matches_eval_minibatch(name):
    """6 x 6 images, B = 5, z_dim 3, H = 20, two layers, K = 12 with chunks of 12, 5 (ragged: 5 + 5 + 2) and 1.  mnist;
    galaxy (three channels, z_scale 0.5); particles with a circular mask and 5 x 5 CTF filters; particles with the mask,
    fit-noise and softplus (the library defines no CTF with fit-noise, so the two are separate cases); mnist --vanilla.
    out3 against eval_minibatch_*(num_samples=12, noise=...), per_image[:, 0].mean() against out3[0] and the three chunkings
    against one another, all to 2e-5 relative; the encoder's forward runs exactly once per call; q_mu / q_std are the
    encoder's posterior in the decoder's units; the reconstruction at the best sample has one row per image.
    MI355X: out3 equals eval_minibatch's bit for bit in all five cases and all three chunkings; per_image[:, 0].mean()
    is within 5.2e-8 of out3[0]."""
    import spatial_vae.models as models
    from spatial_vae_amd import elbo as E
    script, C, softplus, use_ctf, use_mask, vanilla, z_scale, theta_prior = NETS[name]
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(sorted(NETS).index(name) + 60)
    torch.manual_seed(70 + C)
    rotate = translate = not vanilla
    z_dim, dx_scale = 3, 0.1
    inf = z_dim + (3 if not vanilla else 0)
    with contextlib.redirect_stdout(io.StringIO()):
        if vanilla:
            p_net = models.VanillaGenerator(N, z_dim, 20, num_layers=2, activation=nn.Tanh).to(dev)
        else:
            p_net = models.SpatialGenerator(z_dim, 20, n_out=C, num_layers=2, activation=nn.Tanh, softplus=softplus).to(dev)
        q_net = models.InferenceNetwork(N * (C if script == "galaxy" else 1), inf, 24, num_layers=2, activation=nn.Tanh).to(dev)
    with torch.no_grad():                               # widen the posterior: default initialisation leaves log-std near 0
        last = [m for m in q_net.layers if isinstance(m, nn.Linear)][-1]
        last.bias.copy_(torch.from_numpy(np.concatenate([rs.uniform(-1, 1, inf), rs.uniform(-2.0, -0.5, inf)]).astype(np.float32)))
    if script == "galaxy":
        y_np = rs.uniform(0.05, 0.95, size=(B, N, C)).astype(np.float32)
    elif script == "particles":
        y_np = rs.normal(size=(B, N)).astype(np.float32)
    else:
        y_np = rs.uniform(0.05, 0.95, size=(B, N)).astype(np.float32)
    x = torch.from_numpy(cases.coord_grid(SIDE, SIDE).astype(np.float32)).to(dev)
    y = torch.from_numpy(y_np).to(dev)
    noise = torch.from_numpy(rs.normal(size=(B * K, inf)).astype(np.float32)).to(dev)
    mask = ctf = None
    if use_mask:
        mask = torch.from_numpy(cases.circular_mask(SIDE, SIDE).reshape(-1)).to(dev)
    if use_ctf:
        f = (rs.normal(size=(B, 1, 5, 5)) / 5).astype(np.float32)
        f[:, 0, 2, 2] += 1.0
        ctf = torch.from_numpy(f).to(dev)
    kw = dict(rotate=rotate, translate=translate, dx_scale=dx_scale, theta_prior=theta_prior)
    with torch.no_grad():
        if script == "mnist":
            want = E.eval_minibatch_mnist(x, y, p_net, q_net, num_samples=K, noise=noise, **kw)[:3]
        elif script == "galaxy":
            want = E.eval_minibatch_galaxy(x, y, p_net, q_net, z_scale=z_scale, num_samples=K, noise=noise, **kw)[:3]
        else:
            want = E.eval_minibatch_particles(x, y, mask, ctf, p_net, q_net, z_scale=z_scale, num_samples=K, noise=noise, **kw)[:3]
        q_out = q_net.layers(y.view(B, -1)).cpu().numpy()
    want = [float(v) for v in want]
    calls = []
    hook = q_net.register_forward_hook(lambda *a: calls.append(1))
    layer_hook = q_net.layers[0].register_forward_hook(lambda *a: calls.append(1))
    got = {}
    try:
        for chunk in CHUNKS:
            before = len(calls)
            out = E.score_minibatch(script, x, y, p_net, q_net, num_samples=K, chunk=chunk, z_scale=z_scale, mask=mask, ctf=ctf,
                                    noise=noise, return_best=(chunk == 5), **kw)
            torch.cuda.synchronize()
            got[chunk] = (out["per_image"].cpu().numpy(), out["out3"].cpu().numpy())
            assert tuple(out["per_image"].shape) == (B, 6 + 2 * inf)
            # InferenceNetwork's Linear layers run through ops.enc_linear, not the modules: count the encoder by elbo._encode
            assert len(calls) - before <= 1
            if chunk == 5:
                assert out["y_best"].shape[0] == B
                unit = np.ones(inf, np.float32)
                off = 1 if rotate else 0
                unit[off:off + (2 if translate else 0)] = dx_scale
                unit[off + (2 if translate else 0):] = z_scale
                assert np.allclose(out["q_mu"].cpu().numpy(), q_out[:, :inf] * unit, rtol=1e-5, atol=1e-6)
                assert np.allclose(out["q_std"].cpu().numpy(), np.exp(q_out[:, inf:]) * unit, rtol=1e-5, atol=1e-7)
    finally:
        hook.remove()
        layer_hook.remove()
    for chunk, (per_image, out3) in got.items():
        errs = [_rel(out3[i], want[i]) for i in range(3)] + [_rel(per_image[:, 0].astype(np.float64).mean(), out3[0])]
        print("%s chunk %d out3 %s want %s errors %s" % (name, chunk, out3.tolist(), want, errs))
        assert max(errs) <= TOL, (chunk, errs)
        assert np.isfinite(per_image).all() and (per_image[:, 3] >= 1 - 1e-6).all() and (per_image[:, 3] <= K * (1 + 1e-6)).all()
    for chunk in CHUNKS[1:]:
        e = [_rel(got[chunk][1][i], got[CHUNKS[0]][1][i]) for i in range(3)]
        e.append(float(np.abs(got[chunk][0][:, :6] - got[CHUNKS[0]][0][:, :6]).max() / np.abs(got[CHUNKS[0]][0][:, :6]).max()))
        print("%s chunk %d against chunk %d: %s" % (name, chunk, CHUNKS[0], e))
        assert max(e) <= TOL, (chunk, e)


def test_encoder_runs_once_per_call(monkeypatch):
    """score_minibatch with K = 12 in chunks of 1 makes twelve decoder calls and exactly one encoder call (elbo._encode is what
    every path of this package reaches the encoder through).  MI355X: one encoder call, twelve decoder calls."""
    import spatial_vae.models as models
    from spatial_vae_amd import elbo as E
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        p_net = models.SpatialGenerator(3, 20, n_out=1, num_layers=2, activation=nn.Tanh).to(dev)
        q_net = models.InferenceNetwork(N, 6, 24, num_layers=2, activation=nn.Tanh).to(dev)
    x = torch.from_numpy(cases.coord_grid(SIDE, SIDE).astype(np.float32)).to(dev)
    y = torch.rand(B, N, device=dev)
    enc, dec = [], []
    real_encode, real_decode = E._encode, E._decode_score
    monkeypatch.setattr(E, "_encode", lambda *a, **k: (enc.append(1), real_encode(*a, **k))[1])
    monkeypatch.setattr(E, "_decode_score", lambda *a, **k: (dec.append(1), real_decode(*a, **k))[1])
    first = [m for m in q_net.layers if isinstance(m, nn.Linear)][0]
    seen = []
    handle = q_net.register_forward_hook(lambda *a: seen.append(1))
    out = E.score_minibatch("mnist", x, y, p_net, q_net, num_samples=K, chunk=1, rotate=True, translate=True, dx_scale=0.1,
                            theta_prior=math.pi / 4)
    handle.remove()
    torch.cuda.synchronize()
    assert len(enc) == 1 and len(dec) == K and len(seen) <= 1 and first is not None
    assert np.isfinite(out["per_image"].cpu().numpy()).all()
