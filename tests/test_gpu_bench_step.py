"""The benchmark's own training step against the oracle, one BASELINE config at a time (GPU).

bench.py times dp.TrainStep: the decoder and encoder kernels write their gradients into views of one flat buffer (FlatGrads,
64-element alignment), FlatAdam updates every parameter from it and clears it behind itself.  The full-size oracle tests
(test_gpu_fullsize.py) go through eval_minibatch_* and autograd's .grad instead, and at configs 3, 4 and 5 at batches small
enough to fall below the launch size at which the hidden-layer GEMMs take their 64-column forms.  Here the workload is
built from bench.py itself (CONFIGS, build_nets, synthetic_targets, ctf_table, DX_SCALE, LR, coord_grid) at the bench's
batch (cfg 4: B = 8, where the numpy oracle still fits the host), and:

* the dispatch signature -- svae_path_counts of one step -- must equal that of one step at the bench's own batch, so a change
  to the dispatch heuristics that leaves the oracle batch behind fails here;
* one TrainStep with explicit noise is compared with oracle.elbo_minibatch on the same inputs: the ELBO terms, every logit,
  every p_net gradient read out of the flat buffer (captured before the update), d(-elbo)/d(q_out) as a whole and image by
  image, every q_net gradient against a float64 backward from the oracle's d(-elbo)/d(q_out), and every parameter after
  the first Adam update against p - lr g / (|g| + eps) in float64 from the captured g (Adam's first step is ~lr whatever the
  size of g, so the parameters alone say little about the gradient).

Each config is a test function of its own, so that the oracle's host memory (up to ~10 GB at cfg 3) is freed between them.
Each config's largest errors and dispatch signatures go to $SVAE_RECORD_DIR/bench_step_cfg<k>.json when that variable names
a folder (profiles/r04_bench_step.json holds one such run)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from helpers import rel_err
from oracle import elbo_oracle as O
from test_gpu_fullsize import _encoder_grads_float64

pytestmark = pytest.mark.gpu

# the batch the oracle runs at where it is not the bench's own: at cfg 4's B = 128 one fp32 activation plane is 8.6 GB
ORACLE_BATCH = {4: 8}

# d(-elbo)/d(q_out), image by image: max |got - want| over a row / max |want| over that row.  Measured on an MI355X, worst
# image per config: 2.9e-6, 5.0e-6, 5.4e-6, 3.8e-6, 2.7e-6 (cfg 1-5); 1e-4 leaves more than 18x
ROW_TOL = 1e-4


def _eval_fn(cfg):
    from spatial_vae_amd import elbo as E
    return {"mnist": E.eval_minibatch_mnist, "galaxy": E.eval_minibatch_galaxy,
            "particles": E.eval_minibatch_particles}[cfg["script"]]


def _workload(cfg, B, dev):
    """bench.py's step at batch B: default-initialised networks, a TrainStep with the bench's arguments, seeded synthetic
    targets (and CTF filters), an explicit N(0, 1) draw."""
    import bench
    from spatial_vae_amd import dp, ops
    p_net, q_net = bench.build_nets(cfg)
    p_net.to(dev)
    q_net.to(dev)
    step = dp.TrainStep(p_net, q_net, _eval_fn(cfg), lr=bench.LR, rotate=cfg["rotate"], translate=cfg["translate"],
                        dx_scale=bench.DX_SCALE, theta_prior=cfg["theta_prior"])
    rs = np.random.RandomState(1000)
    y = bench.synthetic_targets(cfg, rs, B)
    r = rs.normal(size=(B, bench.inf_dim(cfg))).astype(np.float32)
    ctf = None
    if cfg.get("ctf"):
        ctf = ops.ctf_filter(bench.ctf_table(rs, B), cfg["n"] - 1, cfg["n"] - 1, device=dev).unsqueeze(1)
    x = torch.from_numpy(bench.coord_grid(cfg["n"], cfg["n"])).to(dev)
    y_dev = torch.from_numpy(y).to(dev)
    batch = (y_dev, None, ctf) if cfg["script"] == "particles" else (y_dev,)
    return p_net, q_net, step, x, batch, y, torch.from_numpy(r).to(dev), r, ctf


def _bench_batch_signature(cfg, dev):
    """svae_path_counts of one TrainStep at the bench's own batch (GPU only: nothing is compared)."""
    from spatial_vae_amd import _lib
    p_net, q_net, step, x, batch, _, r_dev, _, _ = _workload(cfg, cfg["B"], dev)
    _lib.path_counts(reset=True)
    step(x, *batch, noise=r_dev)
    torch.cuda.synchronize()
    sig = _lib.path_counts(reset=True)
    del p_net, q_net, step, x, batch, r_dev
    torch.cuda.empty_cache()
    return sig


def _segments(step, net):
    """{parameter name: (offset, numel, shape)} of a module's parameters in the step's flat buffers."""
    index = {id(p): i for i, p in enumerate(step.grads.params)}
    return {k: (step.grads.offsets[index[id(p)]], p.numel(), tuple(p.shape)) for k, p in net.named_parameters()}


def _check_config(k):
    import bench
    from spatial_vae_amd import _lib
    from spatial_vae_amd import elbo as E
    cfg = dict(bench.CONFIGS[k])
    B = ORACLE_BATCH.get(k, cfg["B"])
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    sig_bench = _bench_batch_signature(cfg, dev)

    p_net, q_net, step, x, batch, y, r_dev, r, ctf = _workload(cfg, B, dev)
    p_state = {n: v.detach().cpu().numpy().copy() for n, v in p_net.state_dict().items()}
    q_state = {n: v.detach().cpu().numpy().copy() for n, v in q_net.state_dict().items()}
    seg_p, seg_q = _segments(step, p_net), _segments(step, q_net)

    kept = {}
    orig_encode = E._encode

    def keeping_encode(q, y2d):         # the encoder output as the ELBO sees it, with its gradient retained
        out = orig_encode(q, y2d)
        out.retain_grad()
        kept["q_out"] = out
        return out

    orig_optim_step = step.optim.step

    def keeping_optim_step(*a, **kw):   # the gradient the update reads (FlatAdam clears the buffer behind itself)
        kept["g"] = step.grads.flat.detach().clone()
        return orig_optim_step(*a, **kw)

    E._encode = keeping_encode
    step.optim.step = keeping_optim_step
    try:
        _lib.path_counts(reset=True)
        out = step(x, *batch, noise=r_dev, return_logits=True)
        torch.cuda.synchronize()
        sig = _lib.path_counts(reset=True)
    finally:
        E._encode = orig_encode
        step.optim.step = orig_optim_step
    metrics = step.metrics.detach().cpu().numpy().astype(np.float64)
    logits = out[-1].detach().cpu().numpy()
    q_out = kept["q_out"].detach().cpu().numpy()
    g_q_out = kept["q_out"].grad.detach().cpu().numpy()
    g = kept["g"].cpu().numpy()
    after = {("p", n): v.detach().cpu().numpy() for n, v in p_net.named_parameters()}
    after.update({("q", n): v.detach().cpu().numpy() for n, v in q_net.named_parameters()})
    cleared = int(torch.count_nonzero(step.grads.flat).item())
    ctf_np = ctf.cpu().numpy() if ctf is not None else None
    del out, kept, p_net, q_net, step, x, batch, r_dev, ctf
    torch.cuda.empty_cache()

    # ---- the flat gradient buffer, read through grads.offsets
    covered = np.zeros(g.size, bool)
    for off, n, _ in list(seg_p.values()) + list(seg_q.values()):
        assert not covered[off:off + n].any()
        covered[off:off + n] = True
    gp = {n: g[off:off + m].reshape(shape) for n, (off, m, shape) in seg_p.items()}
    gq = {n: g[off:off + m].reshape(shape) for n, (off, m, shape) in seg_q.items()}

    # ---- the oracle on the same inputs (its encoder output is the HIP encoder's: test_gpu_fullsize checks that one)
    L = cfg["L"]
    spec = O.DecoderSpec(cfg["z_dim"], cfg["H"], n_out=cfg["C"], num_layers=L, activation="tanh")
    grid = bench.coord_grid(cfg["n"], cfg["n"])
    ref = O.elbo_minibatch(cfg["script"], spec, p_state, grid, y, q_out, r, rotate=cfg["rotate"], translate=cfg["translate"],
                           dx_scale=bench.DX_SCALE, theta_prior=cfg["theta_prior"], ctf=ctf_np)
    assert logits.size == ref["logits"].size and set(gp) == set(ref["gP"])
    err = {"batch": B, "bench_batch": cfg["B"]}
    for i, name in enumerate(("elbo", "log_p", "kl")):
        err[name] = abs(metrics[i] - float(ref[name])) / abs(float(ref[name]))
    err["logits"] = rel_err(logits.reshape(ref["logits"].shape), ref["logits"])
    err["p_grads"] = {n: rel_err(v, ref["gP"][n]) for n, v in gp.items()}
    want_q = ref["g_q_out"]
    err["g_q_out"] = rel_err(g_q_out, want_q)
    # image by image: a lost row group of one image barely moves a gradient summed over 800 000 rows, but it moves that
    # image's pose and latent gradients by their own size
    rows = np.abs(g_q_out.astype(np.float64) - want_q).max(1) / np.maximum(np.abs(want_q.astype(np.float64)).max(1), 1e-30)
    err["g_q_out_worst_image"] = float(rows.max())
    err["g_q_out_worst_image_index"] = int(rows.argmax())
    want_gq = _encoder_grads_float64(None, {"q_state": q_state, "y": y}, want_q)
    err["q_grads"] = {n: rel_err(v, want_gq[n]) for n, v in gq.items()}
    del ref, want_gq

    # ---- the first Adam update from the captured gradient, in float64: p - lr g / (|g| + eps) to one fp32 spacing of the
    # result (the rounding of p + update) plus 2e-5 lr (the fp32 constants 1 - beta1, 1 - beta2 of the update)
    lr, eps = bench.LR, 1e-8
    adam_bad = {}
    adam = 0.0
    for (net, n), v in after.items():
        p0_all, g_all = (p_state if net == "p" else q_state)[n].reshape(-1), (gp if net == "p" else gq)[n].reshape(-1)
        v = v.reshape(-1)
        for lo in range(0, v.size, 1 << 24):        # cfg 4's 246 M-entry encoder layer in float64 pieces
            p0, g64 = p0_all[lo:lo + (1 << 24)].astype(np.float64), g_all[lo:lo + (1 << 24)].astype(np.float64)
            want = p0 - lr * g64 / (np.abs(g64) + eps)
            d = np.abs(v[lo:lo + (1 << 24)].astype(np.float64) - want)
            tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2e-5 * lr
            bad = int((d > tol).sum())
            if bad:
                adam_bad["%s.%s" % (net, n)] = adam_bad.get("%s.%s" % (net, n), 0) + bad
            adam = max(adam, float(d.max()) / lr)
    err["adam_max_abs_over_lr"] = adam

    record = {"config": k, "signature_oracle_batch": sig, "signature_bench_batch": sig_bench, "errors": err,
              "seconds": round(time.perf_counter() - t0, 1)}
    out_dir = os.environ.get("SVAE_RECORD_DIR")
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "bench_step_cfg%d.json" % k), "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
    print(json.dumps({"config": k, "signature": sig, "seconds": record["seconds"]}))

    # ---- the dispatch: the oracle batch runs the forms the bench batch runs
    assert sig == sig_bench, ("cfg %d: B=%d dispatches differently from the bench's B=%d" % (k, B, cfg["B"]), sig, sig_bench)
    assert sig["dense4"] == 2 * (L - 1), sig
    assert sig["wgrad2"] == L - 1, sig
    assert sig["dense4_cf"] > 0, sig
    if k >= 2:
        assert sig["dense4_nt2"] > 0, sig
    # ---- the flat buffer: nothing written into the alignment padding, everything cleared by FlatAdam
    assert not g[~covered].any(), "cfg %d: a gradient was written outside its parameter's segment" % k
    assert cleared == 0, "cfg %d: %d gradient entries left after FlatAdam's zero_grad" % (k, cleared)
    # ---- against the oracle
    for name in ("elbo", "log_p", "kl"):
        assert err[name] <= 1e-4, (k, name, err[name])
    assert err["logits"] < 1e-4, (k, err["logits"])
    for n, e in err["p_grads"].items():
        assert e < 2e-4, (k, n, e)
    assert err["g_q_out"] < 2e-4, (k, err["g_q_out"])
    assert err["g_q_out_worst_image"] < ROW_TOL, (k, err["g_q_out_worst_image"], err["g_q_out_worst_image_index"])
    for n, e in err["q_grads"].items():
        assert e < 2e-4, (k, n, e)
    assert not adam_bad, (k, "parameters off the first Adam update (count of entries)", adam_bad)


def test_bench_step_cfg1():
    _check_config(1)


def test_bench_step_cfg2():
    _check_config(2)


def test_bench_step_cfg3():
    _check_config(3)


def test_bench_step_cfg4():
    _check_config(4)


def test_bench_step_cfg5():
    _check_config(5)
