"""CPU-only: infer.py's check of a request against the split (spatial_vae_amd.infer.check_request: every data-dependent
refusal, from the parsed arguments and a record of plain facts, no tensor and no device) and elbo.row_layout, the one
statement of where things are in a score row."""
import numpy as np
import pytest

from spatial_vae_amd import elbo as E
from spatial_vae_amd import infer


def _facts(**kw):
    """Four one-channel 8x8 images of a model that rotates, translates and has three content latents, with a CTF table."""
    base = dict(images=4, n=8, m=8, channels=1, rotate=True, translate=True, inf_dim=6, z_scale=1, split="test", ctf_rows=4)
    return infer.SplitFacts(**dict(base, **kw))


def _args(tmp_path, script, *options, labels=None):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    argv = [script, "--state", str(state), "--out", "s.npz"] + list(options)
    if labels is not None:
        np.save(str(tmp_path / "l.npy"), np.asarray(labels, np.int64))
        argv += ["--labels", str(tmp_path / "l.npy")]
    return infer.infer_arguments(argv)


CLUSTER = ("--cluster", "3", "--cluster_out", "k.npz")
FLIP = ("--ctf_correct", "flip", "--aligned", "a.npy")
WIENER = ("--ctf_correct", "wiener", "--class_averages", "c.npz")


@pytest.mark.parametrize("script,options,labels,facts,message", [
    ("mnist", CLUSTER, None, dict(inf_dim=3), "has none"),
    ("mnist", CLUSTER, None, dict(z_scale=0), "z_scale = 0"),
    ("mnist", ("--cluster", "5", "--cluster_out", "k.npz"), None, {}, "exceeds the 4 images"),
    ("mnist", ("--class_averages", "c.npz"), [0, 1, 0], {}, "--labels has 3 entries, the test split has 4 images"),
    ("mnist", ("--aligned", "a.mrcs"), None, dict(channels=3), "--aligned a.mrcs: an MRC stack holds one channel, these images have 3"),
    ("mnist", ("--recon", "a.mrcs"), None, dict(channels=3), "--recon a.mrcs: an MRC stack holds one channel, these images have 3"),
    ("particles", FLIP, None, dict(ctf_rows=None), "the run has no --ctf-test table"),
    ("particles", FLIP, None, dict(ctf_rows=3), "has 3 rows, the split has 4 images"),
    ("particles", WIENER, None, dict(channels=3), "--ctf_correct takes one-channel images, these have 3"),
    ("particles", FLIP, None, dict(m=6), "needs a square box"),
])
def test_every_data_dependent_refusal(tmp_path, capsys, script, options, labels, facts, message):
    args = _args(tmp_path, script, *options, labels=labels)
    with pytest.raises(SystemExit) as e:
        infer.check_request(args, _facts(**facts))
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert err.startswith("infer.py: ") and message in err
    if "square box" in message:
        assert "these images are 8x6" in err


@pytest.mark.parametrize("script,options,labels", [
    ("mnist", (), None),
    ("mnist", ("--aligned", "a.mrcs", "--recon", "r.npy", "--class_averages", "c.npz"), [0, -1, 2, 1]),
    ("particles", WIENER, None),
    ("mnist", CLUSTER + ("--class_averages", "c.npz"), None),
])
def test_accepted_requests_return(tmp_path, script, options, labels):
    assert infer.check_request(_args(tmp_path, script, *options, labels=labels), _facts()) is None


def test_a_translating_model_that_does_not_rotate_may_have_an_oblong_box(tmp_path):
    assert infer.check_request(_args(tmp_path, "particles", *FLIP), _facts(rotate=False, inf_dim=5, m=6)) is None


def test_the_cluster_refusal_comes_before_the_ctf_one(tmp_path, capsys):
    args = _args(tmp_path, "particles", *(CLUSTER + WIENER))
    with pytest.raises(SystemExit) as e:
        infer.check_request(args, _facts(z_scale=0, ctf_rows=None))
    err = capsys.readouterr().err
    assert e.value.code == 2 and "z_scale = 0" in err and "ctf" not in err.lower()


@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("translate", [False, True])
@pytest.mark.parametrize("z_dim", [0, 3])
def test_row_layout_tiles_the_row_and_is_what_score_arrays_cuts(rotate, translate, z_dim):
    inf_dim = (1 if rotate else 0) + (2 if translate else 0) + z_dim
    lay = E.row_layout(rotate, translate, inf_dim)
    assert (lay.theta.start, lay.theta.stop) == (0, lay.dx.start) and lay.dx.stop == lay.content.start
    assert lay.content.stop == inf_dim == lay.inf_dim
    assert lay.theta.stop - lay.theta.start == (1 if rotate else 0) and lay.dx.stop - lay.dx.start == (2 if translate else 0)
    assert lay.z_dim == z_dim == lay.content.stop - lay.content.start
    assert lay.width == 6 + 2 * inf_dim
    assert (lay.iw.start, lay.iw.stop, lay.best.start, lay.best.stop) == (6, 6 + inf_dim, 6 + inf_dim, lay.width)
    rs = np.random.RandomState(7)
    per_image = rs.normal(size=(5, lay.width)).astype(np.float32)
    q_mu, q_std = rs.normal(size=(5, inf_dim)).astype(np.float32), rs.uniform(size=(5, inf_dim)).astype(np.float32)
    arrays = infer.score_arrays(per_image, q_mu, q_std, rotate, translate)
    rows = {"q": q_mu, "q_std": q_std, "iw": per_image[:, lay.iw], "best": per_image[:, lay.best]}
    names = {"bound", "loglik", "kl", "ess", "index"}
    for kind, row in rows.items():
        if rotate:
            assert np.array_equal(arrays["theta_" + kind], row[:, lay.theta][:, 0])
        if translate:
            assert np.array_equal(arrays["dx_" + kind], row[:, lay.dx]) and arrays["dx_" + kind].shape == (5, 2)
        assert np.array_equal(arrays["z_" + kind], row[:, lay.content]) and arrays["z_" + kind].shape == (5, z_dim)
        names |= {p + kind for p, have in (("theta_", rotate), ("dx_", translate), ("z_", True)) if have}
    assert set(arrays) == names | ({"theta_R"} if rotate else set())
    stacked = np.concatenate([per_image, q_mu, q_std], 1)
    assert all(np.array_equal(a, b) for a, b in zip(infer.split_rows(stacked, lay), (per_image, q_mu, q_std)))
