"""CPU-only: infer.py's command line, its .npz writer, the float64 reference of the streaming scorer held to properties of
the definitions it restates, and the binding of include/svae_stream.h held to that header."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from iw_stream_ref import coords, iw_stream_ref, wrap
from test_binding_cpu import parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    from spatial_vae_amd import cli
    return cli


def _infer():
    from spatial_vae_amd import infer
    return infer


def test_parser_defaults_and_the_split(tmp_path):
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    a = _infer().infer_arguments(["mnist", "--state", str(state), "--out", "s.npz"])
    assert (a.script, a.split, a.num_samples, a.chunk, a.minibatch_size, a.seed, a.device) == ("mnist", "test", 64, 64, 100, 0, -2)
    assert a.train_argv is None and a.generator is None and a.train_path is None and a.ctf_test is None
    g, q = tmp_path / "g.sav", tmp_path / "q.sav"
    g.write_bytes(b"x")
    q.write_bytes(b"x")
    a = _infer().infer_arguments(["particles", "--generator", str(g), "--inference", str(q), "--out", "s.npz", "--num_samples", "5000",
                                "--chunk", "50", "--", "tr.mrcs", "te.mrcs", "--z-dim", "4", "--out", "not-ours"])
    assert a.train_argv == ["tr.mrcs", "te.mrcs", "--z-dim", "4", "--out", "not-ours"] and a.out == "s.npz"
    assert (a.num_samples, a.chunk, a.state) == (5000, 50, None)


@pytest.mark.parametrize("argv,message", [
    (["mnist", "--state", "{state}", "--out", "s.npz", "--num_samples", "0"], "num_samples"),
    (["mnist", "--state", "{state}", "--out", "s.npz", "--chunk", "0"], "chunk"),
    (["mnist", "--state", "{state}", "--out", "s.npz", "--chunk", "1025"], "chunk"),
    (["mnist", "--state", "{missing}", "--out", "s.npz"], "no such file"),
    (["mnist", "--out", "s.npz"], "--state"),
    (["mnist", "--state", "{state}", "--out", "s.npz", "--", "--z_dim", "3"], "nothing may follow"),
    (["mnist", "--generator", "{state}", "--out", "s.npz", "--"], "go together"),
    (["mnist", "--generator", "{state}", "--inference", "{state}", "--out", "s.npz"], "after `--`"),
])
def test_refusals_exit_with_code_2_before_the_library_is_loaded(tmp_path, argv, message):
    """Through the real command line in a fresh process: exit code 2, the reason on stderr, no output file, and the process
    never loaded the kernel library (a marker printed by an exit hook shows _lib's handle was still unset)."""
    state = tmp_path / "a.ckpt"
    state.write_bytes(b"x")
    argv = [a.format(state=state, missing=tmp_path / "nope.ckpt") for a in argv]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['infer.py'] + %r\n"
            "from spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, file=sys.stderr))\n"
            "import infer; sys.exit(infer.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    assert message in out.stderr and "LIB True" in out.stderr
    assert not os.path.exists(tmp_path / "s.npz")


def test_state_file_of_another_script_is_refused(tmp_path):
    """A state file whose stored arguments are not the named script's: exit code 2 from stored_namespace, which runs before a
    device is picked."""
    import train_galaxy
    import train_mnist
    cli, infer = _cli(), _infer()
    stored = cli.plain_args(train_galaxy.galaxy_arguments(["a.npy", "b.npy", "--synthetic", "8"]))
    with pytest.raises(SystemExit) as e:
        infer.stored_namespace({"args": stored}, vars(train_mnist.mnist_arguments([])), "mnist")
    assert e.value.code == 2
    mine = cli.plain_args(train_mnist.mnist_arguments(["--z_dim", "5"]))
    for k in cli.RESUME_ARG_DEFAULTS:          # a file from before these options existed
        mine.pop(k)
    ns = infer.stored_namespace({"args": mine}, vars(train_mnist.mnist_arguments([])), "mnist")
    assert ns.z_dim == 5 and ns.num_samples == 1 and ns.clip_grad_norm is None


def test_npz_round_trip_and_interrupted_write(tmp_path, monkeypatch):
    infer = _infer()
    rs = np.random.RandomState(0)
    per_image = rs.normal(size=(7, 6 + 2 * 6)).astype(np.float32)
    q_mu, q_std = rs.normal(size=(7, 6)).astype(np.float32), rs.uniform(size=(7, 6)).astype(np.float32)
    arrays = infer.score_arrays(per_image, q_mu, q_std, True, True)
    arrays["meta"] = np.array(json.dumps({"k": 1}))
    path = str(tmp_path / "s.npz")
    infer.write_npz(path, arrays)
    back = infer.read_npz(path)                                   # allow_pickle=False: plain arrays only
    assert sorted(back) == sorted(arrays) and all(np.array_equal(back[k], arrays[k]) for k in arrays)
    assert json.loads(str(back["meta"])) == {"k": 1} and os.listdir(tmp_path) == ["s.npz"]
    assert np.array_equal(back["theta_iw"], per_image[:, 6]) and np.array_equal(back["dx_best"], per_image[:, 13:15])
    assert np.array_equal(back["z_q"], q_mu[:, 3:]) and np.array_equal(back["theta_R"], per_image[:, 5])
    no_rot = infer.score_arrays(per_image[:, :6 + 2 * 5], q_mu[:, :5], q_std[:, :5], False, True)
    assert not [k for k in no_rot if k.startswith("theta_")] and no_rot["dx_iw"].shape == (7, 2) and no_rot["z_iw"].shape == (7, 3)
    no_dx = infer.score_arrays(per_image[:, :6 + 2 * 4], q_mu[:, :4], q_std[:, :4], True, False)
    assert not [k for k in no_dx if k.startswith("dx_")] and no_dx["z_best"].shape == (7, 3)

    def broken(f, **kw):
        f.write(b"half a file")
        raise KeyboardInterrupt
    monkeypatch.setattr(np, "savez", broken)
    other = str(tmp_path / "t.npz")
    with pytest.raises(KeyboardInterrupt):
        infer.write_npz(other, arrays)
    with pytest.raises(KeyboardInterrupt):
        infer.write_npz(path, arrays)                             # nor is an earlier file damaged
    assert os.listdir(tmp_path) == ["s.npz"] and sorted(infer.read_npz(path)) == sorted(arrays)


def test_reference_holds_to_properties_of_the_definitions():
    """Independent of how the reference is written: the bound of K equal values is that value and their sample size is K; the
    circular mean of {pi - eps, -pi + eps} under equal weights is +-pi with R = cos(eps); a = -inf samples weigh nothing; the
    best sample is the first at the max."""
    K, eps = 7, 0.05
    v = np.zeros((1, K, 2))
    row, out3, w = iw_stream_ref(np.full((1, K), -3.25), np.full((1, K), 0.75), v, False)
    assert abs(row[0, 0] - (-2.5)) < 1e-14 and abs(row[0, 3] - K) < 1e-12 and np.allclose(w, 1.0 / K)
    assert row[0, 5] == 1 and abs(out3[0] + 2.5) < 1e-14 and out3[1] == -3.25 and out3[2] == -0.75
    v = np.array([[[np.pi - eps, 1.0], [-np.pi + eps, 3.0]]])
    row, _, _ = iw_stream_ref(np.zeros((1, 2)), np.zeros((1, 2)), v, True)
    assert abs(abs(row[0, 6]) - np.pi) < 1e-12 and abs(row[0, 5] - np.cos(eps)) < 1e-12 and abs(row[0, 7] - 2.0) < 1e-14
    assert abs(wrap(row[0, 6] - np.pi)) < 1e-12
    ll = np.array([[0.0, 0.0, 0.0, 0.0]])
    lr = np.array([[-np.inf, 1.0, 1.0, -np.inf]])
    v = np.arange(4.0).reshape(1, 4, 1)
    row, _, w = iw_stream_ref(ll, lr, v, False)
    assert (w[0] == [0, 0.5, 0.5, 0]).all() and row[0, 3] == 2 and row[0, 6] == 1.5 and row[0, 7] == 1.0 and row[0, 4] == 1.0
    assert abs(row[0, 0] - (1.0 + np.log(2.0 / 4.0))) < 1e-14
    row, out3, _ = iw_stream_ref(ll, np.full((1, 4), -np.inf), v, True)
    assert row[0, 0] == -np.inf and row[0, 3] == 0 and row[0, 5] == 0 and row[0, 6] == 0 and row[0, 7] == 0.0
    assert coords(np.zeros(6), np.zeros((6, 2)), np.zeros((6, 3)), 2, 3).shape == (2, 3, 6)


def test_stream_binding_matches_its_header():
    """What is include/svae_stream.h's own (the rules every added header shares are tests/test_binding_cpu.py's): four
    functions, no struct and no integer constant, and its one macro is _lib.iw_stream_cols."""
    from spatial_vae_amd import _lib
    path, H = parse_added_header("svae_stream.h")
    assert _lib.HEADERS["svae_stream.h"] is _lib.STREAM_SIGNATURES
    assert H["structs"] == {} and H["constants"] == {} and len(H["functions"]) == 4
    with open(path) as f:
        assert "#define SVAE_IW_STREAM_COLS(inf_dim) (6 + 2 * (inf_dim))" in f.read()
    assert [_lib.iw_stream_cols(i) for i in (1, 5)] == [8, 16]


def _snapshot_files(snapshot, tmp_path):
    for name in ("a.ckpt", "g.sav", "q.sav"):
        (tmp_path / name).write_bytes(b"x")
    for name, spec in snapshot["label_files"].items():
        np.save(str(tmp_path / name), np.array(spec["data"], dtype=spec["dtype"]))


def test_command_line_reproduces_the_snapshot_taken_before_the_options_became_a_table(tmp_path, capsys, monkeypatch):
    """tests/golden/infer_args_snapshot.json (gen_infer_args_snapshot.py, run at the commit the file names, where
    infer_arguments and check_request were ladders of refusals): the --help text; for every accepted argv the ordered (key, value)
    pairs of vars(args) with their types; for every refused argv -- one at least for each p.error call of that commit, and those
    that break two rules at once -- exit code 2, the usage and the exact last line of stderr; for every (argv, SplitFacts) pair
    -- one at least for each _refuse call of that commit's check_request -- the exact refusal, or none.  {tmp} in an argv or a
    message is the directory holding the files that must exist."""
    infer = _infer()
    with open(os.path.join(ROOT, "tests", "golden", "infer_args_snapshot.json")) as f:
        snapshot = json.load(f)
    assert len(snapshot["p_error_lines"]) == 61 and len(snapshot["refuse_lines"]) == 18
    _snapshot_files(snapshot, tmp_path)
    monkeypatch.setenv("COLUMNS", snapshot["columns"])

    def there(text):
        return text.replace("{tmp}", str(tmp_path))

    with pytest.raises(SystemExit) as e:
        infer.infer_arguments(["--help"])
    assert e.value.code == 0 and " ".join(capsys.readouterr().out.split()) == snapshot["help"]
    for c in snapshot["accepted"]:
        args = infer.infer_arguments([there(a) for a in c["argv"]])
        got = [[k, v.tolist() if isinstance(v, np.ndarray) else v] for k, v in vars(args).items()]
        want = [[k, there(v) if isinstance(v, str) else v] for k, v in zip(snapshot["keys"], c["values"])]
        assert got == want, c["argv"]
        assert [type(v) for _, v in got] == [type(v) for _, v in want], c["argv"]     # 2 is not 2.0 here
        assert args.label_array is None or args.label_array.dtype == np.int64
    assert len(snapshot["refused"]) >= 61 + 10
    for c in snapshot["refused"]:
        with monkeypatch.context() as lowered:
            for k, v in c.get("lowered", {}).items():
                lowered.setattr(infer, k, v)
            with pytest.raises(SystemExit) as e:
                infer.infer_arguments([there(a) for a in c["argv"]])
        usage, message = capsys.readouterr().err.rstrip("\n").rsplit("\n", 1)
        assert e.value.code == 2 and message == there(c["error"]), c["argv"]
        assert " ".join(usage.split()) == snapshot["usage"], c["argv"]
    for c in snapshot["requests"]:
        args = infer.infer_arguments([there(a) for a in c["argv"]])
        capsys.readouterr()
        if c["error"] is None:
            assert infer.check_request(args, infer.SplitFacts(**c["facts"])) is None, (c["argv"], c["facts"])
            assert capsys.readouterr().err == ""
            continue
        with pytest.raises(SystemExit) as e:
            infer.check_request(args, infer.SplitFacts(**c["facts"]))
        assert e.value.code == 2 and capsys.readouterr().err == there(c["error"]) + "\n", (c["argv"], c["facts"])


BASE_META = ["script", "state", "generator", "inference", "num_samples", "chunk", "seed", "split", "images", "mean_bound",
             "mean_loglik", "mean_kl"]
OUTPUT_META = ["pose", "interp", "labels", "aligned", "recon", "class_averages"]
FRC_META = ["frc", "frc_mask_radius", "frc_mask_edge"]
REFINE_META = ["refine", "refine_angles", "refine_step", "refine_shift"]
CLUSTER_META = ["cluster", "cluster_out", "cluster_labels", "cluster_iters", "cluster_restarts", "cluster_seed"]
GMM_META = ["cluster_gmm", "cluster_gmm_reg", "cluster_gmm_tol", "cluster_min_resp"]
PCA_META = ["pca", "pca_pose", "pca_components", "pca_traverse", "pca_steps", "pca_span", "pca_per_class"]
C_NPZ = ["--class_averages", "c.npz"]
K_NPZ = ["--cluster", "3", "--cluster_out", "k.npz"]


@pytest.mark.parametrize("script,extra,keys", [
    ("mnist", [], []),
    ("mnist", ["--pca", "p.npz", "--pose", "best"], PCA_META),
    ("mnist", ["--aligned", "a.npy"], OUTPUT_META),
    ("mnist", ["--recon", "r.npy", "--pose", "q"], OUTPUT_META),
    ("mnist", C_NPZ + ["--labels", "{labels}"], OUTPUT_META),
    ("particles", C_NPZ + ["--ctf_correct", "wiener"], OUTPUT_META + ["ctf_correct", "wiener_lambda"]),
    ("particles", ["--aligned", "a.npy", "--ctf_correct", "flip"], OUTPUT_META + ["ctf_correct", "wiener_lambda"]),
    ("mnist", C_NPZ + ["--frc"], OUTPUT_META + FRC_META),
    ("mnist", C_NPZ + ["--frc", "--frc_mask_radius", "0"], OUTPUT_META + FRC_META),
    ("mnist", C_NPZ + ["--refine", "2"], OUTPUT_META + REFINE_META),
    ("mnist", C_NPZ + ["--refine", "2", "--reassign"], OUTPUT_META + REFINE_META + ["reassign", "reassign_labels"]),
    ("mnist", C_NPZ + ["--refine", "2", "--reassign", "--refine_soft", "--frc"],
     OUTPUT_META + FRC_META + REFINE_META + ["reassign", "reassign_labels", "refine_soft", "refine_soft_classes", "refine_soft_sigma2"]),
    ("mnist", K_NPZ, ["pose"] + CLUSTER_META),
    ("mnist", K_NPZ + C_NPZ, OUTPUT_META + CLUSTER_META),
    ("mnist", K_NPZ + ["--cluster_gmm", "4"], ["pose"] + CLUSTER_META + GMM_META),
    ("mnist", K_NPZ + ["--pca", "p.npz", "--pca_per_class", "--pca_traverse", "1"], ["pose"] + CLUSTER_META + PCA_META),
    ("particles", K_NPZ + C_NPZ + ["--cluster_gmm", "4", "--ctf_correct", "flip", "--frc", "--refine", "1", "--reassign", "--pca", "p.npz"],
     OUTPUT_META + ["ctf_correct", "wiener_lambda"] + FRC_META + REFINE_META + ["reassign", "reassign_labels"] + CLUSTER_META + GMM_META
     + PCA_META),
])
def test_meta_is_made_from_the_groups_in_one_order(tmp_path, script, extra, keys):
    """run_meta without a device: after the twelve keys every file has, the keys of each active group, in the one order
    json.dumps will write.  pose, interp and labels only with an image output; pose again under --cluster, where it keeps its
    first place; the pose --pca used as pca_pose; frc_mask_radius as computed for the box; every value the argument's own, with
    its type; and the --cluster_out file's meta (without="pca") is the same record cut off before the pca_* keys."""
    infer = _infer()
    state, labels = tmp_path / "a.ckpt", tmp_path / "l.npy"
    state.write_bytes(b"x")
    np.save(str(labels), np.array([0, 1, -1, 1]))
    args = infer.infer_arguments([script, "--state", str(state), "--out", "s.npz", "--seed", "7"] + [a.format(labels=labels) for a in extra])
    facts = infer.SplitFacts(images=4, n=12, m=10, channels=1, rotate=True, translate=True, inf_dim=5, z_scale=1, split="test",
                             ctf_rows=4)
    figures = {"images": 4, "mean_bound": -1.5, "mean_loglik": -1.0, "mean_kl": 0.5}
    meta = infer.run_meta(args, facts, figures)
    assert list(meta) == BASE_META + keys
    assert [meta[k] for k in BASE_META] == [script, str(state), None, None, 64, 64, 7, "test", 4, -1.5, -1.0, 0.5]
    computed = {"pca_pose": args.pose, "frc_mask_radius": infer.frc_mask_radius(args, 12, 10) if args.frc else None}
    for k in keys:
        want = computed.get(k, vars(args).get(k))
        assert meta[k] == want and type(meta[k]) is type(want), k
    if "frc" in keys:
        assert meta["frc_mask_radius"] == (0.0 if "--frc_mask_radius" in extra else 2.0) and meta["frc"] is True
    if "cluster" in keys:
        assert meta["cluster_seed"] == 7 and meta["pose"] == "iw"
    if "--labels" in extra:
        assert meta["labels"] == str(labels) and "label_array" not in meta
    cut = infer.run_meta(args, facts, figures, without=("pca",))
    assert list(cut.items()) == [(k, v) for k, v in meta.items() if not k.startswith("pca")]
    assert json.loads(json.dumps(meta)) == meta and list(json.loads(json.dumps(meta))) == list(meta)
