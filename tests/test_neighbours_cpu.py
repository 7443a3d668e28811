"""CPU-only: what is include/svae_neighbours.h's own in its binding, the float64 reference of the neighbour kernels
(tests/neighbours_ref.py) held to a brute-force sort on a fixture full of ties, and neighbours.py's command line: its defaults
and every refusal that needs no GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbours_ref as R
from test_binding_cpu import binding_constants, parse_added_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the header and its table
def test_neighbour_binding_matches_its_header():
    """What is include/svae_neighbours.h's own (the rules every added header shares are tests/test_binding_cpu.py's): two
    functions and their argument names, no struct; the header's one constant is _lib.NEIGHBOUR_LIMITS, and none of this adds an
    upper-case integer to the binding; the positions of the device pointers."""
    from spatial_vae_amd import _lib, ops
    H = parse_added_header("svae_neighbours.h")[1]
    assert _lib.HEADERS["svae_neighbours.h"] is _lib.NEIGHBOUR_SIGNATURES
    assert H["structs"] == {} and len(H["functions"]) == 2
    assert H["constants"] == {"SVAE_NBR_" + k.upper(): v for k, v in _lib.NEIGHBOUR_LIMITS.items()} == {"SVAE_NBR_MAX_K": 256}
    assert _lib.NEIGHBOUR_LIMITS == {"max_k": 256} and R.MAX_K == 256 and R.MAX_T == 257
    names = {k: [a[2] for a in v[1]] for k, v in H["functions"].items()}
    assert names["svae_nbr_search"] == ["query", "B", "query_base", "cand", "M", "cand_base", "D", "K", "best_d2", "best_index",
                                        "stream"]
    assert names["svae_nbr_average"] == ["stack", "cover", "images", "N", "C", "index", "weight", "B", "T", "average", "support",
                                         "stream"]
    assert not [k for k in binding_constants(_lib) if "NBR" in k or "NEIGHBOUR" in k]
    assert ops._POINTER_ARGS["svae_nbr_search"] == (0, 3, 8, 9)
    assert ops._POINTER_ARGS["svae_nbr_average"] == (0, 1, 5, 6, 9, 10)
    assert ops.NeighbourSearch.MAX_K == 256


# ---------------------------------------------------------------- the reference against brute force
def test_reference_chunked_updates_equal_a_full_sort_where_ties_decide():
    """Integer-lattice latents (values in -3..3, D = 2, 150 images, K = 5): every row has tied distances and in at least half the
    rows the cut after K entries falls inside a tie, so the rule `of equal d2 the lower index first` decides what is kept.  The
    reference's running lists -- one call, candidates in chunks in three different orders, queries in three parts -- equal the
    full sort of the (d2, index) tuples exactly."""
    z, K = R.lattice(), 5
    tied, cut = R.ties_at_cut(z, K)
    print("lattice: %d of %d rows have ties, in %d the cut falls inside one" % (tied.sum(), z.shape[0], cut.sum()))
    assert tied.all() and cut.sum() * 2 >= z.shape[0]
    want_d, want_i = R.brute_force(z, K)
    assert (want_i >= 0).all() and (want_i != np.arange(150)[:, None]).all()
    chunks = [(0, 64), (64, 70), (70, 150)]
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        got_d, got_i = R.search_all(z, K, [chunks[o] for o in order])
        assert got_d.tobytes() == want_d.tobytes() and np.array_equal(got_i, want_i), order
    got_d, got_i = R.search_all(z, K, query_chunks=[(0, 50), (50, 51), (51, 150)])
    assert got_d.tobytes() == want_d.tobytes() and np.array_equal(got_i, want_i)
    got_d, got_i = R.search_all(z, K)
    assert got_d.tobytes() == want_d.tobytes() and np.array_equal(got_i, want_i)


def test_reference_leaves_non_finite_latents_out_and_short_lists_end_in_empty_slots():
    """A NaN and an inf latent list nothing and are listed by nobody; with fewer admissible candidates than K the list ends in
    (+inf, -1) slots."""
    z = np.random.RandomState(1).randn(12, 3)
    z[4, 1], z[9, 0] = np.nan, np.inf
    d, i = R.search_all(z, 16, [(0, 5), (5, 12)])
    assert (i[4] == -1).all() and (i[9] == -1).all() and np.isinf(d[4]).all() and np.isinf(d[9]).all()
    ok = [b for b in range(12) if b not in (4, 9)]
    assert not np.isin(i[ok], [4, 9]).any()
    assert ((i[ok] >= 0).sum(1) == 9).all() and (i[ok][:, 9:] == -1).all() and np.isinf(d[ok][:, 9:]).all()
    assert (np.diff(d[ok][:, :9], axis=1) >= 0).all()


def test_reference_average_skips_and_weights():
    """The average's rules on a hand-checked case: out-of-range and uncovered slots are skipped, a pixel nobody covers is +0 with
    support 0, and weights enter numerator and denominator."""
    stack = np.array([[[1.0], [2.0]], [[3.0], [5.0]], [[7.0], [11.0]]], np.float32)
    cover = np.array([[1, 1], [1, 0], [0, 0]], np.uint8)
    index = np.array([[0, 1, -1, 3], [2, 2, -7, 2], [1, 0, 2, 1]], np.int64)
    avg, sup, _ = R.average(stack, cover, index)
    assert avg[:, :, 0].tolist() == [[2.0, 2.0], [0.0, 0.0], [np.float32(7.0 / 3.0), 2.0]] and sup.tolist() == [[2, 1], [0, 0], [3, 1]]
    assert not np.signbit(avg).any()
    w = np.array([[1.0, 3.0, 1.0, 1.0]] * 3)
    avg, sup, _ = R.average(stack, cover, index, w)
    assert avg[0, :, 0].tolist() == [2.5, 2.0] and sup[0].tolist() == [4.0, 1.0]
    ones, _, _ = R.average(stack, None, index[:1])
    assert ones[0, :, 0].tolist() == [2.0, 3.5]


# ---------------------------------------------------------------- the command line
def _pipeline():
    from spatial_vae_amd import neighbours
    return neighbours


def _base(tmp_path, arrays=None, drop=(), **meta):
    """A command line that passes, with stand-in files: a state file (never opened by the parser) and a score file."""
    (tmp_path / "a.ckpt").write_bytes(b"x")
    record = dict({"script": "mnist", "split": "test", "images": 50, "state": "a.ckpt"}, **meta)
    stored = {"theta_iw": np.zeros(50, np.float32), "dx_iw": np.zeros((50, 2), np.float32), "z_iw": np.zeros((50, 2), np.float32),
              "z_q": np.zeros((50, 2), np.float32), "meta": np.array(json.dumps(record))}
    stored.update(arrays or {})
    for k in drop:
        del stored[k]
    np.savez(str(tmp_path / "s.npz"), **stored)
    return ["mnist", "--state", str(tmp_path / "a.ckpt"), "--scores", str(tmp_path / "s.npz"), "--out", str(tmp_path / "n.npz")]


def test_defaults_are_the_stated_conventions(tmp_path):
    args = _pipeline().neighbour_arguments(_base(tmp_path))
    assert (args.neighbours, args.latent, args.pose, args.interp, args.weights) == (32, "iw", "iw", "bicubic", "uniform")
    assert (args.exclude_self, args.stack_gib, args.split, args.minibatch_size) == (False, 32.0, "test", 100)
    assert (args.averages, args.support, args.device) == (None, None, -2)
    assert args.score_meta["images"] == 50 and sorted(args.score_arrays) == ["dx_iw", "theta_iw", "z_iw"]
    assert all(vars(args)[k] is None for k in _pipeline().PATH_OVERRIDES)
    q = _pipeline().neighbour_arguments(_base(tmp_path) + ["--latent", "q", "--averages", "a.mrcs", "--support", "s.npy"])
    assert sorted(q.score_arrays) == ["dx_iw", "theta_iw", "z_q"]


REFUSALS = [
    (["--out", "n.npy"], "--out must end in .npz"),
    (["--scores", "s.npy"], "--scores must end in .npz"),
    (["--averages", "a.npz"], "--averages must end in .npy or .mrcs"),
    (["--averages", "a.npy", "--support", "s.mrcs"], "--support must end in .npy"),
    (["--support", "s.npy"], "--support needs --averages"),
    (["--neighbours", "0"], "--neighbours must be in [1, 256]"),
    (["--neighbours", "257"], "--neighbours must be in [1, 256]"),
    (["--minibatch_size", "0"], "--minibatch_size must be in [1, 2147483647]"),
    (["--stack_gib", "0"], "--stack_gib must be positive"),
    (["--generator", "g.sav"], "give either --state or --generator with --inference"),
    (["--", "--z-dim", "2"], "--state carries the training arguments"),
    (["--scores", "missing.npz"], "no such file: missing.npz"),
    (["--split", "train"], "was written for the split 'test', not 'train'"),
    (["--pose", "refined"], "--pose refined needs the pose_refined of infer.py --refine"),
    (["--latent", "best"], "has no z_best of shape (images, z_dim)"),
    (["--latent", "worst"], "invalid choice"),
    (["--weights", "cauchy"], "invalid choice"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals_made_by_the_parser(tmp_path, capsys, extra, message):
    """neighbour_arguments exits with code 2 and the reason on the last line of stderr."""
    with pytest.raises(SystemExit) as e:
        _pipeline().neighbour_arguments(_base(tmp_path) + extra)
    assert e.value.code == 2 and message in capsys.readouterr().err.strip().splitlines()[-1]


def test_refusals_made_from_the_score_file(tmp_path, capsys):
    """Another script's score file, a file that is no score file, a model without content latents: code 2 from the parser."""
    P = _pipeline()

    def refused(argv, message):
        with pytest.raises(SystemExit) as e:
            P.neighbour_arguments(argv)
        assert e.value.code == 2 and message in capsys.readouterr().err.strip().splitlines()[-1]

    refused(_base(tmp_path, script="galaxy"), "was written for the script 'galaxy', not 'mnist'")
    base = _base(tmp_path)
    np.savez(str(tmp_path / "s.npz"), z_iw=np.zeros((50, 2), np.float32))
    refused(base, "is not a score file of infer.py")
    refused(_base(tmp_path, arrays={"z_iw": np.zeros((50, 0), np.float32)}), "the model has z_dim = 0")
    refined = _base(tmp_path, arrays={"pose_refined": np.zeros((50, 3), np.float32)})
    assert P.neighbour_arguments(refined + ["--pose", "refined"]).score_arrays["pose_refined"].shape == (50, 3)


def test_refusals_that_need_the_split(tmp_path, capsys):
    """Where the split is known: the score file's image count, a missing pose array, latents that do not fit, a split of one
    image, an MRC stack of several channels and the size of the stack -- each exits with code 2 under this script's name; the
    same requests within the limits pass."""
    from spatial_vae_amd.eigen_images import stored_poses
    from spatial_vae_amd.infer_request import SplitFacts
    P = _pipeline()
    base = dict(n=28, m=28, channels=1, rotate=True, translate=True, inf_dim=5, z_scale=1, split="test", ctf_rows=None)
    f50, f49 = SplitFacts(images=50, **base), SplitFacts(images=49, **base)

    def refused(fn, message):
        with pytest.raises(SystemExit) as e:
            fn()
        last = capsys.readouterr().err.strip().splitlines()[-1]
        assert e.value.code == 2 and message in last and last.startswith("neighbours.py: "), last

    argv = _base(tmp_path)
    args = P.neighbour_arguments(argv)
    pose = stored_poses(args, f50, P._refuse)
    assert pose.shape == (50, 3) and pose.dtype == np.float32
    assert P.check_request(args, f50).shape == (50, 2)
    refused(lambda: stored_poses(args, f49, P._refuse), "holds 50 images, the test split has 49")
    refused(lambda: stored_poses(P.neighbour_arguments(argv + ["--pose", "q"]), f50, P._refuse), "has no theta_q of shape (50,)")
    refused(lambda: P.check_request(args, SplitFacts(images=50, **dict(base, inf_dim=3))), "the model has z_dim = 0")
    refused(lambda: P.check_request(args, SplitFacts(images=50, **dict(base, inf_dim=6))), "z_iw has shape (50, 2)")
    one = P.neighbour_arguments(_base(tmp_path, arrays={k: np.zeros((1,) + s, np.float32) for k, s in
                                                        (("theta_iw", ()), ("dx_iw", (2,)), ("z_iw", (2,)))}, images=1))
    refused(lambda: P.check_request(one, SplitFacts(images=1, **base)), "the test split has 1 image")
    mrcs = P.neighbour_arguments(_base(tmp_path) + ["--averages", "a.mrcs"])
    assert P.check_request(mrcs, f50).shape == (50, 2)
    refused(lambda: P.check_request(mrcs, SplitFacts(images=50, **dict(base, channels=3))), "an MRC stack holds one channel")
    small = P.neighbour_arguments(_base(tmp_path) + ["--averages", "a.npy", "--stack_gib", "0.0001"])
    refused(lambda: P.check_request(small, f50), "the aligned stack of 50 images needs 0.000 GiB, --stack_gib allows 0.0001")
    graph_only = P.neighbour_arguments(_base(tmp_path) + ["--stack_gib", "0.0001"])
    assert P.check_request(graph_only, f50).shape == (50, 2)         # no stack without --averages


def test_a_refusal_exits_with_code_2_before_the_library_or_the_device_is_touched(tmp_path):
    """Through the real command line in a fresh process: exit code 2, the reason on the last line of stderr, no output file, and
    the process neither loaded the kernel library nor initialised torch.cuda."""
    argv = _base(tmp_path) + ["--neighbours", "300"]
    code = ("import atexit, sys; sys.path.insert(0, %r); sys.argv = ['neighbours.py'] + %r\n"
            "import torch\nfrom spatial_vae_amd import _lib\n"
            "atexit.register(lambda: print('LIB', _lib._lib is None, 'CUDA', torch.cuda.is_initialized(), file=sys.stderr))\n"
            "import neighbours; sys.exit(neighbours.main())" % (ROOT, argv))
    out = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr[-2000:]
    lines = out.stderr.strip().splitlines()
    assert "--neighbours must be in [1, 256]" in lines[-2] and lines[-1] == "LIB True CUDA False"
    assert sorted(os.listdir(tmp_path)) == ["a.ckpt", "s.npz"]


def test_gaussian_weights_of_the_pipeline_follow_the_formula():
    """graph_arrays on the CPU (it is torch plumbing, no kernel): found, in_degree, the slots with and without the image itself,
    and gaussian weights within 1e-12 of numpy's formula, 1 where the list is empty or its largest distance is 0."""
    import argparse
    import torch
    P = _pipeline()
    z = np.random.RandomState(3).randn(9, 2)
    z[7] = np.nan
    z[1] = z[0]
    d2, index = R.search_all(z, 3)
    d2[0, 1:], index[0, 1:] = np.inf, -1                        # a list whose only entry is at distance 0
    for exclude in (False, True):
        args = argparse.Namespace(exclude_self=exclude, weights="gaussian")
        found, deg, slots, w = (t.numpy() for t in P.graph_arrays(args, torch.from_numpy(d2), torch.from_numpy(index)))
        assert found.tolist() == [1, 3, 3, 3, 3, 3, 3, 0, 3] and deg.tolist() == np.bincount(index[index >= 0], minlength=9).tolist()
        assert deg[7] == 0 and np.array_equal(slots[:, 1:], index)
        assert slots[:, 0].tolist() == ([-1] * 9 if exclude else list(range(9)))
        want = R.gaussian_weights(d2, index)
        assert np.abs(w - want).max() <= 1e-12 and (w[0] == 1).all() and (w[7] == 1).all() and (w[:, 0] == 1).all()
        assert (w[2, 1:] < 1).all() and abs(w[2, 3] - np.exp(-0.5)) <= 1e-12
    args = argparse.Namespace(exclude_self=False, weights="uniform")
    assert (P.graph_arrays(args, torch.from_numpy(d2), torch.from_numpy(index))[3] == 1).all()
