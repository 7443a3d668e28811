"""Writes tests/golden/infer_args_snapshot.json: what infer.py's command line (spatial_vae_amd.infer.infer_arguments) and its
request check (check_request) give for a fixed list of argvs, so that a later rewrite of either can be held to it.

It is run ONCE, at the commit the file records (produced_by_commit), where infer_arguments is a ladder of p.error calls and
check_request a ladder of _refuse calls: the generator notes the source line of every such call that fires and refuses to
write the file unless every one of them fired, so the refused cases below cover every refusal that commit can make.  At a
later commit the ladders are gone and that assertion no longer means anything: do not regenerate, replay
(tests/test_infer_cpu.py::test_command_line_reproduces_the_snapshot_taken_before_the_options_became_a_table).

Files that must exist are created in a temporary directory whose name is stored as {tmp}, in the argvs and in the messages:
a.ckpt, g.sav, q.sav (one byte each) and the label files of LABEL_FILES.

  python tests/golden/gen_infer_args_snapshot.py
"""
import argparse
import contextlib
import inspect
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["COLUMNS"] = "80"        # argparse wraps usage and help to the terminal

from spatial_vae_amd import infer   # noqa: E402

LABEL_FILES = {
    "ok.npy": {"dtype": "int64", "data": [0, 1, 2, -1]},
    "ten.npy": {"dtype": "int32", "data": [0, 1, 2, -1, 0, 1, 2, 0, 1, 2]},
    "empty.npy": {"dtype": "int64", "data": []},
    "float.npy": {"dtype": "float32", "data": [0.0, 1.0]},
    "twod.npy": {"dtype": "int64", "data": [[0, 1], [1, 0]]},
    "below.npy": {"dtype": "int64", "data": [0, -2]},
    "many.npy": {"dtype": "int64", "data": [4096]},
    "half.npy": {"dtype": "int64", "data": [2048, 0]},
}

S = ["mnist", "--state", "{tmp}/a.ckpt", "--out", "s.npz"]
P = ["particles", "--state", "{tmp}/a.ckpt", "--out", "s.npz"]
SAV = ["--generator", "{tmp}/g.sav", "--inference", "{tmp}/q.sav", "--out", "s.npz"]
C = ["--class_averages", "c.npz"]
R = C + ["--refine", "2"]
RR = R + ["--reassign"]
SOFT = RR + ["--refine_soft"]
K = ["--cluster", "3", "--cluster_out", "k.npz"]
K_ALL = K + ["--cluster_labels", "l.npy", "--cluster_iters", "7", "--cluster_restarts", "3", "--cluster_seed", "5"]
G = K + ["--cluster_gmm", "5"]
G_ALL = K_ALL + ["--cluster_gmm", "5", "--cluster_gmm_reg", "1e-4", "--cluster_gmm_tol", "0", "--cluster_min_resp", "0.5"]
PCA = ["--pca", "p.npz"]
PCA_ALL = PCA + ["--pca_components", "2", "--pca_traverse", "2", "--pca_steps", "3", "--pca_span", "1.5"]
LABELS = ["--labels", "{tmp}/ok.npy"]

ACCEPTED = [
    S,
    S + ["--num_samples", "5000", "--chunk", "50", "--minibatch_size", "7", "--seed", "3", "-d", "0"],
    S + ["--chunk", "1024", "--num_samples", "1"],
    S + ["--split", "train"],
    ["galaxy"] + S[1:] + ["--split", "train", "--train_path", "tr.npy", "--test_path", "te.npy"],
    P + ["--train_path", "tr.mrcs", "--test_path", "te.mrcs", "--ctf_train", "ctf_tr.txt", "--ctf_test", "ctf_te.txt"],
    S + ["--aligned", "a.npy"],
    S + ["--aligned", "a.mrcs", "--pose", "best", "--interp", "bilinear"],
    S + ["--recon", "r.npy", "--pose", "q"],
    S + ["--recon", "r.mrcs", "--interp", "bicubic"],
    S + C,
    S + C + ["--pose", "iw", "--aligned", "a.npy", "--recon", "r.npy"],
    S + C + LABELS,
    S + C + ["--labels", "{tmp}/empty.npy"],
    S + C + ["--labels", "{tmp}/ten.npy"],
    S + C + ["--frc"],
    S + C + ["--frc", "--frc_mask_radius", "5", "--frc_mask_edge", "2"],
    S + C + ["--frc", "--frc_mask_radius", "0"],
    S + C + LABELS + ["--frc", "--frc_mask_edge", "1.5"],
    S + R,
    S + R + ["--refine_angles", "3", "--refine_step", "1.5", "--refine_shift", "1"],
    S + C + ["--refine", "10", "--refine_angles", "0", "--refine_step", "2", "--refine_shift", "0"],
    S + C + ["--refine", "1", "--refine_angles", "32", "--refine_shift", "8", "--frc"],
    S + RR,
    S + RR + ["--reassign_labels", "new.npy"] + LABELS,
    S + SOFT,
    S + SOFT + ["--refine_soft_classes", "3", "--refine_soft_sigma2", "0.25"],
    S + SOFT + ["--refine_soft_classes", "64", "--frc", "--reassign_labels", "new.npy"],
    S + K,
    S + K + ["--seed", "9"],
    S + K_ALL,
    S + K + ["--pose", "best"],
    S + K + C + ["--cluster_labels", "l.npy", "--aligned", "a.npy", "--interp", "bilinear"],
    S + ["--cluster", "1024", "--cluster_out", "k.npz", "--cluster_restarts", "16"],
    S + G,
    S + G_ALL,
    S + G + C + ["--cluster_min_resp", "0.25", "--frc", "--refine", "1", "--reassign"],
    S + PCA,
    S + PCA + ["--pose", "q"],
    S + PCA_ALL,
    S + PCA + ["--pca_steps", "50", "--pca_span", "3"],
    S + PCA_ALL + K_ALL + ["--pca_per_class"],
    S + PCA + G_ALL + C + ["--pca_per_class", "--pca_traverse", "0"],
    P + ["--ctf_correct", "flip", "--aligned", "a.mrcs"],
    P + ["--ctf_correct", "flip"] + C + ["--frc", "--refine", "1"],
    P + ["--ctf_correct", "wiener"] + C,
    P + ["--ctf_correct", "wiener", "--wiener_lambda", "0.5"] + C + LABELS,
    P + ["--ctf_correct", "wiener", "--wiener_lambda", "0"] + C + ["--frc"],
    ["particles"] + SAV + ["--", "tr.mrcs", "te.mrcs", "--z-dim", "4", "--out", "not-ours"],
    ["mnist"] + SAV + ["--num_samples", "8", "--"],
    ["mnist"] + SAV + C + ["--", "--z_dim", "3"],
    S + C + LABELS + ["--frc", "--frc_mask_radius", "4", "--refine", "3", "--refine_angles", "2", "--reassign", "--refine_soft",
                      "--refine_soft_sigma2", "1", "--aligned", "a.npy", "--recon", "r.mrcs", "--pose", "best"] + PCA_ALL,
    P + ["--ctf_correct", "flip", "--aligned", "a.npy", "--split", "train"] + C + K_ALL + ["--cluster_gmm", "1000", "--frc",
                                                                                         "--refine", "1", "--pca_per_class"] + PCA,
]

# [argv, {limit of spatial_vae_amd.infer lowered for this case}]; the first block meets every p.error call, the second breaks
# two rules of different groups at once: the one reported is the one the ladder meets first
REFUSED = [[a, {}] for a in [
    S + ["--reassign"],
    S + C + ["--reassign"],
    S + ["--refine_soft_classes", "3"],
    S + RR + ["--refine_soft_sigma2", "1.0"],
    S + ["--refine_soft"],
    S + R + ["--refine_soft"],
    S + SOFT + ["--refine_soft_classes", "0"],
    S + SOFT + ["--refine_soft_classes", "65"],
    S + SOFT + ["--refine_soft_sigma2", "0"],
    S + SOFT + ["--refine_soft_sigma2", "inf"],
    S + SOFT + ["--refine_soft_sigma2", "nan"],
    S + SOFT + ["--refine_soft_sigma2", "-1.5"],
    S + R + ["--reassign_labels", "l.npy"],
    S + C + ["--reassign_labels", "l.npy"],
    S + RR + ["--reassign_labels", "l.npz"],
    S + RR + ["--reassign_labels", "labels"],
    S + C + ["--refine_angles", "3"],
    S + C + ["--refine_step", "1.0"],
    S + ["--refine_shift", "1"],
    S + C + ["--refine", "0"],
    S + C + ["--refine", "11"],
    S + ["--refine", "2"],
    S + ["--aligned", "a.npy", "--refine", "2"],
    P + R + ["--ctf_correct", "wiener"],
    S + R + ["--refine_angles", "33"],
    S + R + ["--refine_angles", "-1"],
    S + R + ["--refine_step", "0"],
    S + R + ["--refine_step", "inf"],
    S + R + ["--refine_step", "nan"],
    S + R + ["--refine_shift", "9"],
    S + R + ["--refine_shift", "-1"],
    S + C + ["--frc_mask_radius", "3"],
    S + C + ["--frc_mask_edge", "3"],
    S + ["--frc"],
    S + ["--aligned", "a.npy", "--frc"],
    S + C + ["--frc", "--frc_mask_radius", "-1"],
    S + C + ["--frc", "--frc_mask_radius", "inf"],
    S + C + ["--frc", "--frc_mask_radius", "nan"],
    S + C + ["--frc", "--frc_mask_edge", "0"],
    S + C + ["--frc", "--frc_mask_edge", "inf"],
    S + ["--cluster_out", "k.npz"],
    S + ["--cluster_labels", "l.npy"],
    S + ["--cluster_iters", "5"],
    S + ["--cluster_restarts", "2"],
    S + ["--cluster_seed", "0"],
    S + ["--cluster", "1", "--cluster_out", "k.npz"],
    S + ["--cluster", "1025", "--cluster_out", "k.npz"],
    S + K + C + LABELS,
    S + ["--cluster", "3"],
    S + ["--cluster", "3", "--cluster_out", "k.npy"],
    S + K + ["--cluster_labels", "l.npz"],
    S + K + ["--cluster_iters", "0"],
    S + K + ["--cluster_restarts", "0"],
    S + K + ["--cluster_restarts", "17"],
    S + K + ["--cluster_gmm_reg", "1e-3"],
    S + K + ["--cluster_gmm_tol", "0"],
    S + ["--cluster_min_resp", "0.5"],
    S + ["--cluster_gmm", "5"],
    S + K + ["--cluster_gmm", "0"],
    S + K + ["--cluster_gmm", "1001"],
    S + G + ["--cluster_gmm_reg", "0"],
    S + G + ["--cluster_gmm_reg", "inf"],
    S + G + ["--cluster_gmm_tol", "-1"],
    S + G + ["--cluster_gmm_tol", "nan"],
    S + G + ["--cluster_min_resp", "1"],
    S + G + ["--cluster_min_resp", "-0.1"],
    S + G + ["--cluster_min_resp", "nan"],
    S + ["--pca_components", "2"],
    S + ["--pca_traverse", "1"],
    S + ["--pca_steps", "3"],
    S + ["--pca_span", "2"],
    S + K + ["--pca_per_class"],
    S + ["--pca", "p.npy"],
    S + ["--pca", "axes"],
    S + PCA + ["--pca_per_class"],
    S + PCA + ["--pca_components", "0"],
    S + PCA + ["--pca_traverse", "-1"],
    S + PCA + ["--pca_steps", "0"],
    S + PCA + ["--pca_steps", "51"],
    S + PCA + ["--pca_span", "0"],
    S + PCA + ["--pca_span", "inf"],
    S + ["--ctf_correct", "flip", "--aligned", "a.npy"],
    ["galaxy"] + S[1:] + ["--ctf_correct", "wiener"] + C,
    P + ["--ctf_correct", "flip"],
    P + ["--ctf_correct", "flip", "--recon", "r.npy"],
    P + ["--ctf_correct", "wiener", "--aligned", "a.npy"],
    P + ["--wiener_lambda", "1"] + C,
    P + ["--ctf_correct", "flip", "--wiener_lambda", "1"] + C,
    P + ["--ctf_correct", "wiener", "--wiener_lambda", "-1"] + C,
    P + ["--ctf_correct", "wiener", "--wiener_lambda", "inf"] + C,
    S + ["--num_samples", "0"],
    S + ["--chunk", "0"],
    S + ["--chunk", "1025"],
    S + ["--minibatch_size", "0"],
    ["mnist", "--out", "s.npz"],
    S + ["--generator", "{tmp}/g.sav", "--inference", "{tmp}/q.sav", "--"],
    ["mnist", "--generator", "{tmp}/g.sav", "--out", "s.npz", "--"],
    ["mnist", "--inference", "{tmp}/q.sav", "--out", "s.npz", "--"],
    ["mnist"] + SAV,
    S + ["--", "--z_dim", "3"],
    ["mnist", "--state", "{tmp}/nope.ckpt", "--out", "s.npz"],
    ["mnist", "--generator", "{tmp}/g.sav", "--inference", "{tmp}/nope.sav", "--out", "s.npz", "--"],
    S + ["--aligned", "a.txt"],
    S + ["--recon", "r.npz"],
    S + ["--recon", "recon"],
    S + ["--class_averages", "c.npy"],
    S + LABELS,
    S + ["--aligned", "a.npy"] + LABELS,
    S + ["--pose", "best"],
    S + ["--interp", "bilinear"],
    S + K + ["--interp", "bilinear"],
    S + PCA + ["--interp", "bicubic"],
    S + C + ["--labels", "{tmp}/nope.npy"],
    S + C + ["--labels", "{tmp}/float.npy"],
    S + C + ["--labels", "{tmp}/twod.npy"],
    S + C + ["--labels", "{tmp}/below.npy"],
    S + C + ["--labels", "{tmp}/many.npy"],
    S + C + ["--frc", "--labels", "{tmp}/half.npy"],
]] + [
    [S + RR + LABELS, {"INFER_MAX_REASSIGN_CLASSES": 2}],
    [S + RR + K, {"INFER_MAX_REASSIGN_CLASSES": 2}],
] + [[a, {}] for a in [
    S + ["--reassign", "--frc"],
    S + ["--refine_angles", "3", "--frc_mask_edge", "2"],
    S + ["--frc", "--cluster", "1", "--cluster_out", "k.npz"],
    S + ["--cluster", "3", "--pca", "p.npy"],
    S + ["--cluster_gmm", "5", "--pca_steps", "3"],
    S + ["--pca", "p.npy", "--ctf_correct", "flip"],
    S + ["--ctf_correct", "flip", "--num_samples", "0"],
    ["mnist", "--state", "{tmp}/nope.ckpt", "--out", "s.npz", "--num_samples", "0"],
    S + ["--chunk", "0", "--aligned", "a.txt"],
    S + ["--aligned", "a.txt"] + LABELS,
    S + ["--wiener_lambda", "1", "--minibatch_size", "0"],
    S + ["--refine", "1", "--cluster_iters", "3"],
    S + ["--refine", "11", "--cluster_iters", "3"],
    S + ["--refine_soft_classes", "3", "--reassign_labels", "x.npy"],
    S + ["--pose", "best", "--cluster_restarts", "2"],
    P + R + ["--ctf_correct", "wiener", "--frc", "--frc_mask_radius", "-1"],
    S + ["--cluster", "3"] + C + LABELS,
    S + C + ["--frc", "--labels", "{tmp}/half.npy", "--refine", "1", "--refine_shift", "9"],
    S + K + ["--cluster_restarts", "17", "--cluster_gmm", "0"],
    S + G + ["--cluster_min_resp", "1", "--pca_per_class"],
    S + PCA + ["--pca_span", "0", "--wiener_lambda", "1"],
    P + ["--ctf_correct", "wiener", "--frc"],
    S + SOFT + ["--refine_soft_sigma2", "0", "--refine_step", "0"],
    S + RR + ["--reassign_labels", "l.npz", "--refine_shift", "9"],
    ["mnist", "--out", "s.npz", "--class_averages", "c.npy", "--labels", "{tmp}/nope.npy"],
    S + ["--interp", "bilinear", "--labels", "{tmp}/nope.npy"],
]]

FACTS = dict(images=10, n=8, m=8, channels=1, rotate=True, translate=True, inf_dim=5, z_scale=1, split="test", ctf_rows=None)
TEN = ["--labels", "{tmp}/ten.npy"]
# [argv, the SplitFacts fields that differ from FACTS]
REQUESTS = [
    [S + K, dict(inf_dim=3)],
    [S + K, dict(rotate=False, translate=False, inf_dim=0)],
    [S + K, dict(z_scale=0)],
    [S + K, dict(images=2, split="train")],
    [S + ["--cluster", "1024", "--cluster_out", "k.npz", "--cluster_gmm", "3"], dict(images=2 ** 18 + 1)],
    [S + PCA, dict(inf_dim=3)],
    [S + PCA, dict(images=0)],
    [S + PCA + ["--pca_components", "3"], {}],
    [S + PCA + ["--pca_traverse", "3"], {}],
    [S + PCA + ["--cluster", "1024", "--cluster_out", "k.npz", "--pca_per_class"], dict(images=2000, inf_dim=67)],
    [S + R, dict(rotate=False, translate=False, inf_dim=3)],
    [S + R, dict(n=1025)],
    [S + R + ["--frc"], dict(m=1025)],
    [S + C + ["--frc"], dict(n=1025, m=1025)],
    [S + C + LABELS, {}],
    [S + ["--aligned", "a.mrcs"], dict(channels=3)],
    [S + ["--aligned", "a.npy", "--recon", "r.mrcs"], dict(channels=3)],
    [P + ["--ctf_correct", "flip", "--aligned", "a.npy"], {}],
    [P + ["--ctf_correct", "wiener"] + C, dict(ctf_rows=5, split="train")],
    [P + ["--ctf_correct", "flip", "--aligned", "a.npy"], dict(ctf_rows=10, channels=3)],
    [P + ["--ctf_correct", "flip", "--aligned", "a.npy"], dict(ctf_rows=10, m=16)],
    # two at once: the first in the ladder's order is the one reported
    [P + K + ["--ctf_correct", "flip", "--aligned", "a.npy"], dict(inf_dim=3)],
    [S + K + PCA, dict(z_scale=0, inf_dim=3)],
    [S + PCA + ["--pca_components", "3"] + R, dict(n=1025)],
    [S + R + ["--frc"] + LABELS, dict(n=1025)],
    [S + C + LABELS + ["--aligned", "a.mrcs"], dict(channels=3)],
    # accepted
    [S, {}],
    [S + K + PCA_ALL + ["--pca_per_class"], {}],
    [S + ["--cluster", "1024", "--cluster_out", "k.npz", "--cluster_gmm", "3"], dict(images=2 ** 18)],
    [S + ["--cluster", "10", "--cluster_out", "k.npz"], {}],
    [S + R + ["--frc"] + TEN, dict(n=1024, m=1024, translate=False, inf_dim=3)],
    [S + C, dict(n=1025, rotate=False, translate=False, inf_dim=2)],
    [S + ["--aligned", "a.mrcs", "--recon", "r.npy"], {}],
    [S + ["--aligned", "a.npy"], dict(channels=3)],
    [P + ["--ctf_correct", "wiener"] + C, dict(ctf_rows=12)],
    [P + ["--ctf_correct", "flip", "--aligned", "a.npy"], dict(ctf_rows=10, m=16, rotate=False, inf_dim=4)],
    [S + PCA + ["--pca_components", "2", "--pca_traverse", "2"], dict(images=1)],
]


def call_lines(fn, call):
    """The source lines of fn on which `call` is called."""
    lines, first = inspect.getsourcelines(fn)
    return {first + i for i, line in enumerate(lines) if call in line}


def main():
    fired = {"p.error(": set(), "_refuse(": set()}
    parser_error, refuse = argparse.ArgumentParser.error, infer._refuse

    def noting_error(self, message):
        frame = sys._getframe(1)
        if frame.f_code is infer.infer_arguments.__code__:
            fired["p.error("].add(frame.f_lineno)
        parser_error(self, message)

    def noting_refuse(message):
        frame = sys._getframe(1)
        if frame.f_code is infer.check_request.__code__:
            fired["_refuse("].add(frame.f_lineno)
        refuse(message)

    argparse.ArgumentParser.error, infer._refuse = noting_error, noting_refuse
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("a.ckpt", "g.sav", "q.sav"):
            with open(os.path.join(tmp, name), "wb") as f:
                f.write(b"x")
        for name, spec in LABEL_FILES.items():
            np.save(os.path.join(tmp, name), np.array(spec["data"], dtype=spec["dtype"]))

        def there(argv):
            return [a.replace("{tmp}", tmp) for a in argv]

        def run(fn, *a):
            """(what fn returns or None, the exit code or None, stdout, stderr) with the directory's name put back as {tmp}."""
            out, err, code, got = io.StringIO(), io.StringIO(), None, None
            with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                try:
                    got = fn(*a)
                except SystemExit as e:
                    code = e.code
            return got, code, out.getvalue().replace(tmp, "{tmp}"), err.getvalue().replace(tmp, "{tmp}")

        def plain(k, v):
            if k == "label_array" and v is not None:
                return [int(x) for x in v]
            return v.replace(tmp, "{tmp}") if isinstance(v, str) else v

        _, code, text, _ = run(infer.infer_arguments, ["--help"])
        assert code == 0
        snapshot = {"help": " ".join(text.split()), "accepted": [], "refused": [], "requests": []}
        keys = None
        for argv in ACCEPTED:
            args, code, _, err = run(infer.infer_arguments, there(argv))
            assert code is None, (argv, err)
            items = [[k, plain(k, v)] for k, v in vars(args).items()]
            assert all(isinstance(v, (bool, int, float, str, list, type(None))) for _, v in items), items
            keys = keys or [k for k, _ in items]
            assert [k for k, _ in items] == keys, (argv, items)     # one order for every argv: stored once
            snapshot["accepted"].append({"argv": argv, "values": [v for _, v in items]})
        usages = set()
        for argv, lowered in REFUSED:
            was = {k: getattr(infer, k) for k in lowered}
            for k, v in lowered.items():
                setattr(infer, k, v)
            _, code, _, err = run(infer.infer_arguments, there(argv))
            for k in lowered:
                setattr(infer, k, was[k])
            assert code == 2, (argv, code)
            usage, message = err.rstrip("\n").rsplit("\n", 1)
            assert message.startswith("infer.py: error: "), err
            usages.add(" ".join(usage.split()))
            snapshot["refused"].append(dict({"argv": argv, "error": message}, **({"lowered": lowered} if lowered else {})))
        assert len(usages) == 1
        snapshot["usage"] = usages.pop()
        for argv, changed in REQUESTS:
            args, code, _, err = run(infer.infer_arguments, there(argv))
            assert code is None, (argv, err)
            got, code, _, err = run(infer.check_request, args, infer.SplitFacts(**dict(FACTS, **changed)))
            assert got is None and code in (None, 2) and (code is None) == (err == "") and err.count("\n") <= 1, (argv, code, err)
            snapshot["requests"].append({"argv": argv, "facts": dict(FACTS, **changed), "error": err.rstrip("\n") or None})
    argparse.ArgumentParser.error, infer._refuse = parser_error, refuse
    for call, fn in (("p.error(", infer.infer_arguments), ("_refuse(", infer.check_request)):
        missed = sorted(call_lines(fn, call) - fired[call])
        assert not missed and fired[call] == call_lines(fn, call), (call, "never fired at lines", missed, sorted(fired[call]))
    seen = [c["error"] for c in snapshot["refused"]]
    print("{} accepted, {} refused ({} p.error lines, {} distinct messages), {} requests ({} _refuse lines)".format(
        len(ACCEPTED), len(REFUSED), len(fired["p.error("]), len(set(seen)), len(REQUESTS), len(fired["_refuse("])))
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "spatial_vae_amd"], cwd=ROOT, capture_output=True, text=True,
                           check=True).stdout.strip()
    assert not dirty, "spatial_vae_amd differs from the commit: " + dirty
    head = {"produced_by_commit": commit, "columns": os.environ["COLUMNS"], "label_files": LABEL_FILES,
            "p_error_lines": sorted(fired["p.error("]), "refuse_lines": sorted(fired["_refuse("]), "keys": keys}
    path = os.path.join(ROOT, "tests", "golden", "infer_args_snapshot.json")
    with open(path, "w") as f:
        f.write("{" + ",\n ".join(json.dumps(k) + ": " + json.dumps(v) for k, v in head.items()))
        for key in ("help", "usage"):
            f.write(",\n " + json.dumps(key) + ": " + json.dumps(snapshot[key]))
        for key in ("accepted", "refused", "requests"):
            f.write(",\n " + json.dumps(key) + ": [\n  " + ",\n  ".join(json.dumps(c) for c in snapshot[key]) + "]")
        f.write("}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
