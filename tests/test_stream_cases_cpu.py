"""tests/stream_cases.py without a GPU: the table covers every entry point that takes a stream, its two input sets are what
the GPU tests assume, and dp.TrainStep.capture refuses a step it cannot capture before it touches torch.cuda."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import stream_cases as S
from spatial_vae_amd import _lib


def test_the_table_covers_exactly_the_entry_points_that_take_a_stream():
    """The names are derived from _lib.ALL_SIGNATURES, the signature tables of every header of _lib.HEADERS (status returned,
    last argument a bare address), never typed: a new export that takes a stream fails here until it has a case."""
    derived = S.stream_entry_points()
    assert len(derived) >= 50 and "svae_decoder_backward" in derived and "svae_wiener_finish" in derived
    assert "svae_eig_rotate" in derived and "svae_nbr_average" in derived
    assert "svae_profile_read" not in derived and "svae_saved_bytes" not in derived
    assert S.covered_entry_points() == derived
    assert set(derived) <= set(_lib.ALL_SIGNATURES)
    assert len(set(S.NAMES)) == len(S.NAMES)


def test_not_capturable_is_small_and_spares_what_the_training_step_needs():
    assert len(S.NOT_CAPTURABLE) <= 3 and set(S.NOT_CAPTURABLE) <= set(S.stream_entry_points())
    needed = ("decoder", "loglik", "latent", "head", "linear", "colsum", "adam", "guard")
    assert not [n for n in S.NOT_CAPTURABLE if any(w in n for w in needed)]


@pytest.mark.parametrize("name", S.NAMES)
def test_both_input_sets_have_one_layout_and_different_values(name):
    case = S.make_case(name)
    a, b = case.inputs(0), case.inputs(1)
    assert list(a) == list(b) and a
    assert set(case.same_in_both_sets) < set(a), "every input is the same in both sets"
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert a[k].dtype in (np.float32, np.float64, np.int32, np.int64, np.uint8), (k, a[k].dtype)
        if a[k].dtype.kind == "f":                          # finite, but for what a case holds on purpose (the guard's one inf)
            assert (np.isfinite(a[k]).all() and np.isfinite(b[k]).all()) != (k in case.non_finite_inputs), k
        if k in case.same_in_both_sets:                     # stated by the case: a mask, a candidate table, a zero record
            assert np.array_equal(a[k], b[k]), "%s: %s differs between the sets" % (name, k)
        else:
            assert not np.array_equal(a[k], b[k]), "%s: %s is the same in both sets" % (name, k)
    again = case.inputs(0)
    assert all(a[k].tobytes() == again[k].tobytes() for k in a)
    assert set(case.state) <= set(a)


def test_integer_inputs_are_valid_in_both_sets():
    for seed in (0, 1):
        for case in S.make_cases():
            i = case.inputs(seed)
            if "quarter" in i:
                assert set(i["quarter"].tolist()) <= {-1, 0, 1, 2, 3} and (i["quarter"] >= 0).sum() == 4
            if "label" in i:
                assert (i["label"] >= -1).all() and (i["label"] < case.n_classes).all()
            if "mask" in i:
                assert set(i["mask"].tolist()) <= {0, 1} and i["mask"].any()
            # the analysis headers give every int32 a meaning: an entry outside the live range is a point in no group, an image
            # that is skipped, an empty slot or a reference folded into no class.  Each set holds live entries and, where the
            # case means to exercise it, -1 and an entry past the range.
            if "label_in" in i:                             # svae_gmm.h: the start's labels, every point in a class
                assert (i["label_in"] >= 0).all() and (i["label_in"] < case.k).all()
            if "group" in i:                                # svae_pca.h: outside [0, G) is no group
                live = (i["group"] >= 0) & (i["group"] < case.G)
                assert live.sum() >= 2 and -1 in i["group"] and (i["group"] >= case.G).any()
            if "ref_index" in i:                            # svae_refine.h: outside [0, n_ref) is skipped
                assert (i["ref_index"] >= -1).all() and (i["ref_index"] < case.n_ref).all() and -1 in i["ref_index"]
            if "cand" in i:                                 # svae_classify.h, svae_expect.h: outside [0, n_ref) is an empty slot
                live = (i["cand"] >= 0) & (i["cand"] < case.n_ref)
                assert (i["cand"] >= -1).all() and -1 in i["cand"] and live.any(1).sum() == len(live) - 1
            if "target" in i and i["target"].dtype == np.int32:     # svae_expect.h: outside [0, n_classes) is folded into no class
                assert i["target"].shape == (case.n_ref,) and (i["target"] >= 0).all()
                assert set(range(case.n_classes)) <= set(i["target"].tolist())
            if "class_of" in i:                             # svae_eigen.h: outside [0, K) is an image in no class
                live = (i["class_of"] >= 0) & (i["class_of"] < case.K)
                assert live.sum() >= 2 and -1 in i["class_of"] and (i["class_of"] >= case.K).any()
                assert i["members"].tolist() == [int((i["class_of"] == k).sum()) for k in range(case.K)]
            if "slots" in i:                                # svae_neighbours.h: outside [0, images) is skipped
                live = (i["slots"] >= 0) & (i["slots"] < case.images)
                assert live.any() and -1 in i["slots"] and (i["slots"] >= case.images).any()
                assert i["stack"].shape[0] == case.images and (i["index"] == -1).all() and np.isposinf(i["d2"]).all()
    g = S.Guard()
    assert np.isfinite(g.inputs(0)["grad"]).all() and np.isinf(g.inputs(1)["grad"]).sum() == 1
    assert np.isfinite(g.inputs(1, finite=True)["grad"]).all()
    assert S.Guard.record(g.inputs(1)["control"]).t == 7 and S.Guard.record(g.inputs(0)["control"]).steps == 0


def test_the_ctf_cases_take_the_forms_their_names_say():
    import ref64
    assert ref64.ctf_form(*S.CTF_LDS_PAIR) == "lds" and S.CTF_LDS_PAIR in ref64.CTF_BOTH_FORMS
    assert ref64.ctf_form(*S.CTF_GLOBAL_PAIR) == "global" and S.CTF_GLOBAL_PAIR in ref64.CTF_PAIRS


def test_capture_on_a_cpu_step_names_the_hip_device():
    """A CPU step has no stream to capture: a RuntimeError that says so and names fused_adam=True, not an AttributeError or
    an assertion from torch.cuda.Stream."""
    from spatial_vae_amd import dp

    def toy(x, y, p_net, q_net, noise=None):
        z = q_net(y)
        rec = p_net(z[:, :2] + noise)
        elbo = -((rec - y) ** 2).sum(1).mean() - (z ** 2).mean()
        return elbo, elbo.detach(), elbo.detach()

    torch.manual_seed(1)
    step = dp.TrainStep(nn.Sequential(nn.Linear(2, 8), nn.Tanh(), nn.Linear(8, 5)),
                        nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 4)), toy, lr=1e-2)
    y, noise = torch.randn(6, 5), torch.randn(6, 2)
    with pytest.raises(RuntimeError, match="HIP device") as info:
        step.capture(None, y, noise=noise)
    assert "fused_adam=True" in str(info.value) and "cpu" in str(info.value)
    assert step._graph is None
    step(None, y, noise=noise)                              # the refused capture left the eager step usable
