"""The suppression options without a GPU: the NumPy restatement (tests/nms_options_reference.py) against hand-worked answers, the
case list's power to tell the rule from seven plausible wrong ones, the Gaussian cases' decision margins, the config fields
(squeezedet_amd.nms) and the --nms flags (squeezedet_amd.drivers, eval.py, demo.py)."""
import argparse
import importlib.util
import os

import numpy as np
import pytest

from squeezedet_amd import drivers, nms
from squeezedet_amd._lib import SqdetError
from tests import nms_options_cases as NC
from tests import nms_options_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in NC.CASES}


def run(case, method, overlap="iou", agnostic=False, **kw):
    return R.suppress(case["out"], case["classes"], method, overlap, agnostic, case["nms_thresh"], case["sigma"], case["score_floor"], **kw)


def kept(res, b=0):
    k = int(res[4][b])
    return res[3][b, :k].tolist(), res[1][b, :k]


# ---------------------------------------------------------------- hand-worked answers
def test_chain_by_hand():
    """A-B-C, shifts of 3: IoU(A,B) = IoU(B,C) = 7/13 > 0.4, IoU(A,C) = 4/16.  The reference's rule drops B and C (B, itself
    dropped, still suppresses C); greedy keeps C; Soft-NMS linear keeps all: B decays by 6/13 under A and again under C."""
    c = CASES["chain"]
    assert kept(run(c, "nongreedy"))[0] == [700]
    assert kept(run(c, "greedy"))[0] == [700, 9000]
    res = run(c, "soft_linear")
    idx, p = kept(res)
    assert idx == [700, 9000, 40]                        # pick order: A, C, then the decayed B
    assert res[0][0, :3, 0].tolist() == [100.0, 106.0, 103.0] and (res[0][0, :3, 1:] == [50, 10, 10]).all()      # the boxes travel with their rows
    np.testing.assert_allclose(p, [0.9, 0.7, 0.8 * (6 / 13) * (6 / 13)], rtol=1e-6)
    idx, p = kept(run(c, "soft_gaussian"))
    u, v = 7 / 13, 4 / 16
    want_c, want_b = 0.7 * np.exp(-v * v / 0.5), 0.8 * np.exp(-u * u / 0.5)       # after A; B (0.448) is picked ahead of ...
    assert idx == [700, 9000, 40] and want_c > want_b
    np.testing.assert_allclose(p, [0.9, want_c, want_b * np.exp(-u * u / 0.5)], rtol=1e-6)
    for b in range(1):                                   # rows past the count are the filter's zeros
        res = run(c, "greedy")
        assert (res[0][b, 2:] == 0).all() and (res[1][b, 2:] == 0).all() and (res[2][b, 2:] == -1).all() and (res[3][b, 2:] == -1).all()


def test_chain_across_classes_by_hand():
    c = CASES["chain_across_classes"]
    for method in ("nongreedy", "greedy"):
        assert kept(run(c, method))[0] == [700, 40, 9000]                  # three classes: nothing suppresses per class
    assert kept(run(c, "nongreedy", agnostic=True))[0] == [700]
    assert kept(run(c, "greedy", agnostic=True))[0] == [700, 9000]         # (classes 0 and 2: still class order)


def test_floor_by_hand():
    """Class 0: 0.9 is picked; its copy decays to 0.004 * (1 - 1) = 0, the neighbour one pixel off (IoU 1560/1640) to
    0.5 * 80/1640 = 0.0244, the other neighbour to 0.002 * 80/1640 < floor; 0.0015 (no overlap) stays above the floor, 0.0005
    never was.  Class 1: 0.0011 is untouched per class.  The floor ends the picks at the first score below 0.001."""
    c = CASES["decay_across_floor"]
    idx, p = kept(run(c, "soft_linear"))
    assert idx == [1, 3, 5, 7]
    np.testing.assert_allclose(p, [0.9, 0.5 * (80 / 1640), 0.0015, 0.0011], rtol=1e-6)
    # class-agnostic Gaussian: the class-1 row at (230, 100) overlaps the picked ones and falls through the floor
    assert kept(run(c, "soft_gaussian", agnostic=True))[0] == [1, 3, 5]


def test_strict_threshold_and_diou_by_hand():
    c = CASES["iou_exactly_at_thresh"]
    assert float(R.iou_center(c["out"][0][0, 0], c["out"][0][0, 1])) == 0.5
    for overlap in R.OVERLAPS:
        assert kept(run(c, "greedy", overlap))[0] == [11, 12]              # 0.5 > 0.5 is false
    c = CASES["offset_iou_vs_diou"]
    assert kept(run(c, "greedy", "iou"))[0] == [1, 3]                      # IoU 0.538 > 0.52
    assert kept(run(c, "greedy", "diou"))[0] == [1, 2, 3]                  # DIoU 0.505 is not
    c = CASES["concentric"]
    for method in ("nongreedy", "greedy"):
        for agn in (False, True):
            assert kept(run(c, method, "iou", agn))[0] == kept(run(c, method, "diou", agn))[0]


def test_bad_counts_pass_through():
    c = CASES["bad_counts_among_good"]
    for method, overlap, agn in NC.COMBOS:
        res = run(c, method, overlap, agn)
        for b in (1, 3):
            for t in range(5):
                assert np.array_equal(res[t][b], c["out"][t][b])
        assert 0 < res[4][0] <= 20 and 0 < res[4][2] <= 9


def test_counts_and_order_properties():
    for c in NC.CASES:
        for method, overlap, agn in NC.COMBOS:
            res = run(c, method, overlap, agn)
            for b in range(len(res[4])):
                k, k0 = int(res[4][b]), int(c["out"][4][b])
                if not 0 <= k0 <= c["out"][1].shape[1]:
                    continue
                cl = res[2][b, :k]
                assert 0 <= k <= k0 and (np.diff(cl) >= 0).all() and ((cl >= 0) & (cl < c["classes"])).all()
                for cc in set(cl.tolist()):                                 # within a class: non-increasing final score
                    assert (np.diff(res[1][b, :k][cl == cc]) <= 0).all(), (c["name"], method)
                assert set(res[3][b, :k].tolist()) <= set(c["out"][3][b, :k0].tolist())


# ---------------------------------------------------------------- the cases discriminate
MUTANT_RUNS = {     # mutation -> the (method, overlap, agnostic) runs it can show in
    "greedy_as_nongreedy": [("greedy", "iou", False)],
    "ge_for_gt": [("greedy", "iou", False), ("nongreedy", "iou", False), ("soft_linear", "iou", False)],
    "no_class_test": [(m, "iou", False) for m in R.METHODS],
    "rank_tie_reversed": [("greedy", "iou", False), ("soft_linear", "iou", False), ("soft_gaussian", "iou", False)],
    "pick_tie_reversed": [("soft_linear", "iou", False), ("soft_gaussian", "iou", False)],
    "no_diou_penalty": [("greedy", "diou", False), ("nongreedy", "diou", False)],
    "floor_moved": [("soft_linear", "iou", False), ("soft_gaussian", "iou", False)],
}


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_fails_a_case(mutation):
    """Each wrong rule must change the output of at least one case under EVERY run listed for it: the cases discriminate."""
    for method, overlap, agn in MUTANT_RUNS[mutation]:
        caught = []
        for c in NC.CASES:
            good, bad = run(c, method, overlap, agn), run(c, method, overlap, agn, mutate=mutation)
            if not all(np.array_equal(g.view(np.uint8), b_.view(np.uint8)) for g, b_ in zip(good, bad)):
                caught.append(c["name"])
        assert caught, "%s under %s/%s is not told from the rule by any case" % (mutation, method, overlap)


def test_named_cases_catch_their_mutation():
    differs = lambda c, m, o, mut: not np.array_equal(run(c, m, o)[3], run(c, m, o, mutate=mut)[3])
    assert differs(CASES["chain"], "greedy", "iou", "greedy_as_nongreedy")
    assert differs(CASES["iou_exactly_at_thresh"], "greedy", "iou", "ge_for_gt")
    assert differs(CASES["chain_across_classes"], "greedy", "iou", "no_class_test")
    assert differs(CASES["equal_probs"], "soft_linear", "iou", "rank_tie_reversed")
    assert differs(CASES["equal_probs"], "soft_gaussian", "iou", "pick_tie_reversed")
    assert differs(CASES["offset_iou_vs_diou"], "greedy", "diou", "no_diou_penalty")
    assert differs(CASES["decay_across_floor"], "soft_linear", "iou", "floor_moved")


def test_gaussian_cases_keep_clear_of_rounding():
    """soft_gaussian is the one rule whose arithmetic is not bit-reproducible across libms (exp): every pick and every floor
    test of every case must have a relative margin >= 1e-9 -- two exps differ by ~1e-16 relative, accumulated over at most 63
    decays that stays at least four orders below."""
    for c in NC.CASES:
        for agn in (False, True):
            _, mg = run(c, "soft_gaussian", "iou", agn, margins=True)
            assert mg.pick >= 1e-9 and mg.floor >= 1e-9, (c["name"], agn, mg.pick, mg.floor)
    _, mg = run(CASES["iou_exactly_at_thresh"], "greedy", margins=True)
    assert mg.overlap == 0.0                                   # (the strict-compare case sits ON the threshold, on purpose)


# ---------------------------------------------------------------- config fields
def test_nms_options_defaults_and_is_default():
    class Bare:
        NMS_THRESH = 0.4
    opt = nms.nms_options(Bare())
    assert opt == nms.NmsOptions("reference", "iou", 0.5, 0.001, False) and nms.is_default(opt)
    assert nms.nms_options({}) == opt
    assert nms.NMS_METHODS == ("reference", "greedy", "soft_linear", "soft_gaussian") and nms.NMS_OVERLAPS == ("iou", "diou")
    assert nms.first_stage_thresh(opt, Bare()) == 0.4
    for field, value in (("NMS_METHOD", "greedy"), ("NMS_OVERLAP", "diou"), ("NMS_CLASS_AGNOSTIC", True), ("NMS_METHOD", "soft_linear")):
        o = nms.nms_options({field: value})
        assert not nms.is_default(o) and nms.first_stage_thresh(o, Bare()) == float("inf")
    # sigma and the floor alone do not leave the default rule
    assert nms.is_default(nms.nms_options({"NMS_SIGMA": 0.3, "NMS_SCORE_FLOOR": 0.01}))
    assert nms.kernel_method(nms.nms_options({"NMS_OVERLAP": "diou"})) == "nongreedy"
    assert nms.kernel_method(nms.nms_options({"NMS_METHOD": "soft_gaussian"})) == "soft_gaussian"
    assert nms.KERNEL_METHODS == R.METHODS and nms.NMS_OVERLAPS == R.OVERLAPS


@pytest.mark.parametrize("fields", [{"NMS_METHOD": "hard"}, {"NMS_OVERLAP": "giou"}, {"NMS_METHOD": "soft_linear", "NMS_OVERLAP": "diou"},
                                    {"NMS_SIGMA": 0.0}, {"NMS_SIGMA": float("nan")}, {"NMS_SCORE_FLOOR": float("inf")}])
def test_nms_options_refusals(fields):
    with pytest.raises(SqdetError):
        nms.nms_options(fields)


def test_apply_names_top_n_detection_beyond_64_rows():
    class Rows:
        shape = (2, 65)

    class Mc:
        TOP_N_DETECTION, ANCHORS, CLASSES, NMS_THRESH = 0, 16848, 3, 0.4
    with pytest.raises(SqdetError, match="TOP_N_DETECTION"):
        nms.apply(nms.nms_options({"NMS_METHOD": "greedy"}), Mc(), (None, Rows(), None, None, None))


# ---------------------------------------------------------------- flags
def _parser():
    ap = argparse.ArgumentParser()
    drivers.add_nms_args(ap)
    return ap


def test_flags_leave_nothing_behind_when_not_given():
    ap = _parser()
    assert vars(ap.parse_args([])) == {}
    a = ap.parse_args(["--nms", "soft_gaussian", "--nms_sigma", "0.3", "--nms_score_floor", "0.01", "--nms_class_agnostic"])
    assert vars(a) == dict(nms="soft_gaussian", nms_sigma=0.3, nms_score_floor=0.01, nms_class_agnostic=True)
    drivers.check_nms_args(ap, a)


def test_nms_policy_sets_the_config():
    from squeezedet_amd import config
    mc = config.kitti_squeezeDet_config()
    ap = _parser()
    policy = drivers.nms_policy(ap.parse_args([]), mc)
    assert policy["default"] and policy["nms_thresh"] == mc.NMS_THRESH and nms.is_default(nms.nms_options(mc))
    policy = drivers.nms_policy(ap.parse_args(["--nms", "greedy", "--nms_overlap", "diou"]), mc)
    assert (mc.NMS_METHOD, mc.NMS_OVERLAP, mc.NMS_CLASS_AGNOSTIC) == ("greedy", "diou", False) and not policy["default"]
    assert "greedy" in drivers.format_nms_policy(policy) and "diou" in drivers.format_nms_policy(policy)
    mc.TOP_N_DETECTION = 100
    with pytest.raises(SystemExit, match="TOP_N_DETECTION"):
        drivers.nms_policy(ap.parse_args(["--nms", "greedy"]), mc)
    drivers.nms_policy(ap.parse_args([]), mc)                  # (the default rule has no such limit)


@pytest.mark.parametrize("argv, text", [
    (["--nms", "soft_linear", "--nms_overlap", "diou"], "diou goes with"),
    (["--nms", "soft_gaussian", "--nms_sigma", "0"], "finite S > 0"),
    (["--nms", "soft_linear", "--nms_score_floor", "inf"], "finite X"),
    (["--nms", "greedy", "--nms_sigma", "0.3"], "needs --nms soft_gaussian"),
    (["--nms_score_floor", "0.01"], "needs --nms soft_linear or soft_gaussian"),
    (["--nms", "fuzzy"], "invalid choice"),
])
def test_flag_refusals(argv, text, capsys):
    ap = _parser()
    with pytest.raises(SystemExit):
        drivers.check_nms_args(ap, ap.parse_args(argv))
    assert text in capsys.readouterr().err


def _script(name):
    spec = importlib.util.spec_from_file_location("nms_flags_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["eval", "demo"])
def test_scripts_take_the_flags(name, capsys):
    mod = _script(name)
    assert not any(k.startswith("nms") for k in vars(mod.parse_args([])))
    a = mod.parse_args(["--nms", "greedy", "--nms_class_agnostic"])
    assert a.nms == "greedy" and a.nms_class_agnostic is True
    with pytest.raises(SystemExit):
        mod.parse_args(["--nms", "soft_linear", "--nms_overlap", "diou"])
    assert "diou goes with" in capsys.readouterr().err
