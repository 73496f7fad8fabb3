"""The anchor-assignment options without a GPU: the NumPy restatement (tests/assign_reference.py) against hand-worked answers, the
reference's pick as a subset of every mode's positives, every case of tests/assign_cases.py reaching the branch it is named after
(asserted on the restatement's own statistics), every tie rule deciding at least one case (the mutation switches), the
invariants of the outputs, and the plumbing: assign.assign_options, the flags, drivers.assign_policy, the checkpoint record and
its resume check, and ops.build_labels' routing on a stub library."""
import argparse
import importlib.util
import json
import os
import types

import numpy as np
import pytest

from squeezedet_amd import assign, drivers
from squeezedet_amd._lib import SqdetError
from tests import assign_cases as AC
from tests import assign_reference as R
from tests import input_path_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _total(ref, field):
    return sum(getattr(s, field) for s in ref.stats)


# ---------------------------------------------------------------- hand-worked
# Two cells at x = 32 and 64 (y = 32), shapes (48,32), (96,64), (32,96): anchors 0..2 and 3..5.  The box (48, 32, 64, 64) spans
# x 16..80, y 0..64; by symmetry anchor a and a + 3 have the same IoU:
#   shape (48,32): 40 * 32 / (1536 + 4096 - 1280) = 5/17;  (96,64): 4096 / 6144 = 2/3;  (32,96): 2048 / 5120 = 2/5
# Stage 1 claims anchor 4 (2/3, the higher index of the tie).
TWO_CELLS = IC.grid(2, 1)
BOX = np.array([[48.0, 32.0, 64.0, 64.0]])


def test_hand_worked_ious():
    from oracle import sqdet_oracle as O
    iou = O.batch_iou(TWO_CELLS, BOX[0])
    assert iou.tolist() == [5 / 17, 2 / 3, 2 / 5, 5 / 17, 2 / 3, 2 / 5]


def test_hand_worked_iou_mode():
    # the order: 4, 1 (2/3), 5, 2 (2/5), 3, 0 (5/17).  K = 3 keeps 4, 1, 5 -- the cap cuts the tie of 5 and 2 by index -- and
    # 4 is the claim: anchors 1 and 5 join it
    a, p, st = R.assign_image(TWO_CELLS, BOX, [4], "iou", 3, iou_thresh=0.35, max_per_box=3)
    assert a.tolist() == [-1, 0, -1, -1, 0, 0] and p.tolist() == [3] and st.cap_cuts == 1 and st.cap_tie_cuts == 1
    # ties to the LOWER index instead: 1, 4, 2
    a, _, _ = R.assign_image(TWO_CELLS, BOX, [4], "iou", 3, iou_thresh=0.35, max_per_box=3, iou_tie_high=False)
    assert a.tolist() == [-1, 0, 0, -1, 0, -1]
    # the threshold ON 2/5: >= keeps anchor 5, > drops it
    a, _, st = R.assign_image(TWO_CELLS, BOX, [4], "iou", 3, iou_thresh=2 / 5, max_per_box=3)
    assert a.tolist() == [-1, 0, -1, -1, 0, 0] and st.boundary_hits == 1
    a, _, _ = R.assign_image(TWO_CELLS, BOX, [4], "iou", 3, iou_thresh=2 / 5, max_per_box=3, thresh_inclusive=False)
    assert a.tolist() == [-1, 0, -1, -1, 0, -1]
    # K = 1: the one place is the claimed anchor's -- nothing is added
    a, p, _ = R.assign_image(TWO_CELLS, BOX, [4], "iou", 3, iou_thresh=0.0, max_per_box=1)
    assert a.tolist() == [-1, -1, -1, -1, 0, -1] and p.tolist() == [1]


def test_hand_worked_atss():
    # topk = 1: both cells are 256 away, the lower index wins: candidates 0, 1, 2.  mean = (5/17 + 2/3 + 2/5) / 3 = 0.453595,
    # var = (0.159477^2 + 0.213072^2 + 0.053595^2) / 3 = 0.024568 (std 0.156743): only anchor 1 (e = 0.213072) passes, and its
    # centre x = 32 lies inside 16..80
    E, iou, st = R.atss_eligible(TWO_CELLS, BOX[0], 3, 1)
    assert E.tolist() == [False, True, False, False, False, False] and st["dist_tie_cuts"] == 3
    a, p, _ = R.assign_image(TWO_CELLS, BOX, [4], "atss", 3, topk=1)
    assert a.tolist() == [-1, 0, -1, -1, 0, -1] and p.tolist() == [2]
    # distance ties to the HIGHER index: candidates 3, 4, 5 -- the only one that passes is the claim
    a, p, _ = R.assign_image(TWO_CELLS, BOX, [4], "atss", 3, topk=1, dist_tie_low=False)
    assert a.tolist() == [-1, -1, -1, -1, 0, -1] and p.tolist() == [1]
    # topk = 2: all six are candidates, the same mean and variance: anchors 1 and 4 pass
    E, _, st = R.atss_eligible(TWO_CELLS, BOX[0], 3, 2)
    assert E.tolist() == [False, True, False, False, True, False] and st["all_candidates"] == 1
    # the sample variance 0.036852 (std 0.191969) still admits e = 0.213072; a box whose left edge is ON x = 32 does not admit
    # anchor 1 under the strict rule
    g = np.array([64.0, 32.0, 64.0, 64.0])             # spans 32..96: the cell at 32 is on the edge, the cell at 64 inside
    E, _, st = R.atss_eligible(TWO_CELLS, g, 3, 2)
    Ec, _, _ = R.atss_eligible(TWO_CELLS, g, 3, 2, strict_inside=False)
    assert st["edge_hits"] == int(Ec.sum() - E.sum()) and not E[:3].any()


def test_hand_worked_conflict():
    # two identical boxes: box 0 claims anchor 4, box 1 anchor 1; anchors 5 and 2 (2/5) are eligible for both at the same IoU and go
    # to box 0, the lower
    both = np.concatenate([BOX, BOX])
    a, p, st = R.assign_image(TWO_CELLS, both, [4, 1], "iou", 3, iou_thresh=0.35, max_per_box=4)
    assert a.tolist() == [-1, 1, 0, -1, 0, 0] and p.tolist() == [3, 1] and st.conflicts == 2 and st.conflict_ties == 2
    a, p, _ = R.assign_image(TWO_CELLS, both, [4, 1], "iou", 3, iou_thresh=0.35, max_per_box=4, conflict_low_box=False)
    assert a.tolist() == [-1, 1, 1, -1, 0, 1] and p.tolist() == [1, 3]


# ---------------------------------------------------------------- the reference's pick stays
@pytest.mark.parametrize("name", ["classes1", "classes20", "three", "one"])
def test_mode_reference_is_label_reference(name):
    """On the cases that ARE input_path_cases' own, stage 1 alone reproduces label_reference tensor for tensor."""
    ref, want = AC.reference(name, "reference"), IC.label_reference(name)
    for got, exp in zip(ref[:5], want):
        assert np.array_equal(got, exp, equal_nan=True)


@pytest.mark.parametrize("mode", AC.MODES)
@pytest.mark.parametrize("name", AC.ASSIGN_CASES)
def test_the_reference_pick_is_a_subset_with_identical_rows(name, mode):
    base, ref = AC.reference(name, "reference"), AC.reference(name, mode)
    assert np.array_equal(ref.aidx, base.aidx)
    claimed = base.mask == 1
    assert (ref.mask[claimed] == 1).all() and np.array_equal(ref.assigned_box[claimed], base.assigned_box[claimed])
    for got, exp in ((ref.delta64, base.delta64), (ref.box, base.box), (ref.labels, base.labels)):
        assert np.array_equal(got[claimed], exp[claimed], equal_nan=True)
    c = AC.assign_case(name).label
    for b in range(len(c.cnt)):
        n = R.clipped_count(c, b)
        assert (ref.positives[b, :n] >= 1).all() and (ref.positives[b, n:] == 0).all()
        assert (base.positives[b, :n] == 1).all()


@pytest.mark.parametrize("mode", ("reference",) + AC.MODES)
@pytest.mark.parametrize("name", AC.ASSIGN_CASES)
def test_invariants(name, mode):
    ref = AC.reference(name, mode)
    B, M = ref.positives.shape
    assert np.array_equal(ref.assigned_box >= 0, ref.mask == 1)
    for b in range(B):
        hist = np.bincount(ref.assigned_box[b][ref.assigned_box[b] >= 0], minlength=M)
        assert np.array_equal(hist, ref.positives[b])
    assert int(ref.mask.sum()) == int(ref.positives.sum())
    case = AC.assign_case(name)
    if mode == "iou":
        assert ref.positives.max() <= case.max_per_box + 1


# ---------------------------------------------------------------- every case reaches its branch
def test_cases_reach_their_branches():
    iou, atss = (lambda n: AC.reference(n, "iou")), (lambda n: AC.reference(n, "atss"))
    assert _total(iou("identical"), "conflict_ties") >= 1 and _total(iou("identical"), "conflicts") >= 1
    assert _total(iou("boundary"), "boundary_hits") >= 2
    assert _total(iou("cap_tie"), "cap_tie_cuts") == 6            # every box: K = 3 on S2 cuts a pair
    c = AC.assign_case("k1")
    assert c.max_per_box == 1 and c.topk == 1 and _total(iou("k1"), "cap_tie_cuts") >= 1 and _total(atss("k1"), "dist_tie_cuts") >= 1
    assert iou("k1").positives.max() <= 2
    c = AC.assign_case("all_candidates")
    assert c.topk >= len(c.label.anchors) // c.apg and _total(atss("all_candidates"), "all_candidates") == 5 and c.max_per_box == 64
    for mode in AC.MODES:                                         # far: the claimed anchor and nothing else
        f = AC.reference("far", mode)
        assert f.positives.sum() == 6 and np.array_equal(f.mask, AC.reference("far", "reference").mask)
    assert IC.label_stats("far")[0].dist_mode == 40               # (input_path_cases' far: the same construction, 40 boxes)
    z = AC.assign_case("zero_width").label
    assert (z.gt[0, :3, 2] == 0).any() and np.isinf(atss("zero_width").delta64).any()
    assert _total(atss("edge"), "edge_hits") >= 1
    assert _total(atss("variance"), "dist_tie_cuts") >= 1
    e = AC.assign_case("empty").label
    assert e.cnt.tolist() == [0, 5] and not iou("empty").mask[0].any() and (iou("empty").assigned_box[0] == -1).all()
    c = AC.assign_case("counts").label
    assert c.cnt[0] > c.gt.shape[1] and c.cnt[1] < 0 and not atss("counts").mask[1].any() and atss("counts").positives[0].min() >= 1
    for name, C in (("classes1", 1), ("classes20", 20)):
        c = AC.assign_case(name).label
        assert c.C == C and (c.cls < 0).any() and (c.cls >= C).any()
        r = iou(name)
        assert ((r.mask == 1) & (r.labels.sum(-1) == 0)).any()     # a positive row without a label
    assert AC.assign_case("apg1").apg == 1 and AC.assign_case("one").apg == 1 and len(AC.assign_case("three").label.anchors) == 3
    k = AC.assign_case("kitti")
    assert len(k.label.anchors) == 16848 and k.apg == 9 and k.label.cnt.tolist() == [21, 18]
    assert _total(iou("kitti"), "cap_cuts") >= 1 and atss("kitti").positives.sum() > 5 * 39
    from oracle import sqdet_oracle as O
    o = AC.assign_case("over_cap")
    assert len(o.label.anchors) // o.apg > AC.STAGE_CAP and (O.batch_iou(o.label.anchors, o.label.gt[0, 0]) > 0).sum() > AC.STAGE_CAP
    assert 0 < (O.batch_iou(o.label.anchors, o.label.gt[0, 1]) > 0).sum() <= AC.STAGE_CAP        # (and a box that is staged beside it)
    assert iou("over_cap").positives[0, 0] == 16 and atss("over_cap").positives.sum() > 3      # (the claim heads the order: 15 more)


# ---------------------------------------------------------------- every tie rule decides a case
@pytest.mark.parametrize("switch, name, mode", [
    ("iou_tie_high", "cap_tie", "iou"), ("iou_tie_high", "k1", "iou"), ("dist_tie_low", "k1", "atss"), ("dist_tie_low", "cap_tie", "atss"),
    ("conflict_low_box", "identical", "iou"), ("strict_inside", "edge", "atss"), ("population_var", "variance", "atss"),
    ("thresh_inclusive", "boundary", "iou")])
def test_each_mutation_changes_a_case(switch, name, mode):
    good, bad = AC.reference(name, mode), AC.reference(name, mode, **{switch: False})
    assert not np.array_equal(good.assigned_box, bad.assigned_box), "%s does not decide %s / %s" % (switch, name, mode)


def test_the_switch_list_is_complete():
    import inspect
    params = inspect.signature(R.assign_image).parameters
    assert all(params[s].default is True for s in R.SWITCHES)
    assert [p for p, v in params.items() if v.default is True] == list(R.SWITCHES)


# ---------------------------------------------------------------- the record
def test_assign_options_defaults_and_is_default():
    assert assign.ASSIGN_MODES == ("reference", "iou", "atss")
    opt = assign.assign_options()
    assert opt == assign.AssignOptions("reference", 0.5, 16, 9) and assign.is_default(opt) and assign.is_default(None)
    assert assign.is_default(assign.assign_options("reference", 0.1, 2, 3))
    assert not assign.is_default(assign.assign_options("iou")) and not assign.is_default(assign.assign_options("atss"))
    assert assign.as_dict(assign.assign_options("iou", 0.4, 8)) == dict(mode="iou", iou_thresh=0.4, max_per_box=8)
    assert assign.as_dict(assign.assign_options("atss", topk=5)) == dict(mode="atss", topk=5) and assign.as_dict(None) == dict(mode="reference")
    for o in (assign.assign_options("iou", 0.4, 8), assign.assign_options("atss", topk=5), assign.assign_options()):
        assert assign.as_dict(assign.from_dict(json.loads(json.dumps(assign.as_dict(o))))) == assign.as_dict(o)


@pytest.mark.parametrize("kw", [dict(mode="topk"), dict(mode="iou", iou_thresh=-0.1), dict(mode="iou", iou_thresh=float("nan")),
                                dict(mode="iou", iou_thresh=float("inf")), dict(mode="iou", max_per_box=0), dict(mode="iou", max_per_box=65),
                                dict(mode="atss", topk=0), dict(mode="atss", topk=33), dict(mode="atss", topk=2.5)])
def test_assign_options_refusals(kw):
    with pytest.raises(SqdetError):
        assign.assign_options(**kw)


def test_positives_summary():
    pos = np.array([[1, 4, 7, 99], [2, 99, 99, 99], [99, 99, 99, 99]])
    assert assign.positives_summary(pos, np.array([3, 1, 0])) == (1, 3.5, 7)
    assert assign.positives_summary(pos, np.array([9, -2, 0])) == (1, (1 + 4 + 7 + 99) / 4, 99)
    assert assign.positives_summary(pos, np.array([0, 0, -1])) == (0, 0.0, 0)
    ref = AC.reference("kitti", "atss")
    lo, mean, hi = assign.positives_summary(ref.positives, AC.assign_case("kitti").label.cnt)
    assert lo >= 1 and mean == ref.positives.sum() / 39 and hi == ref.positives.max()


# ---------------------------------------------------------------- flags
def _parser():
    ap = argparse.ArgumentParser()
    drivers.add_assign_flags(ap)
    return ap


def test_flags_leave_nothing_behind_when_not_given():
    ap = _parser()
    assert vars(ap.parse_args([])) == {}
    a = ap.parse_args(["--assign", "iou", "--assign_iou", "0.4", "--assign_max", "8"])
    assert vars(a) == dict(assign="iou", assign_iou=0.4, assign_max=8)
    drivers.check_assign_args(ap, a)
    a = ap.parse_args(["--assign", "atss", "--assign_topk", "5"])
    drivers.check_assign_args(ap, a)
    assert vars(a) == dict(assign="atss", assign_topk=5)


def test_assign_policy():
    ap = _parser()
    policy, off = drivers.assign_policy(ap.parse_args([]))
    assert policy == off == dict(mode="reference") and assign.is_default(assign.from_dict(policy))
    policy, _ = drivers.assign_policy(ap.parse_args(["--assign", "iou", "--assign_max", "4"]))
    assert policy == dict(mode="iou", iou_thresh=0.5, max_per_box=4) and assign.from_dict(policy) == assign.AssignOptions("iou", 0.5, 4, 9)
    policy, _ = drivers.assign_policy(ap.parse_args(["--assign", "atss"]))
    assert policy == dict(mode="atss", topk=9)


@pytest.mark.parametrize("argv, text", [
    (["--assign", "best"], "invalid choice"), (["--assign_topk", "5"], "needs --assign atss"), (["--assign", "atss", "--assign_iou", "0.4"], "needs --assign iou"),
    (["--assign", "atss", "--assign_max", "4"], "needs --assign iou"), (["--assign", "iou", "--assign_iou", "-1"], "finite number >= 0"),
    (["--assign", "iou", "--assign_max", "65"], "1..64"), (["--assign", "atss", "--assign_topk", "33"], "1..32"), (["--assign", "atss", "--assign_topk", "0"], "1..32")])
def test_flag_refusals(argv, text, capsys):
    ap = _parser()
    with pytest.raises(SystemExit):
        drivers.check_assign_args(ap, ap.parse_args(argv))
    assert text in capsys.readouterr().err


def _script(path):
    spec = importlib.util.spec_from_file_location("assign_flags_" + os.path.basename(path)[:-3], os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_flags_and_the_checkpoint_record(tmp_path):
    """train.py parses the flags; the record round-trips through a checkpoint's JSON; --resume under another policy is refused, and
    a checkpoint without the key counts as `reference`."""
    T = _script("train.py")
    a = T.parse_args(["--train_dir", str(tmp_path), "--assign", "atss", "--assign_topk", "7"])
    policy, off = drivers.assign_policy(a)
    assert policy == dict(mode="atss", topk=7)
    with pytest.raises(SystemExit):
        T.parse_args(["--train_dir", str(tmp_path), "--assign_iou", "0.3"])
    loss_off = dict(bbox_loss="delta_l2", focal_gamma=0.0, bbox_loss_coef=5.0)
    saved = json.loads(json.dumps(dict(loss=loss_off, assign=policy)))
    T.check_resume_record(saved, dict(loss=loss_off, assign=policy), loss_off)
    with pytest.raises(SystemExit, match="assign"):
        T.check_resume_record(saved, dict(loss=loss_off, assign=dict(mode="iou", iou_thresh=0.5, max_per_box=16)), loss_off)
    with pytest.raises(SystemExit, match="assign"):
        T.check_resume_record(saved, dict(loss=loss_off, assign=off), loss_off)
    old = dict(loss=loss_off)                                     # a checkpoint from before the key existed
    T.check_resume_record(old, dict(loss=loss_off, assign=off), loss_off)
    with pytest.raises(SystemExit, match="assign"):
        T.check_resume_record(old, dict(loss=loss_off, assign=policy), loss_off)


def test_bench_train_takes_the_flags(monkeypatch):
    B = _script("tools/bench_train.py")
    monkeypatch.setattr("sys.argv", ["bench_train.py", "--assign", "iou", "--assign_iou", "0.4"])
    a = B.parse_args()
    assert drivers.assign_policy(a)[0] == dict(mode="iou", iou_thresh=0.4, max_per_box=16)


# ---------------------------------------------------------------- routing
class _StubLib:
    """A library object that knows sqdet_build_labels alone: touching any other symbol fails the test."""

    def __init__(self):
        self.calls = []

    def sqdet_build_labels(self, *args):
        self.calls.append(len(args))
        return 0

    def __getattr__(self, name):
        raise AssertionError("the default route touched %s" % name)


def test_default_route_does_not_touch_the_new_symbol(monkeypatch):
    import torch
    from squeezedet_amd import ops
    stub = _StubLib()
    monkeypatch.setattr(ops, "lib", lambda: stub)
    monkeypatch.setattr(ops, "_dev", lambda t, *a: None)
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    c = AC.assign_case("classes1").label
    for opt in (None, assign.assign_options(), assign.assign_options("reference", 0.2, 3, 4)):
        out = ops.build_labels(c.anchors.copy(), c.gt.copy(), c.cls.copy(), c.cnt.copy(), c.C, device="cpu", assign=opt, anchors_per_grid=3)
        assert len(out) == 5 and out[4].dtype == torch.int32
    assert stub.calls == [14, 14, 14]
    with pytest.raises(AssertionError, match="sqdet_build_labels_opt"):
        ops.build_labels(c.anchors.copy(), c.gt.copy(), c.cls.copy(), c.cnt.copy(), c.C, device="cpu", assign=assign.assign_options("atss"),
                         anchors_per_grid=3)
    with pytest.raises(SqdetError, match="anchors_per_grid"):
        ops.build_labels(c.anchors.copy(), c.gt.copy(), c.cls.copy(), c.cnt.copy(), c.C, device="cpu", assign=assign.assign_options("iou"))
