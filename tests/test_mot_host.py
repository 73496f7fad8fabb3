"""The NumPy restatement of the tracking evaluation (tests/mot_reference.py; include/sqdet.h, "tracking evaluation") against
hand-worked numbers, its assign() against brute force and scipy, its mutations against the cases that must catch them, and the
file readers of squeezedet_amd.mot.  No GPU."""
import itertools

import numpy as np
import pytest

from tests import mot_cases as MC
from tests import mot_reference as R


def run_case(name, mutate=None):
    classes, frames, _, _ = MC.CASES[name]
    hyp, gt = MC.pack(frames, 4, 4)
    st = R.State(1, classes)
    R.run(st, *hyp, gt, len(frames), 0.5, mutate)
    table, iou_sum = R.evaluate(st)
    return st, table[0], iou_sum[0]


def mismatches(name, mutate=None):
    """[(what, got, want)] of a case's expectations that do not hold."""
    _, _, overall, per_class = MC.CASES[name]
    _, table, iou_sum = run_case(name, mutate)
    bad = []
    m = R.metrics(table.sum(0), iou_sum.sum())
    for k, want in overall.items():
        got = iou_sum.sum() if k == "iou_sum" else m[k]
        if (abs(got - want) > 1e-12) if k == "iou_sum" else (got != want):
            bad.append((k, got, want))
    for c, exp in per_class.items():
        mc = R.metrics(table[c], iou_sum[c])
        bad += [("class %d %s" % (c, k), mc[k], want) for k, want in exp.items() if mc[k] != want]
    return bad


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_hand_worked_case(name):
    assert mismatches(name) == []


def test_derived_metrics():
    _, table, iou_sum = run_case("one_switch")
    m = R.metrics(table.sum(0), iou_sum.sum())
    assert m["mota"] == 1.0 - 1 / 5 and m["motp"] == 1.0 and m["idf1"] == 6 / 10 and m["precision"] == 1.0 and m["recall"] == 1.0
    _, table, iou_sum = run_case("id_change_halfway")
    assert R.metrics(table.sum(0), iou_sum.sum())["idf1"] == 12 / 20
    _, table, iou_sum = run_case("fragmentation")
    m = R.metrics(table.sum(0), iou_sum.sum())
    assert m["mota"] == 1.0 - 2 / 6 and m["recall"] == 4 / 6 and m["idf1"] == 8 / 10
    assert np.isnan(R.metrics(np.zeros(R.K, np.int64), 0.0)["mota"])


def test_greedy_finds_one_match_where_the_optimum_finds_two():
    _, table, _ = run_case("greedy_vs_optimal", "greedy")
    assert (table[0, 0], table[0, 1], table[0, 2]) == (1, 1, 1)
    _, table, _ = run_case("greedy_vs_optimal")
    assert (table[0, 0], table[0, 1], table[0, 2]) == (2, 0, 0)


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutation_fails_its_case(mutate):
    assert set(MC.MUTATION_CASE) == set(R.MUTATIONS)
    assert mismatches(MC.MUTATION_CASE[mutate], mutate) != [], "%s passes %s" % (mutate, MC.MUTATION_CASE[mutate])


# ------------------------------------------------------------------------------------------------ assign --
def _total(cost, p):
    rows = [int(i) for i in p if i >= 0]
    assert sorted(rows) == list(range(cost.shape[0])), "not every row has one column"
    return sum(int(cost[i, j]) for j, i in enumerate(p) if i >= 0)


def _random_cost(rs, R_, C_, big):
    cost = rs.randint(0, 1 << 20, size=(R_, C_)).astype(np.int64)
    if rs.rand() < 0.5:
        cost = rs.randint(0, 4, size=(R_, C_)).astype(np.int64)          # many ties
    if big:
        cost[rs.rand(R_, C_) < 0.4] = R.BIG
    return cost


def test_assign_is_optimal_by_brute_force():
    rs = np.random.RandomState(0)
    for trial in range(120):
        R_ = int(rs.randint(1, 7))
        C_ = int(rs.randint(R_, 7))
        cost = _random_cost(rs, R_, C_, trial % 2 == 1)
        best = min(sum(int(cost[i, j]) for i, j in enumerate(cols)) for cols in itertools.permutations(range(C_), R_))
        assert _total(cost, R.assign(cost)) == best, cost


def test_assign_matches_scipy_total_cost():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rs = np.random.RandomState(1)
    for trial in range(60):
        R_ = int(rs.randint(1, 13))
        C_ = R_ if trial % 3 == 0 else int(rs.randint(R_, 41))
        cost = _random_cost(rs, R_, C_, trial % 2 == 1)
        ri, ci = lsa(cost)
        assert _total(cost, R.assign(cost)) == int(cost[ri, ci].sum()), (R_, C_)
        neg = -rs.randint(0, 50, size=(R_, C_)).astype(np.int64)          # the IDF1 form: cost -overlap
        ri, ci = lsa(neg)
        assert _total(neg, R.assign(neg)) == int(neg[ri, ci].sum())


def test_assign_ties_go_to_the_lowest_column():
    assert R.assign(np.zeros((2, 4), np.int64)).tolist() == [0, 1, -1, -1]
    assert R.assign(np.asarray([[5, 5, 5]], np.int64)).tolist() == [0, -1, -1]
    # row 1 wants column 0 as well: row 0 is moved along the cheapest path
    assert R.assign(np.asarray([[1, 2, 9], [1, 9, 9]], np.int64)).tolist() == [1, 0, -1]


# ------------------------------------------------------------------------------------------------ end to end --
@pytest.mark.parametrize("seed", range(5))
def test_tracked_scene_has_no_switch_and_no_false_positive(seed):
    frames, labelled = MC.scene_frames(seed)
    hyp, gt = MC.pack(frames, 8, 8)
    st = R.State(1, 3)
    R.run(st, *hyp, gt, len(frames))
    table, iou_sum = R.evaluate(st)
    m = R.metrics(table[0].sum(0), iou_sum[0].sum())
    assert m["idsw"] == 0 and m["fp"] == 0
    assert m["tp"] + m["fn"] == labelled
    assert m["gt_ids"] == 4 and m["hyp_ids"] == 4 and m["tp"] > 0.8 * labelled and m["motp"] == 1.0 and m["idfp"] == 0


def test_identity_table_limit_stops_the_stream():
    """256 object identities are accepted; the 257th sets the status word and neither that frame nor a later one changes a thing."""
    frames = [([(64 * f + k + 1, 0, 0, MC.B(100.0 * k)) for k in range(64)], []) for f in range(4)]
    frames += [([(9000, 0, 0, MC.B(0.0))], []), ([(1, 0, 0, MC.B(0.0))], [])]
    hyp, gt = MC.pack(frames, 1, 64)
    st = R.State(1, 1)
    R.run(st, *[a[:4] for a in hyp], [a[:4] for a in gt], 4)
    assert st.status[0] == 0 and len(st.obj[0]) == 256
    before = st.arrays()
    R.run(st, *[a[4:] for a in hyp], [a[4:] for a in gt], 2)
    after = st.arrays()
    assert st.status[0] == R.STATUS_OBJ
    assert all(np.array_equal(before[k], after[k]) for k in before if k != "status")
    with pytest.raises(ValueError):
        R.evaluate(st)


# ------------------------------------------------------------------------------------------------ files --
def test_readers_and_summary(tmp_path):
    from squeezedet_amd import mot
    gt = tmp_path / "gt.txt"
    gt.write_text("1,1,80,90,40,20,1,1,1.0\n1,2,300,90,40,20,0,1,1.0\n2,1,80,90,40,20,1,1,1.0\n2,3,500,90,40,20,1,8,1.0\n")
    g = mot.MotGroundTruth.from_mot_text(str(gt))
    assert g.n_frames == 2 and g.frames[1][0] == (1, 0, 0, (100.0, 100.0, 40.0, 20.0))
    assert g.frames[1][1][2] == mot.IGNORE and g.frames[2][1][2] == mot.IGNORE            # conf 0; a distractor class
    box, ident, klass, flags, count = g.arrays()
    assert box.dtype == np.float64 and box.shape == (2, 2, 4) and count.tolist() == [2, 2] and ident[1].tolist() == [1, 3]
    res = tmp_path / "res.txt"
    res.write_text("1,5,80.00,90.00,40.00,20.00,0.9000,-1,-1,-1\n2,5,80.00,90.00,40.00,20.00,0.9000,-1,-1,-1\n2,6,1.00,2.00,3.00,4.00,0.5,-1,-1,-1\n")
    boxes, cls, counts, ids, states = mot.load_mot_results(str(res))
    assert boxes.dtype == np.float32 and boxes.shape == (2, 2, 4) and counts.tolist() == [1, 2]
    assert boxes[0, 0].tolist() == [100.0, 100.0, 40.0, 20.0] and ids[1].tolist() == [5, 6] and states[0].tolist() == [2, 0]
    kitti = tmp_path / "0000.txt"
    kitti.write_text("0 0 Car 0 0 -1.5 80 90 120 110 1 1 1 1 1 1 1\n0 -1 DontCare -1 -1 -10 300 90 340 110 -1 -1 -1 -1 -1 -1 -1\n"
                     "1 1 Cyclist 0 0 -1.5 10 20 30 60 1 1 1 1 1 1 1\n")
    k = mot.MotGroundTruth.from_kitti_tracking(str(kitti), ["car", "pedestrian", "cyclist"])
    assert k.frames[1][0] == (1, 0, 0, (100.0, 100.0, 40.0, 20.0)) and k.frames[2] == [(2, 2, 0, (20.0, 40.0, 20.0, 40.0))]
    assert [(r[1], r[2]) for r in k.frames[1][1:]] == [(0, 1), (1, 1), (2, 1)] and len({r[0] for r in k.frames[1]}) == 4
    back = mot.MotGroundTruth.from_arrays(*g.arrays())
    assert back.frames == g.frames
    # the restatement's table through the package's summary
    st, table, iou_sum = run_case("one_switch")
    text = mot.format_summary(mot.summarize(table[None], iou_sum[None]), ["car"])
    assert "OVERALL" in text and "car" in text and " 0.8000" in text and " 0.6000" in text
    assert mot.metrics(table[0], iou_sum[0])["idf1"] == R.metrics(table[0], iou_sum[0])["idf1"]
