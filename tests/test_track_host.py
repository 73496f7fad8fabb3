"""The tracker's definition (include/sqdet.h, "tracking") as tests/track_reference.py restates it, without a GPU: hand-worked
cases with their expected numbers, the 60-frame scene, and mutation checks -- a restatement with one rule changed must fail at
least one of them, so the cases do pin the rules down."""
import numpy as np
import pytest

from tests import track_cases as TC
from tests import track_reference as R


def run_case(name, mutate=None, rows=4):
    """-> (tables, [(ids, states)] per frame), one step per frame."""
    kw, frames, _ = TC.CASES[name]
    p = R.params(**kw)
    T = R.Tables(1)
    boxes, probs, cls, counts = TC.pack(frames, rows)
    out = []
    for f in range(len(frames)):
        ids, sts = R.step(T, 0, boxes[f], probs[f], cls[f], counts[f], p, mutate)
        out.append((ids, sts))
    return T, out


def check_case(name, mutate=None):
    kw, frames, expect = TC.CASES[name]
    T, out = run_case(name, mutate)
    for f, ((ids, sts), (eid, est)) in enumerate(zip(out, expect)):
        n = len(frames[f])
        assert ids[:n].tolist() == eid and sts[:n].tolist() == est, "%s frame %d: %s %s" % (name, f, ids[:n], sts[:n])
        assert (ids[n:] == -1).all() and (sts[n:] == 0).all(), "%s frame %d: a row past count got an id" % (name, f)
    EXTRA[name](T)


def _one(T):
    tr = T.tracks(0)
    assert len(tr) == 1
    return tr[0]


def _birth_confirm(T):
    t = _one(T)
    assert (t["slot"], t["id"], t["state"], t["hits"], t["miss"], t["age"]) == (0, 1, 2, 3, 0, 3)
    assert T.next_id[0] == 2 and T.dropped[0] == 0 and t["score"] == float(np.float32(0.9))
    assert t["box"] == TC.BOX and t["velocity"] == (0.0, 0.0, 0.0, 0.0)          # the row never moved: y = 0 every time


def _tentative_dies(T):
    t = _one(T)
    assert (t["slot"], t["id"], t["state"], t["hits"]) == (0, 2, 1, 1) and T.next_id[0] == 3


def _max_age(T):
    t = _one(T)
    assert (t["slot"], t["id"], t["state"], t["hits"], t["age"]) == (0, 2, 1, 1, 1) and T.next_id[0] == 3


def _class_gate(T):
    t = _one(T)
    assert (t["slot"], t["id"], t["cls"], t["state"]) == (0, 2, 1, 1)            # born into the slot the dead track left


def _iou_equal(T):
    t = _one(T)
    assert (t["id"], t["hits"], t["state"]) == (1, 2, 1) and T.next_id[0] == 2


def _tie(T):
    tr = T.tracks(0)
    assert [(t["slot"], t["id"], t["hits"]) for t in tr] == [(0, 1, 2), (1, 2, 2), (2, 3, 1)] and T.next_id[0] == 4


def _stage_two(T):
    t = _one(T)
    assert (t["id"], t["state"], t["hits"], t["miss"]) == (1, 2, 4, 0) and t["score"] == float(np.float32(0.3))


def _stage_two_poor_overlap(T):
    t = _one(T)
    assert (t["id"], t["state"], t["hits"], t["miss"]) == (1, 2, 3, 1) and T.next_id[0] == 2
    assert R.iou((100.0, 100.0, 40.0, 20.0), (124.0, 100.0, 40.0, 20.0)) == 0.25


def _low_no_birth(T):
    assert T.tracks(0) == [] and T.next_id[0] == 2 and T.dropped[0] == 0


def height_filter(zs, w_pos=1.0 / 20, w_vel=1.0 / 160):
    """The height coordinate of a track that is matched in every frame, written out on its own: zs its measurements
    -> (p, v, pp, pv, vv)."""
    h = max(zs[0], 1.0)
    p, v, pp, pv, vv = zs[0], 0.0, (2.0 * w_pos * h) * (2.0 * w_pos * h), 0.0, (10.0 * w_vel * h) * (10.0 * w_vel * h)
    for z in zs[1:]:
        h = max(p, 1.0)                                             # the height before the predict: the process noise
        qp, qv = (w_pos * h) * (w_pos * h), (w_vel * h) * (w_vel * h)
        p, pp, pv, vv = p + v, ((pp + pv) + (pv + vv)) + qp, pv + vv, vv + qv
        h = max(p, 1.0)                                             # ... and after it: the measurement noise
        r = (w_pos * h) * (w_pos * h)
        y, s = z - p, pp + r
        kp, kv = pp / s, pv / s
        p, v, pp, pv, vv = p + kp * y, v + kv * y, pp - kp * pp, pv - kp * pv, vv - kv * pv
    return p, v, pp, pv, vv


def _growing(T):
    """The height coordinate against height_filter above, and its first steps against numbers worked by hand."""
    t = _one(T)
    zs = [20.0, 24.0, 28.0, 32.0]
    # by hand: birth pp = (2*20/20)^2 = 4, vv = (10*20/160)^2 = 1.5625; predict: pp = 4 + 1.5625 + 1 = 6.5625, pv = 1.5625,
    # vv = 1.5625 + (20/160)^2 = 1.578125; update with r = 1, y = 4: s = 7.5625, p = 20 + 6.5625/7.5625*4, v = 1.5625/7.5625*4
    p1, v1 = 20.0 + (6.5625 / 7.5625) * 4.0, (1.5625 / 7.5625) * 4.0
    assert height_filter(zs[:2])[:2] == (p1, v1)
    assert abs(p1 - 23.47107438016529) < 1e-12 and abs(v1 - 0.8264462809917356) < 1e-12
    p, v, pp, pv, vv = height_filter(zs)
    assert (float(T.x[0, 0, 3, 0]), float(T.x[0, 0, 3, 1])) == (p, v)
    assert tuple(float(q) for q in T.P[0, 0, 3]) == (pp, pv, vv)
    assert t["hits"] == 4 and 28.0 < p < 32.0 and 0.0 < v < 4.0                 # a filter lags a ramp of 4 per frame


EXTRA = {"birth_confirm": _birth_confirm, "tentative_dies": _tentative_dies, "max_age": _max_age, "class_gate": _class_gate,
         "iou_equal": _iou_equal, "tie": _tie, "stage_two": _stage_two, "stage_two_poor_overlap": _stage_two_poor_overlap, "low_no_birth": _low_no_birth, "growing": _growing}


@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_hand_worked_case(name):
    check_case(name)


def test_first_steps_by_hand():
    """Birth and the first predict of BOX (h = 20), exact in binary."""
    kw, frames, _ = TC.CASES["birth_confirm"]
    T = R.Tables(1)
    boxes, probs, cls, counts = TC.pack(frames, 2)
    R.step(T, 0, boxes[0], probs[0], cls[0], counts[0], R.params())
    assert T.x[0, 0].tolist() == [[100.0, 0.0], [100.0, 0.0], [40.0, 0.0], [20.0, 0.0]]
    assert T.P[0, 0].tolist() == [[4.0, 0.0, 1.5625]] * 4
    T2 = R.Tables(1)
    p = R.params(min_hits=1)
    R.step(T2, 0, boxes[0], probs[0], cls[0], counts[0], p)
    assert T2.state[0, 0] == 2                                                          # min_hits <= 1: born confirmed
    R.step(T2, 0, boxes[1], probs[1], cls[1], 0, p)
    assert T2.P[0, 0].tolist() == [[6.5625, 1.5625, 1.578125]] * 4 and (T2.miss[0, 0], T2.age[0, 0], T2.state[0, 0]) == (1, 2, 2)


def test_max_age_boundary():
    """After exactly max_age misses the confirmed track is live; one more frees it."""
    kw, frames, _ = TC.CASES["max_age"]
    p = R.params(**kw)
    T = R.Tables(1)
    boxes, probs, cls, counts = TC.pack(frames, 2)
    for f in range(6):
        R.step(T, 0, boxes[f], probs[f], cls[f], counts[f], p)
    assert [(t["id"], t["miss"]) for t in T.tracks(0)] == [(1, 3)]
    R.step(T, 0, boxes[5], probs[5], cls[5], 0, p)
    assert T.tracks(0) == []


def test_invalid_rows_and_counts():
    """NaN / inf / zero / negative sizes take part in nothing; count is clamped to [0, rows]."""
    rows = [(100.0, 100.0, 40.0, 20.0, 0.9, 0), (np.nan, 100.0, 40.0, 20.0, 0.9, 0), (300.0, np.inf, 40.0, 20.0, 0.9, 0),
            (500.0, 100.0, 0.0, 20.0, 0.9, 0), (600.0, 100.0, 40.0, -3.0, 0.9, 0), (700.0, 100.0, 40.0, 20.0, np.nan, 0)]
    boxes, probs, cls, _ = TC.pack([rows], 6)
    for count, born in ((6, 1), (99, 1), (0, 0), (-7, 0)):
        T = R.Tables(1)
        ids, sts = R.step(T, 0, boxes[0], probs[0], cls[0], count, R.params())
        assert ids.tolist() == ([1] if born else [-1]) + [-1] * 5 and len(T.tracks(0)) == born


def test_slots_fill_and_drop():
    """64 high rows fill every slot; 64 other rows are dropped (max_age 5) or replace them (max_age 0, min_hits 1)."""
    a = [(50.0 * (k % 8), 50.0 * (k // 8), 20.0, 20.0, 0.9, 0) for k in range(64)]
    b = [(r[0] + 10000.0,) + r[1:] for r in a]
    boxes, probs, cls, counts = TC.pack([a, b], 64)
    T = R.Tables(1)
    p = R.params(min_hits=1, max_age=5)
    ids, _ = R.step(T, 0, boxes[0], probs[0], cls[0], 64, p)
    assert ids.tolist() == list(range(1, 65)) and len(T.tracks(0)) == 64
    ids, _ = R.step(T, 0, boxes[1], probs[1], cls[1], 64, p)
    assert (ids == -1).all() and T.dropped[0] == 64 and T.next_id[0] == 65
    T = R.Tables(1)
    p = R.params(min_hits=1, max_age=0)
    R.step(T, 0, boxes[0], probs[0], cls[0], 64, p)
    ids, sts = R.step(T, 0, boxes[1], probs[1], cls[1], 64, p)
    assert ids.tolist() == list(range(65, 129)) and (sts == 2).all() and T.dropped[0] == 0


def scene_ids(seed, mutate=None):
    frames, labels = TC.scene(seed)
    boxes, probs, cls, counts = TC.pack(frames, 8)
    T = R.Tables(1)
    ids, _ = R.run(T, boxes, probs, cls, counts, len(frames), R.params(), mutate)
    return ids, labels, int(T.next_id[0])


@pytest.mark.parametrize("seed", range(5))
def test_scene(seed):
    ids, labels, next_id = scene_ids(seed)
    TC.check_scene(ids, labels, next_id)


def test_scene_frames_in_one_call_equal_single_steps():
    frames, _ = TC.scene(0)
    boxes, probs, cls, counts = TC.pack(frames, 8)
    A, B = R.Tables(1), R.Tables(1)
    ia, sa = R.run(A, boxes, probs, cls, counts, 60, R.params())
    for f in range(60):
        i, s = R.run(B, boxes[f:f + 1], probs[f:f + 1], cls[f:f + 1], counts[f:f + 1], 1, R.params())
        assert np.array_equal(i[0], ia[f]) and np.array_equal(s[0], sa[f])
    for k, v in A.arrays().items():
        assert np.array_equal(v, B.arrays()[k]), k


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutation_is_caught(mutate):
    failed = []
    for name in sorted(TC.CASES):
        try:
            check_case(name, mutate)
        except AssertionError:
            failed.append(name)
    for seed in range(5):
        try:
            TC.check_scene(*scene_ids(seed, mutate))
        except AssertionError:
            failed.append("scene %d" % seed)
    assert failed, "no case notices the mutation %r" % mutate


def test_argument_validation_before_any_launch():
    """rows = 65 is SQDET_EUNSUPPORTED, null pointers and bad parameters are invalid arguments -- decided on the host, so this
    runs without a device (the pointers are never dereferenced)."""
    import ctypes as C
    from squeezedet_amd import _lib, track
    from squeezedet_amd import build as sqbuild
    sqbuild.build(verbose=False)
    lib = _lib.lib()
    fake = C.c_void_p(0x1000)
    tables = track._Tables(*[0x1000] * len(track.FIELDS))

    def call(rows=8, tables=tables, boxes=fake, streams=1, frames=1, **kw):
        p = dict(track.PARAMS, **kw)
        params = track._Params(p["iou_thresh"], p["high_thresh"], p["low_thresh"], p["w_pos"], p["w_vel"], p["min_hits"], p["max_age"])
        return lib.sqdet_track_update(C.byref(tables), boxes, fake, fake, fake, streams, frames, rows, C.byref(params), fake, fake, 0, None)

    assert call(rows=65) == _lib.SQDET_EUNSUPPORTED and b"65 rows" in lib.sqdet_last_error()
    assert call(rows=0) == -1 and call(streams=0) == -1 and call(frames=0) == -1
    assert call(boxes=None) == -1 and b"null" in lib.sqdet_last_error()
    assert call(tables=track._Tables(*[0x1000] * 10 + [None])) == -1 and b"tables" in lib.sqdet_last_error()
    assert call(iou_thresh=0.0) == -1 and call(iou_thresh=float("nan")) == -1 and call(max_age=-1) == -1 and call(w_pos=float("inf")) == -1
    assert lib.sqdet_track_build_items(fake, fake, fake, fake, fake, fake, 1, 300, 0.5, fake, 3, fake, 12, 0, fake, fake, 300, None) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_track_build_items(fake, fake, fake, fake, fake, fake, 1, 8, 0.5, fake, 3, fake, 0, 0, fake, fake, 8, None) == -1
    assert lib.sqdet_track_build_items(fake, fake, fake, fake, fake, fake, 1, 8, 0.5, fake, 3, None, 12, 0, fake, fake, 8, None) == -1
