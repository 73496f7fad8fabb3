"""squeezedet_amd.mot on the GPU: every counter, iou_sum and every table of sqdet_mot_update / sqdet_mot_evaluate against the
sequential NumPy restatement (tests/mot_reference.py), BITWISE, at the smallest shapes at which the kernels can go wrong -- the
sizes of the wave-wide assignment, the identity tables at and one past their limits, the workgroup-wide IDF1 matching on loaded
tables -- then the device-only pipeline Tracker.update -> MotAccumulator.update in a captured graph, and tools/mot_eval.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from squeezedet_amd import _lib, mot, track
from tests import mot_cases as MC
from tests import mot_reference as R
from tests import track_cases as TC
from tests import track_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
CANARY = 0xA5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(got.view("u%d" % got.itemsize) != want.view("u%d" % want.itemsize))
        raise AssertionError("%s differs at %d places, first %s: %r vs %r" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def update(acc, hyp, gt, F=1, **kw):
    acc.update(*dev(*hyp), tuple(dev(*gt)), frames_per_stream=F, **kw)


def check(acc, st, what="", order=None):
    """Every table, then the evaluation: counters and iou_sum, bit for bit.  order: acc's stream k is st's stream order[k]."""
    ref = st.arrays()
    idx = list(range(st.S)) if order is None else list(order)
    for f, t in acc.tables().items():
        same_bits(t.cpu().numpy(), ref[f][idx], "%s table %s" % (what, f))
    table, iou_sum = R.evaluate(st)
    got_table, got_iou = acc.evaluate_raw()
    same_bits(got_table, table[idx], what + " counters")
    same_bits(got_iou, iou_sum[idx], what + " iou_sum")
    return got_table, got_iou


def sl(arrays, f0, f1):
    return [a[f0:f1] for a in arrays]


# ------------------------------------------------------------------------------------------------ cases and the scene --
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_hand_worked_case(name):
    classes, frames, overall, per_class = MC.CASES[name]
    hyp, gt = MC.pack(frames, 4, 4)
    acc, st = mot.MotAccumulator(1, DEV, classes), R.State(1, classes)
    R.run(st, *hyp, gt, len(frames))
    update(acc, hyp, gt, F=len(frames))
    table, iou_sum = check(acc, st, name)
    m = mot.metrics(table[0].sum(0), iou_sum[0].sum())
    for k, want in overall.items():
        assert (abs(m[k] - want) <= 1e-12) if k == "iou_sum" else (m[k] == want), (k, m[k], want)
    for c, exp in per_class.items():
        mc = mot.metrics(table[0, c], iou_sum[0, c])
        assert all(mc[k] == want for k, want in exp.items()), (c, mc)


@pytest.fixture(scope="module")
def scene0():
    """Scene 0 tracked by the tracker's restatement, packed, with the restatement's final state (read only)."""
    frames, labelled = MC.scene_frames(0)
    hyp, gt = MC.pack(frames, 8, 8)
    st = R.State(1, 3)
    R.run(st, *hyp, gt, 60)
    return hyp, gt, st, labelled


@pytest.mark.parametrize("chunk", [60, 7, 1])
def test_scene_in_one_call_in_chunks_and_frame_by_frame(scene0, chunk):
    hyp, gt, st, labelled = scene0
    acc = mot.MotAccumulator(1, DEV, 3)
    for f0 in range(0, 60, chunk):
        f1 = min(f0 + chunk, 60)
        update(acc, sl(hyp, f0, f1), sl(gt, f0, f1), F=f1 - f0)
    table, _ = check(acc, st)
    tot = table[0].sum(0)
    assert tot[3] == 0 and tot[2] == 0 and tot[0] + tot[1] == labelled


def test_state_dict_round_trip_and_reset(scene0):
    hyp, gt, st, _ = scene0
    a = mot.MotAccumulator(1, DEV, 3)
    update(a, sl(hyp, 0, 23), sl(gt, 0, 23), F=23)
    saved = a.state_dict()
    update(a, sl(hyp, 23, 30), sl(gt, 23, 30), F=7)               # a goes on; the copy must not follow
    b = mot.MotAccumulator(1, DEV, 3)
    b.load_state_dict(saved)
    update(b, sl(hyp, 23, 60), sl(gt, 23, 60), F=37)
    check(b, st, "after the reload")
    b.reset()
    for f, t in b.tables().items():
        assert not bool(t.any()), f
    with pytest.raises(_lib.SqdetError):
        mot.MotAccumulator(1, DEV, 3, iou_thresh=0.3).load_state_dict(saved)


# ------------------------------------------------------------------------------------------------ several streams --
def _streams(n_streams, n_frames, rows=20):
    rs = np.random.RandomState(11)
    return [MC.pack(MC.random_frames(rs, n_frames, 5 + 3 * s), rows, rows) for s in range(n_streams)]


def _interleave(per, order, f0, f1):
    """(hyp, gt) of frames [f0, f1) of the streams in `order`, image s*F + f."""
    return tuple([np.concatenate([per[s][part][k][f0:f1] for s in order]) for k in range(5)] for part in range(2))


@pytest.mark.parametrize("F", [1, 4])
def test_three_streams_and_their_permutation(F):
    per = _streams(3, 12)
    st = R.State(3, 3)
    for f0 in range(0, 12, F):
        hyp, gt = _interleave(per, (0, 1, 2), f0, f0 + F)
        R.run(st, *hyp, gt, F)
    assert st.counts[:, :, 0].sum() > 60 and st.counts[:, :, 3].sum() > 0 and st.counts[:, :, 4].sum() > 0
    for order in ((0, 1, 2), (2, 0, 1)):
        acc = mot.MotAccumulator(3, DEV, 3)
        for f0 in range(0, 12, F):
            hyp, gt = _interleave(per, order, f0, f0 + F)
            update(acc, hyp, gt, F=F)
        check(acc, st, "order %s" % (order,), order)


@pytest.mark.parametrize("max_workgroups", [1, 2])
def test_max_workgroups(max_workgroups):
    """S = 5 walked by 1 and 2 workgroups: what one workgroup per stream gives."""
    per = _streams(5, 6)
    st, acc = R.State(5, 3), mot.MotAccumulator(5, DEV, 3)
    for f0 in (0, 3):
        hyp, gt = _interleave(per, range(5), f0, f0 + 3)
        R.run(st, *hyp, gt, 3)
        update(acc, hyp, gt, F=3, max_workgroups=max_workgroups)
    check(acc, st)


# ------------------------------------------------------------------------------------------------ rows, counts, guards --
@pytest.mark.parametrize("rows", [1, 63, 64])
def test_rows_and_objects(rows):
    rs = np.random.RandomState(rows)
    frames = MC.random_frames(rs, 5, rows, extent=3000.0)
    frames = [(o[:rows], h[:rows]) for o, h in frames]
    hyp, gt = MC.pack(frames, rows, rows)
    acc, st = mot.MotAccumulator(1, DEV, 3), R.State(1, 3)
    R.run(st, *hyp, gt, 5)
    update(acc, sl(hyp, 0, 2), sl(gt, 0, 2), F=2)
    update(acc, sl(hyp, 2, 5), sl(gt, 2, 5), F=3)
    check(acc, st)
    assert rows == 1 or st.counts[0, :, 0].sum() > rows


@pytest.mark.parametrize("n_obj,n_hyp", [(64, 64), (3, 64), (64, 3), (33, 31)])
def test_dense_assignment(n_obj, n_hyp):
    """One class, jittered boxes on a 4-px grid: a row has many allowed pairs, continuity takes some and the wave-wide assignment
    the rest, with padding rows or columns where the sides differ."""
    rs = np.random.RandomState(100 * n_obj + n_hyp)
    frames = MC.dense_frames(rs, n_obj, n_hyp)
    hyp, gt = MC.pack(frames, max(n_hyp, 4), max(n_obj, 4))
    acc, st = mot.MotAccumulator(1, DEV, 2), R.State(1, 2)
    pairs = R.run(st, *hyp, gt, len(frames))
    update(acc, hyp, gt, F=len(frames))
    check(acc, st)
    assert sum(len(p) for p in pairs) >= 2 * min(n_obj, n_hyp) and (st.counts[0, 0, 3] > 0 or n_hyp == 3)


class Guarded:
    """[4 KiB of canary | the array, 256-byte aligned | 4 KiB of canary] in one uint8 device tensor."""

    def __init__(self, array):
        array = np.ascontiguousarray(array)
        self.raw = torch.full((2 * GUARD + array.nbytes + 256,), CANARY, dtype=torch.uint8, device=DEV)
        self.off = GUARD + (-(self.raw.data_ptr() + GUARD)) % 256
        self.nbytes = array.nbytes
        body = self.raw[self.off:self.off + array.nbytes]
        body.copy_(torch.from_numpy(bits(array).copy()))
        self.t = body.view(getattr(torch, array.dtype.name)).view(array.shape)

    def intact(self):
        return bool((self.raw[:self.off] == CANARY).all()) and bool((self.raw[self.off + self.nbytes:] == CANARY).all())


def guarded_accumulator(S, classes):
    g = {f: Guarded(np.zeros(shape, dtype)) for f, (shape, dtype) in mot.table_shapes(S, classes).items()}
    return mot.MotAccumulator(S, DEV, classes, tables={f: v.t for f, v in g.items()}), g


def test_invalid_rows_counts_and_guards():
    """Four streams share a frame of 7 hypotheses and 7 objects, most of them invalid -- NaN, inf, zero / negative size, id 0, a
    tentative row, a class out of range, a repeated id -- with counts 7, 99 (above the limit), 0 and -7.  Everything sits between
    canaries."""
    nan, inf = np.nan, np.inf
    good = MC.B(100.0)
    hyps = [(1, 0, good), (2, 0, (nan, 100.0, 40.0, 20.0)), (3, 0, (300.0, 100.0, 0.0, 20.0)), (0, 0, MC.B(400.0)), (5, 0, MC.B(500.0), 1),
            (6, 7, MC.B(600.0)), (1, 0, MC.B(700.0))]
    objs = [(1, 0, 0, good), (2, 0, 0, (300.0, inf, 40.0, 20.0)), (3, 0, 0, (300.0, 100.0, 40.0, -3.0)), (-4, 0, 0, MC.B(400.0)),
            (5, -1, 0, MC.B(500.0)), (1, 0, 0, MC.B(700.0)), (7, 1, 0, MC.B(700.0))]
    hyp, gt = MC.pack([(objs, hyps)] * 8, 7, 7)
    hyp[0][1::2, :, 0] += 3.0                                            # every stream's second frame has moved
    hyp[2][:] = np.asarray([7, 7, 99, 99, 0, 0, -7, -7], np.int32)       # stream s: frames 2s, 2s + 1
    gt[4][:] = np.asarray([7, 99, 7, -7, 7, 0, 0, 7], np.int32)
    st = R.State(4, 2)
    R.run(st, *hyp, gt, 2)
    acc, g_tab = guarded_accumulator(4, 2)
    g_in = [Guarded(a) for a in list(hyp) + list(gt)]
    acc.update(*[g.t for g in g_in[:5]], tuple(g.t for g in g_in[5:]), frames_per_stream=2)
    torch.cuda.synchronize()
    table, _ = check(acc, st)
    assert all(g.intact() for g in list(g_tab.values()) + g_in), "a canary changed"
    # one valid hypothesis (id 1, class 0) and two valid objects (id 1 on it, id 7 of class 1 elsewhere) per full frame
    assert table[0, 0, 0] == 2 and table[0, 1, 1] == 2 and table[1, 0, 0] == 1 and table[1, 0, 2] == 1 and table[:, :, 2].sum() == 1
    assert table[2, :, 1].sum() == 2 and table[2, :, 0].sum() == 0 and table[3, :, 1].sum() == 2
    for a, g in zip(list(hyp) + list(gt), g_in):
        same_bits(g.t.cpu().numpy(), a, "an input")


def test_too_many_rows_or_classes_is_unsupported():
    acc = mot.MotAccumulator(1, DEV, 3)
    z = torch.zeros((1, 65, 4), device=DEV)
    zi, c1 = z[..., 0].int().contiguous(), torch.zeros(1, dtype=torch.int32, device=DEV)
    g = (torch.zeros((1, 4, 4), dtype=torch.float64, device=DEV),) + (torch.zeros((1, 4), dtype=torch.int32, device=DEV),) * 3 + (c1,)
    with pytest.raises(_lib.SqdetUnsupported):
        acc.update(z, zi, c1, zi, zi, g)
    with pytest.raises(_lib.SqdetUnsupported):
        mot.MotAccumulator(1, DEV, 129)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in acc.tables().values())


# ------------------------------------------------------------------------------------------------ identity tables --
def _fill_frames(n_obj_ids, n_hyp_ids):
    """Frames of 64 new object and 64 new hypothesis identities each (the last frame takes the remainder), on top of each other in
    pairs, until the given numbers of identities have appeared."""
    frames, o, h = [], 0, 0
    while o < n_obj_ids or h < n_hyp_ids:
        no, nh = min(64, n_obj_ids - o), min(64, n_hyp_ids - h)
        frames.append(([(o + k + 1, 0, 0, MC.B(100.0 * k)) for k in range(no)], [(h + k + 1, 0, MC.B(100.0 * k)) for k in range(nh)]))
        o, h = o + no, h + nh
    return frames


def test_identity_tables_filled_to_their_limits():
    """Exactly 256 object and 1024 hypothesis identities are accepted, and a frame that only meets known ones afterwards still
    counts."""
    frames = _fill_frames(256, 1024) + [([(256, 0, 0, MC.B(0.0))], [(1024, 0, MC.B(0.0))])]
    hyp, gt = MC.pack(frames, 64, 64)
    st = R.State(1, 1)
    R.run(st, *hyp, gt, len(frames))
    acc, guards = guarded_accumulator(1, 1)
    update(acc, hyp, gt, F=len(frames))
    table, _ = check(acc, st)
    assert all(g.intact() for g in guards.values())
    assert table[0, 0, 12] == 256 and table[0, 0, 13] == 1024 and table[0, 0, 0] == 257 and table[0, 0, 3] == 1


@pytest.mark.parametrize("n_obj_ids,n_hyp_ids,status", [(257, 64, 1), (64, 1025, 2), (257, 1025, 1)])
def test_one_identity_too_many_sets_the_status(n_obj_ids, n_hyp_ids, status):
    frames = _fill_frames(n_obj_ids, n_hyp_ids) + [([(1, 0, 0, MC.B(0.0))], [(1, 0, MC.B(0.0))])]
    hyp, gt = MC.pack(frames, 64, 64)
    st = R.State(1, 1)
    R.run(st, *hyp, gt, len(frames))
    assert st.status[0] == status
    acc, guards = guarded_accumulator(1, 1)
    update(acc, hyp, gt, F=len(frames))
    ref = st.arrays()
    for f, t in acc.tables().items():
        same_bits(t.cpu().numpy(), ref[f], "table %s" % f)
    counters, iou_sum = np.full((1, 1, mot.K), 77, np.int64), np.full((1, 1), 7.0)
    rc = _lib.lib().sqdet_mot_evaluate(C.byref(acc._tables), 1, 1, C.c_void_p(acc._result.data_ptr()), C.c_void_p(counters.ctypes.data),
                                       C.c_void_p(iou_sum.ctypes.data), _lib.stream_ptr())
    assert rc == _lib.SQDET_EUNSUPPORTED and (counters == 77).all() and (iou_sum == 7.0).all()      # the host outputs are untouched
    with pytest.raises(_lib.SqdetUnsupported):
        acc.evaluate()
    assert all(g.intact() for g in guards.values()), "a guard word changed"
    acc.reset()
    update(acc, sl(hyp, 0, 1), sl(gt, 0, 1))
    assert acc.evaluate()["overall"]["tp"] == 64                        # a reset clears the status


# ------------------------------------------------------------------------------------------------ evaluate alone --
@pytest.mark.parametrize("G,T", [(256, 1024), (256, 100), (1, 1), (40, 0)])
def test_evaluate_alone_on_loaded_tables(G, T):
    """sqdet_mot_evaluate on random sparse overlap tables with many ties, loaded through load_state_dict: the restatement's
    counters exactly (idtp depends on the optimum only, its split over classes on the pairs), and scipy's optimum where it imports."""
    rs = np.random.RandomState(G * 7 + T)
    d = MC.sparse_overlap(rs, G, T) if T else MC.sparse_overlap(rs, G, 1)
    if not T:
        d["n_hyp"][0], d["overlap"][:], d["hyp_frames"][:] = 0, 0, 0
    acc = mot.MotAccumulator(1, DEV, 3)
    acc.load_state_dict({k: torch.from_numpy(v) for k, v in d.items()})
    want, want_iou = R.evaluate_tables(d, 3)
    got, got_iou = acc.evaluate_raw()
    same_bits(got, want, "counters"), same_bits(got_iou, want_iou, "iou_sum")
    for f, t in acc.tables().items():
        same_bits(t.cpu().numpy(), d[f], "evaluate changed table %s" % f)
    assert got[0, :, 12].sum() == G and got[0, :, 13].sum() == T
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        return
    if T:
        ov = d["overlap"][0, :G, :T].astype(np.int64)
        ri, ci = linear_sum_assignment(-ov)
        assert got[0, :, 9].sum() == ov[ri, ci].sum()


# ------------------------------------------------------------------------------------------------ the device-only pipeline --
def test_graph_of_tracker_and_accumulator_replayed_over_three_frames():
    """One capture of Tracker.update followed by MotAccumulator.update on a side stream, replayed over three frames whose
    detection and label tensors are overwritten in place: the host pipeline -- the tracker's restatement, then this one's."""
    rows_per_frame, labels = TC.scene(0)
    frames, _ = MC.scene_frames(0)
    det = TC.pack(rows_per_frame, 8)
    kw = dict(min_hits=1)                                       # confirmed at birth: three frames are enough to count
    ids, sts = TR.run(TR.Tables(1), *det, 60, TR.params(**kw))
    gt = MC.pack(frames, 8, 8)[1]
    st = R.State(1, 3)
    R.run(st, *[a[:3] for a in (det[0], det[2], det[3], ids, sts)], [a[:3] for a in gt], 3)
    assert st.counts[0, :, 0].sum() >= 9
    trk, acc = track.Tracker(1, DEV, **kw), mot.MotAccumulator(1, DEV, 3)
    s_det, s_gt = dev(*[a[:1] for a in det]), tuple(dev(*[a[:1] for a in gt]))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = trk.update(*s_det)                                # warm-up outside the capture: the library is loaded, outputs exist
        acc.update(s_det[0], s_det[2], s_det[3], out[0], out[1], s_gt)
        side.synchronize()
        trk.reset(), acc.reset()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = trk.update(*s_det)
            acc.update(s_det[0], s_det[2], s_det[3], out[0], out[1], s_gt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for f in range(3):
        for t, a in zip(list(s_det) + list(s_gt), list(det) + list(gt)):
            t.copy_(torch.from_numpy(a[f:f + 1]))
        graph.replay()
        torch.cuda.synchronize()
        same_bits(out[0].cpu().numpy(), ids[f:f + 1], "replayed ids, frame %d" % f)
    check(acc, st, "after three replays")


def test_mot_eval_tool_on_a_file_in_the_demo_format(tmp_path):
    """tools/mot_eval.py on a results file in demo.py --track_out's format and a MOTChallenge gt.txt, in a child process: the
    restatement's numbers on what the files hold (two-decimal boxes)."""
    rs = np.random.RandomState(5)
    frames = MC.random_frames(rs, 12, 6, classes=1)
    with open(tmp_path / "res.txt", "w") as out:
        for f, (_, hyps) in enumerate(frames):
            for h in hyps:
                if len(h) == 3 or h[3] == 2:
                    cx, cy, w, hh = h[2]
                    out.write("%d,%d,%.2f,%.2f,%.2f,%.2f,%.4f,-1,-1,-1\n" % (f + 1, h[0], cx - w / 2, cy - hh / 2, w, hh, 0.9))
    with open(tmp_path / "gt.txt", "w") as out:
        for f, (objs, _) in enumerate(frames):
            for (ident, _, flags, (cx, cy, w, hh)) in objs:
                out.write("%d,%d,%.2f,%.2f,%.2f,%.2f,%d,1,1.0\n" % (f + 1, ident, cx - w / 2, cy - hh / 2, w, hh, 0 if flags else 1))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mot_eval.py"), "--gt", str(tmp_path / "gt.txt"), "--results",
                        str(tmp_path / "res.txt"), "--json"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    g = mot.MotGroundTruth.from_mot_text(str(tmp_path / "gt.txt"))
    hyp = mot.load_mot_results(str(tmp_path / "res.txt"), 12)
    st = R.State(1, 1)
    R.run(st, *hyp, g.arrays(1, 12), 12)
    table, iou_sum = R.evaluate(st)
    want = mot.metrics(table[0, 0], iou_sum[0, 0])
    assert want["tp"] > 30 and "MOTA" in r.stdout and "OVERALL" in r.stdout
    assert {k: got[k] for k in mot.COUNTERS} == {k: want[k] for k in mot.COUNTERS} and got["iou_sum"] == want["iou_sum"]


def test_demo_video_track_gt_prints_the_summary(tmp_path):
    """demo.py --mode video --track --track_out --track_gt (a MOTChallenge gt.txt, one class, nothing ignored) in a child process:
    the summary comes last, every labelled row is a tp or a fn and every line of the tracks file a tp or a fp."""
    from PIL import Image
    src = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "sample.png")).convert("RGB"))
    (tmp_path / "frames").mkdir()
    for k in range(6):                                          # pairs of equal frames, shifted by 3 px: tracks are confirmed
        Image.fromarray(np.roll(src, 3 * (k // 2), axis=1)).save(str(tmp_path / "frames" / ("%03d.png" % k)))
    with open(tmp_path / "gt.txt", "w") as out:
        for f in range(1, 7):
            for ident, (left, top) in enumerate(((100, 100), (400, 150), (800, 200)), 1):
                out.write("%d,%d,%d,%d,120,80,1,1,1.0\n" % (f, ident, left + 3 * ((f - 1) // 2), top))
    args = ["--mode", "video", "--input_path", str(tmp_path / "frames" / "*.png"), "--crop", "0", "0", "0", "0", "--batch", "4", "--track",
            "--track_opts", "high_thresh=0.0,low_thresh=-1.0,min_hits=2", "--out_dir", str(tmp_path / "out"), "--track_out",
            str(tmp_path / "mot.txt"), "--track_gt", str(tmp_path / "gt.txt"), "--track_gt_format", "mot"]
    r = subprocess.run([sys.executable, "-c", "import sys, demo; demo.main(sys.argv[1:])"] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("OVERALL") and "MOTA" in lines[-3] and lines[-2].startswith("all")
    v = lines[-1].split()
    tp, fp, fn = int(v[6]), int(v[7]), int(v[8])
    tracked = open(tmp_path / "mot.txt").read().splitlines()
    assert tracked and tp + fn == 18 and tp + fp == len(tracked)
