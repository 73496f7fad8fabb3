"""squeezedet_amd.track on the GPU: every table and output of sqdet_track_update against the sequential NumPy restatement
(tests/track_reference.py), BITWISE -- the int arrays, the float64 filters x and P, the float32 score -- at the smallest shapes
at which the kernel can go wrong; sqdet_track_build_items against a Python restatement; demo.py --mode video --track."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from squeezedet_amd import _lib, track, viz
from tests import draw_reference as DR
from tests import track_cases as TC
from tests import track_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
CANARY = 0xA5


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(got.view("u%d" % got.itemsize) != want.view("u%d" % want.itemsize))
        raise AssertionError("%s differs at %d places, first %s: %r vs %r" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))


def tables_equal(trk, T, what=""):
    ref = T.arrays()
    for f, t in trk.tables().items():
        same_bits(t.cpu().numpy(), ref[f], "%s table %s" % (what, f))


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def update(trk, boxes, probs, cls, counts, F=1, **kw):
    """One call on host arrays -> host (ids, states)."""
    i, s = trk.update(*dev(boxes, probs, cls, counts), frames_per_stream=F, **kw)
    return i.cpu().numpy().copy(), s.cpu().numpy().copy()


def random_frames(rs, n_frames, n_obj, extent=600.0):
    """Objects on straight lines with random classes; per frame each is high, low, or absent, plus a few strays."""
    obj = [(rs.uniform(0, extent), rs.uniform(0, extent / 2), rs.uniform(20, 60), rs.uniform(20, 60), rs.uniform(-6, 6), rs.uniform(-3, 3),
            int(rs.randint(3))) for _ in range(n_obj)]
    frames = []
    for f in range(n_frames):
        rows = []
        for (cx, cy, w, h, vx, vy, c) in obj:
            u = rs.rand()
            if u < 0.12:
                continue
            prob = rs.uniform(0.12, 0.45) if u < 0.3 else rs.uniform(0.55, 0.99)
            rows.append((cx + vx * f + rs.uniform(-1, 1), cy + vy * f + rs.uniform(-1, 1), w + rs.uniform(-1, 1), h + rs.uniform(-1, 1), prob, c))
        rs.shuffle(rows)
        frames.append([tuple(r) for r in rows])
    return frames


# ------------------------------------------------------------------------------------------------ cases and the scene --
@pytest.mark.parametrize("name", sorted(TC.CASES))
def test_hand_worked_case(name):
    kw, frames, expect = TC.CASES[name]
    boxes, probs, cls, counts = TC.pack(frames, 4)
    trk, T, p = track.Tracker(1, DEV, **kw), R.Tables(1), R.params(**kw)
    for f in range(len(frames)):
        ids, sts = update(trk, boxes[f:f + 1], probs[f:f + 1], cls[f:f + 1], counts[f:f + 1])
        wi, ws = R.step(T, 0, boxes[f], probs[f], cls[f], counts[f], p)
        same_bits(ids[0], wi, "%s frame %d ids" % (name, f))
        same_bits(sts[0], ws, "%s frame %d states" % (name, f))
        n = len(frames[f])
        assert ids[0, :n].tolist() == expect[f][0] and sts[0, :n].tolist() == expect[f][1]
        tables_equal(trk, T, "%s frame %d" % (name, f))
    assert trk.tracks(0) == T.tracks(0)


@pytest.fixture(scope="module")
def scene0():
    """Scene 0 packed, with the restatement's outputs and final tables (read only)."""
    frames, labels = TC.scene(0)
    arrays = TC.pack(frames, 8)
    T = R.Tables(1)
    ids, sts = R.run(T, *arrays, 60, R.params())
    return arrays, labels, ids, sts, T


@pytest.mark.parametrize("seed", range(5))
def test_scene_frame_by_frame(seed):
    frames, labels = TC.scene(seed)
    boxes, probs, cls, counts = TC.pack(frames, 8)
    trk, T = track.Tracker(1, DEV), R.Tables(1)
    wi, ws = R.run(T, boxes, probs, cls, counts, 60, R.params())
    got = [update(trk, boxes[f:f + 1], probs[f:f + 1], cls[f:f + 1], counts[f:f + 1]) for f in range(60)]
    same_bits(np.concatenate([g[0] for g in got]), wi, "ids")
    same_bits(np.concatenate([g[1] for g in got]), ws, "states")
    tables_equal(trk, T)
    TC.check_scene(np.concatenate([g[0] for g in got]), labels, int(trk.next_id.cpu()[0]))


@pytest.mark.parametrize("chunk", [60, 7])
def test_scene_in_chunks(scene0, chunk):
    """All 60 frames in one call, and in calls of 7 with the last of 4: what 60 single-frame calls give."""
    (boxes, probs, cls, counts), _, wi, ws, T = scene0
    trk = track.Tracker(1, DEV)
    ids, sts, sizes = [], [], []
    for f0 in range(0, 60, chunk):
        f1 = min(f0 + chunk, 60)
        i, s = update(trk, boxes[f0:f1], probs[f0:f1], cls[f0:f1], counts[f0:f1], F=f1 - f0)
        ids.append(i), sts.append(s), sizes.append(f1 - f0)
    assert sizes[-1] == (60 if chunk == 60 else 4)
    same_bits(np.concatenate(ids), wi, "ids")
    same_bits(np.concatenate(sts), ws, "states")
    tables_equal(trk, T)


def test_state_dict_round_trip(scene0):
    (boxes, probs, cls, counts), _, wi, ws, T = scene0
    a = track.Tracker(1, DEV)
    update(a, boxes[:23], probs[:23], cls[:23], counts[:23], F=23)
    saved = a.state_dict()
    update(a, boxes[23:30], probs[23:30], cls[23:30], counts[23:30], F=7)                # a goes on; the copy must not follow
    b = track.Tracker(1, DEV)
    b.load_state_dict(saved)
    ids, sts = update(b, boxes[23:], probs[23:], cls[23:], counts[23:], F=37)
    same_bits(ids, wi[23:], "ids after the reload")
    same_bits(sts, ws[23:], "states after the reload")
    tables_equal(b, T)
    b.reset()
    tables_equal(b, R.Tables(1), "after reset")


# ------------------------------------------------------------------------------------------------ several streams --
def _three_streams():
    """12 frames of three streams with different histories: scene 0 from its start, scene 1 from frame 20, and a stream that
    sees three frames and then nothing (count 0: it only ages)."""
    s0, s1 = TC.scene(0)[0][:12], TC.scene(1)[0][20:32]
    s2 = [[TC._row()], [TC._row()], [TC._row()]] + [[]] * 9
    return [TC.pack(s, 8) for s in (s0, s1, s2)]


def _interleave(streams, order, f0, f1):
    """The arrays of frames [f0, f1) of the streams in `order`, image s*F + f."""
    return [np.concatenate([streams[s][k][f0:f1] for s in order]) for k in range(4)]


@pytest.mark.parametrize("F", [1, 4])
def test_three_streams_and_their_permutation(F):
    streams = _three_streams()
    T = R.Tables(3)
    want = [R.run(T, *_interleave(streams, (0, 1, 2), f0, f0 + F), F, R.params()) for f0 in range(0, 12, F)]
    for order in ((0, 1, 2), (2, 0, 1)):
        trk = track.Tracker(3, DEV)
        for k, f0 in enumerate(range(0, 12, F)):
            ids, sts = update(trk, *_interleave(streams, order, f0, f0 + F), F=F)
            for pos, s in enumerate(order):
                same_bits(ids[pos * F:(pos + 1) * F], want[k][0][s * F:(s + 1) * F], "ids of stream %d" % s)
                same_bits(sts[pos * F:(pos + 1) * F], want[k][1][s * F:(s + 1) * F], "states of stream %d" % s)
        for f, t in trk.tables().items():
            same_bits(t.cpu().numpy(), T.arrays()[f][list(order)], "table %s, order %s" % (f, order))
    idle = T.tracks(2)
    assert [(t["id"], t["state"], t["hits"], t["miss"], t["age"]) for t in idle] == [(1, 2, 3, 9, 12)]


@pytest.mark.parametrize("max_workgroups", [1, 2])
def test_max_workgroups(max_workgroups):
    """S = 5 walked by 1 and 2 workgroups: what one workgroup per stream gives."""
    rs = np.random.RandomState(7)
    per = [TC.pack(random_frames(rs, 6, 9), 16) for _ in range(5)]
    a, b = track.Tracker(5, DEV), track.Tracker(5, DEV)
    T = R.Tables(5)
    for f0 in range(0, 6, 3):
        arrays = _interleave(per, range(5), f0, f0 + 3)
        wi, ws = R.run(T, *arrays, 3, R.params())
        for trk, kw in ((a, {}), (b, dict(max_workgroups=max_workgroups))):
            ids, sts = update(trk, *arrays, F=3, **kw)
            same_bits(ids, wi, "ids"), same_bits(sts, ws, "states")
    tables_equal(a, T), tables_equal(b, T)


# ------------------------------------------------------------------------------------------------ rows and counts --
@pytest.mark.parametrize("rows", [1, 63, 64])
def test_rows(rows):
    rs = np.random.RandomState(rows)
    frames = random_frames(rs, 6, rows, extent=2500.0)
    frames = [fr if f != 3 else fr[:rows // 2] for f, fr in enumerate(frames)]
    boxes, probs, cls, counts = TC.pack(frames, rows)
    assert counts.max() > rows * 0.7
    trk, T = track.Tracker(1, DEV, min_hits=2, max_age=2), R.Tables(1)
    wi, ws = R.run(T, boxes, probs, cls, counts, 6, R.params(min_hits=2, max_age=2))
    ids, sts = update(trk, boxes[:2], probs[:2], cls[:2], counts[:2], F=2)
    i2, s2 = update(trk, boxes[2:], probs[2:], cls[2:], counts[2:], F=4)
    same_bits(np.concatenate([ids, i2]), wi, "ids"), same_bits(np.concatenate([sts, s2]), ws, "states")
    tables_equal(trk, T)
    assert rows == 1 or (wi >= 0).sum() > rows


@pytest.mark.parametrize("n_obj,rows", [(30, 64), (47, 48), (60, 64)])
def test_dense_contention(n_obj, rows):
    """Heavily overlapping boxes of ONE class, jittered, some low, some absent: most slots want a row another slot wants too, so
    the association needs many rounds, rescans on both sides and every length of the 4-wide scan tail."""
    rs = np.random.RandomState(100 + n_obj)
    centre = [(200.0 + 4.0 * (k % 8) + rs.uniform(-2, 2), 150.0 + 4.0 * (k // 8) + rs.uniform(-2, 2), rs.uniform(38, 46), rs.uniform(38, 46))
              for k in range(n_obj)]
    frames = []
    for f in range(7):
        fr = []
        for (cx, cy, w, h) in centre:
            u = rs.rand()
            if u < 0.15:
                continue
            fr.append((cx + 1.5 * f + rs.uniform(-3, 3), cy + rs.uniform(-3, 3), w + rs.uniform(-2, 2), h + rs.uniform(-2, 2),
                       rs.uniform(0.15, 0.45) if u < 0.4 else rs.uniform(0.55, 0.99), 0))
        rs.shuffle(fr)
        frames.append([tuple(r) for r in fr])
    boxes, probs, cls, counts = TC.pack(frames, rows)
    kw = dict(min_hits=2, max_age=1)
    trk, T = track.Tracker(1, DEV, **kw), R.Tables(1)
    wi, ws = R.run(T, boxes, probs, cls, counts, 7, R.params(**kw))
    ids, sts = update(trk, boxes[:3], probs[:3], cls[:3], counts[:3], F=3)
    i2, s2 = update(trk, boxes[3:], probs[3:], cls[3:], counts[3:], F=4)
    same_bits(np.concatenate([ids, i2]), wi, "ids"), same_bits(np.concatenate([sts, s2]), ws, "states")
    tables_equal(trk, T)
    assert (ws == 2).sum() > n_obj                            # tracks were matched again, in stage one and in stage two


def test_rows_65_is_unsupported():
    trk = track.Tracker(1, DEV)
    before = {f: t.clone() for f, t in trk.tables().items()}
    z = torch.zeros((1, 65, 4), device=DEV)
    with pytest.raises(_lib.SqdetUnsupported):
        trk.update(z, z[..., 0].contiguous(), z[..., 0].int().contiguous(), torch.zeros(1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(before[f], t) for f, t in trk.tables().items())


def test_fill_drop_and_refill():
    """64 high rows fill every slot of an empty stream; 64 others are all dropped with max_age 5 (dropped = 64), and free and
    refill every slot with max_age 0 (min_hits 1)."""
    a = [(50.0 * (k % 8), 50.0 * (k // 8), 20.0, 20.0, 0.9, k % 3) for k in range(64)]
    b = [(r[0] + 10000.0,) + r[1:] for r in a]
    arrays = TC.pack([a, b], 64)
    for max_age in (5, 0):
        kw = dict(min_hits=1, max_age=max_age)
        trk, T = track.Tracker(1, DEV, **kw), R.Tables(1)
        wi, ws = R.run(T, *arrays, 2, R.params(**kw))
        ids, sts = update(trk, *arrays, F=2)
        same_bits(ids, wi, "ids"), same_bits(sts, ws, "states")
        tables_equal(trk, T)
        assert ids[0].tolist() == list(range(1, 65)) and len(trk.tracks(0)) == 64
        if max_age == 5:
            assert (ids[1] == -1).all() and int(trk.dropped.cpu()[0]) == 64 and int(trk.next_id.cpu()[0]) == 65
        else:
            assert ids[1].tolist() == list(range(65, 129)) and (sts[1] == 2).all() and int(trk.dropped.cpu()[0]) == 0


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


def test_invalid_rows_counts_and_guards():
    """Four streams share one frame of 6 rows, five of them invalid (NaN, inf, zero / negative size, NaN prob), with count 6, 99
    (above rows), 0 and -7 (the filter's overflow report); then a second frame.  Every table, input and output sits between
    canaries."""
    nan, inf = np.nan, np.inf
    rows = [(100.0, 100.0, 40.0, 20.0, 0.9, 0), (nan, 100.0, 40.0, 20.0, 0.9, 0), (300.0, inf, 40.0, 20.0, 0.9, 0),
            (500.0, 100.0, 0.0, 20.0, 0.9, 0), (600.0, 100.0, 40.0, -3.0, 0.9, 0), (700.0, 100.0, 40.0, 20.0, nan, 0)]
    boxes, probs, cls, _ = TC.pack([rows] * 8, 6)
    boxes[1::2, :, 0] += 3.0                                                            # every stream's second frame has moved
    probs[1, 2], boxes[3, 4, 2] = -inf, inf
    counts = np.asarray([6, 6, 99, 99, 0, 0, -7, -7], np.int32)                          # stream s: frames 2s, 2s + 1
    T = R.Tables(4)
    wi, ws = R.run(T, boxes, probs, cls, counts, 2, R.params())
    ref0 = R.Tables(4)
    g_tab = {f: Guarded(v) for f, v in ref0.arrays().items()}
    g_in = [Guarded(a) for a in (boxes, probs, cls, counts)]
    g_out = [Guarded(np.full((8, 6), 77, np.int32)) for _ in range(2)]
    trk = track.Tracker(4, DEV, tables={f: g.t for f, g in g_tab.items()})
    trk.update(*[g.t for g in g_in], frames_per_stream=2, out=tuple(g.t for g in g_out))
    torch.cuda.synchronize()
    same_bits(g_out[0].t.cpu().numpy(), wi, "ids"), same_bits(g_out[1].t.cpu().numpy(), ws, "states")
    tables_equal(trk, T)
    assert all(g.intact() for g in list(g_tab.values()) + g_in + g_out), "a canary changed"
    assert wi[:4, 0].tolist() == [1, 1, 1, 1] and (wi[:, 1:] == -1).all() and (wi[4:] == -1).all()
    for a, g in zip((boxes, probs, cls, counts), g_in):
        same_bits(g.t.cpu().numpy(), a, "an input")


# ------------------------------------------------------------------------------------------------ graph capture --
def test_graph_capture_replays_three_frames(scene0):
    """One capture of update() on a side stream, replayed over three frames whose detection tensors are overwritten in place:
    three eager calls."""
    (boxes, probs, cls, counts), _, wi, ws, _ = scene0
    eager, T = track.Tracker(1, DEV), R.Tables(1)
    captured = track.Tracker(1, DEV)
    static = dev(boxes[:1], probs[:1], cls[:1], counts[:1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.update(*static)                              # warm-up outside the capture: the library is loaded, outputs exist
        captured.reset()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = captured.update(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    captured.reset()                                          # (capturing runs nothing; the tables are as after the reset)
    for f in range(3):
        for t, a in zip(static, (boxes, probs, cls, counts)):
            t.copy_(torch.from_numpy(a[f:f + 1]))
        graph.replay()
        torch.cuda.synchronize()
        ids, sts = update(eager, boxes[f:f + 1], probs[f:f + 1], cls[f:f + 1], counts[f:f + 1])
        same_bits(out[0].cpu().numpy(), ids, "replayed ids, frame %d" % f)
        same_bits(out[1].cpu().numpy(), sts, "replayed states, frame %d" % f)
        same_bits(ids, wi[f:f + 1], "ids, frame %d" % f)
    for f, t in captured.tables().items():
        same_bits(t.cpu().numpy(), eager.tables()[f].cpu().numpy(), "table %s" % f)


# ------------------------------------------------------------------------------------------------ draw items --
NAMES = ["car", "class_name_that_has_28_bytes", "cyclist"]        # 28 bytes: " #1234567" is cut after its first digit


def _item_frame():
    """2 images x 8 rows: a tentative row, confirmed rows, one below the plot threshold, an unmatched row, an id >= 1000, a label
    cut at 31 bytes, a class out of range, and a confirmed row past the count."""
    boxes = np.zeros((2, 8, 4), np.float32)
    for i in range(2):
        for j in range(8):
            boxes[i, j] = (30.0 + 25.0 * j + 7.0 * i, 40.0 + 6.0 * j, 31.0 + j, 21.0 + 2 * j)
    probs = np.full((2, 8), 0.9, np.float32)
    cls = np.asarray([[0, 2, 0, 1, 2, 7, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], np.int32)
    ids = np.asarray([[3, 4, 5, 1234567, -1, 12, 1000, 9], [65, 2, -1, -1, -1, -1, -1, -1]], np.int32)
    sts = np.asarray([[1, 2, 2, 2, 0, 2, 2, 2], [2, 2, 0, 0, 0, 0, 0, 0]], np.int32)
    probs[0, 2] = 0.3                                        # confirmed, below plot_thresh 0.4
    counts = np.asarray([7, 2], np.int32)                    # image 0: row 7 is past the count
    return boxes, probs, cls, counts, ids, sts


def test_track_items_and_draw():
    boxes, probs, cls, counts, ids, sts = _item_frame()
    want = R.track_items(boxes, probs, cls, counts, ids, sts, NAMES, track.PALETTE, 0.4)
    assert [len(w) for w in want] == [4, 2]
    labels = [it[5] for it in want[0]] + [it[5] for it in want[1]]
    assert b"cyclist #4" in labels and b"car #1000" in labels and b"? #12" in labels
    assert len(NAMES[1]) == 28 and b"class_name_that_has_28_bytes #1" in labels                # 31 bytes: cut inside the digits
    items = track.make_track_items(*dev(boxes, probs, cls, counts, ids, sts), NAMES, plot_thresh=0.4)
    assert items.decode() == want and items.counts.cpu().tolist() == [4, 2]
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, size=(2, 120, 260, 3)).astype(np.uint8)
    got = viz.draw(torch.from_numpy(img).to(DEV), items, order="bgr").cpu().numpy()
    assert np.array_equal(got, DR.draw(img, [want], viz.font(), "bgr")) and not np.array_equal(got, img)


def test_track_items_across_waves():
    """B = 2, M = 130: three waves of rows, the last one of two rows.  Every wave of image 0 keeps some rows and drops some, so
    a kept row's place depends on the waves before it; image 1 counts 65 rows, so its second wave keeps exactly its first row
    though every later row is a confirmed track too."""
    B, M = 2, 130
    j = np.arange(M)
    boxes = np.zeros((B, M, 4), np.float32)
    for i in range(B):
        boxes[i] = np.stack([20.5 + 3.0 * j + i, 30.25 + 2.0 * (j % 50), 11.0 + (j % 7), 9.0 + (j % 5)], 1)
    probs = np.full((B, M), 0.9, np.float32)
    cls = np.stack([j % 3, (j + 1) % 3]).astype(np.int32)
    ids = np.stack([1 + j, 1000 + 7 * j]).astype(np.int32)
    sts = np.full((B, M), 2, np.int32)
    sts[0, j % 3 == 0] = 1                                   # tentative: rows 0, 3, .. 129
    probs[0, j % 5 == 1] = 0.3                               # below plot_thresh
    ids[0, 64] = 0                                           # no track
    ids[0, 127] = -1
    sts[0, 128], sts[0, 129] = 0, 2                          # the last wave drops its first row and keeps its second
    sts[1, 1:40:2] = 0
    counts = np.asarray([130, 65], np.int32)
    want = R.track_items(boxes, probs, cls, counts, ids, sts, NAMES, track.PALETTE, 0.4)
    kept = [[(sts[i, r] == 2 and ids[i, r] > 0 and probs[i, r] > 0.4 and r < counts[i]) for r in range(M)] for i in range(B)]
    for lo, hi in ((0, 64), (64, 128), (128, 130)):
        assert 0 < sum(kept[0][lo:hi]) < hi - lo
    assert not kept[0][128] and kept[0][129] and 0 < sum(kept[1][:64]) < 64 and kept[1][64] and sum(kept[1][64:]) == 1
    assert [len(w) for w in want] == [sum(k) for k in kept]
    items = track.make_track_items(*dev(boxes, probs, cls, counts, ids, sts), NAMES, plot_thresh=0.4)
    assert items.counts.cpu().tolist() == [len(w) for w in want]
    assert items.decode() == want


# ------------------------------------------------------------------------------------------------ demo.py --
def _frames(tmp_path):
    """Six frames: the golden sample, shifted by 3 px after every second frame (a pair of equal frames confirms its tracks)."""
    from PIL import Image
    src = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "sample.png")).convert("RGB"))
    d = tmp_path / "frames"
    d.mkdir()
    for k in range(6):
        Image.fromarray(np.roll(src, 3 * (k // 2), axis=1)).save(str(d / ("%03d.png" % k)))
    return str(d / "*.png")


def _demo(args, check=""):
    """demo.py in a child process under its own timeout (the child is killed and reaped when it runs out), exit status checked;
    `check`: Python run after main() in the same child."""
    code = "import sys, demo; demo.main(sys.argv[1:]); " + check
    r = subprocess.run([sys.executable, "-c", code] + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def test_demo_video_track(tmp_path):
    """demo.py --mode video --track --track_out: six pictures, a MOT file whose every line parses, the same file from a second
    run; --batch 4 pads its second batch, and the padding frames never reach the tracker (frames stay within 1..6)."""
    glob_ = _frames(tmp_path)
    common = ["--mode", "video", "--input_path", glob_, "--crop", "0", "0", "0", "0", "--batch", "4", "--track",
              "--track_opts", "high_thresh=0.0,low_thresh=-1.0,min_hits=2"]
    for k in range(2):                                        # one after the other: nothing starts after a failure
        _demo(common + ["--out_dir", str(tmp_path / ("out%d" % k)), "--track_out", str(tmp_path / ("mot%d.txt" % k))])
    assert sorted(os.listdir(tmp_path / "out0")) == ["%06d.jpg" % k for k in range(1, 7)]
    text = open(tmp_path / "mot0.txt").read()
    assert text == open(tmp_path / "mot1.txt").read()
    lines = text.splitlines()
    assert lines, "no confirmed row in six frames"
    for ln in lines:
        v = ln.split(",")
        assert len(v) == 10 and v[7:] == ["-1", "-1", "-1"]
        frame, tid = int(v[0]), int(v[1])
        left, top, w, h, score = (float(q) for q in v[2:7])
        assert 2 <= frame <= 6 and 1 <= tid < 64 * 6 + 1 and w > 0 and h > 0 and np.isfinite([left, top, score]).all()


def test_demo_video_without_track_is_the_old_path(tmp_path):
    """Without --track the child never imports squeezedet_amd.track, and its pictures are those of the per-detection item path
    (viz.make_items + viz.draw) run here on the same frames."""
    import importlib.util
    from PIL import Image
    glob_ = _frames(tmp_path)
    args = ["--mode", "video", "--input_path", glob_, "--crop", "0", "0", "0", "0", "--batch", "4", "--out_dir", str(tmp_path / "out")]
    _demo(args, check="assert 'squeezedet_amd.track' not in sys.modules, 'the tracker was imported'")
    spec = importlib.util.spec_from_file_location("_root_demo", os.path.join(ROOT, "demo.py"))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
    from squeezedet_amd import drivers, ops
    a = D.parse_args(args)
    mc, model, dtype = D.make_model(a, a.batch)
    files = sorted(os.listdir(tmp_path / "frames"))
    count = 0
    for i0 in (0, 4):
        crops = [drivers.read_bgr(str(tmp_path / "frames" / f)) for f in files[i0:i0 + 4]]
        n = len(crops)
        crops += [crops[-1]] * (4 - n)
        x = ops.preprocess_bgr(torch.from_numpy(np.stack(crops)).to(model.device), mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, dtype)
        pics, _ = D.detect_and_draw(model, x, n)
        for im in pics.cpu().numpy():
            count += 1
            Image.fromarray(im).save(str(tmp_path / ("want_%06d.jpg" % count)))
    assert sorted(os.listdir(tmp_path / "out")) == ["%06d.jpg" % k for k in range(1, 7)]
    for k in range(1, 7):
        assert open(tmp_path / "out" / ("%06d.jpg" % k), "rb").read() == open(tmp_path / ("want_%06d.jpg" % k), "rb").read(), k
