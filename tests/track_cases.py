"""Inputs for the tracker's tests, shared by the host tests (tests/test_track_host.py: the NumPy restatement against hand-worked
numbers) and the GPU tests (tests/test_gpu_track.py: the kernel against the restatement, bit for bit).

A FRAME is a list of rows (cx, cy, w, h, prob, cls).  ``pack(frames, rows)`` turns frames into the arrays the filter emits;
``CASES`` are the hand-worked cases: name -> (params, frames, expected per-frame (ids, states)); ``scene(seed)`` is the
60-frame scene of four objects with clutter."""
import numpy as np

BOX = (100.0, 100.0, 40.0, 20.0)


def pack(frames, rows):
    """frames -> boxes float32 [n,rows,4], probs float32 [n,rows], cls int32 [n,rows], counts int32 [n]; rows past a frame's
    count hold a far-away decoy that would match nothing and must never be read."""
    n = len(frames)
    boxes = np.tile(np.asarray([5000.0, 5000.0, 30.0, 30.0], np.float32), (n, rows, 1))
    probs, cls = np.full((n, rows), 0.99, np.float32), np.zeros((n, rows), np.int32)
    counts = np.zeros(n, np.int32)
    for i, fr in enumerate(frames):
        counts[i] = len(fr)
        for j, r in enumerate(fr):
            boxes[i, j], probs[i, j], cls[i, j] = r[:4], r[4], r[5]
    return boxes, probs, cls, counts


def _row(box=BOX, prob=0.9, cls=0):
    return tuple(box) + (prob, cls)


# name -> (params, frames, expected [(ids, states)] per frame)
CASES = {
    # born tentative, confirmed at the third hit
    "birth_confirm": ({}, [[_row()], [_row()], [_row()]], [([1], [1]), ([1], [1]), ([1], [2])]),
    # a tentative track dies on its first miss: the same box two frames later is a new track
    "tentative_dies": ({}, [[_row()], [], [_row()]], [([1], [1]), ([], []), ([2], [1])]),
    # confirmed, then max_age = 3 misses survived, freed on the fourth: the box is a new track afterwards
    "max_age": (dict(max_age=3), [[_row()]] * 3 + [[]] * 3 + [[_row()]] + [[]] * 4 + [[_row()]],
                [([1], [1]), ([1], [1]), ([1], [2]), ([], []), ([], []), ([], []), ([1], [2]), ([], []), ([], []), ([], []), ([], []),
                 ([2], [1])]),
    # the same box in another class matches nothing: the tentative track dies and the row is born into the slot it leaves
    "class_gate": ({}, [[_row(cls=0)], [_row(cls=1)]], [([1], [1]), ([2], [1])]),
    # IoU exactly 1/2 with iou_thresh 0.5 matches: (0..20) x (5..15) against (0..10) x (5..15): 100 / (200 + 100 - 100)
    "iou_equal": (dict(iou_thresh=0.5), [[_row((10.0, 10.0, 20.0, 10.0))], [_row((5.0, 10.0, 10.0, 10.0))]], [([1], [1]), ([1], [1])]),
    # two identical tracks, THREE identical rows: all six affinities are 1; slot 0 takes row 0, slot 1 row 1, and row 2 is left to
    # be born (any other tie rule leaves another row over).  Frame 0 also shows births in row order.
    "tie": ({}, [[_row(), _row()], [_row(), _row(), _row()]], [([1, 2], [1, 1]), ([1, 2, 3], [1, 1, 1])]),
    # a confirmed track is kept alive by a 0.3 row in stage two
    "stage_two": ({}, [[_row()]] * 3 + [[_row(prob=0.3)]], [([1], [1]), ([1], [1]), ([1], [2]), ([1], [2])]),
    # stage two refuses a poor overlap: a 0.3 row shifted by 24 of 40 px has IoU 16/64 = 0.25 < 0.3, the confirmed track misses
    "stage_two_poor_overlap": ({}, [[_row()]] * 3 + [[_row((124.0, 100.0, 40.0, 20.0), prob=0.3)]],
                               [([1], [1]), ([1], [1]), ([1], [2]), ([-1], [0])]),
    # a low row never gives birth; nor does it match a tentative track
    "low_no_birth": ({}, [[_row(prob=0.3)], [_row()], [_row(prob=0.3)]], [([-1], [0]), ([1], [1]), ([-1], [0])]),
    # a box whose height grows: the measurement noise follows the PREDICTED height
    "growing": ({}, [[_row((100.0, 100.0, 40.0, 20.0 + 4.0 * k))] for k in range(4)], [([1], [1]), ([1], [1]), ([1], [2]), ([1], [2])]),
}


def scene(seed):
    """60 frames of four objects -> (frames, labels): labels[f][j] is the object (0..3) row j of frame f shows, -1 for clutter.
    Objects 0 and 1 (class 0) cross on rows 25 px apart; 2 (class 1) and 3 (class 2) travel almost on top of each other.
    Object 2 is absent in frames 20-24, object 0 is at prob 0.3 in frames 10-13; every frame has three prob-0.2 clutter rows
    below everything else.  Coordinates are jittered by uniform +-1 px; rows are shuffled."""
    rs = np.random.RandomState(1000 + seed)
    start = [(100.0, 200.0, 60.0, 40.0), (700.0, 225.0, 60.0, 40.0), (300.0, 100.0, 50.0, 50.0), (302.0, 101.0, 50.0, 50.0)]
    vel = [(10.0, 0.0, 0.0, 0.0), (-10.0, 0.0, 0.0, 0.0), (3.0, 1.0, 0.5, 0.5), (3.0, 1.0, 0.5, 0.5)]
    klass = [0, 0, 1, 2]
    frames, labels = [], []
    for f in range(60):
        rows = []
        for o in range(4):
            if o == 2 and 20 <= f <= 24:
                continue
            box = [start[o][c] + vel[o][c] * f + rs.uniform(-1.0, 1.0) for c in range(4)]
            rows.append((tuple(box) + (0.3 if o == 0 and 10 <= f <= 13 else 0.9, klass[o]), o))
        for _ in range(3):
            box = (rs.uniform(50.0, 1200.0), rs.uniform(320.0, 360.0), rs.uniform(20.0, 60.0), rs.uniform(20.0, 30.0))
            rows.append((box + (0.2, int(rs.randint(3))), -1))
        order = rs.permutation(len(rows))
        frames.append([rows[k][0] for k in order])
        labels.append([rows[k][1] for k in order])
    return frames, labels


def check_scene(ids_per_frame, labels, next_id):
    """The scene's three conditions; raises AssertionError."""
    seen = {}
    for f, (ids, lab) in enumerate(zip(ids_per_frame, labels)):
        for j, o in enumerate(lab):
            if o < 0:
                assert ids[j] == -1, "frame %d: clutter row %d carries id %d" % (f, j, ids[j])
            elif ids[j] != -1:
                assert seen.setdefault(o, int(ids[j])) == ids[j], "frame %d: object %d switched from id %d to %d" % (f, o, seen[o], ids[j])
    assert sorted(seen) == [0, 1, 2, 3] and len(set(seen.values())) == 4, seen
    assert next_id == 5, "ids issued: next_id = %d" % next_id
