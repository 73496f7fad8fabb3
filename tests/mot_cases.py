"""Inputs for the tracking-evaluation tests, shared by the host tests (tests/test_mot_host.py: the NumPy restatement against
hand-worked numbers) and the GPU tests (tests/test_gpu_mot.py: the kernels against the restatement, bit for bit).

A FRAME is (objects, hypotheses): an object is (id, cls, flags, (cx, cy, w, h)), a hypothesis (id, cls, (cx, cy, w, h)) -- a
confirmed row -- or (id, cls, box, state).  ``pack(frames, rows, G)`` turns frames into the arrays of sqdet_mot_update;
``CASES``: name -> (classes, frames, expected overall counters, expected per-class counters {cls: {...}}).

Boxes are 40 x 20; two of them dx apart along x have IoU (40 - dx) / (40 + dx): 2 -> 38/42, 8 -> 32/48, 10 -> 30/50 = 0.6,
22 -> 18/62 (below 0.5)."""
import numpy as np


def B(x, y=100.0):
    return (float(x), float(y), 40.0, 20.0)


def pack(frames, rows, G):
    """-> (boxes float32 [n,rows,4], cls int32 [n,rows], counts int32 [n], ids int32 [n,rows], states int32 [n,rows]) and
    gt = (gt_box float64 [n,G,4], gt_id, gt_cls, gt_flags int32 [n,G], gt_count int32 [n]).  Rows past a frame's count hold a
    decoy -- a confirmed id-9999 box on top of everything -- that must never be read."""
    n = len(frames)
    boxes = np.tile(np.asarray(B(100.0), np.float32), (n, rows, 1))
    cls, ids, states = np.zeros((n, rows), np.int32), np.full((n, rows), 9999, np.int32), np.full((n, rows), 2, np.int32)
    counts = np.zeros(n, np.int32)
    gt_box = np.tile(np.asarray(B(100.0), np.float64), (n, G, 1))
    gt_id, gt_cls, gt_flags = np.full((n, G), 8888, np.int32), np.zeros((n, G), np.int32), np.zeros((n, G), np.int32)
    gt_count = np.zeros(n, np.int32)
    for i, (objs, hyps) in enumerate(frames):
        counts[i], gt_count[i] = len(hyps), len(objs)
        for j, h in enumerate(hyps):
            ids[i, j], cls[i, j], boxes[i, j] = h[0], h[1], h[2]
            states[i, j] = h[3] if len(h) > 3 else 2
        for j, o in enumerate(objs):
            gt_id[i, j], gt_cls[i, j], gt_flags[i, j], gt_box[i, j] = o
    return (boxes, cls, counts, ids, states), (gt_box, gt_id, gt_cls, gt_flags, gt_count)


def _obj(ident, x, cls=0, flags=0):
    return (ident, cls, flags, B(x))


def _hyp(ident, x, cls=0):
    return (ident, cls, B(x))


_half = ([(1, 0, 0, (10.0, 10.0, 20.0, 10.0))], [(1, 0, (5.0, 10.0, 10.0, 10.0))])

# name -> (classes, frames, expected overall counters, expected per-class counters)
CASES = {
    # one object, one hypothesis, five frames on top of each other
    "perfect": (1, [([_obj(7, 0)], [_hyp(3, 0)])] * 5,
                dict(tp=5, fn=0, fp=0, idsw=0, frag=0, mt=1, pt=0, ml=0, idtp=5, idfn=0, idfp=0, gt_ids=1, hyp_ids=1, iou_sum=5.0), {}),
    # the hypothesis id changes after three of five frames: one switch; IDF1 keeps the longer half: 2*3 / (6 + 2 + 2)
    "one_switch": (1, [([_obj(7, 0)], [_hyp(1, 0)])] * 3 + [([_obj(7, 0)], [_hyp(2, 0)])] * 2,
                   dict(tp=5, fn=0, fp=0, idsw=1, frag=0, mt=1, idtp=3, idfn=2, idfp=2, hyp_ids=2), {}),
    # a track that changes id half-way, six frames then four: ID switches 1, IDF1 from the longer half: 12 / (12 + 4 + 4)
    "id_change_halfway": (1, [([_obj(1, 0)], [_hyp(5, 0)])] * 6 + [([_obj(1, 0)], [_hyp(6, 0)])] * 4,
                          dict(tp=10, idsw=1, idtp=6, idfn=4, idfp=4, mt=1), {}),
    # frame 0 pairs A-h1 and B-h2 far apart.  In frame 1 A is at 0, B at 10, h1 at 8, h2 at 2: the assignment alone would take
    # A-h2 and B-h1 (38/42 each) and count two switches; continuity keeps A-h1 and B-h2 (32/48 each, allowed)
    "continuity": (1, [([_obj(1, 0), _obj(2, 300)], [_hyp(1, 0), _hyp(2, 300)]), ([_obj(1, 0), _obj(2, 10)], [_hyp(1, 8), _hyp(2, 2)])],
                   dict(tp=4, fn=0, fp=0, idsw=0, idtp=4, iou_sum=2.0 + 2 * (32.0 * 20.0) / (48.0 * 20.0)), {}),
    # o1 at 2, o2 at -10, h1 at 0, h2 at 12: o1-h1 38/42, o1-h2 0.6, o2-h1 0.6, o2-h2 18/62 < 0.5.  Greedy takes o1-h1 and is left
    # with a pair that is not allowed; the optimum has two matches
    "greedy_vs_optimal": (1, [([_obj(1, 2), _obj(2, -10)], [_hyp(1, 0), _hyp(2, 12)])], dict(tp=2, fn=0, fp=0, iou_sum=0.6 + 0.6), {}),
    # matched, matched, missed twice, matched twice: one fragmentation, no switch, 4 of 6 is partly tracked
    "fragmentation": (1, [([_obj(1, 0)], [_hyp(1, 0)])] * 2 + [([_obj(1, 0)], [])] * 2 + [([_obj(1, 0)], [_hyp(1, 0)])] * 2,
                      dict(tp=4, fn=2, fp=0, idsw=0, frag=1, mt=0, pt=1, ml=0, idtp=4, idfn=2, idfp=0), {}),
    # matched to 1, missed, matched to 2: the `last` of two frames ago still makes it a switch (and a fragmentation)
    "switch_after_miss": (1, [([_obj(1, 0)], [_hyp(1, 0)]), ([_obj(1, 0)], []), ([_obj(1, 0)], [_hyp(2, 0)])],
                          dict(tp=2, fn=1, fp=0, idsw=1, frag=1, idtp=1, idfn=2, idfp=1), {}),
    # object 1: 4 of 5 frames -- exactly 4/5, mostly tracked; object 2: 1 of 6 -- just under 1/5, mostly lost; object 3: 1 of 5 --
    # exactly 1/5, partly tracked
    "mt_ml": (1, [([_obj(1, 0), _obj(2, 200), _obj(3, 400)], [_hyp(1, 0), _hyp(2, 200), _hyp(3, 400)])] +
              [([_obj(1, 0), _obj(2, 200), _obj(3, 400)], [_hyp(1, 0)])] * 3 + [([_obj(1, 0), _obj(2, 200), _obj(3, 400)], [])] +
              [([_obj(2, 200)], [])],
              dict(tp=6, fn=10, fp=0, mt=1, pt=1, ml=1, frag=0, gt_ids=3, hyp_ids=3), {}),
    # an ignored region swallows the hypothesis on it: neither a false positive nor a frame of its identity; the ignored object is
    # no miss either.  Object 1 and hypothesis 1 are an ordinary match beside it
    "ignored_swallows": (1, [([_obj(50, 0, flags=1), _obj(1, 300), _obj(51, 600, flags=1)], [_hyp(9, 0), _hyp(1, 300)])],
                         dict(tp=1, fn=0, fp=0, ignored_hyp=1, idtp=1, idfp=0, idfn=0, gt_ids=1, hyp_ids=2), {}),
    # the same box in another class matches nothing
    "class_gate": (2, [([_obj(1, 0, cls=0)], [_hyp(1, 0, cls=1)])], dict(tp=0, fn=1, fp=1),
                   {0: dict(fn=1, fp=0, gt_ids=1, hyp_ids=0), 1: dict(fn=0, fp=1, gt_ids=0, hyp_ids=1)}),
    # IoU exactly 1/2 (the tracker's iou_equal boxes) is allowed at iou_thresh 0.5
    "iou_half": (1, [_half], dict(tp=1, fn=0, fp=0, iou_sum=0.5), {}),
    # frame 0: A-h1.  Frame 1: h1 (32/48) and h2 (38/42) both on A; continuity keeps h1, h2 is a false positive -- but the pair
    # A-h2 is allowed and counts in `overlap`.  Frames 2-4: h2 alone.  overlap[A][h1] = 2, overlap[A][h2] = 4: idtp = 4
    "overlap_unmatched": (1, [([_obj(1, 0)], [_hyp(1, 8)]), ([_obj(1, 0)], [_hyp(1, 8), _hyp(2, 2)])] + [([_obj(1, 0)], [_hyp(2, 2)])] * 3,
                          dict(tp=5, fn=0, fp=1, idsw=1, idtp=4, idfn=1, idfp=2), {}),
}

# mutation of tests/mot_reference.py -> the case it must fail
MUTATION_CASE = {"strict_threshold": "iou_half", "no_continuity": "continuity", "greedy": "greedy_vs_optimal",
                 "forget_last": "switch_after_miss", "overlap_matched_only": "overlap_unmatched", "ignored_as_fp": "ignored_swallows"}


def scene_frames(seed):
    """tests/track_cases.scene(seed) run through the tracker's restatement -> (frames, labelled rows): the labelled rows are the
    objects (id = object + 1), the confirmed rows the hypotheses."""
    from tests import track_cases as TC
    from tests import track_reference as TR
    rows_per_frame, labels = TC.scene(seed)
    boxes, probs, cls, counts = TC.pack(rows_per_frame, 8)
    ids, sts = TR.run(TR.Tables(1), boxes, probs, cls, counts, len(rows_per_frame), TR.params())
    frames, labelled = [], 0
    for f, lab in enumerate(labels):
        objs = [(o + 1, int(cls[f, j]), 0, tuple(float(v) for v in boxes[f, j])) for j, o in enumerate(lab) if o >= 0]
        hyps = [(int(ids[f, j]), int(cls[f, j]), tuple(float(v) for v in boxes[f, j]), int(sts[f, j])) for j in range(int(counts[f]))]
        labelled += len(objs)
        frames.append((objs, hyps))
    return frames, labelled


def dense_frames(rs, n_obj, n_hyp, n_frames=3):
    """One class, boxes jittered around a 4-px grid so that a row has many allowed pairs; hypothesis ids are shuffled from frame to
    frame so that continuity leaves a good part to the assignment; a few objects are ignored."""
    frames = []
    cx = [200.0 + 4.0 * (k % 8) for k in range(64)]
    cy = [150.0 + 4.0 * (k // 8) for k in range(64)]
    for f in range(n_frames):
        objs = [(k + 1, 0, 1 if rs.rand() < 0.1 else 0,
                 (cx[k] + rs.uniform(-2, 2), cy[k] + rs.uniform(-2, 2), rs.uniform(38, 46), rs.uniform(38, 46))) for k in range(n_obj)]
        perm = rs.permutation(n_hyp) if f % 2 else np.arange(n_hyp)
        hyps = [(int(perm[k]) + 1, 0, (cx[k] + rs.uniform(-3, 3), cy[k] + rs.uniform(-3, 3), rs.uniform(36, 48), rs.uniform(36, 48)))
                for k in range(n_hyp)]
        frames.append((objs, hyps))
    return frames


def random_frames(rs, n_frames, n_obj, classes=3, extent=900.0):
    """Objects on straight lines; a hypothesis follows each with jitter, drops out, changes id now and then; strays and ignored
    regions are sprinkled in."""
    obj = [(rs.uniform(0, extent), rs.uniform(0, extent / 2), rs.uniform(30, 60), rs.uniform(30, 60), rs.uniform(-5, 5), rs.uniform(-2, 2),
            int(rs.randint(classes))) for _ in range(n_obj)]
    hyp_id = list(range(1, n_obj + 1))
    next_id = n_obj + 1
    frames = []
    for f in range(n_frames):
        objs, hyps = [], []
        for k, (x, y, w, h, vx, vy, c) in enumerate(obj):
            if rs.rand() < 0.1:
                continue
            box = (x + vx * f, y + vy * f, w, h)
            objs.append((k + 1, c, 1 if rs.rand() < 0.05 else 0, box))
            if rs.rand() < 0.07:
                hyp_id[k], next_id = next_id, next_id + 1
            if rs.rand() < 0.85:
                hyps.append((hyp_id[k], c if rs.rand() < 0.95 else (c + 1) % classes,
                             (box[0] + rs.uniform(-6, 6), box[1] + rs.uniform(-6, 6), w + rs.uniform(-4, 4), h + rs.uniform(-4, 4)),
                             2 if rs.rand() < 0.9 else 1))
        for _ in range(int(rs.randint(3))):
            hyps.append((next_id, int(rs.randint(classes)), (rs.uniform(0, extent), rs.uniform(0, extent / 2), 40.0, 40.0)))
            next_id += 1
        order = rs.permutation(len(hyps))
        frames.append((objs, [hyps[k] for k in order]))
    return frames


def sparse_overlap(rs, G, T, classes=3, per_row=6):
    """A random table state for sqdet_mot_evaluate alone: G object and T hypothesis identities, a few overlaps per row with many
    equal values (ties), consistent present / tracked / frames counts.  -> dict of host arrays in the layout of State.arrays()."""
    from tests import mot_reference as R
    d = R.State(1, classes).arrays()
    d["n_obj"][0], d["n_hyp"][0] = G, T
    d["obj_id"][0, :G] = 1 + rs.permutation(G)
    d["hyp_id"][0, :T] = 1 + rs.permutation(T)
    d["obj_cls"][0, :G] = rs.randint(classes, size=G)
    d["hyp_cls"][0, :T] = rs.randint(classes, size=T)
    for g in range(G):
        for t in rs.choice(T, size=min(per_row, T), replace=False):
            d["overlap"][0, g, t] = rs.randint(1, 5)
    d["obj_present"][0, :G] = d["overlap"][0, :G].max(1) + rs.randint(0, 30, size=G)
    d["obj_tracked"][0, :G] = (d["obj_present"][0, :G] * rs.rand(G)).astype(np.int32)
    d["obj_frag"][0, :G] = rs.randint(0, 3, size=G)
    d["hyp_frames"][0, :T] = d["overlap"][0, :, :T].max(0) + rs.randint(0, 10, size=T)
    d["counts"][0] = rs.randint(0, 1000, size=(classes, 5))
    d["iou_sum"][0] = rs.rand(classes) * 100
    return d
