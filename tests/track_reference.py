"""NumPy / Python float64 restatement of the tracker of include/sqdet.h ("tracking"), for the tests of squeezedet_amd.track.  It
is SEQUENTIAL and plain -- one slot, one row, one pair at a time, in ascending index -- where the kernel works a wave at a time,
so the two share no structure.  Every arithmetic expression is one IEEE operation per Python operator on Python floats
(float64), in the order the header writes it; the kernel is built without contraction, so tables and outputs agree bit for bit.

``Tables(S)`` holds what the device tables hold; ``step(tables, s, boxes, probs, cls, count, params)`` is one frame of one stream;
``run(tables, boxes, probs, cls, counts, frames, params)`` a whole sqdet_track_update call.  ``mutate`` names one deliberate
deviation (MUTATIONS) for the mutation checks of tests/test_track_host.py."""
import math

import numpy as np

CAP = 64
DEFAULTS = dict(iou_thresh=0.3, high_thresh=0.5, low_thresh=0.1, min_hits=3, max_age=30, w_pos=1.0 / 20, w_vel=1.0 / 160)
MUTATIONS = ("no_stage_two", "strict_threshold", "births_descending", "no_slot_reuse", "noise_before_predict", "ties_to_higher")
INT_FIELDS = ("cls", "id", "state", "hits", "miss", "age")


def params(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


class Tables:
    """x float64 [S,64,4,2], P float64 [S,64,4,3], cls / id / state / hits / miss / age int32 [S,64], score float32 [S,64],
    next_id / dropped int32 [S] -- after a reset."""

    def __init__(self, S):
        self.S = S
        self.x = np.zeros((S, CAP, 4, 2), np.float64)
        self.P = np.zeros((S, CAP, 4, 3), np.float64)
        for f in INT_FIELDS:
            setattr(self, f, np.zeros((S, CAP), np.int32))
        self.score = np.zeros((S, CAP), np.float32)
        self.next_id = np.ones(S, np.int32)
        self.dropped = np.zeros(S, np.int32)

    def arrays(self):
        d = {"x": self.x, "P": self.P, "score": self.score, "next_id": self.next_id, "dropped": self.dropped}
        d.update({f: getattr(self, f) for f in INT_FIELDS})
        return d

    def copy(self):
        t = Tables(self.S)
        for k, v in self.arrays().items():
            getattr(t, k)[...] = v
        return t

    def tracks(self, s):
        """The live slots of stream s: a list of dicts, ascending slot."""
        out = []
        for t in range(CAP):
            if self.state[s, t] != 0:
                out.append(dict(slot=t, id=int(self.id[s, t]), cls=int(self.cls[s, t]), state=int(self.state[s, t]),
                                hits=int(self.hits[s, t]), miss=int(self.miss[s, t]), age=int(self.age[s, t]),
                                score=float(self.score[s, t]), box=tuple(float(v) for v in self.x[s, t, :, 0]),
                                velocity=tuple(float(v) for v in self.x[s, t, :, 1])))
        return out


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if b > a else a


def iou(b1, b2):
    """util.iou of the reference (utils/util.py) on Python floats."""
    lr = _min(b1[0] + 0.5 * b1[2], b2[0] + 0.5 * b2[2]) - _max(b1[0] - 0.5 * b1[2], b2[0] - 0.5 * b2[2])
    if lr > 0:
        tb = _min(b1[1] + 0.5 * b1[3], b2[1] + 0.5 * b2[3]) - _max(b1[1] - 0.5 * b1[3], b2[1] - 0.5 * b2[3])
        if tb > 0:
            inter = lr * tb
            return inter / (b1[2] * b1[3] + b2[2] * b2[3] - inter)
    return 0.0


def _greedy(M, slots, rows, thresh, strict, ties_high=False):
    """[(slot, row)] in the order taken: the free pair with the largest M, ties to the lower slot, then the lower row, while
    that M >= thresh."""
    slots, rows, taken = list(slots), list(rows), []
    while True:
        best, bt, bd = -1.0, -1, -1
        for t in slots:
            for d in rows:
                if M[t][d] > best or (ties_high and M[t][d] == best):
                    best, bt, bd = M[t][d], t, d
        if bt < 0 or (best <= thresh if strict else not best >= thresh):
            return taken
        taken.append((bt, bd))
        slots.remove(bt)
        rows.remove(bd)


def step(T, s, boxes, probs, cls, count, p, mutate=None):
    """One frame of stream s.  boxes float32 [rows,4], probs float32 [rows], cls int32 [rows] -> (det_track_id, det_track_state)
    int32 [rows]."""
    assert mutate is None or mutate in MUTATIONS
    rows = int(boxes.shape[0])
    assert rows <= CAP
    x, P = T.x[s], T.P[s]
    w_pos, w_vel = float(p["w_pos"]), float(p["w_vel"])
    out_id, out_state = np.full(rows, -1, np.int32), np.zeros(rows, np.int32)
    count = min(max(int(count), 0), rows)                                              # 1
    live = [t for t in range(CAP) if T.state[s, t] != 0]
    pred, r_before = {}, {}
    for t in live:                                                                     # 2
        h = _max(float(x[t, 3, 0]), 1.0)
        r_before[t] = (w_pos * h) * (w_pos * h)
        qp = (w_pos * h) * (w_pos * h)
        qv = (w_vel * h) * (w_vel * h)
        for c in range(4):
            pp, pv, vv = (float(v) for v in P[t, c])
            x[t, c, 0] = float(x[t, c, 0]) + float(x[t, c, 1])
            P[t, c, 0] = ((pp + pv) + (pv + vv)) + qp
            P[t, c, 1] = pv + vv
            P[t, c, 2] = vv + qv
        T.age[s, t] += 1
        pred[t] = (float(x[t, 0, 0]), float(x[t, 1, 0]), _max(float(x[t, 2, 0]), 1.0), _max(float(x[t, 3, 0]), 1.0))
    z = [[float(v) for v in boxes[d]] for d in range(rows)]                            # 3 (float32 widened: exact)
    pr = [float(probs[d]) for d in range(rows)]
    valid = [d for d in range(count) if all(math.isfinite(v) for v in z[d]) and math.isfinite(pr[d]) and z[d][2] > 0 and z[d][3] > 0]
    high = [d for d in valid if pr[d] > p["high_thresh"]]
    low = [d for d in valid if p["low_thresh"] < pr[d] <= p["high_thresh"]]
    M = {t: {d: (iou(pred[t], z[d]) if int(cls[d]) == int(T.cls[s, t]) else 0.0) for d in valid} for t in live}      # 4
    strict = mutate == "strict_threshold"
    ties_high = mutate == "ties_to_higher"
    pairs = _greedy(M, live, high, p["iou_thresh"], strict, ties_high)                            # 5
    if mutate != "no_stage_two":
        rest = [t for t in live if t not in [a for a, _ in pairs] and T.state[s, t] == 2]
        pairs += _greedy(M, rest, low, p["iou_thresh"], strict, ties_high)
    matched_rows = [d for _, d in pairs]
    for t, d in sorted(pairs):                                                         # 6
        h = _max(float(x[t, 3, 0]), 1.0)
        r = r_before[t] if mutate == "noise_before_predict" else (w_pos * h) * (w_pos * h)
        for c in range(4):
            pc, vc = float(x[t, c, 0]), float(x[t, c, 1])
            pp, pv, vv = (float(v) for v in P[t, c])
            y = z[d][c] - pc
            sden = pp + r
            kp = pp / sden
            kv = pv / sden
            x[t, c, 0] = pc + kp * y
            x[t, c, 1] = vc + kv * y
            P[t, c, 0] = pp - kp * pp
            P[t, c, 1] = pv - kp * pv
            P[t, c, 2] = vv - kv * pv
        T.hits[s, t] += 1
        T.miss[s, t] = 0
        T.score[s, t] = probs[d]
        if T.state[s, t] == 1 and T.hits[s, t] >= p["min_hits"]:
            T.state[s, t] = 2
        out_id[d], out_state[d] = T.id[s, t], T.state[s, t]
    free_before = [t for t in range(CAP) if T.state[s, t] == 0]
    for t in live:                                                                     # 7
        if t not in [a for a, _ in pairs]:
            T.miss[s, t] += 1
            if T.state[s, t] == 1 or T.miss[s, t] > p["max_age"]:
                T.state[s, t] = 0
    births = [d for d in high if d not in matched_rows]                                # 8
    if mutate == "births_descending":
        births.reverse()
    for d in births:
        free = [t for t in (free_before if mutate == "no_slot_reuse" else range(CAP)) if T.state[s, t] == 0]
        if not free:
            T.dropped[s] += 1
            continue
        t = free[0]
        h = _max(z[d][3], 1.0)
        a = (2.0 * w_pos) * h
        b = (10.0 * w_vel) * h
        for c in range(4):
            x[t, c] = (z[d][c], 0.0)
            P[t, c] = (a * a, 0.0, b * b)
        T.cls[s, t], T.id[s, t] = cls[d], T.next_id[s]
        T.next_id[s] += 1
        T.hits[s, t], T.miss[s, t], T.age[s, t], T.score[s, t] = 1, 0, 1, probs[d]
        T.state[s, t] = 2 if p["min_hits"] <= 1 else 1
        out_id[d], out_state[d] = T.id[s, t], T.state[s, t]
    return out_id, out_state                                                           # 9: everything else keeps -1 / 0


def run(T, boxes, probs, cls, counts, frames, p, mutate=None):
    """A whole call: n = S*frames images, image s*frames + f = frame f of stream s -> (det_track_id, det_track_state) [n, rows]."""
    n, rows = int(boxes.shape[0]), int(boxes.shape[1])
    assert n == T.S * frames
    ids, sts = np.full((n, rows), -1, np.int32), np.zeros((n, rows), np.int32)
    for s in range(T.S):
        for f in range(frames):
            i = s * frames + f
            ids[i], sts[i] = step(T, s, boxes[i], probs[i], cls[i], counts[i], p, mutate)
    return ids, sts


def track_items(boxes, probs, cls, counts, ids, states, names, palette, plot_thresh, anchor="bottom_left"):
    """sqdet_track_build_items restated: per image the item tuples of tests/draw_reference.py."""
    from tests import draw_reference as R
    out = []
    for i in range(boxes.shape[0]):
        items = []
        for j in range(min(max(int(counts[i]), 0), boxes.shape[1])):
            if states[i, j] == 2 and ids[i, j] > 0 and float(probs[i, j]) > plot_thresh:
                c = int(cls[i, j])
                name = names[c] if 0 <= c < len(names) else "?"
                items.append(R.box_item(boxes[i, j], tuple(int(v) for v in palette[int(ids[i, j]) % len(palette)]),
                                        "%s #%d" % (name, int(ids[i, j])), anchor))
        out.append(items)
    return out
