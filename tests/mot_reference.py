"""NumPy / Python restatement of the tracking evaluation of include/sqdet.h ("tracking evaluation"), for the tests of
squeezedet_amd.mot.  It is SEQUENTIAL and plain -- one stream, one frame, one object, one pair at a time, in ascending row index,
with dictionaries where the device has dense tables -- where the kernels work a wave (sqdet_mot_update) or a workgroup
(sqdet_mot_evaluate) at a time.  Every floating expression is one IEEE float64 operation per Python operator in the order the
header writes it; mot_eval.hip is built without contraction, so every counter, iou_sum and every table agree bit for bit.

``assign(cost)`` is THE assignment of the definition (optimal assignments are not unique: the pairs are part of it).
``State(S, classes)`` holds what the device tables hold; ``step`` is one frame of one stream, ``run`` a whole sqdet_mot_update
call, ``evaluate`` sqdet_mot_evaluate, ``metrics`` the derived figures.  ``mutate`` names one deliberate deviation (MUTATIONS)
for the mutation checks of tests/test_mot_host.py."""
import math

import numpy as np

from tests.track_reference import iou

CAP = 64
MAX_OBJ, MAX_HYP, MAX_CLASSES = 256, 1024, 128
BIG = 1 << 32
INF = 1 << 62
SCALE = 1048576.0
STATUS_OBJ, STATUS_HYP = 1, 2
COUNTERS = ("tp", "fn", "fp", "idsw", "ignored_hyp", "frag", "mt", "pt", "ml", "idtp", "idfn", "idfp", "gt_ids", "hyp_ids")
K = len(COUNTERS)
MUTATIONS = ("strict_threshold", "no_continuity", "greedy", "forget_last", "overlap_matched_only", "ignored_as_fp")


def assign(cost):
    """cost: int64 [R, C], R <= C -> row_of_col int [C] (-1: free).  Shortest augmenting paths with integer potentials: rows are
    inserted in ascending order; in every round the unscanned column of smallest reduced distance is taken, the lowest index
    among equals; the path ends at the first free column taken."""
    cost = np.asarray(cost, np.int64)
    R, C = cost.shape
    assert R <= C
    u, v = np.zeros(R, np.int64), np.zeros(C, np.int64)
    p = np.full(C, -1, np.int64)
    for i in range(R):
        minv, way, used = np.full(C, INF, np.int64), np.full(C, -1, np.int64), np.zeros(C, bool)
        i0, j0 = i, -1
        while True:
            if j0 >= 0:
                used[j0] = True
            free = ~used
            cur = cost[i0] - u[i0] - v
            better = free & (cur < minv)
            minv[better], way[better] = cur[better], j0
            j1 = int(np.argmin(np.where(free, minv, INF)))                    # the first of the smallest
            delta = minv[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            u[i] += delta
            j0 = j1
            if p[j0] < 0:
                break
            i0 = int(p[j0])
        while j0 >= 0:
            w = int(way[j0])
            p[j0] = p[w] if w >= 0 else i
            j0 = w
    return p


def _greedy_assign(cost):
    """(mutation) the cheapest free cell first, the lower row, then the lower column among equals."""
    cost = np.asarray(cost, np.int64)
    R, C = cost.shape
    p = np.full(C, -1, np.int64)
    rows, cols = list(range(R)), list(range(C))
    while rows:
        _, i, j = min((cost[i, j], i, j) for i in rows for j in cols)
        p[j] = i
        rows.remove(i)
        cols.remove(j)
    return p


class State:
    """Per stream: obj / hyp identity tables in dense order, the per-frame counters [classes, 5], iou_sum [classes], overlap
    {(g, t): frames} and the status word."""

    def __init__(self, S, classes):
        self.S, self.classes = S, classes
        self.obj = [[] for _ in range(S)]        # dicts: id, cls, last, present, tracked, frag, run
        self.hyp = [[] for _ in range(S)]        # dicts: id, cls, frames
        self.counts = np.zeros((S, classes, 5), np.int64)
        self.iou_sum = np.zeros((S, classes), np.float64)
        self.overlap = [dict() for _ in range(S)]
        self.status = np.zeros(S, np.int32)

    def arrays(self):
        """The device tables (squeezedet_amd.mot.table_shapes) as NumPy arrays."""
        S = self.S
        d = {f: np.zeros((S, MAX_OBJ), np.int32) for f in ("obj_id", "obj_cls", "obj_last", "obj_present", "obj_tracked", "obj_frag", "obj_run")}
        d.update({f: np.zeros((S, MAX_HYP), np.int32) for f in ("hyp_id", "hyp_cls", "hyp_frames")})
        d.update(n_obj=np.zeros(S, np.int32), n_hyp=np.zeros(S, np.int32), status=self.status.copy(), counts=self.counts.copy(),
                 iou_sum=self.iou_sum.copy(), overlap=np.zeros((S, MAX_OBJ, MAX_HYP), np.int32))
        for s in range(S):
            d["n_obj"][s], d["n_hyp"][s] = len(self.obj[s]), len(self.hyp[s])
            for k, o in enumerate(self.obj[s]):
                for f in ("id", "cls", "last", "present", "tracked", "frag", "run"):
                    d["obj_" + f][s, k] = o[f]
            for k, h in enumerate(self.hyp[s]):
                d["hyp_id"][s, k], d["hyp_cls"][s, k], d["hyp_frames"][s, k] = h["id"], h["cls"], h["frames"]
            for (g, t), n in self.overlap[s].items():
                d["overlap"][s, g, t] = n
        return d


def _valid(box, ident, cls, classes, seen):
    if not (ident > 0 and all(math.isfinite(v) for v in box) and box[2] > 0 and box[3] > 0 and 0 <= cls < classes):
        return False
    if ident in seen:                      # a lower valid row of the frame carries the identity
        return False
    seen.add(ident)
    return True


def step(st, s, boxes, cls, count, ids, states, gt_box, gt_id, gt_cls, gt_flags, gt_count, iou_thresh=0.5, mutate=None):
    """One frame of stream s.  -> {object row: hypothesis row} of the frame's matches (ignored objects included)."""
    assert mutate is None or mutate in MUTATIONS
    if st.status[s]:
        return {}
    rows, G = int(boxes.shape[0]), int(gt_box.shape[0])
    assert rows <= CAP and G <= CAP
    seen, hyps = set(), []
    for j in range(min(max(int(count), 0), rows)):
        b = [float(v) for v in boxes[j]]
        if int(states[j]) == 2 and _valid(b, int(ids[j]), int(cls[j]), st.classes, seen):
            hyps.append(dict(row=j, box=b, id=int(ids[j]), cls=int(cls[j])))
    seen, objs = set(), []
    for j in range(min(max(int(gt_count), 0), G)):
        b = [float(v) for v in gt_box[j]]
        if _valid(b, int(gt_id[j]), int(gt_cls[j]), st.classes, seen):
            objs.append(dict(row=j, box=b, id=int(gt_id[j]), cls=int(gt_cls[j]), ignore=bool(int(gt_flags[j]) & 1)))
    # 5: dense indices, objects before hypotheses, each in row order; one more than a table holds stops the stream
    obj_index = {o["id"]: k for k, o in enumerate(st.obj[s])}
    hyp_index = {h["id"]: k for k, h in enumerate(st.hyp[s])}
    new_obj = [o for o in objs if not o["ignore"] and o["id"] not in obj_index]
    new_hyp = [h for h in hyps if h["id"] not in hyp_index]
    if len(st.obj[s]) + len(new_obj) > MAX_OBJ:
        st.status[s] |= STATUS_OBJ
    if len(st.hyp[s]) + len(new_hyp) > MAX_HYP:
        st.status[s] |= STATUS_HYP
    if st.status[s]:
        return {}
    for o in new_obj:
        obj_index[o["id"]] = len(st.obj[s])
        st.obj[s].append(dict(id=o["id"], cls=o["cls"], last=0, present=0, tracked=0, frag=0, run=0))
    for h in new_hyp:
        hyp_index[h["id"]] = len(st.hyp[s])
        st.hyp[s].append(dict(id=h["id"], cls=h["cls"], frames=0))
    # 1: IoU, allowed pairs and their integer cost
    nO, nH = len(objs), len(hyps)
    V = [[iou(o["box"], h["box"]) if o["cls"] == h["cls"] else 0.0 for h in hyps] for o in objs]
    if mutate == "strict_threshold":
        allowed = [[V[a][b] > iou_thresh for b in range(nH)] for a in range(nO)]
    else:
        allowed = [[V[a][b] >= iou_thresh for b in range(nH)] for a in range(nO)]
    q = [[int(math.floor((1.0 - V[a][b]) * SCALE)) if allowed[a][b] else BIG for b in range(nH)] for a in range(nO)]
    match = {}                                                                          # object index -> hypothesis index
    taken = set()
    # 2: continuity
    if mutate != "no_continuity":
        for a, o in enumerate(objs):
            if o["ignore"]:
                continue
            last = st.obj[s][obj_index[o["id"]]]["last"]
            if last > 0:
                for b, h in enumerate(hyps):
                    if h["id"] == last:
                        if b not in taken and allowed[a][b]:
                            match[a] = b
                            taken.add(b)
                        break
    # 3: optimal assignment of the rest, compacted in order
    ro = [a for a in range(nO) if a not in match]
    rh = [b for b in range(nH) if b not in taken]
    if ro and rh:
        N = max(len(ro), len(rh))
        cost = np.full((N, N), BIG, np.int64)
        for i, a in enumerate(ro):
            for j, b in enumerate(rh):
                cost[i, j] = q[a][b]
        p = _greedy_assign(cost) if mutate == "greedy" else assign(cost)
        for j, i in enumerate(p):
            if 0 <= i < len(ro) and j < len(rh) and cost[i, j] < BIG:
                match[ro[i]] = rh[j]
    # 4: counts
    C = st.counts[s]
    dropped = sorted(match[a] for a, o in enumerate(objs) if o["ignore"] and a in match)
    for b in dropped:
        C[hyps[b]["cls"], 2 if mutate == "ignored_as_fp" else 4] += 1
    matched_h = set(match.values())
    for a, o in enumerate(objs):
        if o["ignore"]:
            continue
        e = st.obj[s][obj_index[o["id"]]]
        e["present"] += 1
        if a in match:
            h = hyps[match[a]]
            C[o["cls"], 0] += 1
            st.iou_sum[s, o["cls"]] = float(st.iou_sum[s, o["cls"]]) + V[a][match[a]]
            if e["last"] > 0 and e["last"] != h["id"]:
                C[o["cls"], 3] += 1
            e["last"] = h["id"]
            e["tracked"] += 1
            if e["run"] == 2:
                e["frag"] += 1
            e["run"] = 1
        else:
            C[o["cls"], 1] += 1
            if e["run"] == 1:
                e["run"] = 2
            if mutate == "forget_last":
                e["last"] = 0
    for b, h in enumerate(hyps):
        if b not in matched_h:
            C[h["cls"], 2] += 1
        if b not in dropped:
            st.hyp[s][hyp_index[h["id"]]]["frames"] += 1
    for a, o in enumerate(objs):
        if o["ignore"]:
            continue
        for b, h in enumerate(hyps):
            if allowed[a][b] and b not in dropped and (mutate != "overlap_matched_only" or match.get(a) == b):
                key = (obj_index[o["id"]], hyp_index[h["id"]])
                st.overlap[s][key] = st.overlap[s].get(key, 0) + 1
    return {objs[a]["row"]: hyps[b]["row"] for a, b in match.items()}


def run(st, boxes, cls, counts, ids, states, gt, frames, iou_thresh=0.5, mutate=None):
    """A whole call: n = S*frames images, image s*frames + f = frame f of stream s.  gt = (gt_box, gt_id, gt_cls, gt_flags,
    gt_count).  -> per image the frame's {object row: hypothesis row}."""
    n = int(boxes.shape[0])
    assert n == st.S * frames
    out = []
    for s in range(st.S):
        for f in range(frames):
            i = s * frames + f
            out.append(step(st, s, boxes[i], cls[i], counts[i], ids[i], states[i], gt[0][i], gt[1][i], gt[2][i], gt[3][i], gt[4][i],
                            iou_thresh, mutate))
    return out


def idf1_assignment(overlap):
    """overlap int [G, T] -> row_of_col of assign() on the G x max(T, G) matrix of cost -overlap (missing columns zero)."""
    G, T = overlap.shape
    cost = np.zeros((G, max(T, G)), np.int64)
    cost[:, :T] = -np.asarray(overlap, np.int64)
    return assign(cost), cost


def evaluate_tables(d, classes):
    """sqdet_mot_evaluate on the arrays of State.arrays() (or of a device state_dict) -> (table int64 [S, classes, K],
    iou_sum float64 [S, classes]); raises ValueError when a status word is set."""
    S = d["n_obj"].shape[0]
    if np.any(np.asarray(d["status"]) != 0):
        raise ValueError("a stream's identity table overflowed")
    out = np.zeros((S, classes, K), np.int64)
    for s in range(S):
        G, T = int(d["n_obj"][s]), int(d["n_hyp"][s])
        out[s, :, :5] = d["counts"][s]
        ov = np.asarray(d["overlap"][s][:G, :T], np.int64)
        idtp_obj = np.zeros(G, np.int64)
        if G:
            p, cost = idf1_assignment(ov)
            for j, i in enumerate(p):
                if i >= 0:
                    idtp_obj[i] = -cost[i, j]
        for g in range(G):
            c = int(d["obj_cls"][s, g])
            present, tracked = int(d["obj_present"][s, g]), int(d["obj_tracked"][s, g])
            out[s, c, 5] += int(d["obj_frag"][s, g])
            if 5 * tracked >= 4 * present:
                out[s, c, 6] += 1
            elif 5 * tracked < present:
                out[s, c, 8] += 1
            else:
                out[s, c, 7] += 1
            out[s, c, 9] += idtp_obj[g]
            out[s, c, 10] += present
            out[s, c, 12] += 1
        for t in range(T):
            c = int(d["hyp_cls"][s, t])
            out[s, c, 11] += int(d["hyp_frames"][s, t])
            out[s, c, 13] += 1
        out[s, :, 10] -= out[s, :, 9]
        out[s, :, 11] -= out[s, :, 9]
    return out, np.asarray(d["iou_sum"], np.float64).copy()


def evaluate(st):
    return evaluate_tables(st.arrays(), st.classes)


def metrics(counters, iou_sum):
    """A counter vector [K] and its iou_sum -> dict of the counters and mota, motp, idf1, precision, recall (nan where a
    denominator is zero)."""
    c = {k: int(v) for k, v in zip(COUNTERS, counters)}

    def div(a, b):
        return a / b if b else float("nan")
    c["mota"] = 1.0 - div(c["fn"] + c["fp"] + c["idsw"], c["tp"] + c["fn"]) if c["tp"] + c["fn"] else float("nan")
    c["motp"] = div(float(iou_sum), c["tp"])
    c["idf1"] = div(2 * c["idtp"], 2 * c["idtp"] + c["idfp"] + c["idfn"])
    c["precision"] = div(c["tp"], c["tp"] + c["fp"])
    c["recall"] = div(c["tp"], c["tp"] + c["fn"])
    return c
