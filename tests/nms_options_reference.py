"""A sequential NumPy restatement of sqdet_suppress_rows (include/sqdet.h): the second suppression stage
over the rows of a filter call, one image and one row at a time.  float32 where the kernel is float32 (the IoU, op for op
postproc.h's iou_center), float64 elsewhere; every operator is one IEEE operation, so the hard rules and Soft-NMS linear are
reproduced bit for bit and Soft-NMS Gaussian up to the two libms' exp.

suppress(..., margins=True) also returns the smallest decision margin it met, so a case list can show that no decision sits
on a rounding boundary; `mutate` swaps one rule for a plausible wrong one (tests/test_nms_options_host.py shows that the cases
tell each of them from the rule)."""
import numpy as np

METHODS = ("nongreedy", "greedy", "soft_linear", "soft_gaussian")
OVERLAPS = ("iou", "diou")
MUTATIONS = ("greedy_as_nongreedy", "ge_for_gt", "no_class_test", "rank_tie_reversed", "pick_tie_reversed", "no_diou_penalty", "floor_moved")

f32 = np.float32


def order_key32(p):
    b = int(np.asarray(p, np.float32).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def make_key(p, idx):
    """postproc.h's composite key: descending = descending prob, ties -> the higher anchor index first."""
    return (order_key32(p) << 32) | (int(idx) & 0xffffffff)


def _corners(b):
    h = f32(0.5)
    return b[0] - h * b[2], b[0] + h * b[2], b[1] - h * b[3], b[1] + h * b[3]


def iou_center(bj, bi):
    """postproc.h iou_center on float32 [cx, cy, w, h], operation for operation."""
    bj, bi = np.asarray(bj, f32), np.asarray(bi, f32)
    with np.errstate(all="ignore"):
        jx0, jx1, jy0, jy1 = _corners(bj)
        ix0, ix1, iy0, iy1 = _corners(bi)
        lr = np.fmax(np.fmin(jx1, ix1) - np.fmax(jx0, ix0), f32(0))
        tb = np.fmax(np.fmin(jy1, iy1) - np.fmax(jy0, iy0), f32(0))
        inter = f32(lr * tb)
        uni = f32(f32(f32(bj[2] * bj[3]) + f32(bi[2] * bi[3])) - inter)
        return f32(inter / uni)


def diou_center(iou, bj, bi, penalty=True):
    """float64: iou - d^2 / c^2 on iou_center's float32 corners (d: centre distance, c: enclosing diagonal)."""
    bj, bi = np.asarray(bj, f32), np.asarray(bi, f32)
    with np.errstate(all="ignore"):
        jx0, jx1, jy0, jy1 = _corners(bj)
        ix0, ix1, iy0, iy1 = _corners(bi)
        dx = np.float64(bj[0]) - np.float64(bi[0])
        dy = np.float64(bj[1]) - np.float64(bi[1])
        ew = np.float64(np.fmax(jx1, ix1)) - np.float64(np.fmin(jx0, ix0))
        eh = np.float64(np.fmax(jy1, iy1)) - np.float64(np.fmin(jy0, iy0))
        if not penalty:
            return np.float64(iou)
        return np.float64(iou) - (dx * dx + dy * dy) / (ew * ew + eh * eh)


class Margins:
    def __init__(self):
        self.overlap = self.pick = self.floor = float("inf")

    def smallest(self):
        return min(self.overlap, self.pick, self.floor)


def suppress_image(boxes, probs, cls, index, cnt, classes, method, overlap="iou", agnostic=False, nms_thresh=0.4, sigma=0.5,
                   score_floor=0.001, mg=None, mutate=None):
    """One image: rows [0, cnt) of boxes [rows,4] f32, probs [rows] f32, cls / index [rows] i32 -> the kept rows as lists
    (box, prob, cls, index) in output order."""
    assert method in METHODS and overlap in OVERLAPS and mutate in (None,) + MUTATIONS
    thresh, sigma, floor = np.float64(nms_thresh), np.float64(sigma), np.float64(score_floor)
    # rank: descending key, equal keys (never from the filter) the lower row first
    tie = -1 if mutate == "pick_tie_reversed" else 1          # (the wrong soft rule: a tie goes to the LOWER rank)
    if mutate == "rank_tie_reversed":      # the other tie rule of the key: the lower anchor index first
        order = sorted(range(cnt), key=lambda r: (-order_key32(probs[r]), int(index[r]) & 0xffffffff, r))
    else:
        order = sorted(range(cnt), key=lambda r: (-make_key(probs[r], index[r]), r))
    B = [np.array(boxes[r], f32) for r in order]      # (copies: the caller overwrites the rows)
    P = [f32(probs[r]) for r in order]
    Cl = [int(cls[r]) for r in order]
    I = [int(index[r]) for r in order]
    valid = [0 <= c < classes for c in Cl]
    same = (lambda i, j: True) if (agnostic or mutate == "no_class_test") else (lambda i, j: Cl[i] == Cl[j])
    above = (lambda o: o >= thresh) if mutate == "ge_for_gt" else (lambda o: o > thresh)

    def ov(i, j):       # i the higher-ranked row
        u = iou_center(B[j], B[i])
        return diou_center(u, B[j], B[i], penalty=mutate != "no_diou_penalty") if overlap == "diou" else np.float64(u)

    def note_overlap(o):
        if mg is not None and o == o:
            mg.overlap = min(mg.overlap, abs(float(o) - float(thresh)))

    n = cnt
    if method in ("nongreedy", "greedy"):
        rule = "nongreedy" if mutate == "greedy_as_nongreedy" else method
        keep = list(valid)
        for j in range(n):
            if not valid[j]:
                continue
            for i in range(j):
                if not valid[i] or not same(i, j):
                    continue
                if rule == "greedy" and not keep[i]:
                    continue
                o = ov(i, j)
                note_overlap(o)
                if above(o):
                    keep[j] = False
                    if rule == "greedy":
                        break           # (j is gone; nothing later changes that)
        picked = [j for j in range(n) if keep[j]]
        score = {j: P[j] for j in picked}
    else:
        assert overlap == "iou", "diou goes with the hard methods only"
        s = [np.float64(p) for p in P]
        rem = [j for j in range(n) if valid[j]]
        touched = set()
        picked = []
        while rem:
            best = rem[0]
            for j in rem[1:]:           # rem is in rank order: a tie stays with the higher rank
                if s[j] > s[best] or (tie < 0 and s[j] == s[best]):
                    best = j
            if mg is not None and len(rem) > 1:
                second = max(float(s[j]) for j in rem if j != best)
                exact_untouched_tie = second == float(s[best]) and not ({best} | {j for j in rem if float(s[j]) == second}) & touched
                if not exact_untouched_tie:     # (bit-equal undecayed probs tie identically in every implementation)
                    mg.pick = min(mg.pick, abs(float(s[best]) - second) / max(abs(float(s[best])), 1e-300))
            if mutate != "floor_moved":
                if mg is not None:
                    mg.floor = min(mg.floor, abs(float(s[best]) - float(floor)) / max(abs(float(s[best])), 1e-300))
                if s[best] < floor:
                    break
            rem.remove(best)
            picked.append(best)
            if mutate == "floor_moved" and s[best] < floor:      # (the wrong place: after the row was kept)
                break
            for j in rem:
                if not same(best, j):
                    continue
                u = np.float64(iou_center(B[j], B[best]))
                with np.errstate(all="ignore"):
                    if method == "soft_linear":
                        note_overlap(u)
                        if above(u):
                            s[j] = s[j] * (np.float64(1.0) - u)
                    else:
                        s[j] = s[j] * np.exp(-(u * u) / sigma)
                        touched.add(j)
        score = {j: f32(s[j]) for j in picked}
    # kept rows by class, then pick order (a stable sort)
    out = sorted(picked, key=lambda j: Cl[j])
    return [B[j] for j in out], [score[j] for j in out], [Cl[j] for j in out], [I[j] for j in out]


def suppress(out, classes, method, overlap="iou", agnostic=False, nms_thresh=0.4, sigma=0.5, score_floor=0.001, margins=False,
             mutate=None):
    """The five arrays of a filter call (boxes [n,rows,4] f32, probs [n,rows] f32, cls / index [n,rows] i32, count [n] i32) ->
    five new arrays, as sqdet_suppress_rows leaves them.  margins=True: -> (arrays, Margins)."""
    boxes, probs, cls, index, count = [np.array(a, copy=True) for a in out]
    n, rows = probs.shape
    mg = Margins() if margins else None
    for b in range(n):
        cnt = int(count[b])
        if cnt < 0 or cnt > rows:
            continue                    # passed through untouched
        kb, kp, kc, ki = suppress_image(boxes[b], probs[b], cls[b], index[b], cnt, classes, method, overlap, agnostic, nms_thresh,
                                        sigma, score_floor, mg, mutate)
        k = len(kp)
        boxes[b], probs[b], cls[b], index[b] = 0, 0, -1, -1
        if k:
            boxes[b, :k], probs[b, :k], cls[b, :k], index[b, :k] = np.stack(kb), np.array(kp, f32), kc, ki
        count[b] = k
    res = (boxes, probs, cls, index, count)
    return (res, mg) if margins else res
