"""A plain-loop float64 NumPy restatement of the COCO bbox evaluation rule (include/sqdet.h "COCO-style evaluation"): the
yardstick of csrc/coco_eval.hip.  Nothing here is shared with squeezedet_amd.coco: its own thresholds (np.linspace), its own
mergesort-order argsort, np.searchsorted.  tests/test_coco_host.py pins it by cases small enough to compute by hand.

    evaluate(dets, gts, classes) -> precision [T,R,K,A,M], recall [T,K,A,M], flags
      dets   per image [(cls, x, y, w, h, score)]  (any order; a class's rows keep their order)
      gts    per image [(cls, x, y, w, h, area, iscrowd, ignore)]
      flags  per class (rank int32 [n], matched bool [A,T,n], ignored bool [A,T,n]) in the class's order"""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]
EPS = 2.220446049250313e-16


def stable_desc(scores):
    """Indices by descending score, equal scores in their order (what np.argsort(-s, kind='mergesort') gives), by insertion."""
    order = []
    for j, s in enumerate(scores):
        p = len(order)
        while p > 0 and scores[order[p - 1]] < s:
            p -= 1
        order.insert(p, j)
    return order


def iou(d, g, crowd):
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    if iw <= 0 or ih <= 0:
        return np.float64(0)
    i = iw * ih
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return i / u


def iou_matrix(dets, gts):
    return [[iou(d[:4], g[:4], g[5]) for g in gts] for d in dets]


def evaluate_image(dets, gts, area_rng, iou_thrs, max_det, ious=None):
    """One (image, class, area range): dets [(x, y, w, h, score)], gts [(x, y, w, h, area, iscrowd, ignore)] ->
    (scores, matched [T,D], ignored [T,D]) of the first max_det rows by score.  ious: iou_matrix(dets, gts), when the caller
    has it (the IoU does not depend on the area range)."""
    ious = ious if ious is not None else iou_matrix(dets, gts)
    lo, hi = area_rng
    g_ig = [bool(g[6] or g[5] or g[4] < lo or g[4] > hi) for g in gts]
    g_order = [k for k in range(len(gts)) if not g_ig[k]] + [k for k in range(len(gts)) if g_ig[k]]
    d_order = stable_desc([d[4] for d in dets])[:max_det]
    T, D = len(iou_thrs), len(d_order)
    matched, ignored = np.zeros((T, D), bool), np.zeros((T, D), bool)
    for ti, t in enumerate(iou_thrs):
        taken = [False] * len(gts)
        for di, j in enumerate(d_order):
            best, m = min(t, 1 - 1e-10), -1
            for k in g_order:
                if taken[k] and not gts[k][5]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[k]:
                    break
                v = ious[j][k]
                if v < best:
                    continue
                best, m = v, k
            if m > -1:
                taken[m] = True
                matched[ti, di], ignored[ti, di] = True, g_ig[m]
            else:
                a = np.float64(dets[j][2]) * np.float64(dets[j][3])
                ignored[ti, di] = a < lo or a > hi
    return [dets[j][4] for j in d_order], matched, ignored


def evaluate(dets, gts, classes, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, area_rngs=AREA_RNGS, max_dets=MAX_DETS):
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), classes, len(area_rngs), len(max_dets)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    flags = []
    for c in range(K):
        per_area = []
        by_image = [([r[1:] for r in di if r[0] == c], [r[1:] for r in gi if r[0] == c]) for di, gi in zip(dets, gts)]
        by_image = [(d, g, iou_matrix(d, g)) for d, g in by_image]
        for a, rng in enumerate(area_rngs):
            scores, ranks, ms, igs, npig = [], [], [], [], 0
            for d, g, ious in by_image:
                npig += sum(1 for x in g if not (x[6] or x[5] or x[4] < rng[0] or x[4] > rng[1]))
                s, m, ig = evaluate_image(d, g, rng, iou_thrs, max_dets[-1], ious)
                scores += s
                ranks += list(range(len(s)))
                ms.append(m)
                igs.append(ig)
            order = stable_desc(scores)
            ranks = np.array(ranks, np.int32)[order] if order else np.zeros(0, np.int32)
            m_all = np.concatenate(ms, axis=1)[:, order] if ms else np.zeros((T, 0), bool)
            ig_all = np.concatenate(igs, axis=1)[:, order] if igs else np.zeros((T, 0), bool)
            per_area.append((ranks, m_all, ig_all))
            if npig == 0:
                continue
            for mi, md in enumerate(max_dets):
                keep = ranks < md
                dm, dig = m_all[:, keep], ig_all[:, keep]
                tps, fps = np.logical_and(dm, ~dig), np.logical_and(~dm, ~dig)
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
                for ti in range(T):
                    tp, fp = tp_sum[ti], fp_sum[ti]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + EPS)
                    recall[ti, c, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[ti, :, c, a, mi] = q
        flags.append((per_area[0][0], np.stack([p[1] for p in per_area]), np.stack([p[2] for p in per_area])))
    return precision, recall, flags


def summarize(precision, recall, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """The twelve statistics, each the mean of its selected entries > -1 (or -1): written out entry by entry, on its own."""
    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    t50, t75 = int(np.where(iou_thrs == .5)[0][0]), int(np.where(iou_thrs == .75)[0][0])
    last = len(max_dets) - 1
    return np.array([mean(precision[:, :, :, 0, last]), mean(precision[t50:t50 + 1, :, :, 0, last]), mean(precision[t75:t75 + 1, :, :, 0, last]),
                     mean(precision[:, :, :, 1, last]), mean(precision[:, :, :, 2, last]), mean(precision[:, :, :, 3, last]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                     mean(recall[:, :, 1, last]), mean(recall[:, :, 2, last]), mean(recall[:, :, 3, last])])
