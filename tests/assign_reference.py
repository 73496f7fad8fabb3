"""The assignment rule of sqdet_build_labels_opt (squeezedet_amd/csrc/assign.hip), restated in plain
sequential NumPy float64 (test infrastructure, no GPU).  Brute force: per box a full sort with the stated tie keys, Python loops.

Stage 1 is the reference's own pick, from oracle.train_oracle.assign_anchors (as input_path_cases.label_reference takes it).
Stage 2 (eligibility) and stage 3 (conflicts) are written out below; every tie rule is a keyword switch of `assign_image`, set to
the plausible wrong choice by the mutation checks of tests/test_assign_host.py:

    iou_tie_high      the iou mode's order: larger IoU, ties -> the HIGHER index        (False: the lower)
    dist_tie_low      atss candidates: smaller distance, ties -> the LOWER index        (False: the higher)
    conflict_low_box  an anchor eligible for several boxes: largest IoU, ties -> LOWER box  (False: the higher)
    strict_inside     atss: the anchor centre strictly inside the box                    (False: edges count)
    population_var    atss: the variance divides by |S|                                  (False: by |S| - 1)
    thresh_inclusive  iou mode: iou >= thresh                                            (False: iou > thresh)
"""
import collections

import numpy as np

from oracle import sqdet_oracle as O
from oracle import train_oracle as TO
from tests.input_path_cases import _mc

SWITCHES = ("iou_tie_high", "dist_tie_low", "conflict_low_box", "strict_inside", "population_var", "thresh_inclusive")

ImageStats = collections.namedtuple("ImageStats", "conflicts conflict_ties cap_cuts cap_tie_cuts boundary_hits edge_hits dist_tie_cuts "
                                                  "all_candidates eligible_claimed")


def iou_eligible(anchors, g, thresh, K, iou_tie_high=True, thresh_inclusive=True):
    """-> (E bool [A], iou [A], stats dict) of one box under the iou mode."""
    iou = O.batch_iou(anchors, g)
    pos = [a for a in range(len(anchors)) if iou[a] > 0]
    order = sorted(pos, key=lambda a: (-iou[a], -a if iou_tie_high else a))
    E = np.zeros(len(anchors), bool)
    for a in order[:K]:
        E[a] = iou[a] >= thresh if thresh_inclusive else iou[a] > thresh
    passing = [a for a in order if iou[a] >= thresh]
    st = dict(cap_cuts=int(len(passing) > K), cap_tie_cuts=int(len(order) > K and iou[order[K - 1]] == iou[order[K]] and iou[order[K]] >= thresh),
              boundary_hits=sum(1 for a in order[:K] if iou[a] == thresh))
    return E, iou, st


def atss_eligible(anchors, g, apg, topk, dist_tie_low=True, strict_inside=True, population_var=True):
    """-> (E bool [A], iou [A], stats dict) of one box under the atss mode."""
    A = len(anchors)
    iou = O.batch_iou(anchors, g)
    gx, gy, gw, gh = g
    d = (gx - anchors[:, 0]) * (gx - anchors[:, 0]) + (gy - anchors[:, 1]) * (gy - anchors[:, 1])
    S, dist_tie_cuts = [], 0
    for s in range(apg):
        of_shape = sorted(range(s, A, apg), key=lambda a: (d[a], a if dist_tie_low else -a))
        S += of_shape[:topk]
        dist_tie_cuts += int(len(of_shape) > topk and d[of_shape[topk - 1]] == d[of_shape[topk]])
    S.sort()
    total = np.float64(0.0)
    for a in S:
        total = total + iou[a]
    mean = total / np.float64(len(S))
    sq = np.float64(0.0)
    for a in S:
        sq = sq + (iou[a] - mean) * (iou[a] - mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = sq / np.float64(len(S) if population_var else len(S) - 1)
    gl, gr, gt, gb = gx - 0.5 * gw, gx + 0.5 * gw, gy - 0.5 * gh, gy + 0.5 * gh
    E = np.zeros(A, bool)
    edge_hits = 0
    for a in S:
        e = iou[a] - mean
        if not (iou[a] > 0 and e >= 0 and e * e >= var):
            continue
        ax, ay = anchors[a, 0], anchors[a, 1]
        inside = gl < ax < gr and gt < ay < gb
        closed = gl <= ax <= gr and gt <= ay <= gb
        edge_hits += int(closed and not inside)
        E[a] = inside if strict_inside else closed
    return E, iou, dict(edge_hits=edge_hits, dist_tie_cuts=dist_tie_cuts, all_candidates=int(len(S) == A))


def assign_image(anchors, gt, picks, mode, apg=1, iou_thresh=0.5, max_per_box=16, topk=9, iou_tie_high=True, dist_tie_low=True,
                 conflict_low_box=True, strict_inside=True, population_var=True, thresh_inclusive=True):
    """One image: gt [n,4], picks = the claimed anchors of stage 1 -> (assigned_box int32 [A], positives int64 [n], ImageStats)."""
    A, n = len(anchors), len(gt)
    assigned = np.full(A, -1, np.int32)
    for i, c in enumerate(picks):
        assigned[c] = i
    stats = collections.Counter()
    E, iou = np.zeros((n, A), bool), np.zeros((n, A))
    for i in range(n):
        if mode == "iou":
            E[i], iou[i], st = iou_eligible(anchors, gt[i], iou_thresh, max_per_box, iou_tie_high, thresh_inclusive)
        elif mode == "atss":
            E[i], iou[i], st = atss_eligible(anchors, gt[i], apg, topk, dist_tie_low, strict_inside, population_var)
        else:
            assert mode == "reference"
            st = {}
        stats.update(st)
    for a in range(A):
        boxes = [i for i in range(n) if E[i, a]]
        if assigned[a] >= 0:
            stats["eligible_claimed"] += len(boxes) > 0
            continue
        if not boxes:
            continue
        top = max(iou[i, a] for i in boxes)
        tied = [i for i in boxes if iou[i, a] == top]
        assigned[a] = tied[0] if conflict_low_box else tied[-1]
        stats["conflicts"] += len(boxes) > 1
        stats["conflict_ties"] += len(tied) > 1
    positives = np.array([(assigned == i).sum() for i in range(n)], np.int64)
    return assigned, positives, ImageStats(*[int(stats[k]) for k in ImageStats._fields])


AssignRef = collections.namedtuple("AssignRef", "aidx mask delta64 box labels assigned_box positives stats")


def clipped_count(case, b):
    return int(min(max(int(case.cnt[b]), 0), case.gt.shape[1]))


def assign_reference(case, mode, apg=1, **kw):
    """A whole case (input_path_cases.LabelCase layout) -> AssignRef: aidx int32 [B,M] (-1 behind the count), mask / box / labels
    float32, delta64 float64 [B,A,4] (the caller rounds it once), assigned_box int32 [B,A], positives int32 [B,M], stats: one
    ImageStats per image.  mode "reference": stage 1 alone."""
    (B, M), A = case.cls.shape, len(case.anchors)
    anchors = np.asarray(case.anchors, np.float64)
    aidx = np.full((B, M), -1, np.int32)
    mask, delta = np.zeros((B, A), np.float32), np.zeros((B, A, 4), np.float64)
    box, lab = np.zeros((B, A, 4), np.float32), np.zeros((B, A, case.C), np.float32)
    assigned_box, positives, stats = np.full((B, A), -1, np.int32), np.zeros((B, M), np.int32), []
    for b in range(B):
        n = clipped_count(case, b)
        gt = case.gt[b, :n]
        with np.errstate(divide="ignore", invalid="ignore"):
            picks, _ = TO.assign_anchors(_mc(anchors), gt)
            assert len(set(picks)) == len(picks)
            aidx[b, :n] = picks
            assigned_box[b], positives[b, :n], st = assign_image(anchors, gt, picks, mode, apg, **kw)
            stats.append(st)
            for a in np.flatnonzero(assigned_box[b] >= 0):
                i = assigned_box[b, a]
                gx, gy, gw, gh = gt[i]
                ax, ay, aw, ah = anchors[a]
                mask[b, a], box[b, a] = 1.0, gt[i].astype(np.float32)
                delta[b, a] = [(gx - ax) / aw, (gy - ay) / ah, np.log(gw / aw), np.log(gh / ah)]
                if 0 <= case.cls[b, i] < case.C:
                    lab[b, a, case.cls[b, i]] = 1.0
    return AssignRef(aidx, mask, delta, box, lab, assigned_box, positives, stats)
