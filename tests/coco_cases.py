"""Hand-computable cases of the COCO bbox rule, shared by tests/test_coco_host.py (against tests/coco_reference.py) and
tests/test_gpu_coco_ap.py (against the kernels).  CASES[name] = (dets, gts, classes): dets per image [(cls, x, y, w, h,
score)] class-major, gts per image [(cls, x, y, w, h, area, iscrowd, ignore)].  check(name, precision, recall, flags, stats)
asserts what each case is there to show; every expected number below is worked out in the comment beside it.

Precision is tp / (fp + tp + eps) with eps = 2^-52, so a lone true positive has 1 / (1 + 2^-52) = 1 - 2^-52, not 1: the
statistics are compared with their exact rationals within TOL = 1e-15.  That bound is derived, not measured: an entry differs
from tp / (tp + fp) by at most eps / (tp + fp) + 2^-53 <= 3.4e-16 relative, and the mean of n such entries adds its own
rounding, at most log2(n) * 2^-53 for NumPy's pairwise sum (n <= 10 * 101 * 2: under 1.3e-15 in all, values <= 1).  Where an
array entry is pinned exactly (P1 below) it is compared bit for bit.

stats: AP, AP50, AP75, AP small, medium, large, AR@1, AR@10, AR@100, AR small, medium, large.
flags[c] = (rank [n], matched [A,T,n], ignored [A,T,n]) in class c's order; thresholds t = 0..9 are 0.50..0.95."""
import numpy as np


def _gt(c, x, y, w, h, area=None, crowd=0, ignore=0):
    return (c, x, y, w, h, w * h if area is None else area, crowd, ignore)


CASES = {
    # (a) every object detected exactly.  Areas 2500 and 1600 (medium) for class 0, 10000 (large) for class 1; no small object:
    # the small bucket has npig = 0 everywhere -> -1.  One object per (image, class), so one detection per image suffices.
    "a": ([[(0, 10, 10, 50, 50, .9), (1, 100, 100, 100, 100, .8)], [(0, 5, 5, 40, 40, .7)]],
          [[_gt(0, 10, 10, 50, 50), _gt(1, 100, 100, 100, 100)], [_gt(0, 5, 5, 40, 40)]], 2),
    # (b) IoU exactly 0.5: 10x10 inside 10x20 -> 100 / (100 + 200 - 100).  Matched at 0.50 only: AP50 = 1, AP = 1/10.
    "b1": ([[(0, 0, 0, 10, 10, .9)]], [[_gt(0, 0, 0, 10, 20)]], 1),
    # IoU 60 / 100 = 0.6 against the third threshold AS np.linspace COMPUTES IT.  Where that is 0.6000000000000001 the row is
    # matched at 0.50 and 0.55 only and AP = 2/10; where linspace gives 0.6 itself (NumPy 2.2 does: its odd one out is
    # 0.8999999999999999) the row passes it too and AP = 3/10.  _passed counts the thresholds the way the rule compares them.
    "b2": ([[(0, 0, 0, 6, 10, .9)]], [[_gt(0, 0, 0, 10, 10)]], 1),
    # IoU 340 / 400 = 0.85 exactly, where 0.5 + 7 * 0.05 is 0.8500000000000001: thresholds recomputed that way would lose one
    "b3": ([[(0, 0, 0, 17, 20, .9)]], [[_gt(0, 0, 0, 20, 20)]], 1),
    # (c) two rows inside one crowd region (IoU = intersection / row area = 1): both matched and ignored -- neither tp nor fp --
    # so the third row, exact on the one ordinary object, has precision 1 / (0 + 1) = 1 at recall 1: AP = 1 (1/3 if the two counted
    # as fp).  With one detection per image only the first crowd row is left: AR@1 = 0.
    "c": ([[(0, 10, 10, 20, 20, .9), (0, 50, 50, 30, 30, .8), (0, 200, 200, 50, 50, .7)]],
          [[_gt(0, 0, 0, 100, 100, crowd=1), _gt(0, 200, 200, 50, 50)]], 1),
    # (d) class 0: two identical objects and one exact row -> the later object is taken (tests/coco_reference.evaluate_image
    # reports the index); one tp of two objects: recall 1/2.  Class 1 shows the same rule in the flags: objects A = [0,0,10,10]
    # and B = [10,0,10,10]; row 1 = [0,0,20,10] has IoU 100 / (200 + 100 - 100) = 0.5 with both, so at 0.50 it takes the
    # later one, B; row 2 = B exactly then finds B taken and has IoU 0 with A: unmatched.  (Lowest index first would give row 2 a
    # match.)  Above 0.50 row 1 matches nothing and row 2 takes B.
    "d": ([[(0, 0, 0, 10, 10, .9), (1, 0, 0, 20, 10, .9), (1, 10, 0, 10, 10, .8)]],
          [[_gt(0, 0, 0, 10, 10), _gt(0, 0, 0, 10, 10), _gt(1, 0, 0, 10, 10), _gt(1, 10, 0, 10, 10)]], 2),
    # (e) a row that is exactly an ignored object (IoU 1) and overlaps a free ordinary one with 100 / 120 = 0.8333: up to 0.80 the
    # ordinary one is taken (tp, not ignored); from 0.85 on only the ignored one passes: matched and ignored.  AP = 7/10.
    "e": ([[(0, 0, 0, 10, 12, .9)]], [[_gt(0, 0, 0, 10, 10), _gt(0, 0, 0, 10, 12, ignore=1)]], 1),
    # (f) area exactly 1024 = 32^2 is inside [0, 1024] and inside [1024, 9216]: small and medium both count it
    "f": ([[(0, 0, 0, 32, 32, .9)]], [[_gt(0, 0, 0, 32, 32)]], 1),
    # (g) three exact rows on three objects of one image: one detection per image finds one of three
    "g": ([[(0, 0, 0, 40, 40, .9), (0, 100, 0, 40, 40, .8), (0, 200, 0, 40, 40, .7)]],
          [[_gt(0, 0, 0, 40, 40), _gt(0, 100, 0, 40, 40), _gt(0, 200, 0, 40, 40)]], 1),
    # (h) equal scores in two images: image 0's row (no object there: fp) comes before image 1's (tp): pr = [0, 1/2], envelope
    # 1/2 everywhere: AP = 1/2.  (The other order would give pr = [1, 1/2] and AP = 1.)
    "h": ([[(0, 0, 0, 40, 40, .5)], [(0, 0, 0, 40, 40, .5)]], [[], [_gt(0, 0, 0, 40, 40)]], 1),
    # (i) class 1 has rows but no object anywhere: its entries are -1 and stay out of the means (AP = 1, not 1/2)
    "i": ([[(0, 0, 0, 40, 40, .9), (1, 50, 50, 40, 40, .8)]], [[_gt(0, 0, 0, 40, 40)]], 2),
}

TOL = 1e-15
P1 = 1 / (1 + 2.220446049250313e-16)          # precision after one true positive and nothing else


def _passed(iou):
    """The share of the ten thresholds an IoU passes: `iou >= min(t, 1 - 1e-10)` for t of np.linspace(.5, .95, 10)."""
    return float(np.sum(iou >= np.minimum(np.linspace(.5, 0.95, 10), 1 - 1e-10))) / 10


_B2, _B3 = _passed(60 / 100), _passed(340 / 400)
STATS = {   # None: not pinned here
    "a": [1, 1, 1, -1, 1, 1, 1, 1, 1, -1, 1, 1],
    "b1": [.1, 1, 0, .1, -1, -1, .1, .1, .1, .1, -1, -1],
    "b2": [_B2, 1, 0, _B2, -1, -1, _B2, _B2, _B2, _B2, -1, -1],
    "b3": [_B3, 1, 1, _B3, -1, -1, _B3, _B3, _B3, _B3, -1, -1],
    "c": [1, 1, 1, -1, 1, -1, 0, 1, 1, -1, 1, -1],
    "d": [None, None, None, None, -1, -1, None, None, None, None, -1, -1],
    "e": [.7, 1, 1, .7, -1, -1, .7, .7, .7, .7, -1, -1],
    "f": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],
    "g": [1, 1, 1, -1, 1, -1, None, 1, 1, -1, 1, -1],
    "h": [.5, .5, .5, -1, .5, -1, 1, 1, 1, -1, 1, -1],
    "i": [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1],
}


def check(name, precision, recall, flags, stats):
    want = STATS[name]
    for k, w in enumerate(want):
        assert w is None or (stats[k] == -1 if w == -1 else abs(stats[k] - w) <= TOL), (name, k, stats[k], w)
    assert np.all((precision == -1) | ((precision >= 0) & (precision <= 1)))
    if name == "c":
        rank, m, ig = flags[0]
        assert rank.tolist() == [0, 1, 2]
        assert m[0].all() and ig[0, :, :2].all() and not ig[0, :, 2].any()       # area all: crowd rows matched + ignored, the third a tp
    if name == "d":
        assert np.all(recall[:, 0, 0, 2] == 0.5)                                  # class 0: one row, two objects
        rank, m, ig = flags[1]
        assert m[0, 0].tolist() == [True, False] and all(m[0, t].tolist() == [False, True] for t in range(1, 10))
        assert not ig[0].any()
        assert recall[:, 1, 0, 2].tolist() == [0.5] * 10
    if name == "e":
        rank, m, ig = flags[0]
        assert m[0, :, 0].all() and ig[0, :, 0].tolist() == [False] * 7 + [True] * 3
    if name == "g":
        assert np.all(recall[:, 0, 0, 0] == 1.0 / 3) and abs(stats[6] - 1.0 / 3) <= TOL
    if name == "h":
        assert np.all(precision[:, :, 0, 0, 2] == 0.5)                           # 1 / (1 + 1 + eps): 2 + 2^-52 rounds to 2
    if name == "i":
        assert np.all(precision[:, :, 1] == -1) and np.all(recall[:, 1] == -1) and np.all(precision[:, :, 0, 0, 2] == P1)


def random_case(seed=7):
    """The seeded case of tests/test_gpu_coco_ap.py: 7 images, 3 classes (class 2 has no object anywhere), at most 160 rows
    per image -> (dets, gts, classes).  Integer coordinates and scores on a grid of 1/16, so equal scores and equal IoUs are
    common.  Image 0: 130 rows of class 0 (more than maxDets[-1] = 100, more than one 64-lane pass).  Image 1: 70 objects of
    class 1 (an object loop longer than 64).  Image 2: no rows.  Image 3: rows but no objects.  Crowd and ignore objects, areas
    of exactly 1024 and 9216, duplicated objects, and rows built to land IoUs exactly on 0.5 and 0.75."""
    rs = np.random.RandomState(seed)
    n_img, classes = 7, 3
    gts, dets = [[] for _ in range(n_img)], [[] for _ in range(n_img)]

    def box(lo=8, hi=120):
        w, h = int(rs.randint(lo, hi)), int(rs.randint(lo, hi))
        return int(rs.randint(0, 400)), int(rs.randint(0, 300)), w, h

    def score():
        return float(rs.randint(1, 16)) / 16.0

    n_gt = [12, 70, 5, 0, 9, 14, 6]
    for i in range(n_img):
        for k in range(n_gt[i]):
            c = 1 if i == 1 else int(rs.randint(0, 2))
            x, y, w, h = box()
            u = rs.uniform()
            gts[i].append(_gt(c, x, y, w, h, crowd=int(u < 0.1), ignore=int(0.1 <= u < 0.2)))
            if rs.uniform() < 0.15:                                   # a duplicate: an IoU tie on every row
                gts[i].append(_gt(c, x, y, w, h))
    gts[0] += [_gt(0, 10, 10, 32, 32), _gt(0, 200, 10, 96, 96), _gt(1, 300, 200, 64, 16)]       # areas 1024, 9216, 1024
    gts[4] += [_gt(0, 0, 0, 10, 20), _gt(1, 40, 40, 20, 20)]
    n_det = [130, 60, 0, 25, 40, 70, 33]
    for i in range(n_img):
        rows = []
        own = [g for g in gts[i]]
        for k in range(n_det[i]):
            c = 0 if i == 0 else int(rs.randint(0, 3))
            u = rs.uniform()
            if own and u < 0.6:                                       # on an object, exact or shifted by a few pixels
                g = own[int(rs.randint(len(own)))]
                d = [0, 0, 0, 0] if u < 0.25 else [int(v) for v in rs.randint(-6, 7, 4)]
                x, y, w, h = g[1] + d[0], g[2] + d[1], max(1, g[3] + d[2]), max(1, g[4] + d[3])
                c = g[0] if i != 0 else 0
            else:
                x, y, w, h = box()
            rows.append((c, x, y, w, h, score()))
        dets[i] = rows
    dets[4] += [(0, 0, 0, 10, 10, .5), (1, 40, 40, 15, 20, .5), (1, 40, 40, 20, 20, .5)]        # IoU exactly 0.5, 0.75, 1
    dets = [sorted(r, key=lambda row: row[0]) for r in dets]          # class-major, order kept within a class
    assert max(len(r) for r in dets) <= 160 and not any(g[0] == 2 for r in gts for g in r)
    return dets, gts, classes


def long_case(seed=300):
    """The second seeded case of tests/test_gpu_coco_ap.py: 300 images (more than the 256 the evaluator's scan over images
    takes at a time), 2 classes with more than 256 kept rows each (the accumulate kernel walks a class's list 256 rows at a
    time, from its end) -> (dets, gts, classes).  Image 5: 120 rows of class 0 (more than maxDets[-1] = 100: 100 are kept).
    Images without rows (i % 11 == 5, i != 5) and without objects (i % 7 == 3), crowd and ignore objects, scores on a grid of
    1/16: equal scores across images are the rule."""
    rs = np.random.RandomState(seed)
    n_img, classes = 300, 2
    gts, dets = [], []
    for i in range(n_img):
        g = []
        for _ in range(0 if i % 7 == 3 else int(rs.randint(1, 4))):
            w, h = int(rs.randint(8, 120)), int(rs.randint(8, 120))
            u = rs.uniform()
            g.append(_gt(int(rs.randint(0, 2)), int(rs.randint(0, 400)), int(rs.randint(0, 300)), w, h, crowd=int(u < 0.1),
                         ignore=int(0.1 <= u < 0.2)))
        rows = []
        for _ in range(120 if i == 5 else 0 if i % 11 == 5 else int(rs.randint(0, 5))):
            c = 0 if i == 5 else int(rs.randint(0, 2))
            if g and rs.uniform() < 0.6:                              # on an object, exact or shifted by a few pixels
                o = g[int(rs.randint(len(g)))]
                d = [0, 0, 0, 0] if rs.uniform() < 0.4 else [int(v) for v in rs.randint(-6, 7, 4)]
                x, y, w, h = o[1] + d[0], o[2] + d[1], max(1, o[3] + d[2]), max(1, o[4] + d[3])
                c = o[0] if i != 5 else 0
            else:
                x, y, w, h = int(rs.randint(0, 400)), int(rs.randint(0, 300)), int(rs.randint(8, 120)), int(rs.randint(8, 120))
            rows.append((c, x, y, w, h, float(rs.randint(1, 16)) / 16.0))
        gts.append(g)
        dets.append(sorted(rows, key=lambda row: row[0]))            # class-major, order kept within a class
    return dets, gts, classes
