"""Small seeded inputs of sqdet_suppress_rows (rows <= 64), shared by tests/test_nms_options_host.py (which shows that they tell
the rule from seven plausible wrong ones) and tests/test_gpu_nms_options.py (the kernel against the restatement on all of them).
A case: dict(name, out=(boxes [n,rows,4] f32, probs [n,rows] f32, cls [n,rows] i32, index [n,rows] i32, count [n] i32), classes,
nms_thresh, sigma, score_floor).  Rows past an image's count hold what the filter leaves there (0, 0, -1, -1)."""
import numpy as np

from tests.nms_options_reference import make_key

A = 16848       # SqueezeDet's anchors at 1248 x 384: the range of the anchor indices


def pack(images, rows, filter_order=True):
    """images: one list of (box, prob, cls, index) per image, or an int (a count to report with no rows behind it)."""
    n = len(images)
    boxes, probs = np.zeros((n, rows, 4), np.float32), np.zeros((n, rows), np.float32)
    cls, index, count = np.full((n, rows), -1, np.int32), np.full((n, rows), -1, np.int32), np.zeros((n,), np.int32)
    for b, img in enumerate(images):
        if isinstance(img, int):
            count[b] = img
            continue
        if filter_order:        # what the filter emits: by class, then descending key
            img = sorted(img, key=lambda r: (r[2], -make_key(np.float32(r[1]), r[3])))
        assert len(img) <= rows
        for r, (bx, p, c, i) in enumerate(img):
            boxes[b, r], probs[b, r], cls[b, r], index[b, r] = bx, p, c, i
        count[b] = len(img)
    return boxes, probs, cls, index, count


def random_image(rs, cnt, classes, clusters=5):
    """cnt rows around a few object centres of a 1242 x 375 image: KITTI-like sizes, plenty of overlaps of every degree."""
    cx, cy = rs.uniform(100, 1100, clusters), rs.uniform(80, 300, clusters)
    w, h = rs.uniform(30, 160, clusters), rs.uniform(30, 120, clusters)
    ccls = rs.randint(0, classes, clusters)
    idx = rs.choice(A, cnt, replace=False)
    rows = []
    for r in range(cnt):
        k = rs.randint(clusters)
        box = [cx[k] + rs.normal(0, 0.12 * w[k]), cy[k] + rs.normal(0, 0.12 * h[k]), w[k] * rs.uniform(0.8, 1.25), h[k] * rs.uniform(0.8, 1.25)]
        c = int(ccls[k]) if rs.rand() < 0.8 else int(rs.randint(classes))
        rows.append((np.asarray(box, np.float32), np.float32(rs.uniform(0.005, 0.999)), c, int(idx[r])))
    return rows


def _case(name, out, classes, nms_thresh=0.4, sigma=0.5, score_floor=0.001):
    return dict(name=name, out=out, classes=classes, nms_thresh=nms_thresh, sigma=sigma, score_floor=score_floor)


def box(cx, cy, w, h):
    return np.asarray([cx, cy, w, h], np.float32)


# shift 3 of a 10-wide box: IoU 7/13 = 0.538; shift 6: 4/16 = 0.25
CHAIN = [(box(100, 50, 10, 10), 0.9, 0, 700), (box(103, 50, 10, 10), 0.8, 0, 40), (box(106, 50, 10, 10), 0.7, 0, 9000)]


def make_cases():
    rs = np.random.RandomState(20170)
    cases = []
    cases.append(_case("counts_rows64", pack([random_image(rs, c, 3) for c in (0, 1, 63, 64)], 64), 3))
    cases.append(_case("counts_rows5_any_order", pack([random_image(rs, c, 3, clusters=2) for c in (0, 1, 4, 5)], 5, filter_order=False), 3))
    cases.append(_case("classes1", pack([random_image(rs, 40, 1), random_image(rs, 17, 1, clusters=2)], 64), 1))
    cases.append(_case("classes20", pack([random_image(rs, 64, 20, clusters=9), random_image(rs, 33, 20)], 64), 20, nms_thresh=0.2))
    cases.append(_case("chain", pack([CHAIN], 5), 3))
    cases.append(_case("chain_across_classes", pack([[(b, p, k, i) for k, (b, p, _, i) in enumerate(CHAIN)]], 5), 3))
    cases.append(_case("identical_boxes", pack([[(box(300, 200, 60, 40), p, c, i) for p, c, i in
                                                 ((0.9, 0, 5), (0.6, 1, 6), (0.5, 0, 7), (0.45, 0, 8), (0.3, 1, 9), (0.2, 2, 10))]], 8), 3))
    # a 2 x 4 box inside a 4 x 4 box: intersection 8, union 16 -- IoU exactly 0.5 (and DIoU: the centres coincide)
    cases.append(_case("iou_exactly_at_thresh", pack([[(box(10, 10, 4, 4), 0.9, 1, 11), (box(10, 10, 2, 4), 0.6, 1, 12)]], 4), 3, nms_thresh=0.5))
    # (the three tie on the untouched prob: the anchor index ranks them 977, 31, 5; their mutual overlaps all differ, so no two decayed scores tie)
    cases.append(_case("equal_probs", pack([[(box(100, 50, 10, 10), 0.75, 0, 31), (box(102, 50, 10, 10), 0.75, 0, 977), (box(105, 50, 10, 10), 0.75, 0, 5),
                                             (box(101, 51, 10, 10), 0.5, 0, 64)]], 6), 2))
    # scores that decay across the floor: heavy overlaps, small probs (linear: 1 - iou of a near copy; Gaussian: exp(-iou^2 / 0.5))
    cases.append(_case("decay_across_floor", pack([[(box(200, 100, 40, 40), 0.9, 0, 1), (box(200, 100, 40, 40), 0.004, 0, 2), (box(201, 100, 40, 40), 0.5, 0, 3),
                                                    (box(200, 101, 40, 40), 0.002, 0, 4), (box(260, 100, 40, 40), 0.0015, 0, 5), (box(500, 100, 40, 40), 0.0005, 0, 6),
                                                    (box(230, 100, 40, 40), 0.0011, 1, 7)]], 8), 2, score_floor=0.001))
    cases.append(_case("concentric", pack([[(box(50, 50, 20, 20), 0.9, 0, 100), (box(50, 50, 16, 16), 0.8, 0, 101), (box(50, 50, 10, 10), 0.7, 0, 102),
                                            (box(50, 50, 24, 18), 0.6, 1, 103)]], 4), 2, nms_thresh=0.5))
    # shift 3: IoU 0.538, DIoU 0.538 - 9 / (13^2 + 10^2) = 0.505 -- either side of 0.52
    cases.append(_case("offset_iou_vs_diou", pack([[(box(100, 50, 10, 10), 0.9, 0, 1), (box(103, 50, 10, 10), 0.8, 0, 2), (box(100, 53, 10, 10), 0.7, 1, 3)]], 4), 2,
                       nms_thresh=0.52))
    img = random_image(rs, 12, 3, clusters=2)
    img[3] = (img[3][0], img[3][1], -1, img[3][3])
    img[7] = (img[7][0], np.float32(0.9995), 3, img[7][3])          # a class past the last one, at the top rank
    cases.append(_case("class_minus_one", pack([img], 16, filter_order=False), 3))
    out = pack([random_image(rs, 20, 3), -70, random_image(rs, 9, 3), 17], 16 + 8)
    out[4][3] = 25                                                     # (a count past the rows: passed through as well)
    for b in (1, 3):                                                   # what must come back untouched is not the filter's zeros
        out[0][b], out[1][b], out[2][b], out[3][b] = rs.uniform(1, 90, (24, 4)), rs.uniform(0, 1, 24), rs.randint(0, 3, 24), rs.randint(0, A, 24)
    cases.append(_case("bad_counts_among_good", out, 3))
    return cases


CASES = make_cases()

# every method x overlap x class-agnostic combination the library accepts
COMBOS = [(m, o, a) for m in ("nongreedy", "greedy", "soft_linear", "soft_gaussian") for o in ("iou", "diou") for a in (False, True)
          if not (o == "diou" and m.startswith("soft"))]
