"""Seeded, deterministic Pascal VOC cases for the GPU VOC evaluator (squeezedet_amd/voc.py, csrc/voc_eval.hip): shared by
make_voc_ap_golden.py (which records what the reference's pascal_voc.evaluate_detections / voc_eval computed for them, into
voc_ap.npz) and the tests.

A case is a dict:  names   the class names
                   image_idx  the image names, in image-set order
                   objects    per image [(name, xmin, ymin, xmax, ymax, difficult)], the XML's 1-based integers
                   rows       per image (boxes float32 [k,4] cx,cy,w,h, probs float32 [k], cls int32 [k]): filter_prediction
                              rows of the image in original-image pixels, in filter order (classes interleaved)
Each case is the smallest at which one step of the metric can go wrong; see CASES."""
import hashlib
import os

import numpy as np

PREFIX_BLOCK = 256      # rows the evaluator's prefix sum (voc_prefix_kernel, SCAN in csrc/voc_eval.hip) handles in one block:
#                         the largest class of `many` has more than PREFIX_BLOCK + 1 rows, so the carried total is exercised
VOC20 = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
         "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
YEAR, IMAGE_SET = "2007", "test"


class _Builder:
    def __init__(self, names):
        self.names, self.image_idx, self.objects, self.dets = tuple(names), [], [], []

    def image(self, objects=(), dets=()):
        """objects: (name, xmin, ymin, xmax, ymax, difficult); dets: (class index, (cx, cy, w, h), score), filter order."""
        self.image_idx.append("%06d" % (len(self.image_idx) + 1))
        self.objects.append([tuple(o) for o in objects])
        self.dets.append(list(dets))

    def case(self):
        rows = []
        for d in self.dets:
            rows.append((np.array([x[1] for x in d], np.float32).reshape(-1, 4), np.array([x[2] for x in d], np.float32),
                         np.array([x[0] for x in d], np.int32)))
        return dict(names=self.names, image_idx=list(self.image_idx), objects=self.objects, rows=rows)


def at(x1, y1, x2, y2):
    """The filter row (cx, cy, w, h) whose detection-file box (1-based) is x1, y1, x2, y2; exact for integers."""
    return ((x1 + x2) / 2.0 - 1.0, (y1 + y2) / 2.0 - 1.0, float(x2 - x1), float(y2 - y1))


def _single():
    b = _Builder(("car",))
    b.image([("car", 10, 10, 50, 50, 0)], [(0, at(10, 10, 50, 50), 0.9)])
    return b.case()


def _greedy():
    b = _Builder(("car", "person"))
    b.image([("car", 1, 1, 10, 10, 0), ("car", 100, 100, 150, 150, 1), ("person", 200, 200, 260, 300, 0)],
            [(0, at(1, 1, 10, 10), 0.9),           # a hit
             (1, at(201, 200, 260, 300), 0.95),    # a hit of the other class
             (0, at(1, 1, 10, 9), 0.8),            # the same object again: false positive
             (0, at(100, 100, 150, 150), 0.7),     # on the difficult object: neither
             (1, at(10, 10, 60, 60), 0.45)])       # misses
    b.image([("car", 1, 1, 10, 10, 0)], [(0, at(1, 1, 10, 5), 0.85)])      # overlap 50 / 100 = exactly 0.5: not a hit
    b.image([("person", 30, 30, 80, 90, 0)], [(0, at(30, 30, 80, 90), 0.5)])   # no object of its class in the image
    b.image([("car", 40, 40, 90, 90, 1)], [])                                # difficult, never detected: not in npos
    return b.case()


def _argmax_first():
    b = _Builder(("car",))
    b.image([("car", 10, 10, 29, 29, 0), ("car", 12, 10, 31, 29, 0)],
            [(0, at(11, 10, 30, 29), 0.9),     # overlap 380 / 420 with both: the first wins
             (0, at(13, 10, 32, 29), 0.8),     # best on the second: takes it
             (0, at(11, 10, 30, 29), 0.7)])    # equal again: the first, already taken -> false positive
    return b.case()


def _arange_edge():
    """npos = 10; tp, tp, tp, fp, fp, tp, tp, tp, fp, tp, fp, fp in score order: recall lands exactly on 0.3, 0.6 and 0.7,
    and 3 * 0.1 > 0.3, 6 * 0.1 > 0.6, 7 * 0.1 > 0.7 in double."""
    b = _Builder(("dog",))
    objs = [("dog", 1 + 60 * k, 1, 50 + 60 * k, 50, 0) for k in range(2)]
    pattern = [1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 0]
    dets = [[] for _ in range(5)]
    hit = 0
    for r, p in enumerate(pattern):
        score = 0.95 - 0.05 * r
        if p:
            img, k = hit // 2, hit % 2
            dets[img].append((0, at(1 + 60 * k, 1, 50 + 60 * k, 50), score))
            hit += 1
        else:
            dets[r % 5].append((0, at(300, 300, 340, 340), score))
    for i in range(5):
        b.image(objs, dets[i])
    return b.case()


def _scores(rs, n):
    """n scores that print differently at '%.3f'."""
    return [(int(v) + 0.25) / 1000.0 for v in rs.permutation(np.arange(5, 1000))[:n]]


def _long_segments():
    """One image, one class, 70 objects and 70 detections: more than a wave of each."""
    rs = np.random.RandomState(70)
    b = _Builder(("sheep",))
    objs = [("sheep", 5 + 40 * (k % 10), 5 + 40 * (k // 10), 34 + 40 * (k % 10), 34 + 40 * (k // 10), int(k % 9 == 4)) for k in range(70)]
    sc = _scores(rs, 70)
    dets = []
    for j in range(70):
        if j < 50:
            o = objs[rs.randint(70) if j % 5 == 0 else j]            # every fifth lands on a random (maybe taken) object
            d = rs.randint(-4, 5, 4)
            dets.append((0, at(o[1] + d[0], o[2] + d[1], o[3] + d[2], o[4] + d[3]), sc[j]))
        else:
            x, y = rs.randint(1, 380), rs.randint(300, 400)
            dets.append((0, at(x, y, x + rs.randint(5, 40), y + rs.randint(5, 40)), sc[j]))
    b.image(objs, [dets[k] for k in rs.permutation(70)])
    return b.case()


def _seeded(names, n_images, seed, heavy=None, never=None, all_difficult=None, cap=64):
    rs = np.random.RandomState(seed)
    C = len(names)
    b = _Builder(names)
    pools = [_scores(rs, 990) for _ in range(C)]
    for k in range(n_images):
        objs, dets = [], []
        nobj = 0 if k % 7 == 3 else rs.randint(1, 7)
        for _ in range(nobj):
            c = rs.randint(C)
            x1, y1 = rs.randint(1, 400), rs.randint(1, 280)
            w, h = rs.randint(12, 120), rs.randint(12, 90)
            diff = 1 if c == all_difficult else int(rs.uniform() < 0.2)
            objs.append((names[c], x1, y1, x1 + w, y1 + h, diff))
            for _ in range(rs.randint(0, 4)):                        # several detections per object, some of another class
                j = rs.normal(0, 0.08, 4) * np.array([w, h, w, h])
                dc = c if rs.uniform() < 0.85 else rs.randint(C)
                dets.append((dc, (x1 + w / 2.0 + j[0], y1 + h / 2.0 + j[1], w + j[2], h + j[3])))
        if k % 11 != 5:
            for _ in range(rs.randint(0, 4) + (rs.randint(9, 16) if heavy is not None else 0)):
                dc = heavy if heavy is not None and rs.uniform() < 0.8 else rs.randint(C)
                dets.append((dc, (rs.uniform(10, 480), rs.uniform(10, 350), rs.uniform(8, 150), rs.uniform(8, 120))))
        else:
            dets = []                                                # an image without detections
        dets = [d for d in dets if d[0] != never][:cap]
        dets = [dets[i] for i in rs.permutation(len(dets))]
        b.image(objs, [(dc, box, pools[dc].pop()) for dc, box in dets])
    return b.case()


def _many():
    """37 images, 5 classes: class 0 has more than PREFIX_BLOCK + 1 rows, class 3 is never detected, class 4 has detections
    and only difficult objects (npos = 0); images without detections (k % 11 == 5) and without objects (k % 7 == 3)."""
    case = _seeded(("a", "b", "c", "d", "e"), 37, 37, heavy=0, never=3, all_difficult=4)
    n0 = sum(int((r[2] == 0).sum()) for r in case["rows"])
    assert n0 > PREFIX_BLOCK + 1, n0
    return case


def _ties():
    """Equal scores in different images, all with the same outcome: every order of the tied rows gives the same curve."""
    b = _Builder(("cat",))
    for k in range(3):
        dets = [(0, at(20, 20, 80, 80), 0.5)]
        if k == 0:
            dets.append((0, at(200, 200, 240, 240), 0.9))
        if k >= 1:
            dets.append((0, at(200, 200, 240, 240), 0.3))
        b.image([("cat", 20, 20, 80, 80, 0)], dets)
    return b.case()


def _voc20():
    return _seeded(VOC20, 6, 20)


def _wide():
    """300 images, 2 classes: more images than PREFIX_BLOCK, so where an image's rows start in its class's list needs the total
    carried from the images before (the evaluator's scan over images works PREFIX_BLOCK at a time).  1-2 objects and 0-3
    detections in most images; images without detections (k % 11 == 5) and without objects (k % 7 == 3)."""
    rs = np.random.RandomState(300)
    names = ("a", "b")
    b = _Builder(names)
    pools = [_scores(rs, 990) for _ in names]
    for k in range(300):
        objs, dets = [], []
        for _ in range(0 if k % 7 == 3 else rs.randint(1, 3)):
            c = rs.randint(2)
            x1, y1 = rs.randint(1, 400), rs.randint(1, 280)
            objs.append((names[c], x1, y1, x1 + rs.randint(12, 120), y1 + rs.randint(12, 90), int(rs.uniform() < 0.2)))
        for _ in range(0 if k % 11 == 5 else rs.randint(0, 4)):
            if objs and rs.uniform() < 0.6:                         # on an object, mostly of its class
                name, x1, y1, x2, y2, _ = objs[rs.randint(len(objs))]
                w, h = x2 - x1, y2 - y1
                j = rs.normal(0, 0.08, 4) * np.array([w, h, w, h])
                dc = names.index(name) if rs.uniform() < 0.85 else rs.randint(2)
                dets.append((dc, (x1 + w / 2.0 + j[0], y1 + h / 2.0 + j[1], w + j[2], h + j[3])))
            else:
                dets.append((rs.randint(2), (rs.uniform(10, 480), rs.uniform(10, 350), rs.uniform(8, 150), rs.uniform(8, 120))))
        b.image(objs, [(dc, box, pools[dc].pop()) for dc, box in dets])
    assert len(b.image_idx) > PREFIX_BLOCK
    return b.case()


CASES = {"single": _single, "greedy": _greedy, "argmax_first": _argmax_first, "arange_edge": _arange_edge,
         "long_segments": _long_segments, "many": _many, "ties": _ties, "voc20": _voc20, "wide": _wide}


def make_case(name):
    return CASES[name]()


def annotation_xml(index, objects):
    out = ["<annotation>", "\t<folder>VOC2007</folder>", "\t<filename>%s.jpg</filename>" % index]
    for name, x1, y1, x2, y2, diff in objects:
        out += ["\t<object>", "\t\t<name>%s</name>" % name, "\t\t<pose>Unspecified</pose>", "\t\t<truncated>0</truncated>",
                "\t\t<difficult>%d</difficult>" % diff, "\t\t<bndbox>", "\t\t\t<xmin>%d</xmin>" % x1, "\t\t\t<ymin>%d</ymin>" % y1,
                "\t\t\t<xmax>%d</xmax>" % x2, "\t\t\t<ymax>%d</ymax>" % y2, "\t\t</bndbox>", "\t</object>"]
    return "\n".join(out + ["</annotation>"]) + "\n"


def write_tree(case, root, year=YEAR, image_set=IMAGE_SET):
    """Writes the case as <root>/VOC<year>/{Annotations/<idx>.xml, ImageSets/Main/<image_set>.txt} (no images)."""
    voc = os.path.join(root, "VOC" + year)
    os.makedirs(os.path.join(voc, "Annotations"))
    os.makedirs(os.path.join(voc, "ImageSets", "Main"))
    for index, objects in zip(case["image_idx"], case["objects"]):
        with open(os.path.join(voc, "Annotations", index + ".xml"), "w") as f:
            f.write(annotation_xml(index, objects))
    with open(os.path.join(voc, "ImageSets", "Main", image_set + ".txt"), "w") as f:
        f.write("".join(i + "\n" for i in case["image_idx"]))
    return voc


def padded_rows(case):
    """The case's rows as filter_prediction_batch delivers them: boxes float32 [N, M, 4], probs float32 [N, M], cls int32
    [N, M], count int32 [N] (M = the largest count, at least 1)."""
    n = len(case["rows"])
    m = max([1] + [len(r[1]) for r in case["rows"]])
    boxes, probs = np.zeros((n, m, 4), np.float32), np.zeros((n, m), np.float32)
    cls, count = np.zeros((n, m), np.int32), np.zeros(n, np.int32)
    for i, (b, p, c) in enumerate(case["rows"]):
        k = len(p)
        boxes[i, :k], probs[i, :k], cls[i, :k], count[i] = b, p, c, k
    return boxes, probs, cls, count


def table_rows(case):
    """Per image [(class index, x1, y1, x2, y2, score)], class-major: the values float() reads back from the detection
    files the reference writes for the case's rows (float32 bbox_transform, + 1 in float32, '{:.1f}'; '{:.3f}')."""
    one, two = np.float32(1), np.float32(2)
    out = []
    for b, p, c in case["rows"]:
        rows = []
        for k in np.argsort(c, kind="stable"):
            cx, cy, w, h = b[k]
            box = [cx - w / two + one, cy - h / two + one, cx + w / two + one, cy + h / two + one]
            rows.append((int(c[k]),) + tuple(float("{:.1f}".format(v)) for v in box) + (float("{:.3f}".format(p[k])),))
        out.append(rows)
    return out


def digest_dir(directory):
    """sha256 over (file name, content) of every file of a directory, in name order."""
    h = hashlib.sha256()
    for fn in sorted(os.listdir(directory)):
        h.update(fn.encode() + b"\0")
        with open(os.path.join(directory, fn), "rb") as f:
            h.update(f.read() + b"\0")
    return h.hexdigest()
