"""Seeded synthetic KITTI trees with detection files for the GPU KITTI evaluator (squeezedet_amd/kitti_ap.py): shared by
make_kitti_ap_golden.py (which records what the reference evaluator wrote for them) and the tests.

Each case covers the corners of the metric: every label type (Car, Van, Pedestrian, Person_sitting, Cyclist, DontCare,
Truck / Misc / Tram, in mixed letter case), heights of exactly 25.00 / 40.00, truncation 0.15 / 0.30 / 0.50 (and just
above), occlusion 0-3, several detections per object, equal '%.3f' scores, detections inside DontCare regions, images
without ground truth or without detections."""
import os

import numpy as np

CLASSES = ("car", "pedestrian", "cyclist")
# (label type, class index of its detections or -1)
TYPES = [("Car", 0), ("car", 0), ("Van", 0), ("Pedestrian", 1), ("PEDESTRIAN", 1), ("Person_sitting", 1), ("Cyclist", 2),
         ("DontCare", -1), ("Truck", 0), ("Misc", -1), ("Tram", -1)]
CASES = {
    # name: (images, max objects per image, detect cyclists, extra false positives per image, detections per image cap)
    "mixed": (60, 9, False, 3, None),      # cyclists never detected: no cyclist files
    "all": (90, 12, True, 4, None),
    "few": (6, 3, True, 1, None),          # fewer than 41 true positives per class
    "large": (3769, 10, True, 64, 64),     # a KITTI-val-sized set, 64 detections per image
    # more than one wave of 64 lanes in one image: 000001 has 105 objects and 81 car rows among its 150 detections
    # (90 objects, the first choice, gave no image with both more than 64 objects and more than 64 rows of one class)
    "wave": (8, 128, True, 40, 150),
}


def _label_line(t, trunc, occ, box):
    x1, y1, x2, y2 = box
    if t == "DontCare":
        return "DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10\n" % (x1, y1, x2, y2)
    return "%s %.2f %d -1.57 %.2f %.2f %.2f %.2f 1.50 1.60 3.90 1.00 1.70 20.00 -1.50\n" % (t, trunc, occ, x1, y1, x2, y2)


def make_case(name, root):
    """Writes <root>/training/label_2, <root>/ImageSets/val.txt and <root>/det/data (the detection files) for `name`.
    Returns (image indices, det result dir)."""
    n_images, max_obj, with_cyclist, n_fp, cap = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    os.makedirs(os.path.join(root, "training", "label_2"))
    os.makedirs(os.path.join(root, "ImageSets"))
    det_dir = os.path.join(root, "det", "data")
    os.makedirs(det_dir)
    idxs = ["%06d" % i for i in range(n_images)]
    score_pool = np.round(rs.uniform(0.05, 1.0, 40), 3)          # shared scores: ties at '%.3f'
    for k, idx in enumerate(idxs):
        nobj = 0 if k % 7 == 3 else rs.randint(0, max_obj + 1)
        lines, dets = [], []
        for _ in range(nobj):
            t, c = TYPES[rs.randint(len(TYPES))]
            x1, y1 = round(rs.uniform(0, 1100), 2), round(rs.uniform(0, 300), 2)
            w = round(rs.uniform(8, 200), 2)
            h = [25.0, 40.0, 24.99, 39.99, round(rs.uniform(10, 160), 2)][rs.randint(5)]
            if rs.uniform() < 0.5:      # heights of exactly 25.00 / 40.00 from whole-pixel rows
                y1 = float(int(y1))
            box = (x1, y1, x1 + w, y1 + h)
            trunc = [0.0, 0.15, 0.3, 0.5, 0.51, 0.16, 0.8][rs.randint(7)]
            occ = rs.randint(0, 4)
            lines.append(_label_line(t, trunc, occ, box))
            if t == "DontCare":          # detections of every class inside / overlapping the region
                for _ in range(rs.randint(0, 3)):
                    cx, cy = x1 + rs.uniform(0.2, 0.8) * w, y1 + rs.uniform(0.2, 0.8) * h
                    dets.append((rs.randint(3), (cx - w / 5, cy - h / 5, cx + w / 5, cy + h / 5)))
                continue
            if c < 0:
                continue
            for _ in range(rs.randint(0, 4)):    # several detections per object, some of the wrong class
                j = rs.normal(0, 0.06, 4) * np.array([w, h, w, h])
                dc = c if rs.uniform() < 0.85 else rs.randint(3)
                dets.append((dc, (box[0] + j[0], box[1] + j[1], box[2] + j[2], box[3] + j[3])))
        if k % 11 == 5:
            dets = []                                               # an image without detections
        else:
            for _ in range(rs.randint(0, n_fp + 1)):
                x1, y1 = rs.uniform(0, 1200), rs.uniform(0, 370)
                dets.append((rs.randint(3), (x1, y1, x1 + rs.uniform(5, 150), y1 + rs.uniform(5, 150))))
        if not with_cyclist:
            dets = [d for d in dets if d[0] != 2]
        if cap:
            dets = dets[:cap]
            while len(dets) < cap and nobj:
                x1, y1 = rs.uniform(0, 1200), rs.uniform(0, 370)
                dets.append((rs.randint(3), (x1, y1, x1 + rs.uniform(5, 150), y1 + rs.uniform(5, 150))))
        with open(os.path.join(root, "training", "label_2", idx + ".txt"), "w") as f:
            f.writelines(lines)
        with open(os.path.join(det_dir, idx + ".txt"), "w") as f:
            for c in range(3):         # class-major, as kitti_eval.write_detection_files writes them
                for dc, b in dets:
                    if dc == c:
                        s = score_pool[rs.randint(len(score_pool))] if rs.uniform() < 0.6 else rs.uniform(0, 1)
                        f.write("{:s} -1 -1 0.0 {:.2f} {:.2f} {:.2f} {:.2f} 0.0 0.0 0.0 0.0 0.0 0.0 0.0 {:.3f}\n".format(
                            CLASSES[c], b[0], b[1], b[2], b[3], s))
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join(idxs) + "\n")
    return idxs, os.path.dirname(det_dir)


def stats_files(result_dir):
    """{file name: text} of the evaluator's stats files in result_dir."""
    out = {}
    for c in CLASSES:
        for kind in ("ap", "detection"):
            fn = os.path.join(result_dir, "stats_%s_%s.txt" % (c, kind))
            if os.path.exists(fn):
                with open(fn) as f:
                    out["stats_%s_%s.txt" % (c, kind)] = f.read()
    return out
