"""KITTI 2D average precision on the GPU (include/sqdet.h, csrc/kitti_eval.hip; the table: det_table.py): the scoring half
of the reference's src/eval.py without detection files or an external evaluator.

  load_kitti(data_path, image_set, mc)     the dataset reader of dataset/kitti.py:14-90: image paths, the `rois` lists
                                           (BatchReader / analysis) and the evaluator's raw ground truth
  KittiEvaluator(mc, gt, device)           a device detection table fed straight from filter_prediction_batch rows;
                                           evaluate() / analyze() / write_stats() / write_error_file()
  evaluate_detection_files(root, set, dir) the same scoring fed from KITTI detection files on disk (what the evaluator
                                           binary is run on in kitti_eval.evaluate_detections)

The values in the table are those the evaluator reads back from the files the reference writes, and the stats files
written here are byte for byte the evaluator's.  The label and detection parsers use float(), which rounds decimal text
to the nearest double as glibc's %lf does."""
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, stream_ptr
from .det_table import MAX_DETECTIONS, MAX_GROUNDTRUTH, DetectionTable, host_ptr as P, ptr as _ptr, row_offsets  # noqa: F401
from .util import bbox_transform_inv

CLASS_NAMES = ("car", "pedestrian", "cyclist")                  # the evaluator's classes (= kitti.py:22)
# the evaluator's type names, compared case-insensitively (strcasecmp); anything else is "other"
TYPE_CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
TYPE_OTHER = 6
DIFFICULTIES = ("easy", "medium", "hard")
ERROR_TYPES = ("loc", "cls", "bg", "missed")                     # SQDET_KITTI_ERR_*
ANALYSIS_KEYS = ("num of detections", "num of objects", "% correct detections", "% localization error",
                 "% classification error", "% background error", "% repeated error", "% recall")

KittiSet = namedtuple("KittiSet", "image_idx image_paths rois gt")


def type_code(name):
    return TYPE_CODES.get(name.lower(), TYPE_OTHER)


def read_image_set(data_path, image_set):
    """ImageSets/<image_set>.txt -> image indices (kitti._load_image_set_idx)."""
    fn = os.path.join(data_path, "ImageSets", image_set + ".txt")
    if not os.path.exists(fn):
        raise FileNotFoundError("File does not exist: {}".format(fn))
    with open(fn) as f:
        return f.read().split()


def parse_label_file(path):
    """A KITTI label file as the evaluator's loadGroundtruth reads it: objects of 15 whitespace-separated fields
    (type, truncation, occlusion, alpha, x1, y1, x2, y2, 7 more), up to the first that does not parse.
    -> list of (type code, x1, y1, x2, y2, truncation, occlusion)."""
    with open(path) as f:
        tok = f.read().split()
    rows = []
    for k in range(0, len(tok) - 14, 15):
        o = tok[k:k + 15]
        try:
            vals = [float(v) for v in o[4:8]]
            trunc, occ = float(o[1]), int(o[2])
            [float(v) for v in o[3:4] + o[8:15]]
        except ValueError:
            break
        rows.append((type_code(o[0]), vals[0], vals[1], vals[2], vals[3], trunc, occ))
    return rows


def _obj_level(obj):
    """kitti._get_obj_level: 1 easy .. 3 hard, 4 beyond (the height carries bbox_transform_inv's +1)."""
    height = float(obj[7]) - float(obj[5]) + 1
    truncation, occlusion = float(obj[1]), float(obj[2])
    if height >= 40 and truncation <= 0.15 and occlusion <= 0:
        return 1
    if height >= 25 and truncation <= 0.3 and occlusion <= 1:
        return 2
    if height >= 25 and truncation <= 0.5 and occlusion <= 2:
        return 3
    return 4


def parse_rois(path, class_names=CLASS_NAMES, exclude_hard=False):
    """kitti._load_kitti_annotation for one label file: [cx, cy, w, h, cls] per object of a known class (case-insensitive),
    hard objects left out when exclude_hard (mc.EXCLUDE_HARD_EXAMPLES)."""
    class_to_idx = {c: i for i, c in enumerate(class_names)}
    rois = []
    with open(path) as f:
        lines = f.readlines()
    for line in lines:
        obj = line.strip().split(" ")
        cls = class_to_idx.get(obj[0].lower().strip())
        if cls is None:
            continue
        if exclude_hard and _obj_level(obj) > 3:
            continue
        xmin, ymin, xmax, ymax = float(obj[4]), float(obj[5]), float(obj[6]), float(obj[7])
        assert 0.0 <= xmin <= xmax, "Invalid bounding box x-coord xmin {} or xmax {} at {}".format(xmin, xmax, path)
        assert 0.0 <= ymin <= ymax, "Invalid bounding box y-coord ymin {} or ymax {} at {}".format(ymin, ymax, path)
        x, y, w, h = bbox_transform_inv([xmin, ymin, xmax, ymax])
        rois.append([x, y, w, h, cls])
    return rois


class GroundTruth:
    """Host tables of one image set: the evaluator's rows (offsets int32 [N+1], box float64 [G,4] x1,y1,x2,y2, truncation,
    occlusion, type) and the analysis rois (roi_offsets, roi_box float64 [R,4] cx,cy,w,h, roi_cls)."""

    def __init__(self, raw, rois):
        if len(raw) != len(rois):
            raise ValueError("GroundTruth: %d label lists for %d roi lists" % (len(raw), len(rois)))
        self.num_images = len(raw)
        self.offsets, flat = row_offsets(raw, "KITTI evaluation: image %d has %d ground-truth rows (limit %d)")
        self.roi_offsets, rflat = row_offsets(rois, "KITTI evaluation: image %d has %d roi rows (limit %d)")
        self.box = np.array([row[1:5] for row in flat], np.float64).reshape(-1, 4)
        self.truncation = np.array([row[5] for row in flat], np.float64)
        self.occlusion = np.array([row[6] for row in flat], np.int32)
        self.type = np.array([row[0] for row in flat], np.int32)
        self.roi_box = np.array([row[:4] for row in rflat], np.float64).reshape(-1, 4)
        self.roi_cls = np.array([int(row[4]) for row in rflat], np.int32)


def load_kitti(data_path, image_set, mc):
    """The reference's kitti imdb without the batch reader: image indices, image paths, rois (kitti._rois order; class
    names and EXCLUDE_HARD_EXAMPLES from mc) and the ground truth the evaluator reads, from <data_path>/training/label_2."""
    idx = read_image_set(data_path, image_set)
    label_dir = os.path.join(data_path, "training", "label_2")
    image_dir = os.path.join(data_path, "training", "image_2")
    raw, rois = [], []
    for i in idx:
        fn = os.path.join(label_dir, i + ".txt")
        raw.append(parse_label_file(fn))
        rois.append(parse_rois(fn, tuple(mc.CLASS_NAMES), bool(mc.EXCLUDE_HARD_EXAMPLES)))
    return KittiSet(idx, [os.path.join(image_dir, i + ".png") for i in idx], rois, GroundTruth(raw, rois))


# ---- the evaluator's number formatting (x86-64 glibc; 0/0 there is the negative default NaN) ----
def cpp_float_g(x):
    """`std::ostream << double` with default settings (%g, 6 significant digits)."""
    return "-nan" if math.isnan(x) else "%g" % x


def cpp_float_f(x):
    """printf("%f")."""
    return "-nan" if math.isnan(x) else "%f" % x


def format_stats(precision3):
    """The two stats files of one class from its [3, 41] precision: (stats_<cls>_ap.txt, stats_<cls>_detection.txt)."""
    ap_txt, det_txt = "", ""
    for p in precision3:
        ap = 0.0
        for i in range(0, 41, 4):
            ap += float(p[i])
            det_txt += cpp_float_f(float(p[i])) + " "
        ap /= 11.0
        ap_txt += "AP=%s\n" % cpp_float_g(ap)
        det_txt += "\n"
    return ap_txt, det_txt


def parse_checkpoint_step(path):
    """Global step of a checkpoint file, as eval.py takes it from 'model.ckpt-<step>': the text after the last '-' of the
    file name, here without the '.npz' extension."""
    name = os.path.basename(path)
    if name.endswith(".npz"):
        name = name[:-4]
    return name.split("-")[-1]


class KittiEvaluator(DetectionTable):
    """Device detection table for one image set + the scoring calls.  gt: a GroundTruth (load_kitti(...).gt).
    max_detections: rows per image the table holds (>= the filter's max_out; default mc.TOP_N_DETECTION, else 512)."""

    def __init__(self, mc, gt, device="cuda:0", max_detections=None):
        if tuple(c.lower() for c in mc.CLASS_NAMES) != CLASS_NAMES:
            raise _lib.SqdetError("KittiEvaluator: the KITTI classes %s are required, got %s" % (CLASS_NAMES, mc.CLASS_NAMES))
        super().__init__(mc, gt, device, max_detections)
        up = self.up
        self.gt_box, self.gt_trunc = up(gt.box, torch.float64), up(gt.truncation, torch.float64)
        self.gt_occ, self.gt_type = up(gt.occlusion, torch.int32), up(gt.type, torch.int32)
        self.roi_offsets, self.roi_box, self.roi_cls = up(gt.roi_offsets, torch.int32), up(gt.roi_box, torch.float64), up(gt.roi_cls, torch.int32)
        self.num_rois = int(gt.roi_offsets[-1])
        self.precision = self.aps_raw = self.evaluated = self.analysis = None
        self._records = None

    def _workspace_bytes(self):
        return lib().sqdet_kitti_eval_workspace_bytes(self.num_gt)

    def _ingest(self, src, dst):
        check(lib().sqdet_kitti_ingest(*src, *dst), "sqdet_kitti_ingest")

    def evaluate(self):
        """-> (aps, names, precision): aps / names exactly as kitti_eval.evaluate_detections returns them (an AP read back
        from its 'AP=%g' text; 0 for a class never detected), precision float64 [9, 41] (class-major, easy / medium / hard).
        One host synchronisation."""
        prec = np.zeros((9, 41), np.float64)
        ap = np.zeros(9, np.float64)
        ev = np.zeros(3, np.int32)
        check(lib().sqdet_kitti_evaluate(*self.scoring_args(), _ptr(self.gt_offsets), _ptr(self.gt_box),
                                         _ptr(self.gt_trunc), _ptr(self.gt_occ), _ptr(self.gt_type), self.num_gt,
                                         _ptr(self.workspace), P(prec), P(ap), P(ev), stream_ptr()), "sqdet_kitti_evaluate")
        self.precision, self.aps_raw, self.evaluated = prec, ap, ev
        aps, names = [], []
        for c, name in enumerate(CLASS_NAMES):
            if ev[c]:
                aps.extend(float(line.split("=")[1]) for line in format_stats(prec[3 * c:3 * c + 3])[0].splitlines())
            else:
                aps.extend([0.0, 0.0, 0.0])
            names.extend(name + "_" + d for d in DIFFICULTIES)
        return aps, names, prec

    def write_stats(self, result_dir):
        """stats_<cls>_ap.txt and stats_<cls>_detection.txt of every evaluated class, as the evaluator writes them."""
        if self.precision is None:
            self.evaluate()
        os.makedirs(result_dir, exist_ok=True)
        for c, name in enumerate(CLASS_NAMES):
            if not self.evaluated[c]:
                continue
            ap_txt, det_txt = format_stats(self.precision[3 * c:3 * c + 3])
            with open(os.path.join(result_dir, "stats_%s_ap.txt" % name), "w") as f:
                f.write(ap_txt)
            with open(os.path.join(result_dir, "stats_%s_detection.txt" % name), "w") as f:
                f.write(det_txt)

    def analyze(self):
        """kitti.analyze_detections on the table -> the reference's dict (NaN where it would divide by zero)."""
        n, R = self.gt.num_images, max(1, self.num_rois)
        dev = self.device
        counters = torch.empty((9,), dtype=torch.int32, device=dev)
        rec_count = torch.empty((n,), dtype=torch.int32, device=dev)
        rec_type = torch.empty((2 * R,), dtype=torch.int32, device=dev)
        rec_cls = torch.empty((2 * R,), dtype=torch.int32, device=dev)
        rec_box = torch.empty((2 * R, 4), dtype=torch.float64, device=dev)
        rec_score = torch.empty((2 * R,), dtype=torch.float64, device=dev)
        check(lib().sqdet_kitti_analyze(*self.table_args(), n, self.cap,
                                        _ptr(self.roi_offsets), _ptr(self.roi_box), _ptr(self.roi_cls), self.num_rois, _ptr(counters),
                                        _ptr(rec_count), _ptr(rec_type), _ptr(rec_cls), _ptr(rec_box), _ptr(rec_score), stream_ptr()),
              "sqdet_kitti_analyze")
        cnt = counters.cpu().numpy().astype(np.int64)
        st = self.status.cpu().numpy()
        if st[0]:
            raise _lib.SqdetError("kitti analyze: the detection table holds a rejected ingest; reset it")
        if cnt[8]:
            raise _lib.SqdetUnsupported("kitti analyze: an image is over the row limits")
        self._records = (rec_count.cpu().numpy(), rec_type.cpu().numpy(), rec_cls.cpu().numpy(), rec_box.cpu().numpy(),
                         rec_score.cpu().numpy())
        self.counters = cnt[:8]
        dets, objs, correct, loc, clse, bg, rep, detected = [float(v) for v in cnt[:8]]
        div = lambda a, b: a / b if b else float("nan")
        self.analysis = dict(zip(ANALYSIS_KEYS, (dets, objs, div(correct, dets), div(loc, dets), div(clse, dets), div(bg, dets),
                                                 div(rep, dets), div(detected, objs))))
        return self.analysis

    def error_records(self):
        """[(image position, error type, cx, cy, w, h, class index, score)] in det_error_file.txt order."""
        if self._records is None:
            self.analyze()
        rc, rt, rcl, rb, rs = self._records
        out = []
        for i in range(self.gt.num_images):
            base = 2 * int(self.gt.roi_offsets[i])
            for r in range(base, base + int(rc[i])):
                out.append((i, ERROR_TYPES[rt[r]], rb[r, 0], rb[r, 1], rb[r, 2], rb[r, 3], int(rcl[r]), rs[r]))
        return out

    def write_error_file(self, path, image_idx):
        """det_error_file.txt of kitti.analyze_detections (image_idx: the image names)."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            for i, t, cx, cy, w, h, c, s in self.error_records():
                f.write("{:s} {:s} {:.1f} {:.1f} {:.1f} {:.1f} {:s} {:.3f}\n".format(
                    image_idx[i], t, cx - w / 2., cy - h / 2., cx + w / 2., cy + h / 2., self.mc.CLASS_NAMES[c], s))

    def write_detection_files(self, det_file_dir, image_idx):
        """The detection files of kitti_eval.write_detection_files, from the table (each value is the double nearest to the
        text it came from, so formatting it again gives that text)."""
        os.makedirs(det_file_dir, exist_ok=True)
        for idx, rows in zip(image_idx, self.tables()):
            with open(os.path.join(det_file_dir, idx + ".txt"), "wt") as f:
                for c, x1, y1, x2, y2, s in rows:
                    f.write("{:s} -1 -1 0.0 {:.2f} {:.2f} {:.2f} {:.2f} 0.0 0.0 0.0 0.0 0.0 0.0 0.0 {:.3f}\n".format(
                        CLASS_NAMES[c], x1, y1, x2, y2, s))


def parse_detection_file(path):
    """A detection file as the evaluator's loadDetections reads it: objects of 16 fields (type, 2 ignored, alpha, x1, y1,
    x2, y2, 7 ignored, score), up to the first that does not parse; rows of other types than the three classes are
    dropped (the evaluator never matches them).  -> [(class index, x1, y1, x2, y2, score)]."""
    with open(path) as f:
        tok = f.read().split()
    rows = []
    for k in range(0, len(tok) - 15, 16):
        o = tok[k:k + 16]
        try:
            v = [float(x) for x in o[1:16]]
        except ValueError:
            break
        c = TYPE_CODES.get(o[0].lower(), TYPE_OTHER)
        if c < 3:
            rows.append((c, v[3], v[4], v[5], v[6], v[14]))
    return rows


def evaluate_detection_files(data_root_path, image_set, det_dir, mc=None, device="cuda:0"):
    """The evaluator binary's job on the GPU: scores <det_dir>/data/<index>.txt against
    <data_root_path>/training/label_2 for the images of ImageSets/<image_set>.txt, writes the stats files into det_dir
    and returns (aps, names) as kitti_eval.evaluate_detections does."""
    from .config import kitti_squeezeDet_config
    mc = mc or kitti_squeezeDet_config()
    idx = read_image_set(data_root_path, image_set)
    label_dir = os.path.join(data_root_path, "training", "label_2")
    raw = [parse_label_file(os.path.join(label_dir, i + ".txt")) for i in idx]
    rows = [parse_detection_file(os.path.join(det_dir, "data", i + ".txt")) for i in idx]
    ev = KittiEvaluator.from_rows(mc, GroundTruth(raw, [[] for _ in idx]), rows, device)
    aps, names, _ = ev.evaluate()
    ev.write_stats(det_dir)
    return aps, names
