"""COCO-style detection metrics on the GPU (include/sqdet.h "COCO-style evaluation", csrc/coco_eval.hip; the table:
det_table.py): average precision over IoU 0.50:0.05:0.95 by object size and average recall at 1 / 10 / 100 detections -- the
published COCOeval bbox protocol -- and COCO-format files.

  CocoGroundTruth(per_image_rows)            rows (cls, x, y, w, h, area, iscrowd, ignore); from_voc / from_kitti / from_json
  CocoEvaluator(mc, gt, device)              a device detection table of (x, y, w, h) rows fed straight from
                                             filter_prediction_batch rows; evaluate() / summarize() / write_results_json()
  evaluate_results_file(annotations, results, device)   scores a COCO results file against a COCO annotation file
  summarize_arrays(precision, recall, ...)   the twelve statistics from the two arrays (host NumPy)

This is a metric over the datasets the drivers have, and a file format; it adds no dataset."""
import json

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, stream_ptr
from .det_table import MAX_DETECTIONS, MAX_GROUNDTRUTH, DetectionTable, host_ptr as P, ptr as _ptr, row_offsets  # noqa: F401

MAX_CLASSES = 128                                                # SQDET_COCO_MAX_CLASSES
MAX_KEPT = 128                                                   # SQDET_COCO_MAX_KEPT: the largest maxDets
IGNORE, CROWD = 1, 2                                             # bits of the ground truth's flag word

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNGS = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
AREA_LABELS = ("all", "small", "medium", "large")
MAX_DETS = (1, 10, 100)


class CocoGroundTruth:
    """Host tables of one image set: offsets int32 [N+1], box float64 [G,4] (x, y, w, h), cls int32 [G], area float64 [G],
    flags int32 [G] (bit 0 ignore, bit 1 iscrowd).  per_image_rows: per image a list of (cls, x, y, w, h, area, iscrowd,
    ignore).  class_names, image_ids, category_ids: what a reader knows of them (None otherwise)."""

    def __init__(self, per_image_rows, class_names=None, image_ids=None, category_ids=None):
        self.num_images = len(per_image_rows)
        self.offsets, flat = row_offsets(per_image_rows, "COCO evaluation: image %d has %d objects (limit %d)")
        self.cls = np.array([row[0] for row in flat], np.int32)
        self.box = np.array([row[1:5] for row in flat], np.float64).reshape(-1, 4)
        self.area = np.array([row[5] for row in flat], np.float64)
        self.flags = np.array([(CROWD if row[6] else 0) | (IGNORE if row[7] else 0) for row in flat], np.int32)
        self.class_names = tuple(class_names) if class_names is not None else None
        self.image_ids = list(image_ids) if image_ids is not None else None
        self.category_ids = list(category_ids) if category_ids is not None else None

    @classmethod
    def from_voc(cls, gt, class_names=None):
        """A voc.GroundTruth: the XML's 1-based, pixel-inclusive corners become 0-based extents -- x = xmin - 1, y = ymin - 1,
        w = xmax - xmin + 1, h = ymax - ymin + 1 -- area = w * h, `difficult` sets the ignore bit; an object whose class is
        not in the class list (-1) is dropped."""
        rows = []
        for i in range(gt.num_images):
            r = []
            for k in range(int(gt.offsets[i]), int(gt.offsets[i + 1])):
                if gt.cls[k] < 0:
                    continue
                xmin, ymin, xmax, ymax = (float(v) for v in gt.box[k])
                w, h = xmax - xmin + 1, ymax - ymin + 1
                r.append((int(gt.cls[k]), xmin - 1, ymin - 1, w, h, w * h, 0, int(gt.difficult[k] != 0)))
            rows.append(r)
        return cls(rows, class_names)

    @classmethod
    def from_kitti(cls, gt, mc):
        """A kitti_ap.GroundTruth: an object whose type is one of mc.CLASS_NAMES becomes (x1, y1, x2 - x1, y2 - y1) of that
        class, area = w * h; every DontCare box becomes one crowd object PER CLASS (a detection of any class on it is
        ignored, and the region is never used up); every other type (van, person_sitting, ...) is dropped.

        This is a localisation metric over KITTI's boxes, NOT KITTI's protocol: there are no difficulty levels, and occlusion,
        truncation and the minimum box height are not looked at -- a heavily occluded car counts like any other."""
        from .kitti_ap import TYPE_CODES
        names = tuple(mc.CLASS_NAMES)
        code_to_cls = {TYPE_CODES[n.lower()]: i for i, n in enumerate(names) if n.lower() in TYPE_CODES}
        rows = []
        for i in range(gt.num_images):
            r = []
            for k in range(int(gt.offsets[i]), int(gt.offsets[i + 1])):
                x1, y1, x2, y2 = (float(v) for v in gt.box[k])
                w, h = x2 - x1, y2 - y1
                code = int(gt.type[k])
                if code == TYPE_CODES["dontcare"]:
                    r.extend((c, x1, y1, w, h, w * h, 1, 0) for c in range(len(names)))
                elif code in code_to_cls:
                    r.append((code_to_cls[code], x1, y1, w, h, w * h, 0, 0))
            rows.append(r)
        return cls(rows, names)

    @classmethod
    def from_json(cls, path, class_names=None):
        """A COCO annotation file: `images` ordered by id, `categories` ordered by id (or, with class_names, in that order,
        by name: a category of another name is dropped with its annotations), `annotations` in file order within their image;
        bbox (x, y, w, h), area from the file when present (else w * h), iscrowd and ignore from the file (default 0)."""
        with open(path) as f:
            d = json.load(f)
        image_ids = sorted(im["id"] for im in d["images"])
        cats = sorted(d["categories"], key=lambda c: c["id"])
        if class_names is not None:
            by_name = {c["name"]: c for c in cats}
            missing = [n for n in class_names if n not in by_name]
            if missing:
                raise _lib.SqdetError("from_json: %s has no category named %r" % (path, missing[0]))
            cats = [by_name[n] for n in class_names]
        cat_index = {c["id"]: i for i, c in enumerate(cats)}
        where = {iid: i for i, iid in enumerate(image_ids)}
        rows = [[] for _ in image_ids]
        for a in d.get("annotations", []):
            if a["category_id"] not in cat_index:
                continue
            if a["image_id"] not in where:
                raise _lib.SqdetError("from_json: annotation %r is of image %r, which %s does not list" % (a.get("id"), a["image_id"], path))
            x, y, w, h = (float(v) for v in a["bbox"])
            rows[where[a["image_id"]]].append((cat_index[a["category_id"]], x, y, w, h, float(a["area"]) if "area" in a else w * h,
                                               int(a.get("iscrowd", 0)), int(a.get("ignore", 0))))
        return cls(rows, [c["name"] for c in cats], image_ids, [c["id"] for c in cats])


def summarize_arrays(precision, recall, iou_thrs=IOU_THRS, area_labels=AREA_LABELS, max_dets=MAX_DETS):
    """The twelve statistics from precision [T,R,K,A,M] and recall [T,K,A,M] on the host: AP, AP50, AP75, AP small / medium /
    large (all at max_dets[-1]), AR at max_dets[0] / [1] / [2], AR small / medium / large (at max_dets[-1]).  Each is the mean
    of the selected entries > -1, or -1 when there is none (or when the lists lack the threshold, the label or the limit)."""
    precision, recall = np.asarray(precision, np.float64), np.asarray(recall, np.float64)
    iou_thrs = np.asarray(iou_thrs, np.float64)
    labels = list(area_labels)

    def stat(ap, iou=None, area="all", m=len(max_dets) - 1):
        s = precision if ap else recall
        if iou is not None:
            s = s[np.where(iou == iou_thrs)[0]]
        if area not in labels:
            return -1.0
        s = s[..., labels.index(area), m]
        good = s[s > -1]
        return float(np.mean(good)) if good.size else -1.0

    last = len(max_dets) - 1
    return np.array([stat(1), stat(1, .5), stat(1, .75), stat(1, area="small"), stat(1, area="medium"), stat(1, area="large"),
                     stat(0, m=0), stat(0, m=min(1, last)), stat(0, m=min(2, last)),
                     stat(0, area="small"), stat(0, area="medium"), stat(0, area="large")], np.float64)


def summary_lines(stats, iou_thrs=IOU_THRS, max_dets=MAX_DETS):
    """The twelve familiar text lines for summarize_arrays' statistics."""
    last = len(max_dets) - 1
    span = "{:0.2f}:{:0.2f}".format(iou_thrs[0], iou_thrs[-1])
    rows = [(1, span, "all", last), (1, "0.50", "all", last), (1, "0.75", "all", last), (1, span, "small", last),
            (1, span, "medium", last), (1, span, "large", last), (0, span, "all", 0), (0, span, "all", min(1, last)),
            (0, span, "all", min(2, last)), (0, span, "small", last), (0, span, "medium", last), (0, span, "large", last)]
    return [" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
        "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, area, max_dets[m], v)
        for (ap, iou, area, m), v in zip(rows, stats)]


class CocoEvaluator(DetectionTable):
    """Device detection table of (x, y, w, h) rows for one image set + the scoring call.  gt: a CocoGroundTruth.  mc: the
    model config (its TOP_N_DETECTION sizes the table, its CLASS_NAMES name the classes when gt has no names); None for a
    table fed from files.  classes / iou_thrs / rec_thrs / area_rngs / max_dets: the protocol's parameters (defaults: COCO's)."""
    ROWS_FROM = "CocoEvaluator"

    def __init__(self, mc, gt, device="cuda:0", max_detections=None, classes=None, iou_thrs=IOU_THRS, rec_thrs=REC_THRS,
                 area_rngs=AREA_RNGS, max_dets=MAX_DETS):
        mc = mc if mc is not None else {}
        names = gt.class_names if gt.class_names is not None else (tuple(mc.CLASS_NAMES) if "CLASS_NAMES" in mc else None)
        if classes is None:
            if names is None:
                raise _lib.SqdetError("CocoEvaluator: no class count (give classes=, or class names in gt or mc)")
            classes = len(names)
        self.class_names = tuple(names) if names is not None and len(names) == classes else tuple(str(c) for c in range(classes))
        if not 0 < classes <= MAX_CLASSES:
            raise _lib.SqdetUnsupported("CocoEvaluator: %d classes (limit %d)" % (classes, MAX_CLASSES))
        self.iou_thrs = np.ascontiguousarray(iou_thrs, np.float64)
        self.rec_thrs = np.ascontiguousarray(rec_thrs, np.float64)
        self.area_rngs = np.ascontiguousarray(area_rngs, np.float64).reshape(-1, 2)
        self.max_dets = np.ascontiguousarray(max_dets, np.int32)
        super().__init__(mc, gt, device, max_detections, classes=int(classes))
        self.gt_box, self.gt_cls = self.up(gt.box, torch.float64), self.up(gt.cls, torch.int32)
        self.gt_area, self.gt_flags = self.up(gt.area, torch.float64), self.up(gt.flags, torch.int32)
        rows = gt.num_images * self.cap
        self.row_rank = torch.zeros((max(1, rows),), dtype=torch.int32, device=self.device)
        self.row_word = torch.zeros((len(self.area_rngs), max(1, rows)), dtype=torch.int32, device=self.device)
        self.precision = self.recall = self.npig = self.num_det = self.stats = self.per_class_ap = None

    def _workspace_bytes(self):
        return lib().sqdet_coco_eval_workspace_bytes(self.gt.num_images, self.cap, self.classes)

    def _ingest(self, src, dst):
        check(lib().sqdet_coco_ingest(*src, self.classes, *dst), "sqdet_coco_ingest")

    def evaluate(self):
        """-> stats, the twelve numbers of summarize_arrays; precision [T,R,K,A,M], recall [T,K,A,M], npig [K,A], num_det [K]
        and per_class_ap {name: AP@[.5:.95], area all, max_dets[-1]; -1 for a class without ground truth} stay in self.  One
        host synchronisation; on an error the previous results stand."""
        T, R, K, A, M = len(self.iou_thrs), len(self.rec_thrs), self.classes, len(self.area_rngs), len(self.max_dets)
        precision, recall = np.zeros((T, R, K, A, M), np.float64), np.zeros((T, K, A, M), np.float64)
        npig, ndet = np.zeros((K, A), np.int32), np.zeros(K, np.int32)
        check(lib().sqdet_coco_evaluate(*self.scoring_args(), K, _ptr(self.gt_offsets),
                                        _ptr(self.gt_box), _ptr(self.gt_cls), _ptr(self.gt_area), _ptr(self.gt_flags), self.num_gt,
                                        P(self.iou_thrs), T, P(self.rec_thrs), R, P(self.area_rngs), A, P(self.max_dets), M,
                                        _ptr(self.workspace), _ptr(self.row_rank), _ptr(self.row_word), P(precision), P(recall),
                                        P(npig), P(ndet), stream_ptr()), "sqdet_coco_evaluate")
        self.precision, self.recall, self.npig, self.num_det = precision, recall, npig, ndet
        self.stats = summarize_arrays(precision, recall, self.iou_thrs, AREA_LABELS[:A], tuple(int(m) for m in self.max_dets))
        self.per_class_ap = {}
        for c, name in enumerate(self.class_names):
            s = precision[:, :, c, 0, M - 1]
            s = s[s > -1]
            self.per_class_ap[name] = float(np.mean(s)) if s.size else -1.0
        return self.stats

    def row_flags(self):
        """The last evaluate()'s per-row results, per class in the class's order (score descending; equal scores by image,
        then rank): [(rank int32 [n], matched bool [A,T,n], ignored bool [A,T,n])]."""
        T, A = len(self.iou_thrs), len(self.area_rngs)
        rank, word = self.row_rank.cpu().numpy(), self.row_word.cpu().numpy()
        out, off = [], 0
        bits = np.arange(T, dtype=np.int32)[None, :, None]
        for n in (int(v) for v in self.num_det):
            w = word[:A, None, off:off + n]
            out.append((rank[off:off + n].copy(), ((w >> bits) & 1).astype(bool), ((w >> (bits + T)) & 1).astype(bool)))
            off += n
        return out

    def summarize(self):
        """The twelve text lines of the last evaluate() (evaluate() is called if there was none)."""
        if self.stats is None:
            self.evaluate()
        return summary_lines(self.stats, self.iou_thrs, tuple(int(m) for m in self.max_dets))

    def write_results_json(self, path, image_ids=None, category_ids=None):
        """The table as a COCO results file: [{"image_id", "category_id", "bbox": [x, y, w, h], "score"}], images in order,
        rows in table order.  image_ids / category_ids: per image / per class (default: the ground truth's, else the indices).
        Floats are written with repr's shortest round-trip digits, so reading the file back gives the table bit for bit."""
        image_ids = image_ids if image_ids is not None else (self.gt.image_ids if self.gt.image_ids is not None else range(self.gt.num_images))
        category_ids = category_ids if category_ids is not None else (self.gt.category_ids if self.gt.category_ids is not None else range(self.classes))
        image_ids, category_ids = list(image_ids), list(category_ids)
        if len(image_ids) != self.gt.num_images or len(category_ids) != self.classes:
            raise _lib.SqdetError("write_results_json: %d image ids and %d category ids for %d images and %d classes"
                                  % (len(image_ids), len(category_ids), self.gt.num_images, self.classes))
        res = [{"image_id": image_ids[i], "category_id": category_ids[c], "bbox": [x, y, w, h], "score": s}
               for i, rows in enumerate(self.tables()) for c, x, y, w, h, s in rows]
        with open(path, "w") as f:
            json.dump(res, f)


def read_results_json(path, gt):
    """A COCO results file -> load_rows' layout for gt (a from_json ground truth): per image (class index, x, y, w, h, score),
    class-major, file order within a class.  A result of an image or category the annotations do not list is an error."""
    with open(path) as f:
        res = json.load(f)
    where = {iid: i for i, iid in enumerate(gt.image_ids)}
    cat_index = {cid: c for c, cid in enumerate(gt.category_ids)}
    rows = [[] for _ in gt.image_ids]
    for k, r in enumerate(res):
        if r["image_id"] not in where or r["category_id"] not in cat_index:
            raise _lib.SqdetError("read_results_json: result %d is of image %r, category %r, which the annotations do not list"
                                  % (k, r["image_id"], r["category_id"]))
        x, y, w, h = (float(v) for v in r["bbox"])
        rows[where[r["image_id"]]].append((cat_index[r["category_id"]], x, y, w, h, float(r["score"])))
    return [sorted(r, key=lambda row: row[0]) for r in rows]            # (sorted is stable: file order within a class)


def evaluate_results_file(annotation_json, results_json, device="cuda:0"):
    """Scores a COCO results file against a COCO annotation file on the device -> the CocoEvaluator after evaluate()
    (its stats, precision, recall, per_class_ap; summarize() gives the text)."""
    gt = CocoGroundTruth.from_json(annotation_json)
    ev = CocoEvaluator.from_rows(None, gt, read_results_json(results_json, gt), device)
    ev.evaluate()
    return ev
