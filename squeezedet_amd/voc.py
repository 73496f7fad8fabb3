"""Pascal VOC: the dataset reader of the reference's src/dataset/pascal_voc.py and its VOC average precision
(src/dataset/voc_eval.py) on the GPU (include/sqdet.h, csrc/voc_eval.hip; the table: det_table.py), without detection files.

  load_voc(data_path, year, image_set, mc)   the reader of pascal_voc.py:36-79: image paths, the `rois` lists (BatchReader)
                                             and the ground truth voc_eval.parse_rec reads from the same XML files
  VocEvaluator(mc, gt, device)               a device detection table fed straight from filter_prediction_batch rows;
                                             evaluate() / curve() / write_detection_files()
  evaluate_detection_files(root, year, set, dir, mc)   the same scoring fed from per-class detection files on disk
  use_07_metric_for(year)                    pascal_voc.py:127

The values in the table are those voc_eval reads back from the files the reference writes.  Not carried over: the
reference's annotations_cache/annots.pkl (voc_eval.py:99-122) -- the XML files are parsed on every load_voc call.
Any mc.CLASS_NAMES of up to 64 names is accepted, so a custom dataset in VOC XML format works the same way."""
import os
import xml.etree.ElementTree as ET
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, stream_ptr
from .det_table import MAX_DETECTIONS, MAX_GROUNDTRUTH, DetectionTable, host_ptr as P, ptr as _ptr, row_offsets  # noqa: F401
from .util import bbox_transform_inv

MAX_CLASSES = 64                                                 # SQDET_VOC_MAX_CLASSES

VocSet = namedtuple("VocSet", "image_idx image_paths rois gt")


def use_07_metric_for(year):
    """pascal_voc.py:127: the 11-point metric before VOC2010."""
    return int(year) < 2010


def read_image_set(voc_path, image_set):
    """<voc_path>/ImageSets/Main/<image_set>.txt -> image indices (pascal_voc._load_image_set_idx)."""
    fn = os.path.join(voc_path, "ImageSets", "Main", image_set + ".txt")
    if not os.path.exists(fn):
        raise FileNotFoundError("File does not exist: {}".format(fn))
    with open(fn) as f:
        return [x.strip() for x in f.readlines()]


def parse_rec(path, class_names):
    """voc_eval.parse_rec (:14-31) reduced to what voc_eval uses: every object, [(class index, xmin, ymin, xmax, ymax,
    difficult)] with the XML's integers; the class by exact name match (voc_eval.py:128), -1 for any other name."""
    idx = {c: i for i, c in enumerate(class_names)}
    rows = []
    for obj in ET.parse(path).findall("object"):
        bbox = obj.find("bndbox")
        rows.append((idx.get(obj.find("name").text, -1), int(bbox.find("xmin").text), int(bbox.find("ymin").text),
                     int(bbox.find("xmax").text), int(bbox.find("ymax").text), int(obj.find("difficult").text)))
    return rows


def parse_rois(path, class_names, index=None):
    """pascal_voc._load_pascal_annotation (:52-79) for one file: [cx, cy, w, h, cls] of every non-difficult object, pixel
    indices made 0-based; the class by name.lower().strip() (a KeyError for an unknown one, as the reference)."""
    class_to_idx = dict(zip(class_names, range(len(class_names))))
    index = index if index is not None else os.path.splitext(os.path.basename(path))[0]
    objs = [obj for obj in ET.parse(path).findall("object") if int(obj.find("difficult").text) == 0]
    bboxes = []
    for obj in objs:
        bbox = obj.find("bndbox")
        xmin = float(bbox.find("xmin").text) - 1
        xmax = float(bbox.find("xmax").text) - 1
        ymin = float(bbox.find("ymin").text) - 1
        ymax = float(bbox.find("ymax").text) - 1
        assert xmin >= 0.0 and xmin <= xmax, \
            "Invalid bounding box x-coord xmin {} or xmax {} at {}.xml".format(xmin, xmax, index)
        assert ymin >= 0.0 and ymin <= ymax, \
            "Invalid bounding box y-coord ymin {} or ymax {} at {}.xml".format(ymin, ymax, index)
        x, y, w, h = bbox_transform_inv([xmin, ymin, xmax, ymax])
        cls = class_to_idx[obj.find("name").text.lower().strip()]
        bboxes.append([x, y, w, h, cls])
    return bboxes


class GroundTruth:
    """Host tables of one image set as voc_eval sees it: offsets int32 [N+1], box float64 [G,4] (xmin, ymin, xmax, ymax, the
    XML's integers), cls int32 [G] (-1: not in the class list), difficult int32 [G]."""

    def __init__(self, raw):
        self.num_images = len(raw)
        self.offsets, flat = row_offsets(raw, "VOC evaluation: image %d has %d objects (limit %d)")
        self.cls = np.array([row[0] for row in flat], np.int32)
        self.box = np.array([row[1:5] for row in flat], np.float64).reshape(-1, 4)
        self.difficult = np.array([row[5] for row in flat], np.int32)


def load_voc(data_path, year, image_set, mc):
    """The reference's pascal_voc imdb without the batch reader, from <data_path>/VOC<year>: image indices
    (ImageSets/Main/<image_set>.txt), image paths (JPEGImages/<idx>.jpg), rois (pascal_voc._rois order) and the ground
    truth voc_eval reads (Annotations/<idx>.xml).  The XML files are parsed here every time: the reference's annots.pkl
    cache is not carried over."""
    voc = os.path.join(data_path, "VOC" + str(year))
    idx = read_image_set(voc, image_set)
    names = tuple(mc.CLASS_NAMES)
    raw, rois = [], []
    for i in idx:
        fn = os.path.join(voc, "Annotations", i + ".xml")
        raw.append(parse_rec(fn, names))
        rois.append(parse_rois(fn, names, i))
    return VocSet(idx, [os.path.join(voc, "JPEGImages", i + ".jpg") for i in idx], rois, GroundTruth(raw))


class VocEvaluator(DetectionTable):
    """Device detection table for one image set + the scoring call.  gt: a GroundTruth (load_voc(...).gt).
    max_detections: rows per image the table holds (>= the filter's max_out; default mc.TOP_N_DETECTION, else 512)."""

    def __init__(self, mc, gt, device="cuda:0", max_detections=None):
        self.class_names = tuple(mc.CLASS_NAMES)
        if not 0 < len(self.class_names) <= MAX_CLASSES:
            raise _lib.SqdetUnsupported("VocEvaluator: %d classes (limit %d)" % (len(self.class_names), MAX_CLASSES))
        super().__init__(mc, gt, device, max_detections, classes=len(self.class_names))
        self.gt_box, self.gt_cls, self.gt_difficult = self.up(gt.box, torch.float64), self.up(gt.cls, torch.int32), self.up(gt.difficult, torch.int32)
        self._curve_rec = self._curve_prec = None
        self.ap07 = self.ap_area = self.npos = self.num_det = None

    def _workspace_bytes(self):
        return lib().sqdet_voc_eval_workspace_bytes(self.gt.num_images, self.cap, self.classes)

    def _ingest(self, src, dst):
        check(lib().sqdet_voc_ingest(*src, self.classes, *dst), "sqdet_voc_ingest")

    def _evaluate(self, curve_cls=-1):
        C = self.classes
        ap07, ap_area = np.zeros(C, np.float64), np.zeros(C, np.float64)
        npos, ndet = np.zeros(C, np.int32), np.zeros(C, np.int32)
        if curve_cls >= 0 and self._curve_rec is None:
            self._curve_rec = torch.empty((self.gt.num_images * self.cap,), dtype=torch.float64, device=self.device)
            self._curve_prec = torch.empty_like(self._curve_rec)
        check(lib().sqdet_voc_evaluate(*self.scoring_args(), C, _ptr(self.gt_offsets), _ptr(self.gt_box),
                                       _ptr(self.gt_cls), _ptr(self.gt_difficult), self.num_gt, _ptr(self.workspace), P(ap07),
                                       P(ap_area), P(npos), P(ndet), int(curve_cls),
                                       _ptr(self._curve_rec) if curve_cls >= 0 else None,
                                       _ptr(self._curve_prec) if curve_cls >= 0 else None, stream_ptr()), "sqdet_voc_evaluate")
        self.ap07, self.ap_area, self.npos, self.num_det = ap07, ap_area, npos, ndet

    def evaluate(self, use_07_metric=True):
        """-> (aps, names) as pascal_voc.evaluate_detections returns them: per class the 11-point AP (use_07_metric) or
        the area under the precision envelope; 0 for a class without detections.  Both forms of every class stay in
        self.ap07 / self.ap_area, with self.npos and self.num_det.  One host synchronisation."""
        self._evaluate()
        aps = [float(v) for v in (self.ap07 if use_07_metric else self.ap_area)]
        return aps, self.class_names

    def curve(self, cls):
        """-> (rec, prec) of class index `cls` as voc_eval returns them (float64 arrays, one value per detection in
        descending-score order; equal scores by image, then row)."""
        cls = int(cls)
        if not 0 <= cls < self.classes:
            raise _lib.SqdetError("curve: class %d of %d" % (cls, self.classes))
        self._evaluate(cls)
        n = int(self.num_det[cls])
        return self._curve_rec[:n].cpu().numpy(), self._curve_prec[:n].cpu().numpy()

    def write_detection_files(self, det_file_dir, image_idx):
        """<det_file_dir>/<cls>.txt of every class, as pascal_voc.evaluate_detections writes them (:98-109), from the table
        (each value is the double nearest to the text it came from, so formatting it again gives that text)."""
        write_detection_files(det_file_dir, self.class_names, image_idx, self.tables())


def write_detection_files(det_file_dir, class_names, image_idx, tables):
    """<det_file_dir>/<cls>.txt of every class from host rows (per image [(class index, x1, y1, x2, y2, score)]): one line
    '<image> <score:.3f> <x1:.1f> <y1:.1f> <x2:.1f> <y2:.1f>' per detection, images in order (pascal_voc.py:98-109)."""
    os.makedirs(det_file_dir, exist_ok=True)
    for c, name in enumerate(class_names):
        with open(os.path.join(det_file_dir, "{:s}.txt".format(name)), "wt") as f:
            for index, rows in zip(image_idx, tables):
                for dc, x1, y1, x2, y2, s in rows:
                    if dc == c:
                        f.write("{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n".format(index, s, x1, y1, x2, y2))


def parse_detection_file(path):
    """A per-class detection file as voc_eval reads it (:139-145): [(image index, score, x1, y1, x2, y2)] in file order."""
    with open(path) as f:
        lines = f.readlines()
    out = []
    for x in (l.strip().split(" ") for l in lines):
        out.append((x[0], float(x[1])) + tuple(float(z) for z in x[2:6]))
    return out


def evaluate_detection_files(data_root_path, year, image_set, det_dir, mc, device="cuda:0"):
    """voc_eval's job on the GPU: scores <det_dir>/<cls>.txt of every class of mc.CLASS_NAMES (a missing file: no
    detections) against <data_root_path>/VOC<year>/Annotations for the images of ImageSets/Main/<image_set>.txt and
    returns (aps, names) as pascal_voc.evaluate_detections does, the metric chosen by the year."""
    voc = os.path.join(data_root_path, "VOC" + str(year))
    idx = read_image_set(voc, image_set)
    names = tuple(mc.CLASS_NAMES)
    where = {name: i for i, name in enumerate(idx)}
    rows = [[] for _ in idx]
    for c, name in enumerate(names):                       # class-major per image, file order within a class
        fn = os.path.join(det_dir, name + ".txt")
        if not os.path.exists(fn):
            continue
        for index, s, x1, y1, x2, y2 in parse_detection_file(fn):
            rows[where[index]].append((c, x1, y1, x2, y2, s))
    gt = GroundTruth([parse_rec(os.path.join(voc, "Annotations", i + ".xml"), names) for i in idx])
    return VocEvaluator.from_rows(mc, gt, rows, device).evaluate(use_07_metric_for(year))
