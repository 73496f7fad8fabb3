"""The anchor-assignment policy of a training run (OURS): which anchors are trained as positives.

The default -- `reference`, one anchor per ground-truth box as the reference's imdb.read_batch picks it -- is what
sqdet_build_labels does: ops.build_labels launches exactly that then and the new entry point is not called.  `iou` and `atss` keep
that pick and add, from the anchors no box claimed, every anchor over an IoU threshold (capped per box) or the anchors ATSS selects
(Zhang et al., CVPR 2020); both run as sqdet_build_labels_opt (squeezedet_amd/csrc/assign.hip).
Importing this needs neither torch nor a GPU (drivers.py and the host tests use it)."""
import math
from collections import namedtuple

from ._lib import SqdetError

ASSIGN_MODES = ("reference", "iou", "atss")          # sqdet_assign_options_t.mode by index
MAX_PER_BOX = 64                                     # sqdet_build_labels_opt's limits
MAX_TOPK = 32

AssignOptions = namedtuple("AssignOptions", "mode iou_thresh max_per_box topk")


def assign_options(mode="reference", iou_thresh=0.5, max_per_box=16, topk=9):
    """The validated record.  An unknown mode, a threshold that is not a finite number >= 0, max_per_box outside 1..64 and topk
    outside 1..32 are refused here, before anything is launched."""
    if mode not in ASSIGN_MODES:
        raise SqdetError("assign mode %r is not one of %s" % (mode, ", ".join(ASSIGN_MODES)))
    for name, v in (("max_per_box", max_per_box), ("topk", topk)):
        if isinstance(v, bool) or int(v) != v:
            raise SqdetError("assign %s must be an integer, got %r" % (name, v))
    opt = AssignOptions(str(mode), float(iou_thresh), int(max_per_box), int(topk))
    if not (math.isfinite(opt.iou_thresh) and opt.iou_thresh >= 0.0):
        raise SqdetError("assign iou_thresh must be a finite number >= 0, got %r" % (iou_thresh,))
    if not 1 <= opt.max_per_box <= MAX_PER_BOX:
        raise SqdetError("assign max_per_box must be in 1..%d, got %d" % (MAX_PER_BOX, opt.max_per_box))
    if not 1 <= opt.topk <= MAX_TOPK:
        raise SqdetError("assign topk must be in 1..%d, got %d" % (MAX_TOPK, opt.topk))
    return opt


def is_default(opt):
    """True for the rule sqdet_build_labels runs itself (None, or mode `reference` whatever the other fields say)."""
    return opt is None or opt.mode == "reference"


def as_dict(opt):
    """The record as a checkpoint and a benchmark line carry it: the mode and the fields that mode reads."""
    if is_default(opt):
        return dict(mode="reference")
    if opt.mode == "iou":
        return dict(mode="iou", iou_thresh=opt.iou_thresh, max_per_box=opt.max_per_box)
    return dict(mode="atss", topk=opt.topk)


def from_dict(d):
    return assign_options(**d)


def positives_summary(positives, gt_counts):
    """(min, mean, max) positives per object over a batch: positives [B,M] as build_labels returns it (a tensor or an array),
    gt_counts [B]; the objects are the first min(max(count, 0), M) of each image.  (0, 0.0, 0) for a batch without objects."""
    import numpy as np
    p = np.asarray(positives.cpu() if hasattr(positives, "cpu") else positives)
    c = np.asarray(gt_counts.cpu() if hasattr(gt_counts, "cpu") else gt_counts)
    live = np.arange(p.shape[1])[None, :] < np.clip(c, 0, p.shape[1])[:, None]
    v = p[live]
    if v.size == 0:
        return 0, 0.0, 0
    return int(v.min()), float(v.mean()), int(v.max())
