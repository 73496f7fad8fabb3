"""Anchor shapes for a dataset: fitted on the device, and a report of how well a config's anchors cover a dataset.

The SqueezeDet loss regresses every object against the one anchor it claims (``ops.build_labels``, the reference's
imdb.py:195-239), so the nine (w, h) shapes of ``mc.ANCHOR_BOX`` should look like the dataset's objects at the network input.
The reference ships fixed shapes -- k-means of KITTI's objects -- and nothing to produce others; this module is OURS:

  * ``dataset_shapes``     the (w, h) of every object, scaled to the network input as ``BatchReader`` scales it;
  * ``fit_anchor_shapes``  Lloyd's k-means under the IoU distance, several seeded restarts at once (``sqdet_anchor_kmeans``,
                           csrc/anchors.hip), the restart of highest mean IoU wins;
  * ``coverage``           ``ops.build_labels`` + ``sqdet_anchor_coverage``: per object the best IoU any anchor offers and the
                           IoU of the anchor it was given, and from them the four numbers the reference prints under
                           ``mc.DEBUG_MODE`` (imdb.py:241-246) plus recall at three IoU thresholds;
  * ``dataset_coverage``   the same over a whole dataset, a chunk of images at a time;
  * ``save_anchor_shapes`` / ``load_anchor_shapes``: the JSON file ``tools/fit_anchors.py`` writes and the drivers'
                           ``--anchor_shapes`` reads; ``config.with_anchor_shapes`` puts the shapes into a config.

Everything is validated on the host before anything is uploaded: the kernels read their data from the device and cannot
reject it.  NumPy only at import; torch and the library are loaded by the calls that run on the device.
"""
import json
from collections import namedtuple

import numpy as np

from .config import check_anchor_shapes

MAX_K = 64                 # SQDET_ANCHOR_KMEANS_MAX_K
MAX_RESTARTS = 64          # SQDET_ANCHOR_KMEANS_MAX_RESTARTS
RECALL_THRESHOLDS = (0.3, 0.5, 0.7)

KMeans = namedtuple("KMeans", "centroids assign counts mean_iou iters")
KMeans.__doc__ = """sqdet_anchor_kmeans' outputs as host arrays, one row per restart: centroids float64 [R,k,2], assign int32
[R,n], counts int32 [R,k], mean_iou float64 [R], iters int32 [R] (the first iteration, counted from 0, whose assignment
changed no box; max_iter if none did)."""

AnchorFit = namedtuple("AnchorFit", "shapes mean_iou iters counts restart restart_mean_iou k seed")
AnchorFit.__doc__ = """fit_anchor_shapes' result: shapes float64 [k,2] sorted by area, then width, ascending; mean_iou, iters
and counts (in the order of shapes) of the winning restart; restart: its index; restart_mean_iou: every restart's mean IoU."""


def _sqdet_error(msg):
    from ._lib import SqdetError
    return SqdetError(msg)


def dataset_shapes(rois, sizes, mc):
    """float64 [n,2]: every object's (w, h) at the network input.  rois: per image a list of [cx, cy, w, h, cls] in original
    pixels; sizes: per image (height, width).  Scaled as BatchReader.next_plan scales a box without augmentation:
    w * (IMAGE_WIDTH / orig_w), h * (IMAGE_HEIGHT / orig_h)."""
    if len(rois) != len(sizes):
        raise ValueError("dataset_shapes: %d roi lists for %d image sizes" % (len(rois), len(sizes)))
    out = []
    for roi, (orig_h, orig_w) in zip(rois, sizes):
        x_scale = mc.IMAGE_WIDTH / float(orig_w)
        y_scale = mc.IMAGE_HEIGHT / float(orig_h)
        for b in roi:
            out.append((b[2] * x_scale, b[3] * y_scale))
    return np.array(out, np.float64).reshape(-1, 2)


def check_shapes(wh):
    """float64 [n,2], n >= 1, finite and strictly positive; ValueError otherwise."""
    a = np.ascontiguousarray(np.asarray(wh, np.float64))
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("box shapes must be [n,2] (w, h), got an array of shape %s" % (a.shape,))
    bad = ~(np.isfinite(a).all(axis=1) & (a > 0).all(axis=1))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError("box shapes must be finite and strictly positive: shape %d is (%r, %r)" % (i, float(a[i, 0]), float(a[i, 1])))
    return a


def draw_init(wh, k, restarts, seed):
    """The initial centroids float64 [restarts,k,2]: rs = RandomState(seed), then per restart in order
    rs.choice(len(u), k, replace=False) over u = np.unique(wh, axis=0) -- k DISTINCT shapes of the dataset."""
    u = np.unique(np.asarray(wh, np.float64), axis=0)
    if len(u) < k:
        raise ValueError("fit_anchor_shapes: k = %d anchors from only %d distinct box shapes" % (k, len(u)))
    rs = np.random.RandomState(seed)
    return np.stack([u[rs.choice(len(u), k, replace=False)] for _ in range(restarts)])


def kmeans(wh, init, max_iter=100, device=None, out=None):
    """sqdet_anchor_kmeans on host arrays: wh [n,2], init [R,k,2] -> KMeans (host arrays; one synchronisation, the copy
    back).  Shapes and centroids are checked on the host first (ValueError); n = 0, max_iter < 1 and the limits k <= 64,
    R <= 64 are the library's to refuse (SqdetError / SqdetUnsupported).  `out`: preallocated device tensors (assign, counts,
    mean_iou, iters), left untouched by a refused call."""
    import torch
    from . import ops
    wh = check_shapes(wh)
    init = np.ascontiguousarray(np.asarray(init, np.float64))
    if init.ndim != 3 or init.shape[2] != 2:
        raise ValueError("init must be [restarts,k,2], got an array of shape %s" % (init.shape,))
    if init.size and (not np.isfinite(init).all() or not (init > 0).all()):
        raise ValueError("init: centroids must be finite and strictly positive")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    cent = torch.from_numpy(init.copy()).to(dev)
    assign, counts, mean_iou, iters = ops.anchor_kmeans(torch.from_numpy(wh).to(dev), cent, int(max_iter), out=out)
    return KMeans(cent.cpu().numpy(), assign.cpu().numpy(), counts.cpu().numpy(), mean_iou.cpu().numpy(), iters.cpu().numpy())


def fit_anchor_shapes(wh, k=9, seed=0, restarts=8, max_iter=100, init=None, device=None):
    """k anchor shapes for the box shapes wh [n,2] (dataset_shapes): Lloyd's k-means under the distance 1 - IoU (boxes on a
    common centre), `restarts` runs at once on the device, each from k distinct shapes of the dataset (draw_init; or the
    given init [restarts,k,2] / [k,2]).  The restart of highest mean IoU wins, the lowest index on a tie.  -> AnchorFit."""
    wh = check_shapes(wh)
    k, restarts, max_iter = int(k), int(restarts), int(max_iter)
    if init is not None:
        init = np.asarray(init, np.float64)
        if init.ndim == 2:
            init = init[None]
        if init.ndim != 3 or init.shape[1:] != (k, 2):
            raise ValueError("init must be [restarts,%d,2] or [%d,2], got an array of shape %s" % (k, k, init.shape))
        restarts = len(init)
    if len(wh) < 1:
        raise ValueError("fit_anchor_shapes: no box shapes")
    if k < 1 or restarts < 1 or max_iter < 1:
        raise ValueError("fit_anchor_shapes: k, restarts and max_iter must be positive (got %d, %d, %d)" % (k, restarts, max_iter))
    if k > MAX_K or restarts > MAX_RESTARTS:
        raise _sqdet_error("fit_anchor_shapes: k = %d, restarts = %d over the limits of %d and %d" % (k, restarts, MAX_K, MAX_RESTARTS))
    if init is None:
        init = draw_init(wh, k, restarts, seed)
    res = kmeans(wh, init, max_iter, device)
    best = int(np.argmax(res.mean_iou))                    # first maximum: the lowest restart on a tie
    c = res.centroids[best]
    order = np.lexsort((c[:, 0], c[:, 0] * c[:, 1]))       # by area, then width
    return AnchorFit(c[order].copy(), float(res.mean_iou[best]), int(res.iters[best]), res.counts[best][order].copy(), best,
                     res.mean_iou.copy(), k, int(seed))


# ------------------------------------------------------------------------------------------------------------ the file --
def save_anchor_shapes(path, shapes, mc, dataset="", image_set="", k=None, seed=None, mean_iou=None, **more):
    """The JSON file of --anchor_shapes: shapes, the input size they were fitted at, dataset, image set, k, seed, mean IoU."""
    shapes = check_anchor_shapes(shapes)
    rec = dict(anchor_shapes=[[float(w), float(h)] for w, h in shapes], image_size=[int(mc.IMAGE_HEIGHT), int(mc.IMAGE_WIDTH)],
               dataset=str(dataset), image_set=str(image_set), k=int(len(shapes) if k is None else k),
               seed=None if seed is None else int(seed), mean_iou=None if mean_iou is None else float(mean_iou))
    rec.update(more)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return rec


def load_anchor_shapes(path):
    """float64 [k,2] from a file of save_anchor_shapes (a bare JSON list of [w, h] pairs is taken too); ValueError on anything else."""
    with open(path) as f:
        try:
            rec = json.load(f)
        except ValueError as e:
            raise ValueError("%s: not a JSON anchor-shape file (%s)" % (path, e))
    if isinstance(rec, dict):
        if "anchor_shapes" not in rec:
            raise ValueError("%s: no 'anchor_shapes' entry" % path)
        rec = rec["anchor_shapes"]
    try:
        return check_anchor_shapes(rec)
    except (ValueError, TypeError) as e:
        raise ValueError("%s: %s" % (path, e))


# The anchor counts the drivers build a net for.  ConvDet has ANCHOR_PER_GRID * (CLASSES + 5) output channels and the conv kernels
# store channels four at a time (config.pad_head_classes pads the classes for that); the fused score epilogue, the training
# kernels and the filter take nine anchors per cell or fall back to their generic forms.  DESIGN.md section 3.10 has what was tried.
RUNNABLE_ANCHOR_COUNTS = (9,)


def load_for_driver(path):
    """load_anchor_shapes for train.py / eval.py / demo.py: a count the nets are not known to run with is refused here, before
    anything is built, by SystemExit with a message that names it."""
    try:
        shapes = load_anchor_shapes(path)
    except (OSError, ValueError) as e:
        raise SystemExit("--anchor_shapes: %s" % e)
    if len(shapes) not in RUNNABLE_ANCHOR_COUNTS:
        raise SystemExit("--anchor_shapes %s: %d anchor shapes per grid cell; the nets are built for %s (fit with --k %d)"
                         % (path, len(shapes), " or ".join(str(c) for c in RUNNABLE_ANCHOR_COUNTS), RUNNABLE_ANCHOR_COUNTS[0]))
    return shapes


def beside_checkpoint(checkpoint_path):
    """The anchor_shapes.json train.py leaves in its --train_dir, found from a checkpoint file in it or from the directory;
    None when there is none."""
    import os
    d = checkpoint_path if os.path.isdir(checkpoint_path) else os.path.dirname(os.path.abspath(checkpoint_path))
    p = os.path.join(d, "anchor_shapes.json")
    return p if os.path.isfile(p) else None


def same_shapes(a, b):
    """Two shape lists are the same list: same count, bitwise the same float64 values in the same order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a, b))


# ------------------------------------------------------------------------------------------------------------ coverage --
class CoverageReport:
    """How a config's anchors cover a set of ground-truth boxes.  Per-object arrays, [B,M] in the padded layout (entries at or
    beyond gt_counts: 0 / -1 / 0 / -1): best_iou, best_index (sqdet_anchor_coverage), claimed_iou and anchor_index (the
    anchor ops.build_labels gave the object).  From them:
      num_objects
      max_iou, min_iou, avg_iou, num_zero_iou   of the CLAIMED anchors: what imdb.read_batch prints under mc.DEBUG_MODE
                                                (imdb.py:135-139, 203-215, 241-246; max starts at 0.0, min at 1.0)
      mean_best_iou                             mean of best_iou
      recall_at {0.3, 0.5, 0.7}                 share of objects whose best_iou reaches the threshold
      num_displaced                             objects whose claimed anchor is worse than their best one, because an earlier
                                                object of the image took it (claimed_iou < best_iou)"""

    def __init__(self, best_iou, best_index, claimed_iou, anchor_index, gt_counts):
        self.best_iou, self.best_index = np.asarray(best_iou, np.float64), np.asarray(best_index, np.int32)
        self.claimed_iou, self.anchor_index = np.asarray(claimed_iou, np.float64), np.asarray(anchor_index, np.int32)
        self.gt_counts = np.asarray(gt_counts, np.int32)
        M = self.best_iou.shape[1]
        valid = np.arange(M)[None, :] < np.minimum(self.gt_counts, M)[:, None]
        self.valid = valid
        best, claimed = self.best_iou[valid], self.claimed_iou[valid]
        n = int(valid.sum())
        self.num_objects = n
        self.max_iou = float(max(0.0, claimed.max())) if n else 0.0
        self.min_iou = float(min(1.0, claimed.min())) if n else 1.0
        self.avg_iou = float(claimed.sum() / n) if n else float("nan")
        self.num_zero_iou = int((claimed <= 0).sum())
        self.mean_best_iou = float(best.sum() / n) if n else float("nan")
        self.recall_at = {t: (float((best >= t).sum() / n) if n else float("nan")) for t in RECALL_THRESHOLDS}
        self.num_displaced = int((claimed < best).sum())

    @classmethod
    def merge(cls, reports):
        """One report over the images of several (chunks of one dataset, padded to the same M)."""
        reports = list(reports)
        cat = lambda name: np.concatenate([getattr(r, name) for r in reports], axis=0)
        return cls(cat("best_iou"), cat("best_index"), cat("claimed_iou"), cat("anchor_index"), cat("gt_counts"))

    def summary(self):
        """The scalar part, JSON-ready."""
        return dict(num_objects=self.num_objects, max_iou=self.max_iou, min_iou=self.min_iou, avg_iou=self.avg_iou,
                    num_zero_iou=self.num_zero_iou, mean_best_iou=self.mean_best_iou,
                    recall_at={"%.1f" % t: v for t, v in self.recall_at.items()}, num_displaced=self.num_displaced)

    def lines(self):
        """[(label, value text)]: the reference's five DEBUG_MODE lines first, then ours."""
        rows = [("max iou", "%.6f" % self.max_iou), ("min iou", "%.6f" % self.min_iou), ("avg iou", "%.6f" % self.avg_iou),
                ("number of objects", "%d" % self.num_objects), ("number of objects with 0 iou", "%d" % self.num_zero_iou),
                ("mean best iou", "%.6f" % self.mean_best_iou)]
        rows += [("recall at iou %.1f" % t, "%.4f" % self.recall_at[t]) for t in RECALL_THRESHOLDS]
        rows.append(("displaced objects", "%d" % self.num_displaced))
        return rows


def format_reports(reports, titles):
    """The reports side by side, one column each."""
    rows = [r.lines() for r in reports]
    width = max(12, max(len(t) for t in titles))
    out = ["%-30s" % "" + "".join(" %*s" % (width, t) for t in titles)]
    for i, (label, _) in enumerate(rows[0]):
        out.append("%-30s" % label + "".join(" %*s" % (width, r[i][1]) for r in rows))
    return "\n".join(out)


def _check_ground_truth(gt_boxes, gt_counts):
    gt = np.ascontiguousarray(np.asarray(gt_boxes, np.float64))
    cnt = np.ascontiguousarray(np.asarray(gt_counts, np.int32))
    if gt.ndim != 3 or gt.shape[2] != 4 or gt.shape[0] < 1 or gt.shape[1] < 1 or cnt.shape != (gt.shape[0],):
        raise ValueError("coverage: gt_boxes [B,M,4] and gt_counts [B] expected, got %s and %s" % (gt.shape, cnt.shape))
    if (cnt < 0).any() or (cnt > gt.shape[1]).any():
        raise ValueError("coverage: gt_counts must lie in [0, %d]" % gt.shape[1])
    valid = np.arange(gt.shape[1])[None, :] < cnt[:, None]
    v = gt[valid]
    if not np.isfinite(v).all() or not (v[:, 2:] > 0).all():
        raise ValueError("coverage: ground-truth boxes must be finite with strictly positive width and height")
    return gt, cnt


def coverage(mc, gt_boxes, gt_classes, gt_counts, device=None):
    """ops.build_labels, then sqdet_anchor_coverage, for ground truth in the padded layout (gt_boxes float64 [B,M,4] cx, cy, w,
    h at the network input, gt_classes [B,M], gt_counts [B]; host arrays) against mc.ANCHOR_BOX -> CoverageReport."""
    import torch
    from . import ops
    gt, cnt = _check_ground_truth(gt_boxes, gt_counts)
    cls = np.ascontiguousarray(np.asarray(gt_classes, np.int32))
    if cls.shape != gt.shape[:2]:
        raise ValueError("coverage: gt_classes must be %s, got %s" % (gt.shape[:2], cls.shape))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    anc = torch.from_numpy(np.ascontiguousarray(np.asarray(mc.ANCHOR_BOX, np.float64))).to(dev)
    gt_d, cnt_d = torch.from_numpy(gt).to(dev), torch.from_numpy(cnt).to(dev)
    aidx = ops.build_labels(anc, gt_d, torch.from_numpy(cls).to(dev), cnt_d, int(mc.CLASSES))[4]
    best, bidx, claimed = ops.anchor_coverage(anc, gt_d, cnt_d, aidx)
    return CoverageReport(best.cpu().numpy(), bidx.cpu().numpy(), claimed.cpu().numpy(), aidx.cpu().numpy(), cnt)


def padded_ground_truth(rois, sizes, mc, chunk_images=256):
    """The padded arrays of a whole dataset, a chunk of images at a time: yields (gt_boxes float64 [B,M,4], gt_classes int32
    [B,M], gt_counts int32 [B]) with B <= chunk_images and M = the dataset's largest object count (at least 1), the boxes
    scaled to the network input as BatchReader scales them without augmentation."""
    if len(rois) != len(sizes) or not len(rois):
        raise ValueError("padded_ground_truth: %d roi lists for %d image sizes" % (len(rois), len(sizes)))
    M = max(1, max(len(r) for r in rois))
    for i0 in range(0, len(rois), int(chunk_images)):
        part = rois[i0:i0 + int(chunk_images)]
        gt = np.zeros((len(part), M, 4), np.float64)
        cls = np.zeros((len(part), M), np.int32)
        cnt = np.zeros(len(part), np.int32)
        for j, (roi, (orig_h, orig_w)) in enumerate(zip(part, sizes[i0:i0 + int(chunk_images)])):
            cnt[j] = len(roi)
            if roi:
                b = np.array([[v[0], v[1], v[2], v[3]] for v in roi], np.float64)
                b[:, 0::2] = b[:, 0::2] * (mc.IMAGE_WIDTH / float(orig_w))
                b[:, 1::2] = b[:, 1::2] * (mc.IMAGE_HEIGHT / float(orig_h))
                gt[j, :len(roi)] = b
                cls[j, :len(roi)] = [int(v[4]) for v in roi]
        yield gt, cls, cnt


def dataset_coverage(mc, rois, sizes, chunk_images=256, device=None):
    """coverage over a whole dataset (rois, sizes as dataset_shapes takes them), chunk_images images at a time so that the
    label tensors build_labels writes stay bounded -> one CoverageReport."""
    return CoverageReport.merge(coverage(mc, gt, cls, cnt, device) for gt, cls, cnt in padded_ground_truth(rois, sizes, mc, chunk_images))
