"""The device detection table under the GPU evaluators (include/sqdet.h "Detection table", csrc/det_table.h):
KittiEvaluator (kitti_ap.py), VocEvaluator (voc.py) and CocoEvaluator (coco.py) derive from DetectionTable, which holds the
table, the ground truth's offsets, the workspace and the leading arguments of the scoring calls; they add their ground-truth
fields, scoring and file writers."""
import numpy as np
import torch

from . import _lib
from ._lib import stream_ptr

MAX_DETECTIONS, MAX_GROUNDTRUTH = 512, 128                       # per image (SQDET_KITTI_MAX_* = SQDET_VOC_MAX_*)


def ptr(t):
    return _lib.C.c_void_p(t.data_ptr())


def host_ptr(a):
    """A host array's address for a C call."""
    return a.ctypes.data_as(_lib.C.c_void_p)


def row_offsets(per_image, message):
    """Per-image row lists -> (offsets int32 [N+1], the rows of all images in one list).  A list over MAX_GROUNDTRUTH:
    SqdetUnsupported(message % (image, rows, limit))."""
    big = [i for i, r in enumerate(per_image) if len(r) > MAX_GROUNDTRUTH]
    if big:
        raise _lib.SqdetUnsupported(message % (big[0], len(per_image[big[0]]), MAX_GROUNDTRUTH))
    return np.concatenate([[0], np.cumsum([len(r) for r in per_image])]).astype(np.int32), [row for r in per_image for row in r]


class DetectionTable:
    """det_box / det_score / det_cls / det_count / status of gt.num_images images on `device`.  max_detections: rows per
    image the table holds (>= the filter's max_out; default mc.TOP_N_DETECTION, else 512).  classes: load_rows rejects a
    class outside [0, classes) (None: not checked).  Also on the device: gt.offsets (gt_offsets; num_gt rows in all) and the
    scoring workspace.  A subclass supplies _ingest(src, dst): its sqdet_*_ingest call, and _workspace_bytes()."""
    ROWS_FROM = "evaluate_detection_files"                      # who from_rows' error names

    def __init__(self, mc, gt, device="cuda:0", max_detections=None, classes=None):
        self.mc, self.gt, self.classes = mc, gt, classes
        self.device = torch.device(device)
        top_n = mc.get("TOP_N_DETECTION", 0)
        cap = int(max_detections or (top_n if top_n > 0 else MAX_DETECTIONS))
        if not 0 < cap <= MAX_DETECTIONS:
            raise _lib.SqdetUnsupported("%s: %d detections per image (limit %d)" % (type(self).__name__, cap, MAX_DETECTIONS))
        self.cap, n, dev = cap, gt.num_images, self.device
        self.det_box = torch.zeros((n, cap, 4), dtype=torch.float64, device=dev)
        self.det_score = torch.zeros((n, cap), dtype=torch.float64, device=dev)
        self.det_cls = torch.zeros((n, cap), dtype=torch.int32, device=dev)
        self.det_count = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.status = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.gt_offsets, self.num_gt = self.up(gt.offsets, torch.int32), int(gt.offsets[-1])
        self.workspace = torch.empty((max(1, self._workspace_bytes()),), dtype=torch.uint8, device=dev)

    @classmethod
    def from_rows(cls, mc, gt, rows, device="cuda:0", **kw):
        """An evaluator (kw: its other constructor arguments) whose table is just large enough for `rows` (load_rows' layout),
        filled with them."""
        cap = max([1] + [len(r) for r in rows])
        if cap > MAX_DETECTIONS:
            raise _lib.SqdetUnsupported("%s: %d detections in one image (limit %d)" % (cls.ROWS_FROM, cap, MAX_DETECTIONS))
        ev = cls(mc, gt, device, max_detections=cap, **kw)
        ev.load_rows(rows)
        return ev

    def up(self, a, dt):
        """A host array on the device (one zero of dtype dt for an empty one: a valid pointer)."""
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a).to(self.device) if a.size else torch.zeros((1,), dtype=dt, device=self.device)

    def table_args(self):
        """The leading arguments of the scoring calls: the four row tensors."""
        return ptr(self.det_box), ptr(self.det_score), ptr(self.det_cls), ptr(self.det_count)

    def scoring_args(self):
        """The leading arguments of the sqdet_*_evaluate calls: the table, its status and its dimensions."""
        return self.table_args() + (ptr(self.status), self.gt.num_images, self.cap)

    def reset(self):
        """Empties the table (stream-ordered)."""
        self.det_count.zero_()
        self.status.zero_()

    def add_rows(self, boxes, probs, cls, count, image_offset, scales=None):
        """filter_prediction_batch rows of images [image_offset, image_offset + n) -> the table, stream-ordered, no host
        sync.  scales: per-image (x_scale, y_scale) the boxes are divided by (None = 1).  A negative count (the filter's
        overflow report) makes the call write nothing; evaluate() then raises."""
        n, max_out = int(probs.shape[0]), int(probs.shape[1])
        for t, name, dt in ((boxes, "boxes", torch.float32), (probs, "probs", torch.float32), (cls, "cls", torch.int32),
                            (count, "count", torch.int32)):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous():
                raise _lib.SqdetError("add_rows: %s must be a contiguous %s tensor on %s" % (name, dt, self.device))
        if tuple(boxes.shape) != (n, max_out, 4) or tuple(cls.shape) != (n, max_out) or tuple(count.shape) != (n,):
            raise _lib.SqdetError("add_rows: shapes %s %s %s %s" % (tuple(boxes.shape), tuple(probs.shape), tuple(cls.shape), tuple(count.shape)))
        if n == 0:
            return
        sc = None
        if scales is not None:
            sc = torch.as_tensor(np.ascontiguousarray(np.asarray(scales, np.float64).reshape(n, 2))).to(self.device, non_blocking=True)
        self._ingest((ptr(boxes), ptr(probs), ptr(cls), ptr(count), ptr(sc) if sc is not None else None, n, max_out),
                     self.table_args() + (ptr(self.status), int(image_offset), self.gt.num_images, self.cap, stream_ptr()))
        if sc is not None:
            sc.record_stream(torch.cuda.current_stream(self.device))

    def tables(self):
        """The table on the host: per image a list of (class index, x1, y1, x2, y2, score), file order."""
        cnt = self.det_count.cpu().numpy()
        box, score, cls = self.det_box.cpu().numpy(), self.det_score.cpu().numpy(), self.det_cls.cpu().numpy()
        return [[(int(cls[i, j]),) + tuple(float(v) for v in box[i, j]) + (float(score[i, j]),) for j in range(max(0, int(cnt[i])))]
                for i in range(len(cnt))]

    def load_rows(self, rows):
        """Fills the table from host rows (per image a list of (class index, x1, y1, x2, y2, score), file order: class-major)."""
        n = self.gt.num_images
        if len(rows) != n:
            raise _lib.SqdetError("load_rows: %d images for a table of %d" % (len(rows), n))
        big = [i for i, r in enumerate(rows) if len(r) > self.cap]
        if big:
            raise _lib.SqdetUnsupported("load_rows: image %d has %d detections (table holds %d)" % (big[0], len(rows[big[0]]), self.cap))
        box = np.zeros((n, self.cap, 4), np.float64)
        score = np.zeros((n, self.cap), np.float64)
        cls = np.zeros((n, self.cap), np.int32)
        cnt = np.zeros(n, np.int32)
        for i, r in enumerate(rows):
            cnt[i] = len(r)
            for j, (c, x1, y1, x2, y2, s) in enumerate(r):
                if self.classes is not None and not 0 <= c < self.classes:
                    raise _lib.SqdetError("load_rows: image %d row %d has class %d of %d" % (i, j, c, self.classes))
                cls[i, j], box[i, j], score[i, j] = c, (x1, y1, x2, y2), s
        self.det_box.copy_(torch.from_numpy(box))
        self.det_score.copy_(torch.from_numpy(score))
        self.det_cls.copy_(torch.from_numpy(cls))
        self.det_count.copy_(torch.from_numpy(cnt))
        self.status.zero_()
