"""CLEAR-MOT and IDF1 evaluation of the tracker, on the device (csrc/mot_eval.hip; include/sqdet.h, "tracking evaluation"): MOTA,
MOTP, identity switches, fragmentations, mostly tracked / mostly lost and IDF1 of ``Tracker.update``'s outputs against labelled
objects.  The reference has no counterpart; the definition is the header's (tests/mot_reference.py restates it in NumPy).

  * ``MotAccumulator(streams, device, classes, iou_thresh=0.5)`` owns the tables of `streams` independent streams.
    ``update(boxes, cls, counts, ids, states, gt, frames_per_stream=1)``: ONE asynchronous launch over the tracker's own device
    arrays -- identities never return to the host; ``evaluate()`` -> per-stream, per-class and overall counters and metrics.
  * ``MotGroundTruth``: labelled objects per frame, from a MOTChallenge ``gt.txt``, a KITTI tracking label file or arrays.
  * ``load_mot_results(path)`` reads what ``demo.py --track_out`` writes; ``score_files`` scores such a file on the device;
    ``format_summary`` prints an evaluation.
"""
import ctypes as C

import numpy as np

from .stream_tables import StreamTables, tables_struct

CAP, MAX_OBJECTS, MAX_HYPOTHESES, MAX_CLASSES = 64, 256, 1024, 128
COUNTERS = ("tp", "fn", "fp", "idsw", "ignored_hyp", "frag", "mt", "pt", "ml", "idtp", "idfn", "idfp", "gt_ids", "hyp_ids")
K = len(COUNTERS)
IGNORE = 1
OBJ_FIELDS = ("obj_id", "obj_cls", "obj_last", "obj_present", "obj_tracked", "obj_frag", "obj_run")
HYP_FIELDS = ("hyp_id", "hyp_cls", "hyp_frames")
FIELDS = OBJ_FIELDS + HYP_FIELDS + ("n_obj", "n_hyp", "status", "counts", "iou_sum", "overlap")
# MOT16/17 gt.txt classes that are scored as "ignore" beside conf 0: person on vehicle, static person, distractor, reflection
MOT_DISTRACTORS = (2, 7, 8, 12)


_Tables = tables_struct(FIELDS)                  # sqdet_mot_tables_t


def table_shapes(streams, classes):
    """{name: (shape, torch dtype name)} of the tables of `streams` streams; a reset is every table zero."""
    S = int(streams)
    d = {f: ((S, MAX_OBJECTS), "int32") for f in OBJ_FIELDS}
    d.update({f: ((S, MAX_HYPOTHESES), "int32") for f in HYP_FIELDS})
    d.update({"n_obj": ((S,), "int32"), "n_hyp": ((S,), "int32"), "status": ((S,), "int32"), "counts": ((S, int(classes), 5), "int64"),
              "iou_sum": ((S, int(classes)), "float64"), "overlap": ((S, MAX_OBJECTS, MAX_HYPOTHESES), "int32")})
    return d


def metrics(counters, iou_sum):
    """One counter vector [K] and its iou_sum -> dict: the counters, mota, motp, idf1, precision, recall (nan: no denominator)."""
    c = {k: int(v) for k, v in zip(COUNTERS, counters)}
    nan = float("nan")
    gt = c["tp"] + c["fn"]
    c["iou_sum"] = float(iou_sum)
    c["mota"] = 1.0 - (c["fn"] + c["fp"] + c["idsw"]) / gt if gt else nan
    c["motp"] = float(iou_sum) / c["tp"] if c["tp"] else nan
    den = 2 * c["idtp"] + c["idfp"] + c["idfn"]
    c["idf1"] = 2 * c["idtp"] / den if den else nan
    c["precision"] = c["tp"] / (c["tp"] + c["fp"]) if c["tp"] + c["fp"] else nan
    c["recall"] = c["tp"] / gt if gt else nan
    return c


class MotAccumulator(StreamTables):
    FIELDS, STRUCT = FIELDS, _Tables

    def __init__(self, streams, device, classes, iou_thresh=0.5, tables=None):
        """tables: {name: device tensor} of the caller's own in the shapes and dtypes of ``table_shapes(streams, classes)``,
        already reset (zero); None: the accumulator allocates them (1 MiB of `overlap` per stream)."""
        import torch
        from ._lib import SqdetError, SqdetUnsupported
        if int(streams) < 1 or int(classes) < 1:
            raise SqdetError("MotAccumulator: streams and classes must be positive")
        if int(classes) > MAX_CLASSES:
            raise SqdetUnsupported("MotAccumulator: %d classes (at most %d)" % (classes, MAX_CLASSES))
        if not 0.0 < float(iou_thresh) <= 1.0:
            raise SqdetError("MotAccumulator: iou_thresh %r must be in (0, 1]" % (iou_thresh,))
        self.classes, self.iou_thresh = int(classes), float(iou_thresh)
        super().__init__(streams, device, table_shapes(streams, classes), tables)
        self._result = torch.zeros((self.streams, self.classes, K), dtype=torch.int64, device=self.device)

    def update(self, boxes, cls, counts, ids, states, gt, frames_per_stream=1, stream=None, max_workgroups=0):
        """boxes float32 [n, rows, 4], cls int32 [n, rows], counts int32 [n] -- the filter's outputs -- and ids, states int32
        [n, rows] -- Tracker.update's -- with n = streams * frames_per_stream; gt = (gt_box float64 [n, G, 4], gt_id, gt_cls,
        gt_flags int32 [n, G], gt_count int32 [n]) on the device (MotGroundTruth.device).  One asynchronous launch on `stream`
        (None: the current one)."""
        import torch
        from . import ops
        from ._lib import SqdetError, check, lib
        F, n, rows = self._frames(boxes, frames_per_stream)
        for t, what in ((cls, "cls"), (ids, "ids"), (states, "states")):
            if tuple(t.shape) != (n, rows):
                raise SqdetError("MotAccumulator.update: %s must be [%d, %d]" % (what, n, rows))
        if tuple(counts.shape) != (n,):
            raise SqdetError("MotAccumulator.update: counts must be [%d]" % n)
        if len(gt) != 5:
            raise SqdetError("MotAccumulator.update: gt is (gt_box, gt_id, gt_cls, gt_flags, gt_count)")
        gt_box, gt_id, gt_cls, gt_flags, gt_count = gt
        if gt_box.dim() != 3 or int(gt_box.shape[0]) != n or int(gt_box.shape[2]) != 4:
            raise SqdetError("MotAccumulator.update: gt_box must be [%d, G, 4]" % n)
        G = int(gt_box.shape[1])
        for t, what in ((gt_id, "gt_id"), (gt_cls, "gt_cls"), (gt_flags, "gt_flags")):
            if tuple(t.shape) != (n, G):
                raise SqdetError("MotAccumulator.update: %s must be [%d, %d]" % (what, n, G))
        if tuple(gt_count.shape) != (n,):
            raise SqdetError("MotAccumulator.update: gt_count must be [%d]" % n)
        if boxes.device != self.device or gt_box.device != self.device:
            raise SqdetError("MotAccumulator.update: rows on %s, ground truth on %s, tables on %s" % (boxes.device, gt_box.device, self.device))
        check(lib().sqdet_mot_update(
            C.byref(self._tables), ops._dev(boxes, "boxes", torch.float32), ops._dev(cls, "cls", torch.int32),
            ops._dev(counts, "counts", torch.int32), ops._dev(ids, "ids", torch.int32), ops._dev(states, "states", torch.int32),
            ops._dev(gt_box, "gt_box", torch.float64), ops._dev(gt_id, "gt_id", torch.int32), ops._dev(gt_cls, "gt_cls", torch.int32),
            ops._dev(gt_flags, "gt_flags", torch.int32), ops._dev(gt_count, "gt_count", torch.int32), self.streams, F, rows, G,
            self.classes, self.iou_thresh, int(max_workgroups), self._stream(stream)), "sqdet_mot_update")

    def evaluate_raw(self, stream=None):
        """-> (counters int64 [S, classes, K], iou_sum float64 [S, classes]) on the host (synchronises once)."""
        from ._lib import check, lib
        counters = np.zeros((self.streams, self.classes, K), np.int64)
        iou_sum = np.zeros((self.streams, self.classes), np.float64)
        check(lib().sqdet_mot_evaluate(C.byref(self._tables), self.streams, self.classes, C.c_void_p(self._result.data_ptr()),
                                       counters.ctypes.data_as(C.c_void_p), iou_sum.ctypes.data_as(C.c_void_p), self._stream(stream)),
              "sqdet_mot_evaluate")
        return counters, iou_sum

    def evaluate(self, stream=None):
        """-> dict: counters, iou_sum (arrays), per_stream [S][classes], per_class [classes] (summed over streams), streams [S]
        (summed over classes) and overall -- each a dict of the counters and mota, motp, idf1, precision, recall."""
        return summarize(*self.evaluate_raw(stream))

    def _settings(self):
        return {"iou_thresh": self.iou_thresh, "classes": self.classes}

    def _settings_error(self, d):
        return "saved with iou_thresh %s and %s classes" % (d.get("iou_thresh"), d.get("classes"))


def summarize(counters, iou_sum):
    S, classes = iou_sum.shape
    return {
        "counters": counters, "iou_sum": iou_sum,
        "per_stream": [[metrics(counters[s, c], iou_sum[s, c]) for c in range(classes)] for s in range(S)],
        "per_class": [metrics(counters[:, c].sum(0), iou_sum[:, c].sum()) for c in range(classes)],
        "streams": [metrics(counters[s].sum(0), iou_sum[s].sum()) for s in range(S)],
        "overall": metrics(counters.sum((0, 1)), iou_sum.sum()),
    }


def format_summary(result, class_names=None):
    """The evaluation as text: one line per class that has objects or hypotheses, then the overall line."""
    head = "%-14s %7s %7s %7s %7s %7s %6s %6s %6s %5s %5s %5s %5s %5s" % (
        "", "MOTA", "MOTP", "IDF1", "Prcn", "Rcll", "TP", "FP", "FN", "IDs", "FM", "MT", "PT", "ML")
    lines = [head]

    def line(name, m):
        return "%-14s %7.4f %7.4f %7.4f %7.4f %7.4f %6d %6d %6d %5d %5d %5d %5d %5d" % (
            name[:14], m["mota"], m["motp"], m["idf1"], m["precision"], m["recall"], m["tp"], m["fp"], m["fn"], m["idsw"], m["frag"],
            m["mt"], m["pt"], m["ml"])
    for c, m in enumerate(result["per_class"]):
        if m["gt_ids"] or m["hyp_ids"]:
            lines.append(line(class_names[c] if class_names is not None and c < len(class_names) else "class %d" % c, m))
    lines.append(line("OVERALL", result["overall"]))
    return "\n".join(lines)


class MotGroundTruth:
    """Labelled objects per frame (frames count from 1): ``frames[f]`` is a list of (id, cls, flags, (cx, cy, w, h))."""

    def __init__(self, frames=None):
        self.frames = dict(frames or {})

    @property
    def n_frames(self):
        return max(self.frames) if self.frames else 0

    @property
    def max_objects(self):
        return max([len(v) for v in self.frames.values()] + [1])

    @classmethod
    def from_mot_text(cls, path, distractors=MOT_DISTRACTORS):
        """A MOTChallenge gt.txt: frame, id, left, top, w, h, conf, class, visibility.  Boxes go to centre form; a row with
        conf 0 or a class among `distractors` is IGNORE; every row is class 0 (the benchmark scores one class)."""
        frames = {}
        for ln in open(path):
            v = ln.replace(",", " ").split()
            if not v:
                continue
            f, ident = int(float(v[0])), int(float(v[1]))
            left, top, w, h = (float(q) for q in v[2:6])
            conf = float(v[6]) if len(v) > 6 else 1.0
            klass = int(float(v[7])) if len(v) > 7 else -1
            flags = IGNORE if conf == 0 or klass in distractors else 0
            frames.setdefault(f, []).append((ident, 0, flags, (left + w / 2, top + h / 2, w, h)))
        return cls(frames)

    @classmethod
    def from_kitti_tracking(cls, path, class_names):
        """A KITTI tracking label file: frame, track id, type, truncated, occluded, alpha, left, top, right, bottom, ...  Frames
        and ids count from 0 there and from 1 here.  A DontCare region, or a type that is not among `class_names`, becomes one
        IGNORE row per class, so that it swallows a hypothesis of any class."""
        names = [n.lower() for n in class_names]
        frames = {}
        for ln in open(path):
            v = ln.split()
            if not v:
                continue
            f, ident, kind = int(v[0]) + 1, int(v[1]) + 1, v[2].lower()
            left, top, right, bottom = (float(q) for q in v[6:10])
            box = ((left + right) / 2, (top + bottom) / 2, right - left, bottom - top)
            rows = frames.setdefault(f, [])
            if kind in names:
                rows.append((ident, names.index(kind), 0, box))
            else:
                for c in range(len(names)):
                    rows.append((1000000 + len(rows), c, IGNORE, box))
        return cls(frames)

    @classmethod
    def from_arrays(cls, gt_box, gt_id, gt_cls, gt_flags, gt_count):
        """Arrays [n, G, ...] of one stream, image i being frame i + 1."""
        frames = {}
        for i in range(len(gt_count)):
            frames[i + 1] = [(int(gt_id[i, j]), int(gt_cls[i, j]), int(gt_flags[i, j]), tuple(float(q) for q in gt_box[i, j]))
                             for j in range(min(max(int(gt_count[i]), 0), gt_box.shape[1]))]
        return cls(frames)

    def arrays(self, first=1, n=None, G=None):
        """Frames first .. first + n - 1 -> (gt_box float64 [n, G, 4], gt_id, gt_cls, gt_flags int32 [n, G], gt_count int32 [n])."""
        from ._lib import SqdetUnsupported
        n = self.n_frames - first + 1 if n is None else int(n)
        G = self.max_objects if G is None else int(G)
        if self.max_objects > CAP:
            raise SqdetUnsupported("MotGroundTruth: %d objects in a frame (at most %d)" % (self.max_objects, CAP))
        box = np.zeros((n, G, 4), np.float64)
        ident, klass, flags = (np.zeros((n, G), np.int32) for _ in range(3))
        count = np.zeros(n, np.int32)
        for i in range(n):
            rows = self.frames.get(first + i, [])
            count[i] = len(rows)
            for j, (a, c, fl, b) in enumerate(rows):
                ident[i, j], klass[i, j], flags[i, j], box[i, j] = a, c, fl, b
        return box, ident, klass, flags, count

    def device(self, device, first=1, n=None, G=None):
        import torch
        return tuple(torch.from_numpy(a).to(device) for a in self.arrays(first, n, G))


def load_mot_results(path, n_frames=None):
    """The MOT-challenge text ``demo.py --track_out`` writes (frame, id, left, top, w, h, score, -1, -1, -1) -> the tracker's
    arrays of one stream, image i being frame i + 1: (boxes float32 [n, rows, 4] (cx, cy, w, h), cls int32 [n, rows] (all 0: the
    file has no class), counts int32 [n], ids int32 [n, rows], states int32 [n, rows] (2: the file holds confirmed rows only))."""
    from ._lib import SqdetUnsupported
    frames = {}
    for ln in open(path):
        v = ln.replace(",", " ").split()
        if not v:
            continue
        left, top, w, h = (float(q) for q in v[2:6])
        frames.setdefault(int(float(v[0])), []).append((int(float(v[1])), (left + w / 2, top + h / 2, w, h)))
    n = max(list(frames) + [1]) if n_frames is None else int(n_frames)
    rows = max([len(r) for r in frames.values()] + [1])
    if rows > CAP:
        raise SqdetUnsupported("load_mot_results: %d rows in a frame (at most %d)" % (rows, CAP))
    boxes, cls = np.zeros((n, rows, 4), np.float32), np.zeros((n, rows), np.int32)
    ids, states, counts = np.full((n, rows), -1, np.int32), np.zeros((n, rows), np.int32), np.zeros(n, np.int32)
    for f, r in frames.items():
        if 1 <= f <= n:
            counts[f - 1] = len(r)
            for j, (ident, box) in enumerate(r):
                boxes[f - 1, j], ids[f - 1, j], states[f - 1, j] = box, ident, 2
    return boxes, cls, counts, ids, states


def score_files(gt_path, results_path, device, fmt="mot", iou_thresh=0.5, class_names=("car", "pedestrian", "cyclist"), chunk=256):
    """Scores a results file against a label file on the device, `chunk` frames a launch -> (evaluation, class names).  The
    results carry no class, so every row -- of a KITTI label file too -- is scored as one class."""
    import torch
    if fmt == "kitti":
        gt = MotGroundTruth.from_kitti_tracking(gt_path, class_names)
        for f, rows in gt.frames.items():         # one class: of a region that was replicated per class, class 0's row stays
            gt.frames[f] = [(a, 0, fl, b) for a, c, fl, b in rows if not fl & IGNORE or c == 0]
    elif fmt == "mot":
        gt = MotGroundTruth.from_mot_text(gt_path)
    else:
        raise ValueError("format must be mot or kitti, not %r" % (fmt,))
    n = max(gt.n_frames, 1)
    res = load_mot_results(results_path)
    n = max(n, res[0].shape[0])
    res = load_mot_results(results_path, n)
    acc = MotAccumulator(1, device, 1, iou_thresh)
    for f0 in range(0, n, chunk):
        f1 = min(f0 + chunk, n)
        acc.update(*[torch.from_numpy(a[f0:f1]).to(device) for a in res], gt.device(device, f0 + 1, f1 - f0), frames_per_stream=f1 - f0)
    return acc.evaluate(), ["all"]
