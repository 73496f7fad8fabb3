"""Boxes and labels drawn into images that are already on the device (csrc/draw.hip; include/sqdet.h, "drawing"): the
reference's _draw_box / _viz_prediction_result of the training image summary (src/train.py:51-99, 287-295), the rectangle +
text of imdb.visualize_detections (src/dataset/imdb.py:254-305) and of the demos (src/demo.py), which draw with cv2 / PIL on
the host, one image at a time.

  * ``make_items(...)``: box rows on the device (the filtered rows of ``ops.detect_filter`` / ``ops.filter_prediction``, or a
    ground-truth table) -> ``DrawItems``, a device table of rectangles with colours and labels; no host round trip.
  * ``pack_items(...)``: the same table from host values (the rows eval.py picks from its error file; tests).
  * ``draw(images, items, ...)``: ONE launch draws a whole batch, table after table, row after row (painter's order).
  * ``ImageSummary(mc, train_dir, max_images)``: what train.py --image_summary calls at a summary step.
  * ``font()``: the 5x7 font as an array.

Images and colours are BGR, as everywhere in this package (what cv2.imread returns); ``order="rgb"`` reverses the channels of
the output for PIL.  Text is this project's own 5x7 font, not cv2's Hershey strokes or PIL's bitmap font: position, colour and
content of a label follow the reference, its glyphs do not.
"""
import ctypes as C
import os

import numpy as np

ITEM_BYTES, MAX_ITEMS, MAX_TABLES, LABEL_MAX, NAME_BYTES = 64, 256, 4, 31, 32
U8 = 2                                                             # SQDET_DRAW_U8
ANCHORS = {"bottom_left": 0, "top_left": 1}
LABELS = {"name": 0, "name: (p)": 1, "name (p)": 2}                # "<name>", "<name>: (%.2f)", "<name> (%.2f)"
ITEM_DTYPE = np.dtype([("rect", "<i4", (4,)), ("bgr", "u1", (3,)), ("anchor", "u1"), ("label_len", "<i4"), ("label", "u1", (32,)),
                       ("pad", "<i4", (2,))])
assert ITEM_DTYPE.itemsize == ITEM_BYTES


def font():
    """uint8 [95, 7]: glyph of chr(32 + i), 7 rows top to bottom, bit 4 = the leftmost of 5 columns (csrc/font5x7.h)."""
    from ._lib import check, lib
    out = np.zeros((95, 7), np.uint8)
    check(lib().sqdet_draw_font5x7(out.ctypes.data_as(C.c_void_p), out.nbytes), "sqdet_draw_font5x7")
    return out


class DrawItems:
    """An item table on the device: ``rows`` uint8 [B, cap, 64] (ITEM_DTYPE), ``counts`` int32 [B]."""

    def __init__(self, rows, counts):
        self.rows, self.counts = rows, counts
        self.n, self.cap = int(rows.shape[0]), int(rows.shape[1])

    def cpu(self):
        """(structured array [B, cap] of ITEM_DTYPE, counts [B]) on the host; synchronises."""
        raw = self.rows.cpu().numpy()
        return np.ascontiguousarray(raw).reshape(self.n, self.cap * ITEM_BYTES).view(ITEM_DTYPE), self.counts.cpu().numpy()

    def decode(self):
        """Per image the list of its items as (x0, y0, x1, y1, (b, g, r), label bytes, anchor name)."""
        rows, counts = self.cpu()
        names = {v: k for k, v in ANCHORS.items()}
        return [[(int(r["rect"][0]), int(r["rect"][1]), int(r["rect"][2]), int(r["rect"][3]), tuple(int(v) for v in r["bgr"]),
                  bytes(r["label"][:max(0, min(int(r["label_len"]), LABEL_MAX))]), names[int(r["anchor"])])
                 for r in rows[i, :max(0, min(int(counts[i]), self.cap))]] for i in range(self.n)]


def pack_items(per_image, device, cap=None):
    """per_image: for every image a list of (x0, y0, x1, y1, (b, g, r), label, anchor) -- label str / bytes (cut at 31 bytes),
    anchor "bottom_left" / "top_left" -> DrawItems on `device`."""
    import torch
    from ._lib import SqdetError
    cap = max([1] + [len(r) for r in per_image]) if cap is None else int(cap)
    if any(len(r) > cap for r in per_image):
        raise SqdetError("pack_items: an image has more than cap = %d items" % cap)
    rows = np.zeros((len(per_image), cap), ITEM_DTYPE)
    for i, items in enumerate(per_image):
        for j, (x0, y0, x1, y1, bgr, label, anchor) in enumerate(items):
            lab = (label.encode("latin-1", "replace") if isinstance(label, str) else bytes(label))[:LABEL_MAX]
            r = rows[i, j]
            r["rect"], r["bgr"], r["anchor"], r["label_len"] = (x0, y0, x1, y1), bgr, ANCHORS[anchor], len(lab)
            r["label"][:len(lab)] = np.frombuffer(lab, np.uint8)
    raw = torch.from_numpy(rows.view(np.uint8).reshape(len(per_image), cap, ITEM_BYTES)).to(device)
    return DrawItems(raw, torch.tensor([len(r) for r in per_image], dtype=torch.int32).to(device))


def pack_names(names, device):
    """Class names as the packed byte table of the item builder: uint8 [classes, 32] on `device`, NUL-padded."""
    import torch
    t = np.zeros((len(names), NAME_BYTES), np.uint8)
    for i, n in enumerate(names):
        b = n.encode("latin-1", "replace")[:NAME_BYTES - 1]
        t[i, :len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(t).to(device)


def _item_tables(who, boxes, dtypes, rows, counts, names, colours, out):
    """What the item builders' wrappers (make_items, track.make_track_items) do before their launch: boxes [B, M, 4] of one of
    `dtypes` (torch dtype names); rows: (tensor or None, message) pairs, each tensor [B, M]; counts: (tensor [B], message) --
    a message may hold %(B)d and %(M)d; names and colours (a list of (b, g, r), or None) packed for the device unless they are
    tensors already; the table to fill: `out`, a new one, or for M == 0 an empty one with nothing to launch.
    -> (B, M, names, colours, out)."""
    import torch
    from ._lib import SqdetError
    if boxes.dtype not in [getattr(torch, d) for d in dtypes] or boxes.dim() != 3 or int(boxes.shape[2]) != 4:
        raise SqdetError("%s: boxes must be [B, M, 4] %s" % (who, " or ".join(dtypes)))
    B, M, dev = int(boxes.shape[0]), int(boxes.shape[1]), boxes.device
    for t, shape, message in [(t, (B, M), m) for t, m in rows] + [(counts[0], (B,), counts[1])]:
        if t is not None and tuple(t.shape) != shape:
            raise SqdetError("%s: %s" % (who, message % {"B": B, "M": M}))
    if not isinstance(names, torch.Tensor):
        names = pack_names(names, dev)
    if colours is not None and not isinstance(colours, torch.Tensor):
        colours = torch.tensor(np.asarray(colours, np.uint8).reshape(-1, 3)).to(dev)
    if M == 0:
        out = DrawItems(torch.zeros((B, 1, ITEM_BYTES), dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    elif out is None:
        out = DrawItems(torch.empty((B, M, ITEM_BYTES), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    if out.n != B:
        raise SqdetError("%s: out holds %d images, boxes %d" % (who, out.n, B))
    return B, M, names, colours, out


def make_items(boxes, classes, counts, names, probs=None, plot_thresh=0.0, form="center", color=(0, 255, 0), class_colors=None,
               label="name", anchor="bottom_left", out=None):
    """Box rows -> DrawItems, on the device (sqdet_draw_build_items).  boxes [B, M, 4] float32 or float64, classes int32 [B, M],
    counts int32 [B]; probs float32 [B, M] or None: image i keeps its rows j < counts[i] with probs[i, j] > plot_thresh.
    form "center" (cx, cy, w, h -> int() of util.bbox_transform, in the boxes' precision) or "diagonal"; color (b, g, r), or
    class_colors: uint8 device tensor [classes, 3] / a list of (b, g, r) per class (the reference's cdict); names: a list of
    class names or pack_names(...)'s tensor; label: "name", "name: (p)" or "name (p)" with p = '%.2f' % float(float32 prob)."""
    import torch
    from . import ops
    from ._lib import SqdetError, check, lib, stream_ptr
    if form not in ("center", "diagonal"):
        raise SqdetError("bounding box format not accepted: {}.".format(form))
    shape = "classes / probs must be [B, M], counts [B]"
    B, M, names, class_colors, out = _item_tables("make_items", boxes, ("float32", "float64"), [(classes, shape), (probs, shape)],
                                                  (counts, shape), names, class_colors, out)
    if class_colors is not None and int(class_colors.shape[0]) != int(names.shape[0]):
        raise SqdetError("make_items: %d class colours for %d names" % (int(class_colors.shape[0]), int(names.shape[0])))
    if M == 0:
        return out
    check(lib().sqdet_draw_build_items(
        ops._dev(boxes, "boxes"), int(boxes.dtype == torch.float64), ops._dev(probs, "probs", torch.float32) if probs is not None else None,
        ops._dev(classes, "classes", torch.int32), ops._dev(counts, "counts", torch.int32), B, M, int(form == "diagonal"),
        float(plot_thresh), ops._dev(names, "names", torch.uint8), int(names.shape[0]),
        ops._dev(class_colors, "class_colors", torch.uint8) if class_colors is not None else None, int(color[0]), int(color[1]),
        int(color[2]), LABELS[label], ANCHORS[anchor], ops._dev(out.rows, "items"), ops._dev(out.counts, "item counts", torch.int32),
        out.cap, stream_ptr()), "sqdet_draw_build_items")
    return out


def draw(images, items=(), bgr_means=None, order="rgb", out=None):
    """images [B, H, W, 3] on the device -- float32 / float16 network input (mean-subtracted BGR; bgr_means is added back and
    the sum rounded half to even, clamped to [0, 255]) or uint8 BGR (bgr_means None) -- with the items of `items` (a DrawItems
    or a list of up to four) drawn over them in order -> uint8 [B, H, W, 3], channels in `order` ("rgb" / "bgr").  One launch
    on the current stream (sqdet_draw_items)."""
    import torch
    from . import ops
    from ._lib import SqdetError, check, dtype_code, lib, stream_ptr
    tables = [items] if isinstance(items, DrawItems) else list(items)
    if images.dim() != 4 or int(images.shape[3]) != 3:
        raise SqdetError("draw: images must be [B, H, W, 3]")
    if order not in ("rgb", "bgr"):
        raise SqdetError("draw: order must be 'rgb' or 'bgr'")
    B, H, W = (int(v) for v in images.shape[:3])
    if images.dtype == torch.uint8:
        kind, means = U8, None
    else:
        if bgr_means is None:
            raise SqdetError("draw: a float network input needs bgr_means")
        kind, means = dtype_code(images.dtype), (C.c_float * 3)(*[float(v) for v in np.asarray(bgr_means, np.float32).reshape(-1)[:3]])
    if any(t.n != B for t in tables):
        raise SqdetError("draw: an item table does not hold %d images" % B)
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=images.device)
    if tuple(out.shape) != (B, H, W, 3):
        raise SqdetError("draw: out must be uint8 %s" % ((B, H, W, 3),))
    k = len(tables)
    ptrs = (C.c_void_p * max(k, 1))(*[ops._dev(t.rows, "items", torch.uint8) for t in tables])
    cnts = (C.c_void_p * max(k, 1))(*[ops._dev(t.counts, "item counts", torch.int32) for t in tables])
    caps = (C.c_int * max(k, 1))(*[t.cap for t in tables])
    check(lib().sqdet_draw_items(ops._dev(images, "images"), ops._dev(out, "out", torch.uint8), kind, B, H, W, means,
                                 int(order == "rgb"), ptrs, cnts, caps, k, stream_ptr()), "sqdet_draw_items")
    return out


class ImageSummary:
    """The image summary of the training graph (src/train.py:74-99, 287-295): at a summary step the first `max_images` images
    of the batch with their ground truth -- (0, 255, 0), the class name -- and the filtered detections above
    mc.PLOT_PROB_THRESH -- (0, 0, 255) BGR, "<name>: (<prob>)" -- drawn over them.

    ``record(step, batch, preds)``: batch is the reader's Batch (image_input, gt_boxes, gt_classes, gt_counts), preds the
    step's ConvDet output; everything runs on the device -- interpret_output + filter_prediction, the two item builds, ONE
    draw launch -- and only the finished uint8 pictures leave it, by one asynchronous copy into pinned memory behind an
    event.  ``<train_dir>/images/step-<step>/<i>.png`` are written once the event has completed: at ``poll()``, at the latest
    at the next ``record()`` or at ``close()`` (TrainSummary's life cycle).  It reads the batch and preds and nothing else:
    no trainer state, no random numbers.

    TF's tf.summary.image rescales a float image to [0, 255] by its own minimum and maximum; here the BGR means are added back,
    so the picture is the (augmented) input image."""

    GT_COLOR, DET_COLOR = (0, 255, 0), (0, 0, 255)

    def __init__(self, mc, train_dir, max_images, device=None, write=True):
        import torch
        self.mc, self.dir, self.max_images, self.write = mc, train_dir, int(max_images), bool(write)
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX).astype(np.float32)).to(self.dev)
        self.names = pack_names(list(mc.CLASS_NAMES), self.dev)
        self._event, self._pending, self._host = torch.cuda.Event(), None, None
        self.written = 0
        self.last = None

    def filtered(self, preds):
        """The filtered rows of preds, as _viz_prediction_result's model.filter_prediction gives them: (boxes, probs, classes,
        anchor indices, counts) on the device."""
        from . import nms, ops
        mc = self.mc
        n, gh, gw, _ = (int(v) for v in preds.shape)
        A = gh * gw * mc.ANCHOR_PER_GRID
        opt = nms.nms_options(mc)     # (the model's suppression policy: what eval.py and demo.py filter with)
        thresh = nms.first_stage_thresh(opt, mc)
        if ops.detect_filter_supported(A, mc.TOP_N_DETECTION):
            out = ops.detect_filter(preds, self.anchors, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH,
                                    mc.TOP_N_DETECTION, thresh)
        else:
            boxes, probs, cls = ops.interpret_output(preds, self.anchors, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT,
                                                     mc.EXP_THRESH)
            out = ops.filter_prediction(boxes, probs, cls, mc.CLASSES, mc.TOP_N_DETECTION, thresh, mc.PROB_THRESH)
        return out if nms.is_default(opt) else nms.apply(opt, mc, out)

    def render(self, batch, preds):
        """uint8 RGB [n, H, W, 3] on the device, n = min(max_images, batch size)."""
        mc = self.mc
        n = min(self.max_images, int(batch.image_input.shape[0]))
        m = int(batch.gt_boxes.shape[1])
        if m + int(mc.TOP_N_DETECTION) > MAX_ITEMS and getattr(batch, "label_per_batch", None) is not None:
            # a mosaic reader pads to four times the dataset's largest object count: keep the columns these images use (known to the
            # host), so that the two tables fit one draw launch wherever the boxes themselves do
            m = max(1, max(len(lab) for lab in batch.label_per_batch[:n]))
        gt = make_items(batch.gt_boxes[:n, :m].contiguous(), batch.gt_classes[:n, :m].contiguous(), batch.gt_counts[:n].contiguous(), self.names,
                        color=self.GT_COLOR, label="name")
        ob, op, oc, _, cnt = self.filtered(preds[:n].contiguous())
        det = make_items(ob, oc, cnt, self.names, probs=op, plot_thresh=mc.PLOT_PROB_THRESH, color=self.DET_COLOR, label="name: (p)")
        return draw(batch.image_input[:n].contiguous(), [gt, det], bgr_means=mc.BGR_MEANS, order="rgb")

    def record(self, step, batch, preds):
        import torch
        self.drain()                                    # the pinned buffer is free again
        with torch.cuda.device(self.dev):
            pics = self.render(batch, preds)
            if self._host is None or tuple(self._host.shape) != tuple(pics.shape):
                self._host = torch.empty(tuple(pics.shape), dtype=torch.uint8).pin_memory()
            self._host.copy_(pics, non_blocking=True)
            self._event.record(torch.cuda.current_stream())
        self._pending = (int(step), pics)               # (pics stays alive until its copy has landed)

    def poll(self):
        """Writes the pending pictures if their copy has landed; never waits."""
        if self._pending is not None and self._event.query():
            self._emit()

    def drain(self):
        if self._pending is not None:
            self._event.synchronize()
            self._emit()

    def close(self):
        self.drain()

    def _emit(self):
        step, _ = self._pending
        self._pending = None
        self.last = (step, self._host.numpy().copy())
        if self.write:
            from PIL import Image
            d = os.path.join(self.dir, "images", "step-%d" % step)
            os.makedirs(d, exist_ok=True)
            for i, im in enumerate(self.last[1]):
                Image.fromarray(im).save(os.path.join(d, "%d.png" % i))
                self.written += 1
