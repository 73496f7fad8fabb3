"""Training batch reader: the reference's ``imdb.read_batch`` (src/dataset/imdb.py:100-239) with its drift / flip data
augmentation, the per-pixel half on the GPU.

Per image the reference subtracts ``BGR_MEANS``, shifts the image by a random drift (dx, dy) -- cropping on one side,
zero-padding on the other --, mirrors it with probability 1/2, resizes it from its drifted size to the network input and
moves, mirrors and rescales the boxes to match.  Here the few scalars per image (batch order, random draws, box transform)
stay on the host in NumPy float64, in the reference's order and with its calls, so that they are the reference's bit for
bit; the image warp is one launch of ``sqdet_augment_bgr`` (csrc/augment.hip) for the whole batch.

Random draws come from one ``np.random.RandomState(seed)`` instead of the global ``np.random``: with the same seed, the
same dataset, and the reference's global generator seeded the same way before ``kitti.__init__``, the permutations, the
drifts and the flips are the reference's.

Divergences from the reference, on purpose:
  * an image with no boxes draws its drift from the full [-DRIFT, DRIFT] range; the reference crashes on it (``min()`` of
    an empty sequence, imdb.py:158-159);
  * the anchor assignment (imdb.py:195-239) is not done here -- ``ops.build_labels`` / the trainers do it on the GPU from
    ``gt_boxes`` / ``gt_classes`` / ``gt_counts`` -- and ``mc.DEBUG_MODE``'s IoU statistics come from ``anchors.coverage`` /
    ``anchors.dataset_coverage`` (``train.py --anchor_report``), for a whole dataset instead of per batch.

Beyond the reference (all off by default; with ``mc.AUG_GEOMETRY == "drift"`` and ``mc.AUG_COLOR`` false -- or a config without
these fields -- the reader draws the reference's numbers and launches ``sqdet_augment_bgr`` as before):
  * ``mc.AUG_GEOMETRY = "ssd"``: per image a zoom-out canvas and an IoU-constrained crop window in it (``ssd_window``), the boxes
    cut to the window (``window_boxes``);
  * ``mc.AUG_COLOR``: per image a 3x4 colour matrix (``draw_color_matrix`` / ``color_matrix``).
Both are a few float64 scalars per image on the host and still ONE launch per batch: ``sqdet_augment_bgr_window``.
  * ``mc.AUG_MOSAIC_PROB > 0``: with that probability a batch image is a MOSAIC of four dataset images, each a crop shown at
    roughly half scale in its own pane of the network input (``mosaic_part`` / ``mosaic_part_boxes``); the other images keep the
    policy above as part 0 of a mosaic with one pane.  The whole batch is ONE launch of ``sqdet_augment_bgr_mosaic``.

Kept on purpose, as in the reference: the shuffled branch reshuffles as soon as ``cur + BATCH_SIZE >= len`` (imdb.py:
121-123), so the last full batch of every epoch is never served and each epoch serves ``ceil(len / B) - 1`` batches.
"""
from collections import namedtuple

import numpy as np

Batch = namedtuple("Batch", ["image_input", "gt_boxes", "gt_classes", "gt_counts", "aug", "bbox_per_batch",
                             "label_per_batch", "batch_idx", "window", "mode", "color", "split", "parts", "part_window", "part_flip",
                             "part_color"], defaults=(None,) * 8)
Batch.__doc__ = """One training batch.  image_input: device [B, IMAGE_HEIGHT, IMAGE_WIDTH, 3] in the reader's dtype;
gt_boxes float64 [B, M, 4] (cx, cy, w, h in network-input pixels), gt_classes int32 [B, M], gt_counts int32 [B]: device
tensors padded to M = the dataset's largest object count (four times that with the mosaic on), ready for ops.build_labels / trainer.step / GraphedStep.step;
aug: host int32 [B, 3] = (dx, dy, flip) per image; bbox_per_batch / label_per_batch: host lists as the reference returns
them; batch_idx: the dataset indices of the batch; window / mode / color and split / parts / part_window / part_flip / part_color: as in Plan (None with the options off)."""

# the plan of one batch, all host side: dataset indices, per-image (dx, dy, flip), the reference's box / label lists.  With
# AUG_GEOMETRY "ssd" or AUG_COLOR also: window int64 [B, 4] = (x0, y0, cw, ch) in original-image pixels (aug[:, :2] is its corner),
# canvas int64 [B, 4] = the zoom-out canvas the window was drawn in, mode = per image "whole" | 0.1 .. 0.9 | "any" | "drift",
# trial int64 [B] = the 1-based trial that was accepted (0: none was made, or all failed and the window is the whole canvas),
# color float32 [B, 12] = the row-major 3x4 colour matrices, or None without AUG_COLOR.  With AUG_MOSAIC_PROB > 0 also (else None):
# split int64 [B, 2] = (xc, yc), parts int64 [B, 4] = the dataset index of every pane's image (-1: a pane that is not used),
# part_window int64 [B, 4, 4] = (x0, y0, cw, ch) per pane, part_flip int64 [B, 4], part_color float32 [B, 4, 12] or None; the fields
# above then describe part 0 (mode "mosaic" for a mosaic image), bbox_per_batch / label_per_batch hold the boxes of panes 0, 1, 2, 3
_PLAN_FIELDS = ["batch_idx", "aug", "bbox_per_batch", "label_per_batch", "window", "mode", "color", "canvas", "trial"]
MOSAIC_FIELDS = ["split", "parts", "part_window", "part_flip", "part_color"]


class Plan(namedtuple("Plan", _PLAN_FIELDS, defaults=(None, None, None, None, None))):
    """The plan with the mosaic off: the nine-field tuple it has always been; the mosaic's fields read None."""
    __slots__ = ()
    split = parts = part_window = part_flip = part_color = None


# the plan with the mosaic on: Plan's fields, then the mosaic's
MosaicPlan = namedtuple("MosaicPlan", _PLAN_FIELDS + MOSAIC_FIELDS)

CROP_MODES = ("whole", 0.1, 0.3, 0.5, 0.7, 0.9, "any")
BT601_BGR = np.array([0.114, 0.587, 0.299])                      # luma weights of (b, g, r)
RGB_TO_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
YIQ_TO_RGB = np.linalg.inv(RGB_TO_YIQ)


def _cfg(mc, key, default):
    """A config written before these fields existed means "off"."""
    return mc.get(key, default) if hasattr(mc, "get") else getattr(mc, key, default)


def window_iou(win, boxes):
    """IoU of the window (x0, y0, cw, ch), as the box of its pixel centres [x0, x0 + cw - 1] x [y0, y0 + ch - 1], with each
    [cx, cy, w, h] box; float64 [n]."""
    x0, y0, cw, ch = [float(v) for v in win]
    wx1, wy1, wx2, wy2 = x0, y0, x0 + cw - 1.0, y0 + ch - 1.0
    bx1, by1 = boxes[:, 0] - boxes[:, 2] / 2.0, boxes[:, 1] - boxes[:, 3] / 2.0
    bx2, by2 = boxes[:, 0] + boxes[:, 2] / 2.0, boxes[:, 1] + boxes[:, 3] / 2.0
    iw = np.maximum(np.minimum(wx2, bx2) - np.maximum(wx1, bx1), 0.0)
    ih = np.maximum(np.minimum(wy2, by2) - np.maximum(wy1, by1), 0.0)
    inter = iw * ih
    union = (wx2 - wx1) * (wy2 - wy1) + (bx2 - bx1) * (by2 - by1) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def centres_inside(win, boxes):
    """[n] bool: the box centres on the window's pixels, x0 <= cx <= x0 + cw - 1 (and y alike)."""
    x0, y0, cw, ch = [float(v) for v in win]
    return (boxes[:, 0] >= x0) & (boxes[:, 0] <= x0 + cw - 1.0) & (boxes[:, 1] >= y0) & (boxes[:, 1] <= y0 + ch - 1.0)


def ssd_window(rs, mc, w, h, boxes, mode=None):
    """The "ssd" geometry of one w x h image with [n, 4] boxes (cx, cy, w, h in its pixels): (window, canvas, mode, trial), both
    rectangles as (x0, y0, width, height) in original-image pixels.  Draws from rs in this order:
      zoom-out, when AUG_ZOOM_OUT_MAX > 1: randint(2); if 1, the ratio r ~ U[1, max], the canvas int(r w) x int(r h), and the
        image's integer offset in it, randint(0, Wc - w + 1) then randint(0, Hc - h + 1);
      the mode, randint(7) into CROP_MODES (not drawn when `mode` is given);
      for a mode other than "whole", up to AUG_CROP_TRIALS trials: the width and the height as U[AUG_CROP_MIN_SCALE, 1] of the
        canvas, truncated to pixels; a trial whose aspect is outside AUG_CROP_ASPECT is dropped without a position; else
        randint(0, Wc - cw + 1), randint(0, Hc - ch + 1).  Accepted: at least one box centre inside and max IoU >= mode ("any":
        the centre only; no boxes: always).  When every trial fails the window is the whole canvas.
    The aspect of a trial is (cw / Wc) / (ch / Hc), RELATIVE to the canvas: the window is stretched to the fixed network input
    whatever its shape, so this is the factor by which the resize distorts the objects (KITTI's 3.3 : 1 images could hardly
    ever hold a window whose pixel aspect is below 2)."""
    w, h = int(w), int(h)
    cx0, cy0, Wc, Hc = 0, 0, w, h
    zoom = float(_cfg(mc, "AUG_ZOOM_OUT_MAX", 1.0))
    if zoom > 1.0 and rs.randint(2) > 0.5:
        r = rs.uniform(1.0, zoom)
        Wc, Hc = max(int(r * w), w), max(int(r * h), h)
        cx0 = -int(rs.randint(0, Wc - w + 1))
        cy0 = -int(rs.randint(0, Hc - h + 1))
    canvas = (cx0, cy0, Wc, Hc)
    if mode is None:
        mode = CROP_MODES[rs.randint(len(CROP_MODES))]
    if mode == "whole":
        return canvas, canvas, mode, 0
    lo = float(_cfg(mc, "AUG_CROP_MIN_SCALE", 0.3))
    a_lo, a_hi = [float(v) for v in _cfg(mc, "AUG_CROP_ASPECT", (0.5, 2.0))]
    # (centres_inside / window_iou, box by box in Python floats -- the same float64 operations: up to 50 trials per image on a
    # handful of boxes, where a NumPy call per operation costs more than the whole test)
    corners = [(float(b[0]), float(b[1]), float(b[0] - b[2] / 2.0), float(b[1] - b[3] / 2.0), float(b[0] + b[2] / 2.0),
                float(b[1] + b[3] / 2.0)) for b in boxes]
    for trial in range(1, int(_cfg(mc, "AUG_CROP_TRIALS", 50)) + 1):
        cw = max(1, int(rs.uniform(lo, 1.0) * Wc))
        ch = max(1, int(rs.uniform(lo, 1.0) * Hc))
        aspect = (cw / float(Wc)) / (ch / float(Hc))
        if aspect < a_lo or aspect > a_hi:
            continue
        win = (cx0 + int(rs.randint(0, Wc - cw + 1)), cy0 + int(rs.randint(0, Hc - ch + 1)), cw, ch)
        if not corners:
            return win, canvas, mode, trial
        wx1, wy1, wx2, wy2 = float(win[0]), float(win[1]), win[0] + cw - 1.0, win[1] + ch - 1.0
        if not any(wx1 <= c[0] <= wx2 and wy1 <= c[1] <= wy2 for c in corners):
            continue
        if mode == "any":
            return win, canvas, mode, trial
        best = 0.0
        for _, _, bx1, by1, bx2, by2 in corners:
            inter = max(min(wx2, bx2) - max(wx1, bx1), 0.0) * max(min(wy2, by2) - max(wy1, by1), 0.0)
            union = (wx2 - wx1) * (wy2 - wy1) + (bx2 - bx1) * (by2 - by1) - inter
            if union > 0:
                best = max(best, inter / union)
        if best >= mode:
            return win, canvas, mode, trial
    return canvas, canvas, mode, 0


def window_boxes(win, boxes):
    """The boxes ([n, 4] cx, cy, w, h) an image keeps under the window: (kept [n] bool, [k, 4] boxes in window coordinates) --
    those whose centre is inside, shifted by the window's corner, their corners clipped to [0, cw - 1] x [0, ch - 1]."""
    x0, y0, cw, ch = [float(v) for v in win]
    keep = centres_inside(win, boxes)
    b = boxes[keep]
    x1 = np.clip(b[:, 0] - b[:, 2] / 2.0 - x0, 0.0, cw - 1.0)
    x2 = np.clip(b[:, 0] + b[:, 2] / 2.0 - x0, 0.0, cw - 1.0)
    y1 = np.clip(b[:, 1] - b[:, 3] / 2.0 - y0, 0.0, ch - 1.0)
    y2 = np.clip(b[:, 1] + b[:, 3] / 2.0 - y0, 0.0, ch - 1.0)
    return keep, np.stack([(x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1], 1).reshape(-1, 4)


def color_matrix(brightness=None, contrast=None, saturation=None, hue_degrees=None):
    """The float64 3x4 matrix on (b, g, r, 1) of the given factors (None: not applied), composed in this fixed order:
    brightness (an offset), contrast (a gain on all of it), saturation (about the BT.601 luma), hue (a rotation of the I-Q plane
    of YIQ).  Nothing applied is the exact identity.  Diverges from SSD's photometric distortion on purpose: SSD clamps (and
    rounds to bytes) between its steps, converts to HSV for saturation and hue, and draws the order of contrast; here the steps
    are linear maps multiplied into ONE matrix with no intermediate clamp, and the kernel clamps once to [0, 255] at the end."""
    A = np.eye(4)
    if brightness is not None:
        T = np.eye(4)
        T[:3, 3] = float(brightness)
        A = T @ A
    if contrast is not None:
        T = np.eye(4)
        T[:3, :3] *= float(contrast)
        A = T @ A
    if saturation is not None:
        T = np.eye(4)
        T[:3, :3] = float(saturation) * np.eye(3) + (1.0 - float(saturation)) * np.tile(BT601_BGR, (3, 1))
        A = T @ A
    if hue_degrees is not None:
        t = np.deg2rad(float(hue_degrees))
        rot = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(t), -np.sin(t)], [0.0, np.sin(t), np.cos(t)]])
        rgb = YIQ_TO_RGB @ rot @ RGB_TO_YIQ
        T = np.eye(4)
        T[:3, :3] = rgb[::-1, ::-1]                                  # the same map on (b, g, r)
        A = T @ A
    return A[:3]


def draw_color_factors(rs, mc):
    """(brightness, contrast, saturation, hue_degrees), each None with probability 1/2: per factor randint(2), then, if 1, its
    value U[range] -- in color_matrix's order."""
    out = []
    b = float(_cfg(mc, "AUG_BRIGHTNESS", 32.0))
    hd = float(_cfg(mc, "AUG_HUE_DEGREES", 18.0))
    for lo, hi in ((-b, b), _cfg(mc, "AUG_CONTRAST", (0.5, 1.5)), _cfg(mc, "AUG_SATURATION", (0.5, 1.5)), (-hd, hd)):
        out.append(rs.uniform(float(lo), float(hi)) if rs.randint(2) > 0.5 else None)
    return tuple(out)


def draw_color_matrix(rs, mc):
    """One image's colour matrix, float32 [12] (row-major 3x4): composed in float64, rounded once."""
    return color_matrix(*draw_color_factors(rs, mc)).astype(np.float32).reshape(12)


def mosaic_panes(xc, yc, W, H):
    """The four panes of a W x H input cut at (xc, yc), as (px0, py0, pw, ph): top left, top right, bottom left, bottom right."""
    return [(0, 0, xc, yc), (xc, 0, W - xc, yc), (0, yc, xc, H - yc), (xc, yc, W - xc, H - yc)]


def mosaic_part(rs, mc, w, h, pw, ph):
    """One part of a mosaic: the window of a w x h image that fills a pw x ph pane, as ((x0, y0, cw, ch), flip, colour matrix or
    None).  Draws from rs in this order:
      the zoom z = max(pw / w, ph / h) * U[1, AUG_MOSAIC_ZOOM_MAX] -- at U = 1 the largest window of the pane's shape that the
        image holds --, the window cw = min(w, max(1, int(pw / z))), ch = min(h, max(1, int(ph / z)));
      its corner, randint(0, w - cw + 1) then randint(0, h - ch + 1);
      the mirror, randint(2);
      with AUG_COLOR, draw_color_matrix.
    The window is always a crop inside its image, shown at the isotropic zoom z up to the truncation to pixels: no padding and no
    trial loop."""
    w, h, pw, ph = int(w), int(h), int(pw), int(ph)
    z = max(pw / float(w), ph / float(h)) * rs.uniform(1.0, float(_cfg(mc, "AUG_MOSAIC_ZOOM_MAX", 1.5)))
    cw, ch = min(w, max(1, int(pw / z))), min(h, max(1, int(ph / z)))
    x0 = int(rs.randint(0, w - cw + 1))
    y0 = int(rs.randint(0, h - ch + 1))
    flip = 1 if rs.randint(2) > 0.5 else 0
    color = draw_color_matrix(rs, mc) if _cfg(mc, "AUG_COLOR", False) else None
    return (x0, y0, cw, ch), flip, color


def mosaic_part_boxes(win, flip, pane, boxes, min_box):
    """The boxes ([n, 4] cx, cy, w, h in the part's original pixels) in network-input pixels, for the window `win` shown in
    pane = (px0, py0, pw, ph): (kept [n] bool, [k, 4]).  In this order: window_boxes (centre inside, shifted, clipped), the mirror
    cw - 1 - cx, the scaling by pw / cw and ph / ch, the filter -- a box narrower or lower than min_box is dropped --, the pane's
    origin added to the centre."""
    px0, py0, pw, ph = [float(v) for v in pane]
    cw, ch = float(win[2]), float(win[3])
    keep, b = window_boxes(win, boxes)
    if flip:
        b[:, 0] = cw - 1 - b[:, 0]
    b[:, 0::2] = b[:, 0::2] * (pw / cw)
    b[:, 1::2] = b[:, 1::2] * (ph / ch)
    big = (b[:, 2] >= float(min_box)) & (b[:, 3] >= float(min_box))
    keep[np.flatnonzero(keep)[~big]] = False
    b = b[big]
    b[:, 0] = b[:, 0] + px0
    b[:, 1] = b[:, 1] + py0
    return keep, b


def _mosaic_part_rows(win, flip, pane, roi, min_box):
    """mosaic_part_boxes on a roi list ([cx, cy, w, h, cls] rows), box by box in Python floats: ([[cx, cy, w, h]], [cls]) of the
    boxes kept.  The same float64 operations in the same order -- np.clip is min(max(v, lo), hi) -- so the rows are
    mosaic_part_boxes' bit for bit (tests/test_mosaic_host.py compares them); a part has a handful of boxes, where a NumPy call per
    operation costs ten times the arithmetic, as in ssd_window."""
    x0, y0, cw, ch = [float(v) for v in win]
    px0, py0, pw, ph = [float(v) for v in pane]
    sx, sy, min_box = pw / cw, ph / ch, float(min_box)
    rows, labels = [], []
    for b in roi:
        cx, cy, w, h = float(b[0]), float(b[1]), float(b[2]), float(b[3])
        if not (x0 <= cx <= x0 + cw - 1.0 and y0 <= cy <= y0 + ch - 1.0):
            continue
        x1, x2 = min(max(cx - w / 2.0 - x0, 0.0), cw - 1.0), min(max(cx + w / 2.0 - x0, 0.0), cw - 1.0)
        y1, y2 = min(max(cy - h / 2.0 - y0, 0.0), ch - 1.0), min(max(cy + h / 2.0 - y0, 0.0), ch - 1.0)
        cx, cy, w, h = (x1 + x2) / 2.0, (y1 + y2) / 2.0, x2 - x1, y2 - y1
        if flip:
            cx = cw - 1 - cx
        cx, w, cy, h = cx * sx, w * sx, cy * sy, h * sy
        if w >= min_box and h >= min_box:
            rows.append([cx + px0, cy + py0, w, h])
            labels.append(b[4])
    return rows, labels


def mosaic_prob(mc):
    """mc.AUG_MOSAIC_PROB where it applies: 0.0 without DATA_AUGMENTATION or for a config without the field."""
    p = float(_cfg(mc, "AUG_MOSAIC_PROB", 0.0)) if mc.DATA_AUGMENTATION else 0.0
    if not 0.0 <= p <= 1.0:
        raise ValueError("BatchReader: mc.AUG_MOSAIC_PROB must be in [0, 1], got %r" % (p,))
    return p


def reference_drift(rs, mc, boxes):
    """The reference's drift (imdb.py:150-166) of an image with [n, 4] boxes (cx, cy, w, h in its pixels): (dx, dy), each in
    [-DRIFT, DRIFT] and so small that no box is cut at the left or the top -- the bound is min(cx - w / 2 + 1) as a float, which
    randint truncates.  Draws from rs dy BEFORE dx, one randint each; nothing with DRIFT_X = DRIFT_Y = 0.  Diverges from the
    reference on purpose: an image with no boxes draws from the full range, where the reference crashes."""
    assert mc.DRIFT_X >= 0 and mc.DRIFT_Y > 0, 'mc.DRIFT_X and mc.DRIFT_Y must be >= 0'
    if not (mc.DRIFT_X > 0 or mc.DRIFT_Y > 0):
        return 0, 0
    max_drift_x, max_drift_y = mc.DRIFT_X + 1, mc.DRIFT_Y + 1
    if len(boxes):
        max_drift_x = min(boxes[:, 0] - boxes[:, 2] / 2.0 + 1)
        max_drift_y = min(boxes[:, 1] - boxes[:, 3] / 2.0 + 1)
        assert max_drift_x >= 0 and max_drift_y >= 0, 'bbox out of image'
    dy = rs.randint(-mc.DRIFT_Y, min(mc.DRIFT_Y + 1, max_drift_y))
    dx = rs.randint(-mc.DRIFT_X, min(mc.DRIFT_X + 1, max_drift_x))
    return dx, dy


# one batch image of a plan, as a mosaic -- a single image is part 0 of a mosaic with one pane, split (IMAGE_WIDTH, IMAGE_HEIGHT):
# aug = (dx, dy, flip), the boxes in network-input pixels, the labels, window, mode, color, canvas, trial, and split, parts,
# part_window, part_flip, part_color with four entries each.  The fields are MosaicPlan's after batch_idx, one row of each; a
# plan's columns are lists or arrays of these types (float32: None without AUG_COLOR).
_ImagePlan = namedtuple("_ImagePlan", MosaicPlan._fields[1:])
_PLAN_COLUMNS = (np.int32, list, list, np.int64, list, np.float32, np.int64, np.int64) + (np.int64,) * 4 + (np.float32,)
_NO_COLOR = np.zeros(12, np.float32)
_NO_COLOR.setflags(write=False)
_NO_PART = (-1, (0, 0, 0, 0), 0, _NO_COLOR)         # a pane without pixels: (source, window, flip, colour matrix)


class BatchReader:
    """``BatchReader(mc, images, rois, seed=0, device=None, dtype=torch.float32, resident=False)``

    images: list of uint8 [H, W, 3] BGR arrays (as cv2.imread delivers; any sizes).  rois: per image a list of
    [cx, cy, w, h, cls] in original pixels (kitti._rois, dataset/kitti.py:50-90).  resident=True uploads every image
    once and gathers each batch on the device by byte offset; otherwise each batch is packed into a pinned host buffer
    and copied asynchronously on the current stream.  mc supplies BATCH_SIZE, IMAGE_WIDTH / IMAGE_HEIGHT, BGR_MEANS and
    DATA_AUGMENTATION / DRIFT_X / DRIFT_Y and, optional, AUG_GEOMETRY / AUG_ZOOM_OUT_MAX / AUG_COLOR with their ranges and
    AUG_MOSAIC_PROB / _CENTER / _ZOOM_MAX / _MIN_BOX (config.base_model_config).  With the mosaic on, max_objects -- the M of every
    Batch -- is FOUR times the dataset's largest object count: the three further images of a mosaic are drawn independently, so one
    image can fill all four panes, and the sum of the four largest counts would not bound that.  The first shuffle is drawn here, as kitti.__init__ does."""

    def __init__(self, mc, images, rois, seed=0, device=None, dtype=None, resident=False):
        if len(images) != len(rois) or not images:
            raise ValueError("BatchReader: %d images for %d roi lists" % (len(images), len(rois)))
        self.mc = mc
        self.images = []
        for k, im in enumerate(images):
            im = np.ascontiguousarray(im)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("BatchReader: image %d must be uint8 [H, W, 3], got %s %s" % (k, im.dtype, im.shape))
            self.images.append(im)
        self.rois = [[list(b) for b in r] for r in rois]
        self.sizes = np.array([im.shape[:2] for im in self.images], np.int64)
        self.nbytes = self.sizes[:, 0] * self.sizes[:, 1] * 3
        self.max_objects = max(1, max(len(r) for r in self.rois))
        self.parts_per_image = 1
        if mosaic_prob(mc) > 0.0:
            self.parts_per_image = 4
            self.max_objects *= 4
            anchor_box = _cfg(mc, "ANCHOR_BOX", None)
            limit = 1024 if anchor_box is None else min(1024, len(anchor_box))      # what sqdet_build_labels accepts
            if self.max_objects > limit:
                raise ValueError("BatchReader: a mosaic can hold %d objects, ops.build_labels takes at most %d per image"
                                 % (self.max_objects, limit))
        self.rs = np.random.RandomState(seed)
        self.device, self.dtype, self.resident = device, dtype, bool(resident)
        self._image_idx = list(range(len(self.images)))
        self._perm_idx, self._cur_idx = None, 0
        self._shuffle_image_idx()
        self._src = None          # resident: the whole dataset on the device; packed: the device staging buffer
        self._pinned, self._copied = None, None

    # ------------------------------------------------------------------------------------------------------ host half --
    def _shuffle_image_idx(self):
        self._perm_idx = [self._image_idx[i] for i in self.rs.permutation(np.arange(len(self._image_idx)))]
        self._cur_idx = 0

    def _next_indices(self, shuffle):
        """imdb.py:109-128 (and 70-83), quirks included."""
        B, n = self.mc.BATCH_SIZE, len(self._image_idx)
        if shuffle:
            if self._cur_idx + B >= n:
                self._shuffle_image_idx()
            batch_idx = self._perm_idx[self._cur_idx:self._cur_idx + B]
            self._cur_idx += B
        else:
            if self._cur_idx + B >= n:
                batch_idx = self._image_idx[self._cur_idx:] + self._image_idx[:self._cur_idx + B - n]
                self._cur_idx += B - n
            else:
                batch_idx = self._image_idx[self._cur_idx:self._cur_idx + B]
                self._cur_idx += B
        return batch_idx

    # ---------------------------------------------------------------------------------------------- resumable state --
    def state_dict(self):
        """Where the reader stands: the generator's state, the current permutation and its cursor, and the dataset length
        (checked on load).  A reader built the same way that loads it serves the same batches from here on."""
        kind, keys, pos, has_gauss, cached = self.rs.get_state()
        return dict(rs_kind=str(kind), rs_keys=np.asarray(keys, np.uint32).copy(), rs_pos=int(pos), rs_has_gauss=int(has_gauss),
                    rs_cached_gaussian=float(cached), perm_idx=np.asarray(self._perm_idx, np.int64).copy(),
                    cur_idx=int(self._cur_idx), num_images=len(self._image_idx))

    def load_state_dict(self, d):
        if int(d["num_images"]) != len(self._image_idx):
            raise ValueError("BatchReader: state of a dataset of %d images, this one has %d" % (int(d["num_images"]), len(self._image_idx)))
        perm = [int(v) for v in np.asarray(d["perm_idx"]).reshape(-1)]
        if sorted(perm) != list(range(len(self._image_idx))) or not 0 <= int(d["cur_idx"]) <= len(perm) + self.mc.BATCH_SIZE:
            raise ValueError("BatchReader: the saved permutation or cursor does not fit this dataset")
        self.rs.set_state((str(d["rs_kind"]), np.asarray(d["rs_keys"], np.uint32), int(d["rs_pos"]), int(d["rs_has_gauss"]),
                           float(d["rs_cached_gaussian"])))
        self._perm_idx, self._cur_idx = perm, int(d["cur_idx"])

    def next_plan(self, shuffle=True):
        """The host half of read_batch: batch order, random draws and box transform (imdb.py:100-190), in NumPy float64 in
        the reference's order.  Advances the reader; needs no GPU.

        Four steps: the flags are validated, the indices taken, every image becomes one _ImagePlan -- _single_image under the "drift"
        or "ssd" policy, _mosaic_image as a mosaic --, and the records' columns become the plan's arrays.

        With AUG_MOSAIC_PROB > 0 every batch image first draws a coin, random_sample() < AUG_MOSAIC_PROB.  If it fails, the image's
        own policy runs unchanged (_single_image) and is part 0 of a mosaic with split = (IMAGE_WIDTH, IMAGE_HEIGHT), a drift as its
        window.  If it succeeds, the draws are (_mosaic_image), in this order: xc = int(U[AUG_MOSAIC_CENTER] * IMAGE_WIDTH), then yc alike with
        IMAGE_HEIGHT; three further dataset indices, randint(len(images)) each, independent of the epoch's permutation (part 0 is the
        batch image itself); then per pane 0..3 that has pixels the draws of mosaic_part.  The image's boxes and labels are those of
        pane 0, then 1, 2 and 3 (mosaic_part_boxes): ops.build_labels lets earlier boxes claim their anchors first."""
        mc = self.mc
        prob = mosaic_prob(mc)
        if (prob > 0.0) != (self.parts_per_image == 4):
            raise ValueError("BatchReader: mc.AUG_MOSAIC_PROB was switched %s after the reader was built" % ("on" if prob > 0.0 else "off"))
        geometry = _cfg(mc, "AUG_GEOMETRY", "drift")
        if geometry not in ("drift", "ssd"):
            raise ValueError("BatchReader: mc.AUG_GEOMETRY must be 'drift' or 'ssd', got %r" % (geometry,))
        augment = bool(mc.DATA_AUGMENTATION)
        ssd, jitter = augment and geometry == "ssd", augment and bool(_cfg(mc, "AUG_COLOR", False))
        batch_idx = self._next_indices(shuffle)
        rows = [self._mosaic_image(idx) if prob > 0.0 and self.rs.random_sample() < prob else self._single_image(idx, augment, ssd, jitter)
                for idx in batch_idx]
        # the reference's four fields, nine with "ssd" or colour, all fourteen with the mosaic: only those columns are made
        n = 14 if prob > 0.0 else 9 if ssd or jitter else 4
        columns = [list(c) if kind is list else np.array(c, kind) if jitter or kind is not np.float32 else None
                   for c, kind in zip(zip(*rows), _PLAN_COLUMNS[:n - 1])]
        return (MosaicPlan if n == 14 else Plan)(batch_idx, *columns)

    def _image_plan(self, bbox, label, mode, trial, canvas, split, panes):
        """The record of one batch image from its four panes, each (source index, window, flip, colour matrix) or _NO_PART: the
        single-image fields describe the first pane that has pixels -- part 0, unless AUG_MOSAIC_CENTER left it none --, and the canvas,
        where no zoom-out drew one (None), is that part's whole image."""
        source, win, flip, color = next(p for p in panes if p[0] >= 0)
        if canvas is None:
            canvas = (0, 0, self.images[source].shape[1], self.images[source].shape[0])
        return _ImagePlan((win[0], win[1], flip), bbox, label, win, mode, color, canvas, trial, split, *zip(*panes))

    def _single_image(self, idx, augment, ssd, jitter):
        """One image under the "drift" or the "ssd" policy (imdb.py:141-190): its geometry's draws (reference_drift / ssd_window), the
        mirror, randint(2), and with AUG_COLOR draw_color_matrix; nothing is drawn without DATA_AUGMENTATION.  The drift (dx, dy) is the
        window (dx, dy, w - dx, h - dy); the image is the only pane of a mosaic split at (IMAGE_WIDTH, IMAGE_HEIGHT)."""
        mc, rs = self.mc, self.rs
        h, w = self.images[idx].shape[:2]
        roi = self.rois[idx]
        label = [b[4] for b in roi]
        gt_bbox = np.array([[b[0], b[1], b[2], b[3]] for b in roi]) if roi else np.zeros((0, 4))
        win, canvas, mode, trial, flip = (0, 0, w, h), None, "drift", 0, 0
        if ssd:
            win, canvas, mode, trial = ssd_window(rs, mc, w, h, gt_bbox)
            keep, gt_bbox = window_boxes(win, gt_bbox)
            label = [c for c, kept in zip(label, keep) if kept]
        elif augment:
            dx, dy = reference_drift(rs, mc, gt_bbox)
            gt_bbox[:, 0] = gt_bbox[:, 0] - dx
            gt_bbox[:, 1] = gt_bbox[:, 1] - dy
            win = (dx, dy, w - dx, h - dy)
        if augment and rs.randint(2) > 0.5:
            flip = 1
            gt_bbox[:, 0] = float(win[2]) - 1 - gt_bbox[:, 0]
        gt_bbox[:, 0::2] = gt_bbox[:, 0::2] * (mc.IMAGE_WIDTH / float(win[2]))
        gt_bbox[:, 1::2] = gt_bbox[:, 1::2] * (mc.IMAGE_HEIGHT / float(win[3]))
        color = draw_color_matrix(rs, mc) if jitter else _NO_COLOR
        return self._image_plan(gt_bbox, label, mode, trial, canvas, (int(mc.IMAGE_WIDTH), int(mc.IMAGE_HEIGHT)),
                                ((idx, win, flip, color), _NO_PART, _NO_PART, _NO_PART))

    def _mosaic_image(self, idx):
        """One mosaic of image idx and three more (next_plan states the draws): every pane that has pixels shows a mosaic_part of its
        image, and the boxes are those of pane 0, then 1, 2 and 3."""
        mc, rs = self.mc, self.rs
        W, H = int(mc.IMAGE_WIDTH), int(mc.IMAGE_HEIGHT)
        lo, hi = [float(v) for v in _cfg(mc, "AUG_MOSAIC_CENTER", (0.3, 0.7))]
        xc = min(max(int(rs.uniform(lo, hi) * W), 0), W)
        yc = min(max(int(rs.uniform(lo, hi) * H), 0), H)
        sources = [idx] + [int(rs.randint(len(self.images))) for _ in range(3)]
        min_box = _cfg(mc, "AUG_MOSAIC_MIN_BOX", 2.0)
        boxes, labels, panes = [], [], []
        for source, pane in zip(sources, mosaic_panes(xc, yc, W, H)):
            if pane[2] <= 0 or pane[3] <= 0:
                panes.append(_NO_PART)
                continue
            sh, sw = self.images[source].shape[:2]
            win, flip, M = mosaic_part(rs, mc, sw, sh, pane[2], pane[3])
            panes.append((source, win, flip, _NO_COLOR if M is None else M))
            rows, kept = _mosaic_part_rows(win, flip, pane, self.rois[source], min_box)     # = mosaic_part_boxes
            boxes += rows
            labels += kept
        return self._image_plan(np.array(boxes, np.float64).reshape(-1, 4), labels, "mosaic", 0, None, (xc, yc), panes)

    # ---------------------------------------------------------------------------------------------------- device half --
    def _torch(self):
        import torch
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(self.device)
        if self.dtype is None:
            self.dtype = torch.float32
        return torch

    def _source(self, batch_idx):
        """(flat device uint8 buffer, byte offset of each batch image in it).  With the mosaic on batch_idx lists up to four images
        per batch image, and the packed mode's buffers hold 4 * BATCH_SIZE of the largest images; an image that is listed twice is
        packed twice."""
        torch = self._torch()
        if self.resident:
            if self._src is None:
                self._offsets = np.concatenate([[0], np.cumsum(self.nbytes)[:-1]]).astype(np.int64)
                self._src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in self.images])).to(self.device)
            return self._src, self._offsets[batch_idx]
        nb = self.nbytes[batch_idx]
        offsets = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int64)
        total = int(nb.sum())
        if self._pinned is None or self._pinned.numel() < total:
            cap = int(np.sort(self.nbytes)[::-1][:max(1, self.mc.BATCH_SIZE)].sum()) * self.parts_per_image   # the largest possible batch
            cap = max(cap, total)
            self._pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self._src = torch.empty(cap, dtype=torch.uint8, device=self.device)
            self._copied = None
        if self._copied is not None:
            self._copied.synchronize()          # the previous batch's copy out of the pinned buffer has finished
        host = self._pinned.numpy()
        for o, i in zip(offsets, batch_idx):
            host[o:o + self.nbytes[i]] = self.images[i].reshape(-1)
        self._src[:total].copy_(self._pinned[:total], non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        return self._src[:total], offsets

    def _warp(self, p):
        """The plan's images in ONE launch; its shape chooses the entry point: split -> the mosaic, window -> the window form, else the
        drift with the reference's five-column geometry."""
        from . import ops
        mc = self.mc
        dst = (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, self.dtype)
        if p.split is not None:
            used = p.parts >= 0
            src, offsets = self._source(p.parts[used])
            part_offsets = np.zeros(p.parts.shape, np.int64)
            part_offsets[used] = offsets
            geom = np.zeros(p.parts.shape + (7,), np.int64)              # src_h, src_w, x0, y0, cw, ch, flip
            geom[used] = np.concatenate([self.sizes[p.parts[used]], p.part_window[used], p.part_flip[used][:, None]], axis=1)
            return ops.augment_bgr_mosaic(src, part_offsets, geom, p.split, p.part_color, *dst)
        src, offsets = self._source(p.batch_idx)
        sizes, aug = self.sizes[p.batch_idx], p.aug.astype(np.int64)
        if p.window is not None:
            return ops.augment_bgr_window(src, offsets, np.concatenate([sizes, p.window, aug[:, 2:3]], axis=1), p.color, *dst)
        return ops.augment_bgr(src, offsets, np.concatenate([sizes, aug], axis=1), *dst)     # src_h, src_w, dx, dy, flip

    def read_batch(self, shuffle=True):
        """imdb.read_batch (imdb.py:100-190): the next batch as a Batch, image_input and ground truth on the device."""
        torch = self._torch()
        p = self.next_plan(shuffle)
        image_input = self._warp(p)
        B, M = len(p.batch_idx), self.max_objects
        gt = np.zeros((B, M, 4), np.float64)
        cls = np.zeros((B, M), np.int32)
        cnt = np.zeros(B, np.int32)
        for k, (bb, lab) in enumerate(zip(p.bbox_per_batch, p.label_per_batch)):
            cnt[k] = len(lab)
            gt[k, :len(lab)] = bb
            cls[k, :len(lab)] = lab
        to = lambda a: torch.from_numpy(a).to(self.device, non_blocking=True)
        return Batch(image_input, to(gt), to(cls), to(cnt), *[getattr(p, f) for f in Batch._fields[4:]])

    def read_image_batch(self, shuffle=True):
        """imdb.read_image_batch (imdb.py:63-98): the next batch's images only -- mean-subtracted, then resized, with no drift
        and no flip -- as (image_input on the device, [(x_scale, y_scale)] per image).  Draws nothing but the reshuffles."""
        self._torch()
        batch_idx = self._next_indices(shuffle)
        scales = []
        for idx in batch_idx:
            orig_h, orig_w = [float(v) for v in self.sizes[idx]]
            scales.append((self.mc.IMAGE_WIDTH / orig_w, self.mc.IMAGE_HEIGHT / orig_h))
        return self._warp(Plan(batch_idx, np.zeros((len(batch_idx), 3), np.int32), None, None)), scales
