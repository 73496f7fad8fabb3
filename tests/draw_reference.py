"""NumPy restatement of the drawing contract of include/sqdet.h ("drawing"), for the tests of squeezedet_amd.viz.  It SCATTERS --
item after item, each writing its own pixels, the way cv2.rectangle / putText calls follow each other in the reference's
_draw_box -- where the kernel gathers per pixel, so the two share no structure.  An item is the tuple viz.pack_items takes and
DrawItems.decode() returns: (x0, y0, x1, y1, (b, g, r), label bytes, "bottom_left" | "top_left")."""
import numpy as np

COORD_LIM = 1 << 30
LABEL_MAX = 31


def restore(x, bgr_means):
    """The network input (float16 / float32, mean-subtracted BGR) back to uint8: rint(float32(x) + float32(mean)), half to
    even, clamped to [0, 255]."""
    m = np.asarray(bgr_means, np.float32).reshape(3)
    v = np.rint(np.asarray(x).astype(np.float32) + m)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)


def draw_item(img, item, font):
    """Draws one item into img (uint8 [H, W, 3] BGR, in place): the one-pixel outline cv2.rectangle(.., 1) paints, then the
    label, both clipped."""
    H, W = img.shape[:2]
    x0, y0, x1, y1 = (int(np.clip(v, -COORD_LIM, COORD_LIM)) for v in item[:4])
    colour, label, anchor = np.asarray(item[4], np.uint8), bytes(item[5])[:LABEL_MAX], item[6]
    xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    cx0, cx1, cy0, cy1 = max(xa, 0), min(xb, W - 1), max(ya, 0), min(yb, H - 1)        # the clipped spans
    if cx0 <= cx1:
        for y in (y0, y1):
            if 0 <= y < H:
                img[y, cx0:cx1 + 1] = colour
    if cy0 <= cy1:
        for x in (x0, x1):
            if 0 <= x < W:
                img[cy0:cy1 + 1, x] = colour
    lx, ly = x0, (y0 if anchor == "top_left" else y1 - 7)
    for k, ch in enumerate(label):
        glyph = font[ch - 32] if 32 <= ch <= 126 else font[ord("?") - 32]
        for gy in range(7):
            y = ly + gy
            if not 0 <= y < H:
                continue
            for gx in range(5):
                x = lx + 6 * k + 1 + gx
                if 0 <= x < W and (int(glyph[gy]) >> (4 - gx)) & 1:
                    img[y, x] = colour


def draw(images_bgr, tables, font, order="rgb"):
    """images_bgr uint8 [B, H, W, 3]; tables: a list of per-image item lists (each [B][...]), drawn table after table, row
    after row -> uint8 [B, H, W, 3] in `order`."""
    out = np.array(images_bgr, np.uint8, copy=True)
    for i in range(out.shape[0]):
        for t in tables:
            for item in t[i]:
                draw_item(out[i], item, font)
    return out[..., ::-1].copy() if order == "rgb" else out


def box_item(box, colour, label, anchor="bottom_left", form="center"):
    """_draw_box's integers for one box: int() of bbox_transform(box) in the box's own precision (box: a NumPy row)."""
    if form == "center":
        cx, cy, w, h = box
        box = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]
    x0, y0, x1, y1 = (0 if np.isnan(b) else int(np.clip(b, -COORD_LIM, COORD_LIM)) for b in box)
    return (x0, y0, x1, y1, tuple(colour), label.encode("latin-1")[:LABEL_MAX] if isinstance(label, str) else label, anchor)
