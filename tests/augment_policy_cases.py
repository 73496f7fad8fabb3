"""Inputs and the NumPy restatement for sqdet_augment_bgr_window (squeezedet_amd/csrc/augment.hip; test infrastructure, no GPU).
Shared by tests/test_augment_policy_host.py, which shows on the restatement alone that the cases discriminate the mistakes a
window / colour kernel can make, and by tests/test_gpu_augment_window.py.

window_restatement is include/sqdet.h's definition in float32 NumPy, on the conventions of input_path_cases.augment_restatement
(oracle.preproc_oracle._coords for the taps, the blend h0 = a * (1 - fx) + b * fx, out = h0 * (1 - fy) + h1 * fy): colour on the
source bytes -> clamp -> mean -> window with 0.0f padding -> flip -> resize.  `mutate` names one of five wrong variants.

Cases: three sources ((37, 53), (61, 201), (9, 7), stored once each, in this order, so that the buffer ends with an odd-sized image
whose last pixel pair is read) x WINDOWS(h, w) x both flips = 60 images of ONE launch, every image addressing its source by byte
offset; into input_path_cases.AUG_DSTS at AUG_BASE_OFFSETS; under COLORS."""
import functools

import numpy as np

from oracle import preproc_oracle as PO
from tests import input_path_cases as IC

MEANS = IC.MEANS
SOURCES = [(37, 53), (61, 201), (9, 7)]
MUTATIONS = ["color_after_interpolation", "offset_on_padding", "no_clamp", "image_border_taps", "flip_before_window"]


def windows(h, w):
    """name -> (x0, y0, cw, ch) for an h x w source."""
    inside = (1, 2, w - 3, h - 4) if w < 16 else (w // 4, h // 4, w // 2, h // 3)
    return {"inside": inside, "containing": (-5, -3, w + 9, h + 8),
            "left": (-4, 1, w // 2 + 4, h - 2), "right": (w // 2, 1, w // 2 + 6, h - 2),
            "top": (1, -3, w - 2, h // 2 + 3), "bottom": (1, h // 2, w - 2, h // 2 + 5),
            "1x1": (w // 2, h // 2, 1, 1), "cw=1": (w // 2, 0, 1, h), "ch=1": (0, h // 2, w, 1), "outside": (w + 2, -1, 5, 4)}


# (index of the source, window name, window, flip)
WIN_IMAGES = [(si, name, win, fl) for si, (h, w) in enumerate(SOURCES) for name, win in windows(h, w).items() for fl in (0, 1)]

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
SATURATE = np.array([[3, 0, 0, -300], [0, 3, 0, -300], [0, 0, 3, -300]], np.float32)      # bytes < 100 -> 0, > 185 -> 255
CROSS = np.array([[0.5, -0.25, 0.75, 10.5], [-0.3, 1.2, 0.1, -7.25], [0.2, 0.3, -0.6, 64.0]], np.float32)
COLORS = ["null", "identity", "saturate", "cross", "mixed"]       # mixed: image k takes (identity, saturate, cross)[k % 3]


def color_of(name):
    """[n, 3, 4] float32 for the WIN_IMAGES batch, or None."""
    n = len(WIN_IMAGES)
    if name == "null":
        return None
    if name == "mixed":
        return np.stack([(IDENTITY, SATURATE, CROSS)[k % 3] for k in range(n)])
    return np.tile({"identity": IDENTITY, "saturate": SATURATE, "cross": CROSS}[name], (n, 1, 1))


@functools.lru_cache(maxsize=None)
def win_source():
    """(the three images, flat uint8 buffer, byte offset of every WIN_IMAGES row)."""
    rs = np.random.RandomState(43)
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in SOURCES]
    starts = np.concatenate([[0], np.cumsum([im.size for im in images])[:-1]]).astype(np.int64)
    flat = np.concatenate([im.reshape(-1) for im in images])
    flat.setflags(write=False)
    return images, flat, starts[[si for si, _, _, _ in WIN_IMAGES]]


def win_geom():
    """[n, 7] = (src_h, src_w, x0, y0, cw, ch, flip)."""
    return np.array([list(SOURCES[si]) + list(win) + [fl] for si, _, win, fl in WIN_IMAGES])


def apply_color(a, M, clamp=True):
    """float32 [..., 3] (b, g, r) -> ((M[k][0] b + M[k][1] g) + M[k][2] r) + M[k][3], clamped to [0, 255]; float32 throughout."""
    a, M = a.astype(np.float32), np.asarray(M, np.float32).reshape(3, 4)
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    c = np.stack([((M[k, 0] * b + M[k, 1] * g) + M[k, 2] * r) + M[k, 3] for k in range(3)], -1)
    assert c.dtype == np.float32
    return np.minimum(np.maximum(c, np.float32(0)), np.float32(255)) if clamp else c


def sub_mean(c):
    return (c.astype(np.float64) - MEANS).astype(np.float32)


def take_window(v, win, fill=0.0):
    """D[i, j] = v[i + y0, j + x0] inside v, `fill` outside; D is ch x cw."""
    x0, y0, cw, ch = win
    h, w = v.shape[:2]
    d = np.empty((ch, cw) + v.shape[2:], np.float32)
    d[...] = fill
    iy0, iy1, ix0, ix1 = max(y0, 0), min(y0 + ch, h), max(x0, 0), min(x0 + cw, w)
    if iy1 > iy0 and ix1 > ix0:
        d[iy0 - y0:iy1 - y0, ix0 - x0:ix1 - x0] = v[iy0:iy1, ix0:ix1]
    return d


def _blend(d, sy, sy1, fy, sx, sx1, fx):
    ax0, fxb = (np.float32(1) - fx)[None, :, None], fx[None, :, None]
    h0 = d[sy][:, sx] * ax0 + d[sy][:, sx1] * fxb
    h1 = d[sy1][:, sx] * ax0 + d[sy1][:, sx1] * fxb
    return (h0 * (np.float32(1) - fy)[:, None, None] + h1 * fy[:, None, None]).astype(np.float32)


def _resize(d, hd, wd):
    return _blend(d, *PO._coords(hd, d.shape[0]), *PO._coords(wd, d.shape[1]))


def _loose_coords(n_dst, n_src):
    """_coords without the clamp at the window's border: taps in [-1, n_src], for a window taken one pixel larger all round."""
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / float(n_dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s + 1, s + 2, (f - s.astype(np.float32)).astype(np.float32)


def window_restatement(im_u8, win, flip, M, hd, wd, mutate=None):
    """One image: uint8 [h, w, 3], win = (x0, y0, cw, ch), M = 3x4 float32 or None -> float32 [hd, wd, 3].  mutate (MUTATIONS):
    color_after_interpolation -- the window, flip and resize run on the raw bytes, the matrix, clamp and mean on the result (0
      where only padding was blended);
    offset_on_padding -- the matrix runs on the byte image padded with 0, so padding becomes clamp(M[k][3]);
    no_clamp -- the clamp to [0, 255] is dropped;
    image_border_taps -- the bilinear taps are not clamped to the window: a crop blends in the image pixels around it;
    flip_before_window -- the IMAGE is mirrored, then the window is taken."""
    assert mutate is None or mutate in MUTATIONS
    x0, y0, cw, ch = win
    raw = im_u8.astype(np.float32)
    inside = take_window(np.ones(im_u8.shape[:2] + (1,), np.float32), win) > 0
    if mutate == "color_after_interpolation":
        d, m = take_window(raw, win), inside.astype(np.float32)
        if flip:
            d, m = d[:, ::-1], m[:, ::-1]
        out = _resize(d, hd, wd)
        out = sub_mean(out if M is None else apply_color(out, M))
        return np.where(_resize(m, hd, wd) > 0, out, np.float32(0)).astype(np.float32)
    c = raw if M is None else apply_color(raw, M, clamp=mutate != "no_clamp")
    v = sub_mean(c)
    if mutate == "flip_before_window":
        return _resize(take_window(v[:, ::-1] if flip else v, win), hd, wd)
    if mutate == "image_border_taps":
        d = take_window(v, (x0 - 1, y0 - 1, cw + 2, ch + 2))
        if flip:
            d = d[:, ::-1]
        return _blend(d, *_loose_coords(hd, ch), *_loose_coords(wd, cw))
    d = take_window(v, win)
    if mutate == "offset_on_padding" and M is not None:
        pad = apply_color(np.zeros(3, np.float32), M)
        d = np.where(inside, d, pad).astype(np.float32)
    if flip:
        d = d[:, ::-1]
    return _resize(d, hd, wd)


def window_pad_mask(h, w, win, flip, hd, wd):
    """[hd, wd] bool: the destination pixels all of whose taps with a non-zero weight are padding (the restatement is 0.0)."""
    d = take_window(np.ones((h, w, 1), np.float32), win)
    return _resize(d[:, ::-1] if flip else d, hd, wd)[..., 0] == 0


@functools.lru_cache(maxsize=None)
def win_reference(hd, wd, color, mutate=None):
    """([n, hd, wd, 3] float32 restatement of the WIN_IMAGES batch under COLORS entry `color`, [n, hd, wd] padding mask)."""
    images = win_source()[0]
    Ms = color_of(color)
    ref = np.stack([window_restatement(images[si], win, fl, None if Ms is None else Ms[k], hd, wd, mutate)
                    for k, (si, _, win, fl) in enumerate(WIN_IMAGES)])
    pad = np.stack([window_pad_mask(*SOURCES[si], win, fl, hd, wd) for si, _, win, fl in WIN_IMAGES])
    ref.setflags(write=False)
    pad.setflags(write=False)
    return ref, pad


def drift_as_window(geom5):
    """[n, 5] (src_h, src_w, dx, dy, flip) -> the same drift as [n, 7] (src_h, src_w, dx, dy, src_w - dx, src_h - dy, flip)."""
    g = np.asarray(geom5, np.int64)
    return np.stack([g[:, 0], g[:, 1], g[:, 2], g[:, 3], g[:, 1] - g[:, 2], g[:, 0] - g[:, 3], g[:, 4]], 1)


# ---------------------------------------------------------------------------------------------------- policy dataset
POLICY_SIZES = [(120, 260), (97, 143), (200, 180), (64, 301)]


def policy_dataset(n=9, seed=17):
    """n uint8 images of POLICY_SIZES with 0..4 boxes each ([cx, cy, w, h, cls], inside the image; image 2 has none)."""
    rs = np.random.RandomState(seed)
    images, rois = [], []
    for i in range(n):
        h, w = POLICY_SIZES[i % len(POLICY_SIZES)]
        images.append(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        k = 0 if i == 2 else int(rs.randint(1, 5))
        bw, bh = rs.uniform(8, w / 2.0, k), rs.uniform(8, h / 2.0, k)
        x0, y0 = rs.uniform(0, w - bw - 1), rs.uniform(0, h - bh - 1)
        rois.append([[x0[j] + bw[j] / 2, y0[j] + bh[j] / 2, bw[j], bh[j], int(rs.randint(3))] for j in range(k)])
    return images, rois


def policy_config(geometry="ssd", zoom=2.0, color=True, batch=4, size=(96, 160)):
    import squeezedet_amd as S
    mc = S.kitti_squeezeDet_config_for_input(*size)
    mc.BATCH_SIZE, mc.DRIFT_X, mc.DRIFT_Y = batch, 12, 6
    mc.AUG_GEOMETRY, mc.AUG_ZOOM_OUT_MAX, mc.AUG_COLOR = geometry, zoom, color
    return mc
