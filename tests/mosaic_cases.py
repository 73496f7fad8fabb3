"""Inputs and the NumPy restatement for sqdet_augment_bgr_mosaic (squeezedet_amd/csrc/augment.hip; test infrastructure, no GPU).
Shared by tests/test_mosaic_host.py, which shows on the restatement alone that named cases discriminate the mistakes a mosaic kernel
can make, and by tests/test_gpu_mosaic.py.

mosaic_restatement is include/sqdet.h's definition: augment_policy_cases.window_restatement(im, win, flip, M, ph, pw) -- imported,
not restated -- pasted into each pane that has pixels.  `mutate` names one of six wrong variants.

Cases, per destination of DSTS (input_path_cases.AUG_DSTS and (9, 520), where a pane spans two 256-pixel chunks): one batch with an
image per split of XCS(W) x YCS(H) -- the chunk edge and its neighbours, the 4-pixel group edge, the image's own edges, and with
them every form in which one, two or four panes have pixels --, the parts of the panes taken in turn from
augment_policy_cases.WIN_IMAGES (three sources x ten windows x both flips), and a last image, "tail", whose bottom right pane shows
the whole of the buffer's last source image, so that its last pixel pair is read.  A pane without pixels gets GARBAGE for its
offset, geometry and matrix."""
import functools

import numpy as np

from oracle import preproc_oracle as PO
from tests import augment_policy_cases as AC
from tests import input_path_cases as IC

MEANS = IC.MEANS
DSTS = list(IC.AUG_DSTS) + [(9, 520)]
BASE_OFFSETS = IC.AUG_BASE_OFFSETS
COLORS = ["null", "cross", "mixed"]                 # mixed: part q = 4 * image + pane takes (identity, saturate, cross)[q % 3]
MUTATIONS = ["seam_blend", "pane_origin_off_by_one", "scale_from_full_size", "flip_in_output_coordinates", "parts_swapped",
             "empty_pane_examined"]
GARBAGE_GEOM = (-7, 0, 1 << 20, -(1 << 20), 0, -3, 5)
GARBAGE_OFFSET = -(1 << 40)


def XCS(W):
    return sorted({min(max(x, 0), W) for x in (0, 1, 3, 4, 255, 256, 257, W - 1, W)})


def YCS(H):
    return sorted({min(max(y, 0), H) for y in (0, 1, H - 1, H)})


def panes(xc, yc, W, H):
    """(px0, py0, pw, ph) of panes 0..3."""
    return [(0, 0, xc, yc), (xc, 0, W - xc, yc), (0, yc, xc, H - yc), (xc, yc, W - xc, H - yc)]


@functools.lru_cache(maxsize=None)
def mosaic_images(hd, wd):
    """[(name, (xc, yc), [part 0..3])], a part = (index of the source, window name, window, flip) or None for a pane without pixels."""
    out, q = [], 0
    for yc in YCS(hd):
        for xc in XCS(wd):
            parts = []
            for _, _, pw, ph in panes(xc, yc, wd, hd):
                if pw > 0 and ph > 0:
                    parts.append(AC.WIN_IMAGES[(7 * q) % len(AC.WIN_IMAGES)])          # 7 and 60 are coprime: every window in turn
                    q += 1
                else:
                    parts.append(None)
            out.append(("xc=%d,yc=%d" % (xc, yc), (xc, yc), parts))
    h, w = AC.SOURCES[2]
    whole = [(si, "whole", (0, 0, AC.SOURCES[si][1], AC.SOURCES[si][0]), fl) for si, fl in ((0, 1), (1, 0), (1, 1))]
    out.append(("tail", (wd // 2, hd // 2), whole + [(2, "whole", (0, 0, w, h), 0)]))
    return out


def mosaic_arrays(hd, wd):
    """(part_offsets int64 [n,4], geom int64 [n,4,7], split int64 [n,2]) of mosaic_images, GARBAGE in the panes without pixels."""
    starts = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in AC.SOURCES])[:-1]]).astype(np.int64)
    imgs = mosaic_images(hd, wd)
    off = np.full((len(imgs), 4), GARBAGE_OFFSET, np.int64)
    geom = np.tile(np.array(GARBAGE_GEOM, np.int64), (len(imgs), 4, 1))
    split = np.array([s for _, s, _ in imgs], np.int64)
    for i, (_, _, parts) in enumerate(imgs):
        for p, part in enumerate(parts):
            if part is not None:
                si, _, win, fl = part
                off[i, p], geom[i, p] = starts[si], list(AC.SOURCES[si]) + list(win) + [fl]
    return off, geom, split


def color_of(name, n):
    """[n, 4, 3, 4] float32 (NaN in no pane: the caller overwrites the panes without pixels if it wants garbage there), or None."""
    if name == "null":
        return None
    if name == "cross":
        return np.tile(AC.CROSS, (n, 4, 1, 1))
    assert name == "mixed"
    return np.stack([(AC.IDENTITY, AC.SATURATE, AC.CROSS)[q % 3] for q in range(4 * n)]).reshape(n, 4, 3, 4)


def color_with_garbage(name, hd, wd):
    """color_of as the launch gets it, [n, 4, 12] float32 with NaN in the panes without pixels (or None)."""
    imgs = mosaic_images(hd, wd)
    M = color_of(name, len(imgs))
    if M is None:
        return None
    M = M.reshape(len(imgs), 4, 12).copy()
    for i, (_, _, parts) in enumerate(imgs):
        for p, part in enumerate(parts):
            if part is None:
                M[i, p] = np.nan
    return M


def _window(im_u8, win, flip, M):
    """The window D of window_restatement (colour, mean, window, mirror), for the variants that resize it differently."""
    raw = im_u8.astype(np.float32)
    d = AC.take_window(AC.sub_mean(raw if M is None else AC.apply_color(raw, M)), win)
    return d[:, ::-1] if flip else d


def _coords_from(n_dst, n_src, first, count):
    """oracle.preproc_oracle._coords(n_dst, n_src) for destination indices [first, first + count)."""
    s0, s1, f = PO._coords(n_dst, n_src)
    return s0[first:first + count], s1[first:first + count], f[first:first + count]


def mosaic_restatement(sources, parts, split, Ms, hd, wd, mutate=None):
    """One output image, float32 [hd, wd, 3].  sources: the uint8 images; parts: four (source index, name, window, flip) or None (a
    pane without pixels: never looked at); split = (xc, yc); Ms: [4, 3, 4] or None.  mutate (MUTATIONS):
    seam_blend -- the two windows of a pane row are put side by side and the row is resized as one strip: the taps at the seam blend
      the neighbouring pane's first (last) column in;
    pane_origin_off_by_one -- the right-hand panes start at column xc + 1;
    scale_from_full_size -- the resize coordinates are those of (cw, ch) -> (wd, hd), read at the pane's own pixels;
    flip_in_output_coordinates -- a mirrored part mirrors about the OUTPUT's centre column instead of its pane's;
    parts_swapped -- panes 1 and 2 show each other's part;
    empty_pane_examined -- a pane without pixels is validated like the others: garbage there leaves the image unwritten (NaN)."""
    assert mutate is None or mutate in MUTATIONS
    xc, yc = split
    P = panes(xc, yc, wd, hd)
    out = np.full((hd, wd, 3), np.nan, np.float32)
    parts = list(parts)
    M = [None if Ms is None else Ms[p] for p in range(4)]
    if mutate == "parts_swapped" and parts[1] is not None and parts[2] is not None:
        parts[1], parts[2], M[1], M[2] = parts[2], parts[1], M[2], M[1]
    if mutate == "empty_pane_examined" and any(part is None for part in parts):
        return out
    for p, ((px0, py0, pw, ph), part) in enumerate(zip(P, parts)):
        if pw <= 0 or ph <= 0:
            continue
        si, _, win, fl = part
        im = sources[si]
        if mutate == "scale_from_full_size":
            d = _window(im, win, fl, M[p])
            pane = AC._blend(d, *_coords_from(hd, d.shape[0], py0, ph), *_coords_from(wd, d.shape[1], px0, pw))
        elif mutate == "flip_in_output_coordinates" and fl:
            plain = AC.window_restatement(im, win, 0, M[p], ph, pw)
            pane = plain[:, np.clip(wd - 1 - (px0 + np.arange(pw)) - px0, 0, pw - 1)]
        elif mutate == "seam_blend" and 0 < xc < wd:
            other = parts[p ^ 1]
            d = _window(im, win, fl, M[p])
            e = _window(sources[other[0]], other[2], other[3], M[p ^ 1])
            sy, sy1, fy = PO._coords(ph, d.shape[0])
            ey, _, _ = PO._coords(ph, e.shape[0])
            sx, sx1, fx = _loose(pw, d.shape[1])
            # the strip of this pane row: this window's columns with ONE column of the neighbour's on the side of the seam
            if p & 1:
                strip0, strip1 = np.concatenate([e[ey][:, -1:], d[sy]], 1), np.concatenate([e[ey][:, -1:], d[sy1]], 1)
                sx, sx1 = np.minimum(sx + 1, d.shape[1]), np.minimum(sx1 + 1, d.shape[1])
            else:
                strip0, strip1 = np.concatenate([d[sy], e[ey][:, :1]], 1), np.concatenate([d[sy1], e[ey][:, :1]], 1)
                sx, sx1 = np.maximum(sx, 0), np.maximum(sx1, 0)
            ax0, fxb = (np.float32(1) - fx)[None, :, None], fx[None, :, None]
            h0 = strip0[:, sx] * ax0 + strip0[:, sx1] * fxb
            h1 = strip1[:, sx] * ax0 + strip1[:, sx1] * fxb
            pane = (h0 * (np.float32(1) - fy)[:, None, None] + h1 * fy[:, None, None]).astype(np.float32)
        else:
            pane = AC.window_restatement(im, win, fl, M[p], ph, pw)
        if mutate == "pane_origin_off_by_one" and px0 > 0:
            out[py0:py0 + ph, px0 + 1:px0 + pw] = pane[:, :pw - 1]
        else:
            out[py0:py0 + ph, px0:px0 + pw] = pane
    return out


def _loose(n_dst, n_src):
    """_coords without the clamp at the window's border, as indices into the window: taps in [-1, n_src]."""
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (float(n_src) / float(n_dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, s + 1, (f - s.astype(np.float32)).astype(np.float32)


def mosaic_pad_mask(parts, split, hd, wd):
    """[hd, wd] bool: the pixels whose taps are zero padding only."""
    out = np.zeros((hd, wd), bool)
    for (px0, py0, pw, ph), part in zip(panes(split[0], split[1], wd, hd), parts):
        if pw > 0 and ph > 0:
            si, _, win, fl = part
            out[py0:py0 + ph, px0:px0 + pw] = AC.window_pad_mask(*AC.SOURCES[si], win, fl, ph, pw)
    return out


@functools.lru_cache(maxsize=None)
def mosaic_reference(hd, wd, color, mutate=None):
    """([n, hd, wd, 3] float32 restatement of the mosaic_images batch under COLORS entry `color`, [n, hd, wd] padding mask)."""
    sources = AC.win_source()[0]
    imgs = mosaic_images(hd, wd)
    Ms = color_of(color, len(imgs))
    ref = np.stack([mosaic_restatement(sources, parts, split, None if Ms is None else Ms[i], hd, wd, mutate)
                    for i, (_, split, parts) in enumerate(imgs)])
    pad = np.stack([mosaic_pad_mask(parts, split, hd, wd) for _, split, parts in imgs])
    ref.setflags(write=False)
    pad.setflags(write=False)
    return ref, pad


def plan_restatement(images, plan, mc):
    """[B, H, W, 3] float32: the restatement of a BatchReader Plan with the mosaic on."""
    H, W = int(mc.IMAGE_HEIGHT), int(mc.IMAGE_WIDTH)
    out = []
    for k in range(len(plan.batch_idx)):
        parts = [None if plan.parts[k, p] < 0 else (int(plan.parts[k, p]), "plan", tuple(int(v) for v in plan.part_window[k, p]),
                                                    int(plan.part_flip[k, p])) for p in range(4)]
        Ms = None if plan.part_color is None else plan.part_color[k].reshape(4, 3, 4)
        out.append(mosaic_restatement(images, parts, tuple(int(v) for v in plan.split[k]), Ms, H, W))
    return np.stack(out)
