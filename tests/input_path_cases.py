"""Inputs for the two kernels that produce what a training step consumes, at their edges (test infrastructure, no GPU):
squeezedet_amd/csrc/labels.hip (sqdet_build_labels) and squeezedet_amd/csrc/augment.hip (sqdet_augment_bgr).  Shared by
tests/test_input_path_host.py, which shows on the oracle alone that every case reaches the branch it is named after and that
the comparison functions reject wrong results, and by tests/test_gpu_input_path.py.

Labels.  The anchor tables are DYADIC: grid(nx, ny) puts the three shapes (48,32), (96,64), (32,96) on the centres
32 * (i + 1), index (iy * nx + ix) * 3 + shape, so that every product, sum and difference of batch_iou and of the squared
distance is exact in float64 and two mirror-symmetric anchors have bit-equal IoUs / distances: exact ties, which the KITTI
tables (centres k * 1248 / 79) never produce.  S2 is S twice: every value ties between a and a + 273.
label_case(name) -> LabelCase; label_reference(name) -> the picks of oracle.train_oracle.assign_anchors and the dense tensors;
two_pass(...) is labels.hip's decomposition (best ignoring claims, in-order resolve, sweep over the free anchors on a clash)
restated in NumPy, with both tie rules switchable for the mutation checks.

Augment.  AUG_GEOMS x both flips, packed back to back (odd byte counts), into the AUG_DSTS sizes; augment_reference is the one
of tests/test_augment_host.py, augment_pad_mask marks the outputs that are zero padding only, check_augment is the comparison;
load_pairs / store_classes restate which load and store branch of the kernel a destination pixel group takes."""
import collections
import functools
import types

import numpy as np

from oracle import preproc_oracle as PO
from oracle import sqdet_oracle as O
from oracle import train_oracle as TO
from tests.test_augment_host import augment_reference

# ================================================================== labels
SHAPES3 = ((48.0, 32.0), (96.0, 64.0), (32.0, 96.0))
LABELS_LDS_CAP = 60000            # labels.hip: SQDET_UNSUPPORTED(lds > 60000, ...)
LABELS_MAX_OBJECTS = 1024         # labels.hip: one thread of labels_resolve_kernel per box
BIG_A = 480000


def grid(nx, ny, shapes=SHAPES3, step=32.0):
    """[ny * nx * len(shapes), 4] float64 (cx, cy, w, h): row (iy * nx + ix) * len(shapes) + k is shape k at (step * (ix + 1), step * (iy + 1))."""
    iy, ix, k = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(len(shapes)), indexing="ij")
    sh = np.asarray(shapes, np.float64)
    return np.stack([step * (ix + 1.0), step * (iy + 1.0), sh[k, 0], sh[k, 1]], -1).reshape(-1, 4)


def labels_lds_bytes(A):
    """The dynamic LDS of labels_resolve_kernel: one bit per anchor, in 32-bit words."""
    return (A + 31) // 32 * 4


@functools.lru_cache(maxsize=None)
def table(name):
    if name == "S":
        t = grid(13, 7)
    elif name == "S2":
        t = np.concatenate([table("S"), table("S")])
    elif name == "three":
        t = grid(1, 1)
    elif name == "one":
        t = grid(1, 1, SHAPES3[:1])
    elif name == "cap":
        t = grid(20, 18)
    elif name == "big":
        t = grid(400, 400)[:BIG_A]
    else:
        raise KeyError(name)
    t.setflags(write=False)
    return t


LabelCase = collections.namedtuple("LabelCase", "name anchors gt cls cnt C")
LABEL_CASES = ["dup", "mirror", "full", "far", "cap", "big", "classes1", "classes20", "degenerate", "three", "one"]
MIRROR_BOXES = [[48.0, 64.0, 48.0, 32.0], [48.0, 48.0, 40.0, 40.0], [-100.0, 48.0, 8.0, 8.0], [48.0, 64.0, 48.0, 32.0]]
MIRROR_PICKS = [42, 43, 0, 39]


def _random_boxes(rs, n, W, H):
    return np.stack([rs.uniform(0, W, n), rs.uniform(0, H, n), rs.uniform(16, 120, n), rs.uniform(16, 120, n)], 1)


def _lattice_boxes(rs, n):
    """Boxes on the table's own lattice (centres and sizes multiples of 16 over S): exact IoU ties between different anchors."""
    return np.stack([16.0 * rs.randint(0, 29, n), 16.0 * rs.randint(0, 17, n), 16.0 * rs.randint(1, 8, n), 16.0 * rs.randint(1, 8, n)], 1)


def _pack(anchors, per_image, counts, cls, C, name, M=None):
    """per_image: list of [n_i, 4]; the rows behind an image's boxes are filled with a box that would win anchor 0."""
    M = M or max(len(g) for g in per_image)
    gt = np.tile(np.asarray(anchors[0], np.float64), (len(per_image), M, 1))
    for b, g in enumerate(per_image):
        gt[b, :len(g)] = g
    return LabelCase(name, anchors, gt, np.asarray(cls, np.int32).reshape(len(per_image), M), np.asarray(counts, np.int32), C)


@functools.lru_cache(maxsize=None)
def label_case(name):
    rs = np.random.RandomState(LABEL_CASES.index(name) + 101)
    if name == "dup":
        far = np.tile([[-300.0, -200.0, 20.0, 20.0]], (3, 1))
        g0 = np.concatenate([_random_boxes(rs, 12, 448, 256), far, _random_boxes(rs, 8, 448, 256)])
        return _pack(table("S2"), [g0, _random_boxes(rs, 7, 448, 256)], [23, 7], rs.randint(0, 3, (2, 23)), 3, name)
    if name == "mirror":
        return _pack(table("S"), [np.array(MIRROR_BOXES)], [4], [[0, 1, 2, 1]], 3, name)
    if name == "full":
        return _pack(table("S"), [_lattice_boxes(rs, 273)], [273], rs.randint(0, 3, (1, 273)), 3, name)
    if name == "far":
        g = _random_boxes(rs, 40, 448, 256)
        g[:, 0] -= 5000.0
        return _pack(table("S2"), [g], [40], rs.randint(0, 3, (1, 40)), 3, name)
    if name == "cap":
        M = LABELS_MAX_OBJECTS
        g = [_random_boxes(rs, M, 672, 608) for _ in range(3)]
        return _pack(table("cap"), g, [M, M + 6, -3], rs.randint(0, 3, (3, M)), 3, name)
    if name == "big":
        last = table("big")[BIG_A - 1]
        return _pack(table("big"), [np.array([last, last, [-4000.0, 300.0, 50.0, 40.0]])], [3], [[0, 0, 0]], 1, name)
    if name in ("classes1", "classes20"):
        C = 1 if name == "classes1" else 20
        cls = rs.randint(0, C, (2, 9))
        cls[0, [1, 4]] = [-1, C]                      # one below, one above the range
        cls[1, [0, 5, 8]] = [C, C - 1, -1]
        return _pack(table("S"), [_random_boxes(rs, 9, 448, 256), _random_boxes(rs, 9, 448, 256)], [9, 9], cls, C, name)
    if name == "degenerate":
        g = np.array([[200.0, 100.0, 60.0, 40.0], [100.0, 96.0, 0.0, 40.0], [64.0, 64.0, 48.0, 32.0]])
        return _pack(table("S"), [g], [3], [[2, 0, 1]], 3, name)
    if name == "three":
        a = table("three")
        g0 = np.array([a[1], a[1], [-50.0, 500.0, 10.0, 10.0]])       # IoU 1, a clash, the distance sweep: all three claimed
        g1 = np.array([[40.0, 30.0, 20.0, 90.0]])
        return _pack(a, [g0, g1], [3, 1], [[0, 1, 2], [1, 0, 0]], 3, name)
    if name == "one":
        return _pack(table("one"), [np.array([[40.0, 40.0, 30.0, 30.0]]), np.zeros((0, 4))], [1, 0], [[1], [0]], 2, name)
    raise KeyError(name)


def clipped_count(case, b):
    return int(min(max(int(case.cnt[b]), 0), case.gt.shape[1]))


def _mc(anchors):
    return types.SimpleNamespace(ANCHOR_BOX=anchors)


LabelRef = collections.namedtuple("LabelRef", "aidx mask delta64 box labels")


@functools.lru_cache(maxsize=None)
def label_reference(name):
    """oracle.train_oracle.assign_anchors per image and the dense tensors of train.py:163-224: aidx int32 [B,M] (-1 behind the
    count), mask / box / labels float32, delta64 float64 [B,A,4] (the caller rounds it once)."""
    c = label_case(name)
    (B, M), A = c.cls.shape, len(c.anchors)
    aidx = np.full((B, M), -1, np.int32)
    mask, delta = np.zeros((B, A), np.float32), np.zeros((B, A, 4), np.float64)
    box, lab = np.zeros((B, A, 4), np.float32), np.zeros((B, A, c.C), np.float32)
    for b in range(B):
        n = clipped_count(c, b)
        with np.errstate(divide="ignore"):
            picks, deltas = TO.assign_anchors(_mc(c.anchors), c.gt[b, :n])
        assert len(set(picks)) == len(picks)
        for j, a in enumerate(picks):
            aidx[b, j], mask[b, a], delta[b, a], box[b, a] = a, 1.0, deltas[j], c.gt[b, j].astype(np.float32)
            if 0 <= c.cls[b, j] < c.C:
                lab[b, a, c.cls[b, j]] = 1.0
    for t in (aidx, mask, delta, box, lab):
        t.setflags(write=False)
    return LabelRef(aidx, mask, delta, box, lab)


def _sqdist(anchors, g):
    d = g - anchors
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3]


def best_free(anchors, g, taken, iou_tie_high=True, dist_tie_low=True):
    """labels.hip best_anchor: among the anchors not in `taken` the largest overlap > 0 (ties: higher index), else the smallest
    squared distance (ties: lower index).  Returns (index, "iou" | "dist", number of free anchors tied at the winning value)."""
    ov = np.where(taken, -1.0, O.batch_iou(anchors, g))
    m = ov.max()
    if m > 0:
        idx = np.flatnonzero(ov == m)
        return int(idx[-1] if iou_tie_high else idx[0]), "iou", len(idx)
    dist = np.where(taken, np.inf, _sqdist(anchors, g))
    idx = np.flatnonzero(dist == dist.min())
    return int(idx[0] if dist_tie_low else idx[-1]), "dist", len(idx)


PassStats = collections.namedtuple("PassStats", "picks clashes dist_mode iou_ties dist_ties")


def two_pass(anchors, gt, iou_tie_high=True, dist_tie_low=True):
    """labels_best_kernel + labels_resolve_kernel for one image: every box's best anchor ignoring the claims, then the boxes in
    order -- a free candidate is accepted, a claimed one triggers best_free over the free anchors.  clashes: boxes whose candidate
    was claimed; dist_mode: boxes whose final pick came from the distance sweep; iou_ties / dist_ties: boxes whose final pick
    was tied with another free anchor."""
    none = np.zeros(len(anchors), bool)
    cand = [best_free(anchors, g, none, iou_tie_high, dist_tie_low) for g in gt]
    taken = none.copy()
    picks, clashes, dist_mode, iou_ties, dist_ties = [], 0, 0, 0, 0
    for g, (a, mode, ties) in zip(gt, cand):
        if taken[a]:
            clashes += 1
            a, mode, ties = best_free(anchors, g, taken, iou_tie_high, dist_tie_low)
        taken[a] = True
        picks.append(a)
        dist_mode += mode == "dist"
        iou_ties += mode == "iou" and ties > 1
        dist_ties += mode == "dist" and ties > 1
    return PassStats(picks, clashes, dist_mode, iou_ties, dist_ties)


@functools.lru_cache(maxsize=None)
def label_stats(name, iou_tie_high=True, dist_tie_low=True):
    """two_pass per image of the case."""
    c = label_case(name)
    return [two_pass(c.anchors, c.gt[b, :clipped_count(c, b)], iou_tie_high, dist_tie_low) for b in range(len(c.cnt))]


# ================================================================== augment
MEANS = np.array([[[103.939, 116.779, 123.68]]])
AUGMENT_MAX_DRIFT = 65535
# (source (h, w), dx, dy): the drifts of test_gpu_augment.test_kernel_small_and_odd_sizes ((52, 36) and (6, 8) leave one row and
# one column: dx = w - 1, dy = h - 1), and the two extreme drifts, one axis each (the drifted image stays a few MB)
AUG_GEOMS = [((37, 53), 5, 3), ((37, 53), 52, 36), ((37, 53), -30, -20), ((9, 7), 6, 8), ((61, 201), -1, 1),
             ((9, 7), -AUGMENT_MAX_DRIFT, 0), ((5, 11), 0, -AUGMENT_MAX_DRIFT)]
# each with both flips; the last image of the buffer is one whose last pixel pair is read: its 8-byte load would pass the end
AUG_IMAGES = [(s, dx, dy, fl) for fl in (1, 0) for (s, dx, dy) in AUG_GEOMS[::-1]] + [((37, 53), 5, 3, 1)]
# (Hd, Wd): 261 -- odd, two workgroups per row, float16 rows cycle 8-byte / scalar / 4-byte / scalar stores, float32 alternates;
# 262 -- float16 alternates 8-byte / 4-byte; 259 and 5 -- a last group of 3 and of 1 pixel
AUG_DSTS = [(7, 261), (12, 262), (7, 259), (12, 5)]
AUG_BASE_OFFSETS = [0, 1]         # elements between a 256-byte aligned address and the start of the destination view
F32_ABS, F32_EQUAL_SHARE = 2e-4, 0.999      # tests/test_gpu_augment.py _check


@functools.lru_cache(maxsize=None)
def aug_source():
    """(images, flat uint8 buffer, byte offsets)."""
    rs = np.random.RandomState(41)
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s, _, _, _ in AUG_IMAGES]
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])[:-1]]).astype(np.int64)
    flat = np.concatenate([im.reshape(-1) for im in images])
    flat.setflags(write=False)
    return images, flat, offsets


def aug_geom():
    return np.array([[s[0], s[1], dx, dy, fl] for s, dx, dy, fl in AUG_IMAGES])


def _drift_flip(a, dx, dy, flip, fill=0.0):
    h, w = a.shape[:2]
    d = np.full((h - dy, w - dx) + a.shape[2:], fill, np.float32)
    d[max(-dy, 0):, max(-dx, 0):] = a[max(dy, 0):, max(dx, 0):]
    return d[:, ::-1] if flip else d


def augment_pad_mask(h, w, dx, dy, flip, hd, wd):
    """[hd, wd] bool: the destination pixels all of whose taps with a non-zero weight are zero padding (the reference is 0.0)."""
    return PO.resize_linear(_drift_flip(np.ones((h, w, 1), np.float32), dx, dy, flip), hd, wd)[..., 0] == 0


def augment_restatement(im_u8, dx, dy, flip, hd, wd, swap_pair=True, pad_with_zero=True):
    """augment_reference with the two mistakes the host test feeds to check_augment: swap_pair = False leaves the two pixels of
    a mirrored pair in memory order (taps sx and sx1 exchanged under flip), pad_with_zero = False pads the uint8 image with 0
    BEFORE the mean subtraction (padding = -mean)."""
    im = im_u8.astype(np.float32)
    im -= MEANS
    d = _drift_flip(im, dx, dy, flip)
    if not pad_with_zero:
        inside = _drift_flip(np.ones(im.shape[:2] + (1,), np.float32), dx, dy, flip) > 0
        d = np.where(inside, d, (np.zeros(3, np.float32) - MEANS.reshape(3)).astype(np.float32)).astype(np.float32)
    sy, sy1, fy = PO._coords(hd, d.shape[0])
    sx, sx1, fx = PO._coords(wd, d.shape[1])
    if flip and not swap_pair:
        sx, sx1 = sx1, sx
    ax0, fxb = (np.float32(1) - fx)[None, :, None], fx[None, :, None]
    h0 = d[sy][:, sx] * ax0 + d[sy][:, sx1] * fxb
    h1 = d[sy1][:, sx] * ax0 + d[sy1][:, sx1] * fxb
    return (h0 * (np.float32(1) - fy)[:, None, None] + h1 * fy[:, None, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def aug_reference(hd, wd):
    """([n, hd, wd, 3] float32 reference, [n, hd, wd] padding mask) of the AUG_IMAGES batch."""
    images = aug_source()[0]
    ref = np.stack([augment_reference(im, dx, dy, fl, hd, wd, MEANS) for im, (_, dx, dy, fl) in zip(images, AUG_IMAGES)])
    pad = np.stack([augment_pad_mask(s[0], s[1], dx, dy, fl, hd, wd) for s, dx, dy, fl in AUG_IMAGES])
    ref.setflags(write=False)
    pad.setflags(write=False)
    return ref, pad


def f16_bound(ref32):
    """float16 output against the float32 reference: the float32 allowance, plus one correctly rounded conversion of a value that
    far from the reference (relative 2^-11 in the normal range, absolute 2^-25 below it)."""
    return F32_ABS + 2.0 ** -11 * (np.abs(ref32.astype(np.float64)) + F32_ABS) + 2.0 ** -25


def check_augment(out, ref, pad, f16=False, what=""):
    """One image [hd, wd, 3] (float32 array; a float16 output converted) against the reference: float32 -- the project's
    criterion, <= 2e-4 and >= 99.9 % of the elements equal; float16 -- within f16_bound; both -- exactly 0 where the reference is
    zero padding.  Returns the share of elements that are NOT equal to the reference."""
    assert out.shape == ref.shape and pad.shape == ref.shape[:2] and out.dtype == np.float32
    assert np.isfinite(out).all(), "%s: a non-finite output (an unwritten cell?)" % what
    assert (ref[pad] == 0).all()
    assert (out[pad] == 0).all(), "%s: %d padding elements are not 0, largest %g" % (what, (out[pad] != 0).sum(), np.abs(out[pad]).max())
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    unequal = float((out != ref).mean())
    if f16:
        q = err / f16_bound(ref)
        assert q.max() <= 1.0, "%s: float16 error is %g of its bound (abs %g)" % (what, q.max(), err.max())
    else:
        assert err.max() <= F32_ABS, "%s: max abs error %g" % (what, err.max())
        assert 1.0 - unequal >= F32_EQUAL_SHARE, "%s: only %.4f of the elements are equal" % (what, 1.0 - unequal)
    return unequal


def load_pairs(h, w, dx, dy, flip, hd, wd, off, src_bytes):
    """augment_kernel's load branch per destination pixel: ([hd, wd] bool: True -- the unaligned 8-byte pair load, False -- byte
    loads; [hd, wd] bool: byte loads ONLY because the 8-byte load would pass the end of the buffer)."""
    Hs, Ws = h - dy, w - dx
    sy, sy1, _ = PO._coords(hd, Hs)
    sx, sx1, _ = PO._coords(wd, Ws)
    oy0, oy1 = sy + dy, sy1 + dy
    r0, r1 = (oy0 >= 0) & (oy0 < h), (oy1 >= 0) & (oy1 < h)
    o0, o1 = off + np.where(r0, oy0, 0) * w * 3, off + np.where(r1, oy1, 0) * w * 3
    ox, ox1 = ((Ws - 1 - sx, Ws - 1 - sx1) if flip else (sx, sx1))
    ox, ox1 = ox + dx, ox1 + dx
    c0, c1 = (ox >= 0) & (ox < w), (ox1 >= 0) & (ox1 < w)
    lo = np.minimum(ox, ox1)
    inside = ((sx1 != sx) & c0 & c1)[None, :] & (r0 & r1)[:, None]
    fits = (o0[:, None] + lo[None, :] * 3 + 8 <= src_bytes) & (o1[:, None] + lo[None, :] * 3 + 8 <= src_bytes)
    return inside & fits, inside & ~fits


STORE_CLASSES = {4: {"vector", "scalar_full", "scalar_tail"}, 2: {"vector", "h2", "scalar_full", "scalar_tail"}}


def store_classes(esize, wd, rows, base_bytes):
    """augment_kernel's store branch per (row, group of 4 pixels): {class: count} over the given rows (row = image * Hd + y) of a
    destination of element size `esize` whose first element lies at byte `base_bytes` (mod 8)."""
    x0 = np.arange(0, wd, 4)
    addr = base_bytes + esize * 3 * (np.asarray(rows)[:, None] * wd + x0[None, :])
    full = np.broadcast_to((x0 + 4 <= wd)[None, :], addr.shape)
    vec = full & (addr % 8 == 0)
    h2 = full & ~vec & (addr % 4 == 0) & (esize == 2)
    out = {"vector": int(vec.sum()), "h2": int(h2.sum()), "scalar_full": int((full & ~vec & ~h2).sum()), "scalar_tail": int((~full).sum())}
    return {k: v for k, v in out.items() if v}
