"""Generates tests/golden/augment.npz by RUNNING THE REFERENCE'S OWN ``imdb.read_batch`` (dataset/imdb.py:100-239) with
data augmentation on, imported unchanged through oracle/ref_imdb_half.py.  Only runnable where the reference tree is
mounted; the output is committed so that the GPU box (which has no reference tree) can check against it.

The module-level ``cv2`` of the loaded module is replaced by a stub: ``imread`` returns registered seeded uint8 images
and ``resize`` is oracle.preproc_oracle.resize_linear (cv2's INTER_LINEAR float32 path).  The imdb is built as
kitti.__init__ builds it -- global ``np.random.seed(seed)``, then the first shuffle --, and every ``np.random.randint``
call is recorded.

Two cases:
  * pixels: five small images of four sizes, drift 20 / 10, a 96x32 network input, one batch of four images: the uint8
    inputs, the draws, the boxes and the output pixels.  The seed is picked so that the batch holds a crop, a pad, a zero
    drift and both flips.
  * labels: the full kitti_squeezeDet_config (1248x384, batch 20, drift 150 / 100) on 30 zero images of the four KITTI
    sizes, three shuffled batches: the batch order, the draws, the boxes, aidx and deltas.  Every pick is decided by a
    strict inequality (np.argsort's order among ties is unspecified).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_augment_golden.py [out.npz]
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import preproc_oracle as PO  # noqa: E402
from oracle import ref_imdb_half as ref_imdb  # noqa: E402
from oracle import ref_numpy_half as ref  # noqa: E402

KITTI_SIZES = [(370, 1224), (374, 1238), (376, 1241), (375, 1242)]
PIXEL_SIZES = [(40, 120), (41, 122), (43, 124), (44, 126)]
PIXEL = dict(n_images=5, batch=4, width=96, height=32, drift_x=20, drift_y=10)
LABEL = dict(n_images=30, batches=3, seed=5)


def make_rois(rs, ns, h, w, n_obj, min_wh, max_wh):
    """KITTI-like annotations: [xmin, ymin, xmax, ymax] inside the image -> [cx, cy, w, h, cls] through the reference's
    own bbox_transform_inv, as dataset/kitti.py:78-89 does."""
    rois = []
    for _ in range(n_obj):
        bw, bh = rs.uniform(min_wh[0], max_wh[0]), rs.uniform(min_wh[1], max_wh[1])
        x0, y0 = rs.uniform(0, w - bw - 1), rs.uniform(0, h - bh - 1)
        cx, cy, ww, hh = ns.util.bbox_transform_inv([x0, y0, x0 + bw, y0 + bh])
        rois.append([cx, cy, ww, hh, int(rs.randint(3))])
    return rois


def run_reference(mc, images, rois, seed, n_batches):
    """The reference's imdb as kitti.__init__ builds it, then n_batches x read_batch(shuffle=True).
    Returns per batch (batch indices, draws [(low, high, value)], labels, deltas, aidx, bboxes, images)."""
    mod = ref_imdb._load()
    stub = types.ModuleType("cv2")
    stub.imread = lambda path: images[int(os.path.basename(path).split(".")[0])].copy()
    # (an all-zero image resizes to zeros: the label case's 1248x384 resizes are skipped, with the same result)
    stub.resize = lambda im, size: PO.resize_linear(im, size[1], size[0]) if im.any() else np.zeros((size[1], size[0], 3), np.float32)
    saved_cv2, mod.cv2 = mod.cv2, stub        # (restored below: the loaded module is shared with ref_imdb_half.read_batch)
    try:
        return _run(mod, mc, images, rois, seed, n_batches)
    finally:
        mod.cv2 = saved_cv2


def _run(mod, mc, images, rois, seed, n_batches):
    mc = type(mc)(mc)
    mc.DEBUG_MODE = False
    db = mod.imdb("synthetic", mc)
    db._image_idx = ["%06d" % i for i in range(len(images))]
    db._rois = {idx: [list(r) for r in rois[i]] for i, idx in enumerate(db._image_idx)}
    order = []

    def path_at(idx):
        order.append(int(idx))
        return "synthetic/%s.png" % idx
    db._image_path_at = path_at
    draws = []
    randint = np.random.randint

    def recording_randint(*a, **k):
        v = randint(*a, **k)
        draws.append((float(a[0]), float(a[1]) if len(a) > 1 else np.nan, float(v)))
        return v
    np.random.seed(seed)
    db._perm_idx = None
    db._cur_idx = 0
    db._shuffle_image_idx()          # kitti.__init__'s first shuffle
    out = []
    np.random.randint = recording_randint
    try:
        for _ in range(n_batches):
            del order[:], draws[:]
            ims, labels, deltas, aidx, bboxes = db.read_batch(shuffle=True)
            out.append((list(order), list(draws), labels, deltas, aidx, bboxes, ims))
    finally:
        np.random.randint = randint
    return out


def tied_images(mc, ns, batch):
    """Indices (into the batch) of images with a pick that is not decided by a strict inequality (make_golden.py)."""
    anchors = np.asarray(mc.ANCHOR_BOX)
    bad = []
    for i, (aidx, bboxes) in enumerate(zip(batch[4], batch[5])):
        taken = set()
        for k, a in enumerate(aidx):
            ov = ns.util.batch_iou(anchors, bboxes[k])
            free = np.ones(len(anchors), bool)
            free[list(taken)] = False
            rest = free.copy()
            rest[a] = False
            if ov[a] > 0:
                ok = ov[a] > ov[rest].max()
            else:
                dist = np.sum(np.square(bboxes[k] - anchors), axis=1)
                ok = ov[free].max() <= 0 and dist[a] < dist[rest].min()
            if not ok:
                bad.append(i)
                break
            taken.add(int(a))
    return bad


def pixel_case(ns, out):
    P = PIXEL
    mc = ns.cfg_squeezeDet.kitti_squeezeDet_config()
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.BATCH_SIZE = P["width"], P["height"], P["batch"]
    mc.DRIFT_X, mc.DRIFT_Y, mc.DATA_AUGMENTATION = P["drift_x"], P["drift_y"], True
    rs = np.random.RandomState(11)
    sizes = [PIXEL_SIZES[i % 4] for i in range(P["n_images"])]
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in sizes]
    # boxes away from the left / top edge so that positive drifts (crops) are possible
    rois = [[r for r in make_rois(rs, ns, h, w, 2, (8, 6), (30, 16)) ] for (h, w) in sizes]
    for r, (h, w) in zip(rois, sizes):
        for b in r:
            assert b[0] - b[2] / 2 >= 0 and b[1] - b[3] / 2 >= 0
    for seed in range(1000):
        (order, draws, labels, deltas, aidx, bboxes, ims), = run_reference(mc, images, rois, seed, 1)
        d = np.array([v for _, _, v in draws]).reshape(-1, 3)          # per image: dy, dx, flip
        dy, dx, fl = d[:, 0], d[:, 1], d[:, 2] > 0.5
        if ((dx > 0) | (dy > 0)).any() and ((dx < 0) | (dy < 0)).any() and ((dx == 0) | (dy == 0)).any() \
                and fl.any() and (~fl).any() and sorted(set(s for s in (sizes[i] for i in order))) == sorted(set(sizes[:4])):
            break
    else:
        raise RuntimeError("no seed gives a crop, a pad, a zero drift and both flips")
    print("pixels: seed %d, batch %s, (dy, dx, flip) %s" % (seed, order, d.astype(int).tolist()))
    out["px_seed"] = np.array(seed)
    out["px_params"] = np.array([P["n_images"], P["batch"], P["width"], P["height"], P["drift_x"], P["drift_y"]])
    out["px_sizes"] = np.array(sizes)
    out["px_images"] = np.concatenate([im.reshape(-1) for im in images])
    out["px_rois"] = np.array(rois, np.float64)                        # [n_images, 2, 5]
    out["px_batch_idx"] = np.array(order)
    out["px_draws"] = np.array(draws, np.float64)
    out["px_bbox"] = np.array(bboxes, np.float64)                      # [batch, 2, 4]
    out["px_pixels"] = np.stack(ims).astype(np.float32)


def label_case(ns, out):
    L = LABEL
    mc = ns.cfg_squeezeDet.kitti_squeezeDet_config()
    rs = np.random.RandomState(23)
    sizes = [KITTI_SIZES[i % 4] for i in range(L["n_images"])]
    images = [np.zeros(s + (3,), np.uint8) for s in sizes]
    # small boxes: a box much smaller or larger than an anchor has the same IoU with every anchor it lies in / holds
    new = lambda h, w: make_rois(rs, ns, h, w, int(rs.randint(1, 3)), (30, 30), (60, 60))
    rois = [new(h, w) for (h, w) in sizes]
    # re-draw the boxes of the FIRST image (in the order read) whose pick hangs on a tie until it is tie-free and no
    # earlier pick broke; a re-draw changes every later image's draws, so the tie-free prefix only grows
    def first_bad(batches):
        seq = [(k, i) for k, b in enumerate(batches) for i in range(len(b[0]))]
        bad = {(k, i) for k, b in enumerate(batches) for i in tied_images(mc, ns, b)}
        return next((t for t, ki in enumerate(seq) if ki in bad), None), seq
    batches = run_reference(mc, images, rois, L["seed"], L["batches"])
    t, seq = first_bad(batches)
    redraws = 0
    while t is not None:
        k, i = seq[t]
        img = batches[k][0][i]
        for _ in range(1000):
            saved, rois[img] = rois[img], new(*sizes[img])
            redraws += 1
            cand = run_reference(mc, images, rois, L["seed"], L["batches"])
            t2, _ = first_bad(cand)
            if t2 is None or t2 > t:
                break
            rois[img] = saved
        else:
            raise RuntimeError("could not make the label case tie-free")
        batches, t = cand, t2
    M = max(len(r) for r in rois)
    B = mc.BATCH_SIZE
    out["lb_seed"] = np.array(L["seed"])
    out["lb_sizes"] = np.array(sizes)
    out["lb_rois"] = np.zeros((len(rois), M, 5))
    out["lb_counts"] = np.array([len(r) for r in rois])
    for i, r in enumerate(rois):
        out["lb_rois"][i, :len(r)] = r
    for k, (order, draws, labels, deltas, aidx, bboxes, _) in enumerate(batches):
        bb, dl, ai = np.zeros((B, M, 4)), np.zeros((B, M, 4)), -np.ones((B, M), np.int64)
        for i in range(B):
            n = len(aidx[i])
            bb[i, :n], dl[i, :n], ai[i, :n] = bboxes[i], np.asarray(deltas[i], np.float64), aidx[i]
        out["lb%d_batch_idx" % k] = np.array(order)
        out["lb%d_draws" % k] = np.array(draws, np.float64)
        out["lb%d_bbox" % k], out["lb%d_delta" % k], out["lb%d_aidx" % k] = bb, dl, ai
        print("labels: batch %d: %s, %d objects" % (k, order, sum(len(a) for a in aidx)))
    print("labels: tie-free after %d re-draws" % redraws)


def main(path=os.path.join(HERE, "augment.npz")):
    ns = ref.load()
    out = {}
    pixel_case(ns, out)
    label_case(ns, out)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
