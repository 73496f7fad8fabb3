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

Kept on purpose, as in the reference: the shuffled branch reshuffles as soon as ``cur + BATCH_SIZE >= len`` (imdb.py:
121-123), so the last full batch of every epoch is never served and each epoch serves ``ceil(len / B) - 1`` batches.
"""
from collections import namedtuple

import numpy as np

Batch = namedtuple("Batch", ["image_input", "gt_boxes", "gt_classes", "gt_counts", "aug", "bbox_per_batch",
                             "label_per_batch", "batch_idx"])
Batch.__doc__ = """One training batch.  image_input: device [B, IMAGE_HEIGHT, IMAGE_WIDTH, 3] in the reader's dtype;
gt_boxes float64 [B, M, 4] (cx, cy, w, h in network-input pixels), gt_classes int32 [B, M], gt_counts int32 [B]: device
tensors padded to M = the dataset's largest object count, ready for ops.build_labels / trainer.step / GraphedStep.step;
aug: host int32 [B, 3] = (dx, dy, flip) per image; bbox_per_batch / label_per_batch: host lists as the reference returns
them; batch_idx: the dataset indices of the batch."""

# the plan of one batch, all host side: dataset indices, per-image (dx, dy, flip), the reference's box / label lists
Plan = namedtuple("Plan", ["batch_idx", "aug", "bbox_per_batch", "label_per_batch"])


class BatchReader:
    """``BatchReader(mc, images, rois, seed=0, device=None, dtype=torch.float32, resident=False)``

    images: list of uint8 [H, W, 3] BGR arrays (as cv2.imread delivers; any sizes).  rois: per image a list of
    [cx, cy, w, h, cls] in original pixels (kitti._rois, dataset/kitti.py:50-90).  resident=True uploads every image
    once and gathers each batch on the device by byte offset; otherwise each batch is packed into a pinned host buffer
    and copied asynchronously on the current stream.  mc supplies BATCH_SIZE, IMAGE_WIDTH / IMAGE_HEIGHT, BGR_MEANS and
    DATA_AUGMENTATION / DRIFT_X / DRIFT_Y.  The first shuffle is drawn here, as kitti.__init__ does."""

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
        the reference's order.  Advances the reader; needs no GPU."""
        mc = self.mc
        batch_idx = self._next_indices(shuffle)
        aug = np.zeros((len(batch_idx), 3), np.int32)
        label_per_batch, bbox_per_batch = [], []
        for k, idx in enumerate(batch_idx):
            orig_h, orig_w = [float(v) for v in self.sizes[idx]]
            roi = self.rois[idx]
            label_per_batch.append([b[4] for b in roi[:]])
            gt_bbox = np.array([[b[0], b[1], b[2], b[3]] for b in roi[:]]) if roi else np.zeros((0, 4))
            dx = dy = flip = 0
            if mc.DATA_AUGMENTATION:
                assert mc.DRIFT_X >= 0 and mc.DRIFT_Y > 0, 'mc.DRIFT_X and mc.DRIFT_Y must be >= 0'
                if mc.DRIFT_X > 0 or mc.DRIFT_Y > 0:
                    if len(gt_bbox):
                        # the drift never cuts a box (imdb.py:154-160); a float bound, which randint truncates
                        max_drift_x = min(gt_bbox[:, 0] - gt_bbox[:, 2] / 2.0 + 1)
                        max_drift_y = min(gt_bbox[:, 1] - gt_bbox[:, 3] / 2.0 + 1)
                        assert max_drift_x >= 0 and max_drift_y >= 0, 'bbox out of image'
                    else:                      # no boxes: the full range (the reference crashes here)
                        max_drift_x, max_drift_y = mc.DRIFT_X + 1, mc.DRIFT_Y + 1
                    dy = self.rs.randint(-mc.DRIFT_Y, min(mc.DRIFT_Y + 1, max_drift_y))
                    dx = self.rs.randint(-mc.DRIFT_X, min(mc.DRIFT_X + 1, max_drift_x))
                    gt_bbox[:, 0] = gt_bbox[:, 0] - dx
                    gt_bbox[:, 1] = gt_bbox[:, 1] - dy
                    orig_h -= dy
                    orig_w -= dx
                if self.rs.randint(2) > 0.5:
                    flip = 1
                    gt_bbox[:, 0] = orig_w - 1 - gt_bbox[:, 0]
            x_scale = mc.IMAGE_WIDTH / orig_w
            y_scale = mc.IMAGE_HEIGHT / orig_h
            gt_bbox[:, 0::2] = gt_bbox[:, 0::2] * x_scale
            gt_bbox[:, 1::2] = gt_bbox[:, 1::2] * y_scale
            bbox_per_batch.append(gt_bbox)
            aug[k] = (dx, dy, flip)
        return Plan(batch_idx, aug, bbox_per_batch, label_per_batch)

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
        """(flat device uint8 buffer, byte offset of each batch image in it)."""
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
            cap = int(np.sort(self.nbytes)[::-1][:max(1, self.mc.BATCH_SIZE)].sum())   # the largest possible batch
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

    def _warp(self, batch_idx, aug):
        from . import ops
        src, offsets = self._source(batch_idx)
        geom = np.concatenate([self.sizes[batch_idx], aug.astype(np.int64)], axis=1)   # src_h, src_w, dx, dy, flip
        return ops.augment_bgr(src, offsets, geom, self.mc.IMAGE_HEIGHT, self.mc.IMAGE_WIDTH, self.mc.BGR_MEANS, self.dtype)

    def read_batch(self, shuffle=True):
        """imdb.read_batch (imdb.py:100-190): the next batch as a Batch, image_input and ground truth on the device."""
        torch = self._torch()
        p = self.next_plan(shuffle)
        image_input = self._warp(p.batch_idx, p.aug)
        B, M = len(p.batch_idx), self.max_objects
        gt = np.zeros((B, M, 4), np.float64)
        cls = np.zeros((B, M), np.int32)
        cnt = np.zeros(B, np.int32)
        for k, (bb, lab) in enumerate(zip(p.bbox_per_batch, p.label_per_batch)):
            cnt[k] = len(lab)
            gt[k, :len(lab)] = bb
            cls[k, :len(lab)] = lab
        to = lambda a: torch.from_numpy(a).to(self.device, non_blocking=True)
        return Batch(image_input, to(gt), to(cls), to(cnt), p.aug, p.bbox_per_batch, p.label_per_batch, p.batch_idx)

    def read_image_batch(self, shuffle=True):
        """imdb.read_image_batch (imdb.py:63-98): the next batch's images only -- mean-subtracted, then resized, with no drift
        and no flip -- as (image_input on the device, [(x_scale, y_scale)] per image).  Draws nothing but the reshuffles."""
        self._torch()
        batch_idx = self._next_indices(shuffle)
        scales = []
        for idx in batch_idx:
            orig_h, orig_w = [float(v) for v in self.sizes[idx]]
            scales.append((self.mc.IMAGE_WIDTH / orig_w, self.mc.IMAGE_HEIGHT / orig_h))
        return self._warp(batch_idx, np.zeros((len(batch_idx), 3), np.int32)), scales
