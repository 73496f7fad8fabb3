"""sqdet_augment_bgr (csrc/augment.hip) and BatchReader on the GPU: the kernel against the NumPy restatement of
imdb.py:141-186 on hand-picked geometry, the reader against the reference's own read_batch (tests/golden/augment.npz),
resident against packed, DATA_AUGMENTATION = False, rejected calls, and a short GraphedStep training run on reader
batches."""
import numpy as np
import pytest
import torch

from squeezedet_amd import _lib
from tests.test_augment_host import augment_reference, golden, label_case, pixel_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEANS = np.array([[[103.939, 116.779, 123.68]]])
KITTI_SIZES = [(370, 1224), (374, 1238), (376, 1241), (375, 1242)]


def _pack(images):
    offsets = np.concatenate([[0], np.cumsum([im.size for im in images])[:-1]]).astype(np.int64)
    flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(DEV)
    return flat, offsets


def _geometry_cases(D=(40, 20)):
    """(dx, dy, flip) per image: dx, dy each in {-D, -1, 0, 1, largest allowed (here the drift bound D)}, both flips."""
    vals_x, vals_y = [-D[0], -1, 0, 1, D[0]], [-D[1], -1, 0, 1, D[1]]
    return [(vals_x[i % 5], vals_y[(i * 2 + i // 5) % 5], i % 2) for i in range(10)]


def _check(out, ref, f16=False):
    if f16:
        assert np.abs(out - ref).max() <= 0.07
    else:
        assert np.abs(out - ref).max() <= 2e-4
        assert (out == ref).mean() >= 0.999


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("layout", ["packed", "resident"])
def test_kernel_matches_restatement(dtype, layout):
    """All four KITTI sizes in one batch, each with its own drift / flip, into the 384x1248 network input; packed (the
    batch's images back to back) or resident (a dataset buffer, gathered by offset in another order)."""
    from squeezedet_amd import ops
    rs = np.random.RandomState(3)
    geo = _geometry_cases()
    sizes = [KITTI_SIZES[i % 4] for i in range(len(geo))]
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in sizes]
    if layout == "packed":
        flat, offsets = _pack(images)
        order = list(range(len(images)))
    else:
        order = list(rs.permutation(len(images)))
        flat, all_off = _pack([images[i] for i in order][::-1])      # stored in another order than read
        offsets = all_off[::-1]
    geom = np.array([[sizes[i][0], sizes[i][1], geo[i][0], geo[i][1], geo[i][2]] for i in order])
    out = ops.augment_bgr(flat, offsets, geom, 384, 1248, MEANS, dtype).float().cpu().numpy()
    for k, i in enumerate(order):
        _check(out[k], augment_reference(images[i], geo[i][0], geo[i][1], geo[i][2], 384, 1248, MEANS), dtype == torch.float16)


def test_kernel_small_and_odd_sizes():
    """Down- and up-scaling, odd widths, the largest drift that leaves one row / column, and an image that ends the buffer."""
    from squeezedet_amd import ops
    rs = np.random.RandomState(4)
    cases = [((37, 53), (5, 3, 1)), ((37, 53), (52, 36, 0)), ((37, 53), (-30, -20, 1)), ((9, 7), (6, 8, 1)), ((61, 201), (-1, 1, 0))]
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s, _ in cases]
    flat, offsets = _pack(images)
    for hd, wd in ((96, 160), (24, 40), (5, 3)):
        geom = np.array([[s[0], s[1]] + list(g) for s, g in cases])
        out = ops.augment_bgr(flat, offsets, geom, hd, wd, MEANS, torch.float32).cpu().numpy()
        for k, (s, g) in enumerate(cases):
            _check(out[k], augment_reference(images[k], g[0], g[1], g[2], hd, wd, MEANS))


def test_reader_matches_reference_pixels():
    from squeezedet_amd import BatchReader, ops
    g = golden()
    mc, images, rois, seed = pixel_case(g)
    for resident in (False, True):
        b = BatchReader(mc, images, rois, seed=seed, device=DEV, resident=resident).read_batch()
        assert b.batch_idx == g["px_batch_idx"].tolist()
        _check(b.image_input.cpu().numpy(), g["px_pixels"])
        assert np.array_equal(np.array(b.bbox_per_batch), g["px_bbox"])
        assert np.array_equal(b.gt_boxes.cpu().numpy(), g["px_bbox"]) and b.gt_counts.tolist() == [2] * 4
    # labels: the full config, three shuffled batches, anchor assignment + deltas on the GPU
    mc, images, rois, seed = label_case(g)
    r = BatchReader(mc, images, rois, seed=seed, device=DEV, resident=True)
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(DEV)
    for k in range(3):
        b = r.read_batch()
        assert b.batch_idx == g["lb%d_batch_idx" % k].tolist()
        n = b.gt_counts.cpu().numpy()
        gt = b.gt_boxes.cpu().numpy()
        want = g["lb%d_bbox" % k]
        for i in range(len(n)):
            assert np.array_equal(gt[i, :n[i]], want[i, :n[i]])
        mask, delta, box, lab, aidx = ops.build_labels(anchors, b.gt_boxes, b.gt_classes, b.gt_counts, mc.CLASSES)
        aidx, ga = aidx.cpu().numpy(), g["lb%d_aidx" % k]
        delta, gd = delta.cpu().numpy(), g["lb%d_delta" % k]
        for i in range(len(n)):
            assert aidx[i, :n[i]].tolist() == ga[i, :n[i]].tolist()
            np.testing.assert_allclose(delta[i, aidx[i, :n[i]]], gd[i, :n[i]].astype(np.float32), rtol=0, atol=1e-6)


def _dataset(n=7, seed=8):
    rs = np.random.RandomState(seed)
    sizes = [KITTI_SIZES[i % 4] for i in range(n)]
    images = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in sizes]
    rois = []
    for h, w in sizes:
        k = rs.randint(0, 4)                                 # an image with no boxes included
        bw, bh = rs.uniform(30, 200, k), rs.uniform(30, 120, k)
        x0, y0 = rs.uniform(0, w - bw - 1), rs.uniform(0, h - bh - 1)
        rois.append([[x0[j] + bw[j] / 2, y0[j] + bh[j] / 2, bw[j], bh[j], int(rs.randint(3))] for j in range(k)])
    return images, rois


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_resident_equals_packed(dtype):
    import squeezedet_amd as S
    from squeezedet_amd import BatchReader
    mc = S.kitti_squeezeDet_config()
    mc.BATCH_SIZE = 3
    images, rois = _dataset()
    rp = BatchReader(mc, images, rois, seed=2, device=DEV, dtype=dtype)
    rr = BatchReader(mc, images, rois, seed=2, device=DEV, dtype=dtype, resident=True)
    for _ in range(5):                                       # across a reshuffle
        a, b = rp.read_batch(), rr.read_batch()
        assert a.batch_idx == b.batch_idx and np.array_equal(a.aug, b.aug)
        assert a.image_input.dtype == dtype and torch.equal(a.image_input, b.image_input)
        assert torch.equal(a.gt_boxes, b.gt_boxes) and torch.equal(a.gt_classes, b.gt_classes)
        assert torch.equal(a.gt_counts, b.gt_counts)
        for k, i in enumerate(a.batch_idx):
            dx, dy, fl = a.aug[k]
            _check(a.image_input[k].float().cpu().numpy(), augment_reference(images[i], dx, dy, fl, 384, 1248, mc.BGR_MEANS),
                   dtype == torch.float16)


def test_no_augmentation_and_read_image_batch():
    import squeezedet_amd as S
    from squeezedet_amd import BatchReader
    mc = S.kitti_squeezeDet_config()
    mc.BATCH_SIZE, mc.DATA_AUGMENTATION = 4, False
    images, rois = _dataset()
    b = BatchReader(mc, images, rois, seed=1, device=DEV).read_batch()
    assert (b.aug == 0).all()
    for k, i in enumerate(b.batch_idx):
        _check(b.image_input[k].cpu().numpy(), augment_reference(images[i], 0, 0, 0, 384, 1248, mc.BGR_MEANS))
    r = BatchReader(mc, images, rois, seed=1, device=DEV, resident=True)
    x, scales = r.read_image_batch(shuffle=False)
    assert len(scales) == 4 and scales[0] == (1248 / float(images[0].shape[1]), 384 / float(images[0].shape[0]))
    for k in range(4):
        _check(x[k].cpu().numpy(), augment_reference(images[k], 0, 0, 0, 384, 1248, mc.BGR_MEANS))


@pytest.mark.parametrize("bad", ["dx>=w", "dy>=h", "dx>65535", "dy<-65535", "flip=2", "past_end", "neg_offset", "dims"])
def test_rejected_calls_leave_dst_unchanged(bad):
    from squeezedet_amd import ops
    rs = np.random.RandomState(6)
    images = [rs.randint(0, 256, size=(20, 30, 3)).astype(np.uint8) for _ in range(2)]
    flat, offsets = _pack(images)
    geom = np.array([[20, 30, 2, -1, 0], [20, 30, -3, 4, 1]])
    hd, wd = 16, 24
    if bad == "dx>=w":
        geom[1, 2] = 30
    elif bad == "dy>=h":
        geom[0, 3] = 20
    elif bad == "dx>65535":
        geom[0, 2] = -70000
    elif bad == "dy<-65535":
        geom[1, 3] = -65536
    elif bad == "flip=2":
        geom[0, 4] = 2
    elif bad == "past_end":
        offsets = offsets + 1
    elif bad == "neg_offset":
        offsets = offsets - 1
    else:
        hd = 0
    out = torch.full((2, 16, 24, 3), 1234.5, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.SqdetError):
        ops.augment_bgr(flat, offsets, geom, hd, wd, MEANS, torch.float32, out=out)
    torch.cuda.synchronize()
    assert (out == 1234.5).all()


def test_graphed_training_on_reader_batches():
    """A few GraphedStep steps of SqueezeDetTrainer (128x256 input) on reader batches of images with planted, coloured
    boxes: the losses stay finite and fall."""
    import squeezedet_amd as S
    from oracle import sqdet_oracle as O
    from squeezedet_amd import BatchReader, nets
    from squeezedet_amd.train import GraphedStep, SqueezeDetTrainer
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    mc.LOAD_PRETRAINED_MODEL, mc.IS_TRAINING, mc.BATCH_SIZE = False, True, 4
    mc.DRIFT_X, mc.DRIFT_Y = 12, 6
    rs = np.random.RandomState(12)
    colours = np.array([[40, 40, 230], [40, 230, 40], [230, 40, 40]], np.uint8)
    images, rois = [], []
    for i in range(6):
        h, w = [(122, 250), (126, 254), (131, 262), (134, 266)][i % 4]
        im = rs.randint(90, 140, size=(h, w, 3)).astype(np.uint8)
        r = []
        for j in range(3):
            bw, bh = rs.uniform(30, 70), rs.uniform(25, 50)
            x0, y0 = rs.uniform(16, w - bw - 2), rs.uniform(8, h - bh - 2)
            c = int(rs.randint(3))
            im[int(y0):int(y0 + bh), int(x0):int(x0 + bw)] = colours[c]
            r.append([x0 + bw / 2, y0 + bh / 2, bw, bh, c])
        images.append(im)
        rois.append(r)
    m = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float32)
    m.load_params(O.init_params("squeezeDet", seed=3))
    tr = SqueezeDetTrainer(m)
    gs = GraphedStep(tr, torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(DEV), mc.CLASSES)
    reader = BatchReader(mc, images, rois, seed=4, device=DEV, resident=True)
    losses = []
    for _ in range(16):
        b = reader.read_batch()
        out = gs.step(b.image_input, b.gt_boxes, b.gt_classes, b.gt_counts)
        losses.append(sum(float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")))
    assert np.isfinite(losses).all()
    assert np.mean(losses[-4:]) < 0.8 * np.mean(losses[:4]), losses
