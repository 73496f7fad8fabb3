"""BatchReader's host half (batch order, random draws, box transform) against the reference's imdb.read_batch with data
augmentation on (tests/golden/augment.npz, made by tests/golden/make_augment_golden.py), and a NumPy restatement of the
pixel path against the reference's pixels.  No GPU."""
import os

import numpy as np
import pytest

from oracle import preproc_oracle as PO

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "augment.npz")
REFERENCE = "/root/reference"


def augment_reference(im_u8, dx, dy, flip, dst_h, dst_w, bgr_means):
    """imdb.py:141-186 for one image, in NumPy: mean subtraction in float64 rounded once to float32, drift with zero
    padding, mirror, cv2.resize (oracle.preproc_oracle.resize_linear)."""
    im = im_u8.astype(np.float32)
    im -= np.asarray(bgr_means, np.float64).reshape(1, 1, 3)
    h, w = im.shape[:2]
    d = np.zeros((h - dy, w - dx, 3), np.float32)
    d[max(-dy, 0):, max(-dx, 0):] = im[max(dy, 0):, max(dx, 0):]
    if flip:
        d = d[:, ::-1]
    return PO.resize_linear(d, dst_h, dst_w)


def golden():
    return np.load(GOLDEN)


def pixel_case(g):
    """(mc, images, rois, seed) of the fixture's pixel case, on this package's config."""
    import squeezedet_amd as S
    n_images, batch, width, height, drift_x, drift_y = [int(v) for v in g["px_params"]]
    mc = S.kitti_squeezeDet_config()
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.BATCH_SIZE = width, height, batch
    mc.DRIFT_X, mc.DRIFT_Y, mc.DATA_AUGMENTATION = drift_x, drift_y, True
    images, o = [], 0
    for h, w in g["px_sizes"]:
        images.append(g["px_images"][o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    rois = [[list(b) for b in r] for r in g["px_rois"]]
    return mc, images, rois, int(g["px_seed"])


def label_case(g):
    import squeezedet_amd as S
    mc = S.kitti_squeezeDet_config()
    images = [np.zeros((h, w, 3), np.uint8) for h, w in g["lb_sizes"]]
    rois = [[list(b) for b in r[:n]] for r, n in zip(g["lb_rois"], g["lb_counts"])]
    return mc, images, rois, int(g["lb_seed"])


def draws_of(aug):
    """The reference's randint results of a batch, per image (dy, dx, flip)."""
    return np.stack([aug[:, 1], aug[:, 0], aug[:, 2]], 1).reshape(-1).astype(np.float64)


def test_host_half_matches_reference_pixel_case():
    from squeezedet_amd import BatchReader
    g = golden()
    mc, images, rois, seed = pixel_case(g)
    p = BatchReader(mc, images, rois, seed=seed).next_plan()
    assert list(p.batch_idx) == g["px_batch_idx"].tolist()
    assert np.array_equal(draws_of(p.aug), g["px_draws"][:, 2])
    assert np.array_equal(np.array(p.bbox_per_batch), g["px_bbox"])
    assert p.label_per_batch == [[b[4] for b in rois[i]] for i in p.batch_idx]
    # the case covers a crop, a pad, a zero drift and both flips
    dx, dy, fl = p.aug.T
    assert ((dx > 0) | (dy > 0)).any() and ((dx < 0) | (dy < 0)).any() and ((dx == 0) | (dy == 0)).any()
    assert fl.any() and not fl.all()


def test_host_half_matches_reference_label_case():
    """Full kitti_squeezeDet_config, three shuffled batches: the reshuffle at cur + B >= len, the float max_drift bound,
    the draws and the float64 boxes, bit for bit."""
    from squeezedet_amd import BatchReader
    g = golden()
    mc, images, rois, seed = label_case(g)
    r = BatchReader(mc, images, rois, seed=seed)
    for k in range(3):
        p = r.next_plan()
        assert list(p.batch_idx) == g["lb%d_batch_idx" % k].tolist()
        assert np.array_equal(draws_of(p.aug), g["lb%d_draws" % k][:, 2])
        bb = g["lb%d_bbox" % k]
        for i, b in enumerate(p.bbox_per_batch):
            assert np.array_equal(b, bb[i, :len(b)])


def test_restatement_matches_reference_pixels():
    g = golden()
    mc, images, rois, seed = pixel_case(g)
    d = g["px_draws"][:, 2].reshape(-1, 3)
    for k, i in enumerate(g["px_batch_idx"]):
        out = augment_reference(images[i], int(d[k, 1]), int(d[k, 0]), d[k, 2] > 0.5, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS)
        assert np.array_equal(out, g["px_pixels"][k])


def test_no_augmentation_draws_nothing():
    from squeezedet_amd import BatchReader
    g = golden()
    mc, images, rois, seed = pixel_case(g)
    mc.DATA_AUGMENTATION = False
    r = BatchReader(mc, images, rois, seed=seed)
    state = r.rs.get_state()[1].copy()
    p = r.next_plan()
    assert (p.aug == 0).all() and np.array_equal(r.rs.get_state()[1], state)
    for b, i in zip(p.bbox_per_batch, p.batch_idx):
        h, w = images[i].shape[:2]
        want = np.array([bx[:4] for bx in rois[i]])
        want[:, 0::2] *= mc.IMAGE_WIDTH / float(w)
        want[:, 1::2] *= mc.IMAGE_HEIGHT / float(h)
        assert np.array_equal(b, want)


def test_image_without_boxes_uses_full_drift_range():
    from squeezedet_amd import BatchReader
    import squeezedet_amd as S
    mc = S.kitti_squeezeDet_config()
    mc.BATCH_SIZE, mc.DRIFT_X, mc.DRIFT_Y = 2, 3, 2
    images = [np.zeros((20, 30, 3), np.uint8) for _ in range(3)]
    r = BatchReader(mc, images, [[], [], []], seed=0)
    seen = np.concatenate([r.next_plan().aug for _ in range(200)])
    assert set(seen[:, 0]) == set(range(-3, 4)) and set(seen[:, 1]) == set(range(-2, 3))


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference tree is not mounted here")
def test_fixture_regenerates(tmp_path):
    """The reference, run again: the pixel case from scratch, the label case on the committed boxes."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_augment_golden", os.path.join(HERE, "golden", "make_augment_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    g = golden()
    ns = G.ref.load()
    out = {}
    G.pixel_case(ns, out)
    for k, v in out.items():
        assert np.array_equal(v, g[k], equal_nan=v.dtype.kind == "f"), k
    _, images, rois, seed = label_case(g)
    mc = ns.cfg_squeezeDet.kitti_squeezeDet_config()
    for k, (order, draws, labels, deltas, aidx, bboxes, _) in enumerate(G.run_reference(mc, images, rois, seed, 3)):
        assert order == g["lb%d_batch_idx" % k].tolist()
        assert np.array_equal(np.array(draws, np.float64), g["lb%d_draws" % k], equal_nan=True)
        for i in range(len(aidx)):
            n = len(aidx[i])
            assert np.array_equal(bboxes[i], g["lb%d_bbox" % k][i, :n])
            assert aidx[i] == g["lb%d_aidx" % k][i, :n].tolist()
            assert np.array_equal(np.asarray(deltas[i], np.float64), g["lb%d_delta" % k][i, :n])
