"""The window / colour augmentation without a GPU: the restatement of sqdet_augment_bgr_window and its cases
(tests/augment_policy_cases.py) discriminate the mistakes such a kernel can make; BatchReader's host policy (squeezedet_amd/imdb.py:
ssd_window, window_boxes, color_matrix) obeys its rules, leaves the reference's draws alone when off and resumes bit for bit; the
host-side geometry validator of ops.augment_bgr_window rejects every bad row before anything is touched."""
import numpy as np
import pytest
import torch

from squeezedet_amd import BatchReader, _lib, imdb, ops
from tests import augment_policy_cases as AC
from tests import input_path_cases as IC


# ------------------------------------------------------------------ restatement and cases
def test_cases_hold_their_edges():
    assert len(AC.WIN_IMAGES) == 60 and {si for si, _, _, _ in AC.WIN_IMAGES} == {0, 1, 2}
    images, flat, offsets = AC.win_source()
    assert flat.size == sum(im.size for im in images) and images[-1].shape[:2] == (9, 7) and images[-1].size % 2 == 1
    for (h, w) in AC.SOURCES:
        W = AC.windows(h, w)
        x0, y0, cw, ch = W["inside"]
        assert x0 > 0 and y0 > 0 and x0 + cw < w and y0 + ch < h                     # strictly inside
        x0, y0, cw, ch = W["containing"]
        assert x0 < 0 and y0 < 0 and x0 + cw > w and y0 + ch > h                     # strictly containing
        assert W["left"][0] < 0 < W["left"][0] + W["left"][2] < w
        assert 0 < W["right"][0] < w < W["right"][0] + W["right"][2]
        assert W["top"][1] < 0 < W["top"][1] + W["top"][3] < h
        assert 0 < W["bottom"][1] < h < W["bottom"][1] + W["bottom"][3]
        assert W["1x1"][2:] == (1, 1) and W["cw=1"][2] == 1 and W["ch=1"][3] == 1
        assert W["outside"][0] >= w
    for hd, wd in IC.AUG_DSTS:
        ref, pad = AC.win_reference(hd, wd, "cross")
        for k, (si, name, win, fl) in enumerate(AC.WIN_IMAGES):
            assert (ref[k][pad[k]] == 0).all()
            if name == "outside":
                assert pad[k].all() and (ref[k] == 0).all()
            if name in ("inside", "1x1", "cw=1", "ch=1"):
                assert not pad[k].any()
            if name in ("containing", "left", "right", "top", "bottom"):
                assert 0 < pad[k].mean() < 1 or min(hd, wd) < 6
    # the colour cases: one saturates at both ends, one has negative and cross-channel gains and an offset
    px = AC.win_source()[0][0].reshape(-1, 3).astype(np.float32)
    sat = AC.apply_color(px, AC.SATURATE)
    assert (sat == 0).any() and (sat == 255).any() and ((sat > 0) & (sat < 255)).any()
    assert (AC.CROSS[:, :3] < 0).any() and (AC.CROSS[:, 3] != 0).all() and (AC.CROSS[~np.eye(3, 4, dtype=bool)][:6] != 0).any()


def test_drift_window_restates_the_drift():
    """The window (dx, dy, w - dx, h - dy) without a matrix is augment_restatement, bit for bit, on the drift cases."""
    images = IC.aug_source()[0]
    g7 = AC.drift_as_window(IC.aug_geom())
    for hd, wd in IC.AUG_DSTS[:2]:
        ref = IC.aug_reference(hd, wd)[0]
        for k, im in enumerate(images):
            if max(g7[k, 4], g7[k, 5]) > 1000:
                continue                                                            # (the 65535-pixel drifts: covered on the GPU)
            out = AC.window_restatement(im, tuple(g7[k, 2:6]), g7[k, 6], None, hd, wd)
            assert np.array_equal(out, ref[k]), k


def test_identity_matrix_is_no_matrix():
    for hd, wd in IC.AUG_DSTS:
        assert np.array_equal(AC.win_reference(hd, wd, "identity")[0].view(np.uint32), AC.win_reference(hd, wd, "null")[0].view(np.uint32))


@pytest.mark.parametrize("mutate", AC.MUTATIONS)
def test_cases_discriminate_the_wrong_variant(mutate):
    """Each wrong variant differs from the restatement on the case set -- by more than check_augment allows -- and exactly on
    the cases that can show it."""
    hd, wd = IC.AUG_DSTS[1]
    differs = {}
    for color in AC.COLORS:
        ref, pad = AC.win_reference(hd, wd, color)
        bad = AC.win_reference(hd, wd, color, mutate)[0]
        differs[color] = [k for k in range(len(ref)) if not np.array_equal(ref[k], bad[k])]
        for k in differs[color][:3]:
            with pytest.raises(AssertionError):
                IC.check_augment(np.array(bad[k]), ref[k], pad[k], what=mutate)
    names = lambda color: {AC.WIN_IMAGES[k][1] for k in differs[color]}
    if mutate == "color_after_interpolation":
        assert differs["saturate"] and differs["cross"]
    elif mutate == "offset_on_padding":
        assert not differs["null"] and not differs["identity"]
        assert {"containing", "left", "right", "top", "bottom", "outside"} <= names("cross")
        assert not names("cross") & {"inside", "1x1"}
    elif mutate == "no_clamp":
        assert not differs["null"] and not differs["identity"] and differs["saturate"] and differs["cross"]
    elif mutate == "image_border_taps":
        assert "inside" in names("null") and "inside" in names("cross")
    else:
        flipped = {AC.WIN_IMAGES[k][3] for k in differs["null"]}
        assert flipped == {1} and {"inside", "left", "right"} <= names("null")


# ------------------------------------------------------------------ policy
def _plans_equal(p, q):
    assert list(p.batch_idx) == list(q.batch_idx) and np.array_equal(p.aug, q.aug) and p.label_per_batch == q.label_per_batch
    assert all(np.array_equal(a, b) for a, b in zip(p.bbox_per_batch, q.bbox_per_batch))
    for a, b in ((p.window, q.window), (p.color, q.color), (p.canvas, q.canvas), (p.trial, q.trial)):
        assert (a is None) == (b is None) and (a is None or np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)))
    assert p.mode == q.mode


def test_options_off_draw_the_reference_sequence():
    import squeezedet_amd as S
    images, rois = AC.policy_dataset()
    rois = [r or [[20.0, 20.0, 10.0, 10.0, 0]] for r in rois]
    mc = S.kitti_squeezeDet_config_for_input(96, 160)
    mc.BATCH_SIZE, mc.DRIFT_X, mc.DRIFT_Y = 4, 12, 6
    assert mc.AUG_GEOMETRY == "drift" and mc.AUG_ZOOM_OUT_MAX == 1.0 and mc.AUG_COLOR is False
    old = type(mc)({k: v for k, v in mc.items() if not k.startswith("AUG_")})
    assert not any(k.startswith("AUG_") for k in old) and len(old) < len(mc)
    a, b = BatchReader(mc, images, rois, seed=5), BatchReader(old, images, rois, seed=5)
    for _ in range(50):
        p, q = a.next_plan(), b.next_plan()
        _plans_equal(p, q)
        assert p.window is None and p.color is None and p.mode is None
    assert np.array_equal(a.rs.get_state()[1], b.rs.get_state()[1])
    assert p.aug[:, :2].any() and len(p) == 9 and p._fields[:4] == ("batch_idx", "aug", "bbox_per_batch", "label_per_batch")


def test_ssd_windows_obey_their_mode():
    images, rois = AC.policy_dataset()
    mc = AC.policy_config()
    r = BatchReader(mc, images, rois, seed=11)
    seen, accepted, fallbacks, zoomed = set(), 0, 0, 0
    for _ in range(50):
        p = r.next_plan()
        assert p.window.shape == (4, 4) and p.color.shape == (4, 12) and p.color.dtype == np.float32
        for k, idx in enumerate(p.batch_idx):
            h, w = images[idx].shape[:2]
            boxes = np.array([b[:4] for b in rois[idx]]).reshape(-1, 4)
            x0, y0, cw, ch = [int(v) for v in p.window[k]]
            cx0, cy0, Wc, Hc = [int(v) for v in p.canvas[k]]
            mode, flip = p.mode[k], int(p.aug[k, 2])
            seen.add(mode)
            assert tuple(p.aug[k, :2]) == (x0, y0) and flip in (0, 1)
            # the canvas holds the image and is at most AUG_ZOOM_OUT_MAX times it
            assert cx0 <= 0 and cy0 <= 0 and cx0 + Wc >= w and cy0 + Hc >= h and w <= Wc <= 2 * w and h <= Hc <= 2 * h
            zoomed += (Wc, Hc) != (w, h)
            if mode == "whole" or p.trial[k] == 0:
                assert (x0, y0, cw, ch) == (cx0, cy0, Wc, Hc)
                fallbacks += mode != "whole"
            else:
                accepted += 1
                assert 1 <= p.trial[k] <= 50
                assert cx0 <= x0 and cy0 <= y0 and x0 + cw <= cx0 + Wc and y0 + ch <= cy0 + Hc
                assert int(0.3 * Wc) <= cw <= Wc and int(0.3 * Hc) <= ch <= Hc
                assert 0.5 <= (cw / float(Wc)) / (ch / float(Hc)) <= 2.0
                if len(boxes):
                    inside = (boxes[:, 0] >= x0) & (boxes[:, 0] <= x0 + cw - 1) & (boxes[:, 1] >= y0) & (boxes[:, 1] <= y0 + ch - 1)
                    assert inside.any()
                    if mode != "any":
                        assert _iou_xyxy((x0, y0, x0 + cw - 1.0, y0 + ch - 1.0), boxes).max() >= mode
            # the kept boxes, restated: centre inside, shifted, clipped, mirrored, scaled
            want_boxes, want_labels = [], []
            for bx, by, bw, bh, c in rois[idx]:
                if x0 <= bx <= x0 + cw - 1 and y0 <= by <= y0 + ch - 1:
                    x1, x2 = [min(max(v - x0, 0.0), cw - 1.0) for v in (bx - bw / 2.0, bx + bw / 2.0)]
                    y1, y2 = [min(max(v - y0, 0.0), ch - 1.0) for v in (by - bh / 2.0, by + bh / 2.0)]
                    ccx = (x1 + x2) / 2.0
                    ccx = cw - 1 - ccx if flip else ccx
                    sx, sy = mc.IMAGE_WIDTH / float(cw), mc.IMAGE_HEIGHT / float(ch)
                    want_boxes.append([ccx * sx, (y1 + y2) / 2.0 * sy, (x2 - x1) * sx, (y2 - y1) * sy])
                    want_labels.append(c)
            got = p.bbox_per_batch[k]
            assert np.array_equal(got, np.array(want_boxes).reshape(-1, 4)) and p.label_per_batch[k] == want_labels
            assert len(got) >= (1 if rois[idx] else 0) and len(got) <= r.max_objects
            if len(got):
                assert (got[:, 0] - got[:, 2] / 2 >= -1e-9).all() and (got[:, 0] + got[:, 2] / 2 <= mc.IMAGE_WIDTH * (cw - 1.0) / cw + 1e-9).all()
                assert (got[:, 1] - got[:, 3] / 2 >= -1e-9).all() and (got[:, 1] + got[:, 3] / 2 <= mc.IMAGE_HEIGHT * (ch - 1.0) / ch + 1e-9).all()
                assert (got[:, 0] >= 0).all() and (got[:, 0] <= mc.IMAGE_WIDTH).all()
    assert seen == set(imdb.CROP_MODES) and accepted > 50 and zoomed > 20
    print("ssd windows: %d accepted trials, %d fallbacks to the canvas, %d zoomed out of 200" % (accepted, fallbacks, zoomed))


def _iou_xyxy(win, boxes):
    """A plain IoU written for the test: window corners against [cx, cy, w, h] boxes."""
    out = []
    for cx, cy, bw, bh in boxes:
        b = (cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2)
        iw, ih = min(win[2], b[2]) - max(win[0], b[0]), min(win[3], b[3]) - max(win[1], b[1])
        inter = max(iw, 0.0) * max(ih, 0.0)
        out.append(inter / ((win[2] - win[0]) * (win[3] - win[1]) + bw * bh - inter))
    return np.array(out)


def test_fifty_failures_fall_back_to_the_canvas():
    mc = AC.policy_config(zoom=1.0)
    tiny = np.array([[150.0, 100.0, 4.0, 4.0]])
    rs = np.random.RandomState(3)
    win, canvas, mode, trial = imdb.ssd_window(rs, mc, 300, 200, tiny, mode=0.9)
    assert win == canvas == (0, 0, 300, 200) and mode == 0.9 and trial == 0
    # 50 trials were made: the generator stands where 50 trials' draws leave it (2 per trial, 2 more where the aspect passed)
    rs2, positions = np.random.RandomState(3), 0
    for _ in range(50):
        cw, ch = max(1, int(rs2.uniform(0.3, 1.0) * 300)), max(1, int(rs2.uniform(0.3, 1.0) * 200))
        if 0.5 <= (cw / 300.0) / (ch / 200.0) <= 2.0:
            positions += 1
            rs2.randint(0, 300 - cw + 1), rs2.randint(0, 200 - ch + 1)
    assert positions > 10 and np.array_equal(rs.get_state()[1], rs2.get_state()[1]) and rs.get_state()[2] == rs2.get_state()[2]
    # the same image under "any" accepts a trial, and a box-less image accepts the first trial whose aspect passes
    assert imdb.ssd_window(np.random.RandomState(3), mc, 300, 200, tiny, mode="any")[3] > 0
    assert imdb.ssd_window(np.random.RandomState(3), mc, 300, 200, np.zeros((0, 4)), mode=0.9)[3] > 0
    keep, kept = imdb.window_boxes(win, tiny)
    assert keep.all() and np.array_equal(kept, tiny)


def test_state_dict_resumes_to_identical_plans():
    images, rois = AC.policy_dataset()
    a = BatchReader(AC.policy_config(), images, rois, seed=2)
    for _ in range(7):
        a.next_plan()
    state = a.state_dict()
    want = [a.next_plan() for _ in range(10)]
    b = BatchReader(AC.policy_config(), images, rois, seed=99)
    b.load_state_dict(state)
    for p in want:
        q = b.next_plan()
        _plans_equal(p, q)
        assert q.color is not None and q.window is not None
    assert any((p.color != np.tile(AC.IDENTITY.reshape(12), (4, 1))).any() for p in want)


def test_color_jitter_alone_keeps_the_drift():
    """AUG_COLOR with the reference's geometry: the drift as a window, colour draws behind each image's flip."""
    images, rois = AC.policy_dataset()
    rois = [r or [[20.0, 20.0, 10.0, 10.0, 0]] for r in rois]
    p = BatchReader(AC.policy_config(geometry="drift", zoom=1.0), images, rois, seed=4).next_plan()
    for k, idx in enumerate(p.batch_idx):
        h, w = images[idx].shape[:2]
        dx, dy = int(p.aug[k, 0]), int(p.aug[k, 1])
        assert tuple(p.window[k]) == (dx, dy, w - dx, h - dy) and p.mode[k] == "drift"
    assert p.color.shape == (4, 12)


# ------------------------------------------------------------------ colour composition
def test_color_composition():
    assert np.array_equal(imdb.color_matrix(), np.eye(3, 4))
    assert np.array_equal(imdb.color_matrix().astype(np.float32), AC.IDENTITY)
    px = np.array([[0.0, 0.0, 0.0], [255.0, 255.0, 255.0], [12.0, 200.0, 97.0], [250.0, 3.0, 128.0]])          # (b, g, r)
    h = np.concatenate([px, np.ones((4, 1))], 1)
    apply = lambda M: h @ M.T
    np.testing.assert_allclose(apply(imdb.color_matrix(brightness=-21.5)), px - 21.5, rtol=0, atol=1e-12)
    np.testing.assert_allclose(apply(imdb.color_matrix(contrast=1.3)), px * 1.3, rtol=0, atol=1e-12)
    luma = (0.114 * px[:, 0] + 0.587 * px[:, 1] + 0.299 * px[:, 2])[:, None]
    np.testing.assert_allclose(apply(imdb.color_matrix(saturation=0.6)), luma + 0.6 * (px - luma), rtol=0, atol=1e-10)
    # hue: rotate (I, Q) of YIQ by 15 degrees, written out per pixel on (r, g, b)
    t = np.deg2rad(15.0)
    A = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]])
    want = []
    for b, g, r in px:
        y, i, q = A @ np.array([r, g, b])
        r2, g2, b2 = np.linalg.solve(A, np.array([y, i * np.cos(t) - q * np.sin(t), i * np.sin(t) + q * np.cos(t)]))
        want.append([b2, g2, r2])
    np.testing.assert_allclose(apply(imdb.color_matrix(hue_degrees=15.0)), np.array(want), rtol=0, atol=1e-9)
    grey = apply(imdb.color_matrix(hue_degrees=-18.0))[1]
    np.testing.assert_allclose(grey, [255.0] * 3, rtol=0, atol=1e-9)                  # a grey pixel has no hue to turn
    # the fixed order: brightness, then contrast, then saturation, then hue
    M = imdb.color_matrix(10.0, 1.2, 0.7, 9.0)
    step = px + 10.0
    step = step * 1.2
    l2 = (0.114 * step[:, 0] + 0.587 * step[:, 1] + 0.299 * step[:, 2])[:, None]
    step = l2 + 0.7 * (step - l2)
    step = np.concatenate([step, np.ones((4, 1))], 1) @ imdb.color_matrix(hue_degrees=9.0).T
    np.testing.assert_allclose(apply(M), step, rtol=0, atol=1e-9)
    # the draws: per factor a coin, then its value; all four coins 0 -> the exact identity, rounded to float32
    class Coins:
        def __init__(self, coins):
            self.coins, self.values = list(coins), []

        def randint(self, n):
            return self.coins.pop(0)

        def uniform(self, lo, hi):
            self.values.append((lo, hi))
            return (lo + hi) / 2.0 + 0.25 * (hi - lo)
    mc = AC.policy_config()
    off = Coins([0, 0, 0, 0])
    assert imdb.draw_color_factors(off, mc) == (None,) * 4 and not off.values
    assert np.array_equal(imdb.draw_color_matrix(Coins([0, 0, 0, 0]), mc), AC.IDENTITY.reshape(12))
    on = Coins([1, 1, 1, 1])
    assert imdb.draw_color_factors(on, mc) == (16.0, 1.25, 1.25, 9.0)
    assert on.values == [(-32.0, 32.0), (0.5, 1.5), (0.5, 1.5), (-18.0, 18.0)]
    m = imdb.draw_color_matrix(Coins([0, 1, 0, 0]), mc)
    assert m.dtype == np.float32 and np.array_equal(m.reshape(3, 4), (np.eye(3, 4) * 1.25).astype(np.float32))


# ------------------------------------------------------------------ the geometry validator
@pytest.mark.parametrize("bad", ["x0>65535", "x0<-65535", "y0>65535", "y0<-65535", "cw=0", "cw=65536", "ch=0", "ch=65536", "flip=2",
                                 "flip=-1", "past_end", "neg_offset"])
def test_validator_rejects_before_anything_is_touched(bad):
    geom = np.array([[20, 30, 2, -1, 28, 21, 0], [20, 30, -3, 4, 40, 9, 1]])
    offsets = np.array([0, 1800])
    col, val = {"x0>65535": (2, 65536), "x0<-65535": (2, -65536), "y0>65535": (3, 65536), "y0<-65535": (3, -65536), "cw=0": (4, 0),
                "cw=65536": (4, 65536), "ch=0": (5, 0), "ch=65536": (5, 65536), "flip=2": (6, 2), "flip=-1": (6, -1)}.get(bad, (None, None))
    if col is not None:
        geom[1, col] = val
    elif bad == "past_end":
        offsets = offsets + 1
    else:
        offsets = offsets - 1
    src = torch.zeros(3600, dtype=torch.uint8)
    out = torch.full((2, 16, 24, 3), 1234.5)
    with pytest.raises(_lib.SqdetError, match="bad geometry"):
        ops.augment_bgr_window(src, offsets, geom, None, 16, 24, IC.MEANS, torch.float32, out=out)
    assert bool((out == 1234.5).all())
    with pytest.raises(_lib.SqdetError, match="bad geometry"):
        ops.check_augment_window_geometry(geom, offsets, 3600, np.tile(AC.IDENTITY.reshape(12), (2, 1)))


def test_validator_accepts_the_extremes_and_checks_the_matrices():
    geom = np.array([[20, 30, 65535, -65535, 65535, 1, 1], [20, 30, -65535, 65535, 1, 65535, 0]])
    g, o, c = ops.check_augment_window_geometry(geom, [0, 1800], 3600, np.tile(AC.CROSS.reshape(12), (2, 1)))
    assert g.dtype == np.int32 and o.dtype == np.int64 and c.dtype == np.float32 and c.shape == (2, 12)
    assert ops.check_augment_window_geometry(geom, [0, 1800], 3600)[2] is None
    # above 65535 only a drift's own window (it ends at the image's far edge), which ops.augment_bgr accepts as (dx, dy)
    drift = AC.drift_as_window([[5, 11, 0, -65535, 1], [9, 7, -65535, 0, 0]])
    assert drift[:, 4:6].max() == 65542 and ops.check_augment_window_geometry(drift, [0, 165], 3600)[0].tolist() == drift.tolist()
    for col in (4, 5):
        off_by_one = drift.copy()
        off_by_one[5 - col, col] += 1
        with pytest.raises(_lib.SqdetError, match="bad geometry"):
            ops.check_augment_window_geometry(off_by_one, [0, 165], 3600)
    for bad in (np.zeros((1, 12)), np.full((2, 12), np.nan)):
        with pytest.raises(_lib.SqdetError, match="color"):
            ops.check_augment_window_geometry(geom, [0, 1800], 3600, bad)
