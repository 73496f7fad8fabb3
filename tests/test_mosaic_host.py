"""The mosaic augmentation without a GPU: that the cases of tests/mosaic_cases.py discriminate the mistakes a mosaic kernel can
make (on the NumPy restatement alone), BatchReader's mosaic policy (squeezedet_amd/imdb.py) -- off: today's plans byte for byte; on:
boxes, windows, zoom, resumable state, a hand-worked part, a geometric cross-check against the restated pixels -- and the host
validator ops.check_augment_mosaic_geometry."""
import copy
import pickle

import numpy as np
import pytest

from tests import augment_policy_cases as AC
from tests import mosaic_cases as MC

MOSAIC_FIELDS = ("AUG_MOSAIC_PROB", "AUG_MOSAIC_CENTER", "AUG_MOSAIC_ZOOM_MAX", "AUG_MOSAIC_MIN_BOX")


# ------------------------------------------------------------------------------------------------------------ the cases
def test_cases_cover_what_they_claim():
    assert MC.DSTS[:4] == [(7, 261), (12, 262), (7, 259), (12, 5)] and MC.DSTS[4] == (9, 520)
    assert MC.XCS(261) == [0, 1, 3, 4, 255, 256, 257, 260, 261] and MC.XCS(5) == [0, 1, 3, 4, 5] and MC.YCS(7) == [0, 1, 6, 7]
    for hd, wd in MC.DSTS:
        imgs = MC.mosaic_images(hd, wd)
        live = {tuple(part is not None for part in parts) for _, _, parts in imgs}
        for p in range(4):                                                        # all in one pane, for each of the four panes
            assert tuple(q == p for q in range(4)) in live, (hd, wd, p)
        assert (True,) * 4 in live
        used = {(part[0], part[1], part[3]) for _, _, parts in imgs for part in parts if part is not None}
        if wd > 5:
            assert {(si, name, fl) for si, name, _, fl in AC.WIN_IMAGES} <= used, "not every window x flip x source is shown"
        off, geom, split = MC.mosaic_arrays(hd, wd)
        name, s, parts = imgs[-1]
        assert name == "tail" and s[0] > 0 and s[1] > 0 and parts[3][0] == 2
        h, w = AC.SOURCES[2]
        assert off[-1, 3] + h * w * 3 == AC.win_source()[1].size, "the last source image must end exactly at src_bytes"
        for i, (_, _, parts) in enumerate(imgs):
            for p, part in enumerate(parts):
                assert (part is None) == (off[i, p] == MC.GARBAGE_OFFSET) == (tuple(geom[i, p]) == MC.GARBAGE_GEOM)
    assert any(2 * 256 < wd - xc for _, (xc, _), _ in MC.mosaic_images(9, 520) if xc > 0), "no right-hand pane spans three chunks"


def test_one_pane_is_the_window_restatement():
    sources = AC.win_source()[0]
    hd, wd = 7, 261
    part = AC.WIN_IMAGES[5]
    want = AC.window_restatement(sources[part[0]], part[2], part[3], AC.CROSS, hd, wd)
    for p, split in enumerate([(wd, hd), (0, hd), (wd, 0), (0, 0)]):
        parts = [part if q == p else None for q in range(4)]
        Ms = np.full((4, 3, 4), np.nan, np.float32)
        Ms[p] = AC.CROSS
        got = MC.mosaic_restatement(sources, parts, split, Ms, hd, wd)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), p


# a named case per mutation: (destination, colour, case)
CATCHES = {"seam_blend": ((7, 261), "cross", "xc=256,yc=1"),
           "pane_origin_off_by_one": ((9, 520), "null", "xc=257,yc=8"),
           "scale_from_full_size": ((7, 261), "mixed", "xc=256,yc=6"),
           "flip_in_output_coordinates": ((7, 261), "cross", "xc=257,yc=1"),
           "parts_swapped": ((12, 5), "null", "xc=3,yc=11"),
           "empty_pane_examined": ((7, 261), "cross", "xc=261,yc=7")}


@pytest.mark.parametrize("mutation", MC.MUTATIONS)
def test_a_named_case_catches_each_mutation(mutation):
    (hd, wd), color, name = CATCHES[mutation]
    names = [n for n, _, _ in MC.mosaic_images(hd, wd)]
    i = names.index(name)
    ref, _ = MC.mosaic_reference(hd, wd, color)
    mut, _ = MC.mosaic_reference(hd, wd, color, mutation)
    assert np.isfinite(ref).all(), "the restatement leaves no pixel unwritten"
    differs = ~((ref[i] == mut[i]) | (np.isnan(ref[i]) & np.isnan(mut[i])))
    assert differs.any(), "%s is not caught by %s -> %s %s" % (mutation, name, (hd, wd), color)
    caught = [n for k, n in enumerate(names) if not np.array_equal(ref[k], mut[k], equal_nan=True)]
    print("%s: caught by %d of %d cases of %s, %d elements of %s" % (mutation, len(caught), len(names), (hd, wd), differs.sum(), name))
    assert set(CATCHES) == set(MC.MUTATIONS)


# ---------------------------------------------------------------------------------------------------------- the policy
def _reader(mc, seed=5, n=9):
    import squeezedet_amd as S
    images, rois = AC.policy_dataset(n)
    return S.BatchReader(mc, images, rois, seed=seed), images, rois


def _mosaic_config(prob=1.0, color=True, geometry="ssd", batch=6):
    mc = AC.policy_config(geometry=geometry, color=color, batch=batch)
    mc.AUG_MOSAIC_PROB = prob
    return mc


def _same(a, b):
    return pickle.dumps(a) == pickle.dumps(b)


@pytest.mark.parametrize("geometry,color", [("drift", False), ("drift", True), ("ssd", False), ("ssd", True)])
def test_off_the_plans_are_todays(geometry, color):
    """AUG_MOSAIC_PROB = 0, a config without the fields and DATA_AUGMENTATION off with a probability set: the plans of a seeded
    reader, field by field and byte for byte, with the five new fields None."""
    import squeezedet_amd as S
    zero = AC.policy_config(geometry=geometry, color=color)
    assert zero.AUG_MOSAIC_PROB == 0.0 and zero.AUG_MOSAIC_CENTER == (0.3, 0.7) and zero.AUG_MOSAIC_ZOOM_MAX == 1.5 and zero.AUG_MOSAIC_MIN_BOX == 2.0
    without = copy.deepcopy(zero)
    for f in MOSAIC_FIELDS:
        del without[f]
    ra, rb = _reader(zero)[0], _reader(without)[0]
    assert ra.max_objects == rb.max_objects == 4
    for _ in range(5):
        pa, pb = ra.next_plan(), rb.next_plan()
        assert pa._fields == S.imdb.Plan._fields and _same(tuple(pa), tuple(pb))
        assert pa.split is None and pa.parts is None and pa.part_window is None and pa.part_flip is None and pa.part_color is None
        assert (pa.window is None) == (geometry == "drift" and not color)
    assert _same(ra.state_dict(), rb.state_dict())
    off, on = copy.deepcopy(zero), copy.deepcopy(zero)
    off.DATA_AUGMENTATION = on.DATA_AUGMENTATION = False
    on.AUG_MOSAIC_PROB = 1.0
    ra, rb = _reader(off)[0], _reader(on)[0]
    for _ in range(3):
        assert _same(tuple(ra.next_plan()), tuple(rb.next_plan()))


def test_a_failed_coin_keeps_the_images_own_policy():
    """prob just above 0: every coin fails, so beside the coin's own draw the policy runs as it does today and becomes part 0."""
    for geometry in ("drift", "ssd"):
        mc = _mosaic_config(prob=1e-300, geometry=geometry)
        r = _reader(mc)[0]
        for _ in range(3):
            p = r.next_plan()
            W, H = mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT
            assert (p.split == (W, H)).all() and (p.parts[:, 0] == p.batch_idx).all() and (p.parts[:, 1:] == -1).all()
            assert np.array_equal(p.part_window[:, 0], p.window) and np.array_equal(p.part_flip[:, 0], p.aug[:, 2])
            assert np.array_equal(p.part_color[:, 0], p.color) and "mosaic" not in p.mode
            assert np.array_equal(p.window[:, :2], p.aug[:, :2])


@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_on_boxes_windows_and_zoom(prob):
    mc = _mosaic_config(prob=prob)
    r, images, rois = _reader(mc)
    assert r.max_objects == 4 * max(len(x) for x in rois)
    W, H = mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT
    mosaics = plain = boxes_seen = 0
    for _ in range(12):
        p = r.next_plan()
        for k in range(len(p.batch_idx)):
            xc, yc = [int(v) for v in p.split[k]]
            if p.mode[k] != "mosaic":
                plain += 1
                assert (xc, yc) == (W, H)
                continue
            mosaics += 1
            assert int(0.3 * W) <= xc <= int(0.7 * W) and int(0.3 * H) <= yc <= int(0.7 * H)
            assert p.parts[k, 0] == p.batch_idx[k] and (p.parts[k] >= 0).all()
            bb, lab = p.bbox_per_batch[k], p.label_per_batch[k]
            assert len(bb) == len(lab) <= r.max_objects
            at = 0
            for q, (px0, py0, pw, ph) in enumerate(MC.panes(xc, yc, W, H)):
                h, w = images[p.parts[k, q]].shape[:2]
                x0, y0, cw, ch = [int(v) for v in p.part_window[k, q]]
                assert 0 <= x0 and x0 + cw <= w and 0 <= y0 and y0 + ch <= h and cw >= 1 and ch >= 1, "a window leaves its image"
                # cw = int(pw / z), ch = int(ph / z): z lies in (pw / (cw + 1), pw / cw] and in (ph / (ch + 1), ph / ch], so the two
                # zooms differ by less than the longer of these two intervals; and z is at least the zoom that fills the pane
                zx, zy = pw / float(cw), ph / float(ch)
                assert max(pw / (cw + 1.0), ph / (ch + 1.0)) < min(zx, zy) * (1 + 1e-12)
                assert abs(zx - zy) < max(pw / (cw * (cw + 1.0)), ph / (ch * (ch + 1.0))) + 1e-9
                assert min(zx, zy) >= max(pw / float(w), ph / float(h)) - 1e-9
                assert max(pw / (cw + 1.0), ph / (ch + 1.0)) < max(pw / float(w), ph / float(h)) * mc.AUG_MOSAIC_ZOOM_MAX + 1e-9
                # this pane's boxes: what mosaic_part_boxes gives for the part's rois, in order
                import squeezedet_amd as S
                roi = rois[p.parts[k, q]]
                gt = np.array([b[:4] for b in roi]) if roi else np.zeros((0, 4))
                keep, want = S.imdb.mosaic_part_boxes((x0, y0, cw, ch), int(p.part_flip[k, q]), (px0, py0, pw, ph), gt, mc.AUG_MOSAIC_MIN_BOX)
                got = bb[at:at + len(want)]
                assert np.array_equal(got, want) and lab[at:at + len(want)] == [b[4] for b, kp in zip(roi, keep) if kp]
                at += len(want)
                for cx, cy, bw, bh in got:
                    boxes_seen += 1
                    assert bw >= mc.AUG_MOSAIC_MIN_BOX and bh >= mc.AUG_MOSAIC_MIN_BOX
                    # (centre and size are rounded separately after the scaling: a corner clipped to the window's border comes back
                    # to within a few ulps of the pane's, 1e-13 at these sizes)
                    e = 1e-9
                    assert px0 - e <= cx - bw / 2 and cx + bw / 2 <= px0 + pw + e and py0 - e <= cy - bh / 2 and cy + bh / 2 <= py0 + ph + e, "a box leaves its pane"
            assert at == len(bb)
    assert mosaics > 0 and boxes_seen > 20 and (plain > 0) == (prob < 1.0)


def test_state_resumes_to_the_same_plans():
    mc = _mosaic_config(prob=0.5)
    a = _reader(mc, seed=11)[0]
    for _ in range(2):
        a.next_plan()
    b = _reader(mc, seed=99)[0]
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for _ in range(4):
        assert _same(tuple(a.next_plan()), tuple(b.next_plan()))


def test_a_hand_worked_part():
    """window (10, 20, 40, 30) mirrored into the 96 x 45 pane at (64, 0): scales 2.4 and 1.5.
    A (30, 35, 20, 10): corners 10..30 x 10..20 in the window -> centre (20, 15) -> mirrored 39 - 20 = 19 -> (45.6, 22.5, 48, 15)
      -> + (64, 0) = (109.6, 22.5, 48, 15);
    B (48, 48, 20, 1): corners 28..48 clipped to 28..39 x 27.5..28.5 -> (33.5, 28, 11, 1) -> mirrored 5.5 -> (13.2, 42, 26.4, 1.5):
      lower than 2, dropped;
    C (5, 30, 4, 4): its centre is left of the window, dropped."""
    import squeezedet_amd as S
    boxes = np.array([[30.0, 35.0, 20.0, 10.0], [48.0, 48.0, 20.0, 1.0], [5.0, 30.0, 4.0, 4.0]])
    keep, got = S.imdb.mosaic_part_boxes((10, 20, 40, 30), 1, (64, 0, 96, 45), boxes, 2.0)
    assert keep.tolist() == [True, False, False]
    assert got.shape == (1, 4) and np.allclose(got[0], [109.6, 22.5, 48.0, 15.0], rtol=1e-13, atol=0)
    keep, got = S.imdb.mosaic_part_boxes((10, 20, 40, 30), 0, (64, 0, 96, 45), boxes, 1.5)
    assert keep.tolist() == [True, True, False]
    assert np.allclose(got, [[64 + 20 * 2.4, 22.5, 48.0, 15.0], [64 + 33.5 * 2.4, 42.0, 26.4, 1.5]], rtol=1e-13, atol=0)


def test_boxes_enclose_their_pixels():
    """Every image holds ONE solid 255 rectangle on noise below 200, its roi the box of the rectangle's pixel centres.  In the
    restated output of a mosaic plan, the pixels of a pane that are solid (every tap inside the rectangle) lie inside that pane's
    transformed box to within one pixel, and reach its sides to within two source pixels."""
    import squeezedet_amd as S
    rs = np.random.RandomState(23)
    images, rois = [], []
    for i in range(8):
        h, w = AC.POLICY_SIZES[i % 4]
        im = rs.randint(0, 200, size=(h, w, 3)).astype(np.uint8)
        bw, bh = int(rs.randint(w // 3, w // 2)), int(rs.randint(h // 3, h // 2))
        x1, y1 = int(rs.randint(0, w - bw)), int(rs.randint(0, h - bh))
        im[y1:y1 + bh + 1, x1:x1 + bw + 1] = 255
        images.append(im)
        rois.append([[x1 + bw / 2.0, y1 + bh / 2.0, float(bw), float(bh), 1]])
    mc = _mosaic_config(prob=1.0, color=False)
    r = S.BatchReader(mc, images, rois, seed=2)
    W, H = mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT
    checked = 0
    for _ in range(3):
        p = r.next_plan()
        out = MC.plan_restatement(images, p, mc) + MC.MEANS.astype(np.float32)
        for k in range(len(p.batch_idx)):
            at = 0
            for q, (px0, py0, pw, ph) in enumerate(MC.panes(*[int(v) for v in p.split[k]], W, H)):
                _, n_kept = S.imdb.mosaic_part_boxes(p.part_window[k, q], int(p.part_flip[k, q]), (px0, py0, pw, ph),
                                                     np.array([rois[p.parts[k, q]][0][:4]]), mc.AUG_MOSAIC_MIN_BOX)
                ys, xs = np.nonzero((out[k, py0:py0 + ph, px0:px0 + pw] > 254.5).all(-1))
                if len(n_kept) == 0:
                    continue
                cx, cy, bw, bh = p.bbox_per_batch[k][at]
                at += 1
                if len(ys):
                    checked += 1
                    assert cx - bw / 2 - 1 <= px0 + xs.min() and px0 + xs.max() <= cx + bw / 2 + 1, (k, q)
                    assert cy - bh / 2 - 1 <= py0 + ys.min() and py0 + ys.max() <= cy + bh / 2 + 1, (k, q)
                    # ... and the box is no looser than that: the solid pixels reach to within two source pixels of its sides
                    slack = 2.0 * max(pw / float(p.part_window[k, q, 2]), ph / float(p.part_window[k, q, 3])) + 1
                    assert px0 + xs.min() <= cx - bw / 2 + slack and px0 + xs.max() >= cx + bw / 2 - slack, (k, q)
                    assert py0 + ys.min() <= cy - bh / 2 + slack and py0 + ys.max() >= cy + bh / 2 - slack, (k, q)
            assert at == len(p.bbox_per_batch[k])
    assert checked >= 20


def test_object_count_is_checked_at_construction():
    import squeezedet_amd as S
    images, rois = AC.policy_dataset()
    mc = _mosaic_config()
    rois = [list(x) for x in rois]
    rois[0] = [[10.0, 10.0, 4.0, 4.0, 0]] * 257                                   # 4 x 257 > 1024
    with pytest.raises(ValueError, match="mosaic"):
        S.BatchReader(mc, images, rois, seed=0)
    mc.AUG_MOSAIC_PROB = 0.0
    assert S.BatchReader(mc, images, rois, seed=0).max_objects == 257
    mc.AUG_MOSAIC_PROB = 1.5
    with pytest.raises(ValueError, match="AUG_MOSAIC_PROB"):
        S.BatchReader(mc, images, rois, seed=0)


# ------------------------------------------------------------------------------------------------------ the validator
def test_validator_accepts_the_cases_and_garbage_in_an_empty_pane():
    from squeezedet_amd import ops
    nbytes = AC.win_source()[1].size
    for hd, wd in MC.DSTS:
        off, geom, split = MC.mosaic_arrays(hd, wd)
        for color in MC.COLORS:
            o, g, s, c = ops.check_augment_mosaic_geometry(off, geom, split, nbytes, hd, wd, MC.color_with_garbage(color, hd, wd))
            assert o.dtype == np.int64 and g.dtype == np.int32 and s.dtype == np.int32 and o.shape == (len(s), 4) and g.shape == (len(s), 4, 7)
            live = off != MC.GARBAGE_OFFSET
            assert np.array_equal(o[live], off[live]) and np.array_equal(g[live], geom[live]) and np.array_equal(s, split)
            assert (o[~live] == 0).all() and (g[~live] == 0).all()
            assert (c is None) == (color == "null") and (c is None or (np.isfinite(c).all() and c.shape == (len(s), 4, 12)))


BAD = {"xc<0": ("split", (0, 0), -1), "xc>W": ("split", (0, 0), 262), "yc<0": ("split", (0, 1), -1), "yc>H": ("split", (0, 1), 8),
       "flip=2": ("geom", (0, 1, 6), 2), "cw=0": ("geom", (0, 2, 4), 0), "ch=0": ("geom", (0, 0, 5), 0), "src_h=0": ("geom", (0, 3, 0), 0),
       "x0 too far": ("geom", (0, 0, 2), 65536), "y0 too far": ("geom", (0, 0, 3), -65536), "cw too large": ("geom", (0, 1, 4), 65536),
       "offset<0": ("off", (0, 2), -1), "past the end": ("off", (0, 3), None), "nan matrix": ("color", (0, 1, 5), np.nan)}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_validator_rejects(bad):
    from squeezedet_amd import _lib, ops
    hd, wd = 7, 261
    nbytes = AC.win_source()[1].size
    part = AC.WIN_IMAGES[0]
    h, w = AC.SOURCES[part[0]]
    arrays = dict(off=np.zeros((2, 4), np.int64), geom=np.tile(np.array([h, w] + list(part[2]) + [0], np.int64), (2, 4, 1)),
                  split=np.array([[100, 3], [wd, hd]], np.int64), color=np.tile(AC.CROSS.reshape(12), (2, 4, 1)))
    ops.check_augment_mosaic_geometry(arrays["off"], arrays["geom"], arrays["split"], nbytes, hd, wd, arrays["color"])
    which, at, value = BAD[bad]
    arrays[which][at] = nbytes - h * w * 3 + 1 if value is None else value
    with pytest.raises(_lib.SqdetError, match="augment_bgr_mosaic"):
        ops.check_augment_mosaic_geometry(arrays["off"], arrays["geom"], arrays["split"], nbytes, hd, wd, arrays["color"])
    if which != "split":                                  # the same garbage in a pane without pixels is not looked at
        at2 = (1, 1 + at[1] % 3) + tuple(at[2:])
        arrays[which][at] = arrays[which][(1, 0) + tuple(at[2:])]
        arrays[which][at2] = nbytes if value is None else value
        ops.check_augment_mosaic_geometry(arrays["off"], arrays["geom"], arrays["split"], nbytes, hd, wd, arrays["color"])


def test_validator_rejects_wrong_shapes():
    from squeezedet_amd import _lib, ops
    with pytest.raises(_lib.SqdetError, match="augment_bgr_mosaic"):
        ops.check_augment_mosaic_geometry(np.zeros((2, 3)), np.zeros((2, 4, 7)), np.zeros((2, 2)), 100, 4, 4)
    with pytest.raises(_lib.SqdetError, match="augment_bgr_mosaic"):
        ops.check_augment_mosaic_geometry(np.zeros((0, 4)), np.zeros((0, 4, 7)), np.zeros((0, 2)), 100, 4, 4)
    with pytest.raises(_lib.SqdetError, match="augment_bgr_mosaic"):
        ops.check_augment_mosaic_geometry(np.zeros((1, 4)), np.zeros((1, 4, 7)), np.zeros((1, 2)), 100, 4, 4, np.zeros((1, 3, 12)))
