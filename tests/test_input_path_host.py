"""The cases, references and comparison functions of tests/test_gpu_input_path.py checked on their own: no GPU.

  * every label case of tests/input_path_cases.py reaches the branch it is named after in oracle.train_oracle.assign_anchors:
    the tie multiplicities, the clash counts and the distance-mode counts are pinned here, so that a later edit of a case cannot
    silently lose its edge;
  * labels.hip's decomposition (csrc/labels.hip lines 10-13: the best anchor ignoring the claims, the in-order resolve, the
    sweep over the free anchors only on a clash) restated in NumPy gives assign_anchors' picks on every case;
  * the mutation checks, in NumPy and never on a kernel: either tie rule reversed changes the picks of the cases built for it,
    a mirrored pixel pair left unswapped and a padding of -mean fail check_augment;
  * the augment cases reach every load and store branch of augment_kernel for each type and flip;
  * the LDS cap: 480000 anchors need exactly the 60000 bytes labels.hip allows, 480001 need 60004."""
import numpy as np
import pytest

from oracle import sqdet_oracle as O
from tests import input_path_cases as IC

# name: per image (boxes, clashes, distance-mode picks, picks tied in IoU, picks tied in distance) of the oracle's run
EXPECTED_STATS = {
    "dup": [(23, 3, 3, 20, 2), (7, 0, 0, 7, 0)],
    "mirror": [(4, 1, 1, 2, 1)],
    "full": [(273, 160, 38, 105, 5)],
    "far": [(40, 22, 40, 0, 21)],
    "cap": [(1024, 541, 80, 89, 0), (1024, 568, 62, 95, 0), (0, 0, 0, 0, 0)],
    "big": [(3, 1, 1, 0, 0)],
    "classes1": [(9, 1, 0, 3, 0), (9, 0, 0, 1, 0)],
    "classes20": [(9, 1, 0, 0, 0), (9, 1, 0, 1, 0)],
    "degenerate": [(3, 0, 1, 0, 0)],
    "three": [(3, 1, 1, 0, 0), (1, 0, 0, 0, 0)],
    "one": [(1, 0, 0, 0, 0), (0, 0, 0, 0, 0)],
}


def test_tables_are_dyadic_and_sized_as_named():
    sizes = {"S": 273, "S2": 546, "three": 3, "one": 1, "cap": 1080, "big": 480000}
    for name, A in sizes.items():
        t = IC.table(name)
        assert t.shape == (A, 4) and t.dtype == np.float64
        assert np.array_equal(t * 0.5, np.round(t * 0.5)) and np.abs(t).max() < 2 ** 15      # even integers: every product is exact
    assert 273 % 32 != 0 and 273 % 64 != 0 and 273 > 256 and 3 < 64
    assert np.array_equal(IC.table("S2")[273:], IC.table("S"))
    assert IC.table("S")[39].tolist() == [32.0, 64.0, 48.0, 32.0] and IC.table("S")[42].tolist() == [64.0, 64.0, 48.0, 32.0]
    assert IC.table("cap").shape[0] >= IC.LABELS_MAX_OBJECTS


@pytest.mark.parametrize("name", IC.LABEL_CASES)
def test_label_case_reaches_its_branch_and_two_pass_equals_the_oracle(name):
    c, ref, stats = IC.label_case(name), IC.label_reference(name), IC.label_stats(name)
    assert name in EXPECTED_STATS and len(stats) == len(c.cnt) == len(EXPECTED_STATS[name])
    for b, s in enumerate(stats):
        n = IC.clipped_count(c, b)
        assert s.picks == ref.aidx[b, :n].tolist(), "%s image %d: the two-pass restatement differs from assign_anchors" % (name, b)
        assert (ref.aidx[b, n:] == -1).all()
        assert (n, s.clashes, s.dist_mode, s.iou_ties, s.dist_ties) == EXPECTED_STATS[name][b], (name, b)
        assert int(ref.mask[b].sum()) == n
    assert c.gt.shape[1] <= len(c.anchors) and c.gt.shape[1] <= IC.LABELS_MAX_OBJECTS


def _iou(name, b, i):
    c = IC.label_case(name)
    return O.batch_iou(c.anchors, c.gt[b, i])


def test_dup_every_value_ties_across_the_two_copies():
    c, ref = IC.label_case("dup"), IC.label_reference("dup")
    s = IC.label_stats("dup")[0]
    for i in range(23):
        ov = _iou("dup", 0, i)
        assert np.array_equal(ov[:273], ov[273:])
        assert (ov == ov.max()).sum() > 1
    far = [12, 13, 14]
    assert all(_iou("dup", 0, i).max() == 0 for i in far) and np.array_equal(c.gt[0, 12], c.gt[0, 13])
    iou_picks = [ref.aidx[0, i] for i in range(23) if i not in far]
    # IoU picks land in the upper copy (a clash may push one down), distance picks: the lower copy, its twin, the next lower one
    assert sum(a >= 273 for a in iou_picks) >= 18 and s.dist_mode == 3
    a0, a1, a2 = (int(ref.aidx[0, i]) for i in far)
    assert a0 < 273 and a1 == a0 + 273 and a2 < 273 and a2 != a0


def test_mirror_picks():
    ref = IC.label_reference("mirror")
    assert ref.aidx[0].tolist() == IC.MIRROR_PICKS == [42, 43, 0, 39]
    ov = _iou("mirror", 0, 0)
    assert ov.max() == 0.5 and np.flatnonzero(ov == ov.max()).tolist() == [39, 42]            # two-way tie: the higher index
    ov = _iou("mirror", 0, 1)
    assert np.flatnonzero(ov == ov.max()).tolist() == [1, 4, 40, 43]                           # four-way tie
    c = IC.label_case("mirror")
    assert _iou("mirror", 0, 2).max() == 0
    d = IC._sqdist(c.anchors, c.gt[0, 2])
    assert np.flatnonzero(d == d.min()).tolist() == [0, 39]                                    # distance tie: the lower index
    assert np.array_equal(c.gt[0, 3], c.gt[0, 0])                                              # the clash takes the tie's runner-up


def test_full_cap_big_classes_degenerate_edges():
    c = IC.label_case("full")
    assert c.gt.shape[1] == len(c.anchors) == 273 and IC.label_reference("full").mask.sum() == 273     # every anchor claimed
    c = IC.label_case("cap")
    assert c.gt.shape[1] == 1024 and c.cnt.tolist() == [1024, 1030, -3]
    assert (IC.label_reference("cap").aidx[2] == -1).all() and (IC.label_reference("cap").aidx[:2] >= 0).all()
    c, ref = IC.label_case("big"), IC.label_reference("big")
    assert len(c.anchors) == 480000 and c.C == 1 and ref.aidx[0, 0] == 479999 and ref.aidx[0, 0] >> 5 == IC.labels_lds_bytes(480000) // 4 - 1
    assert np.array_equal(c.gt[0, 0], c.gt[0, 1]) and ref.aidx[0, 1] != 479999 and _iou("big", 0, 2).max() == 0
    for name, C in (("classes1", 1), ("classes20", 20)):
        c, ref = IC.label_case(name), IC.label_reference(name)
        out = (c.cls < 0) | (c.cls >= C)
        assert c.C == C and (c.cls == -1).any() and (c.cls == C).any() and out.sum() == 4
        for b, j in zip(*np.nonzero(out)):                       # mask, delta and box written, the label row all zero
            a = ref.aidx[b, j]
            assert ref.mask[b, a] == 1 and ref.box[b, a].any() and not ref.labels[b, a].any()
        assert ref.labels.sum() == 18 - 4
    c, ref = IC.label_case("degenerate"), IC.label_reference("degenerate")
    assert c.gt[0, 1, 2] == 0 and _iou("degenerate", 0, 1).max() == 0
    assert ref.delta64[0, ref.aidx[0, 1], 2] == -np.inf and np.isfinite(ref.delta64[0, ref.aidx[0, 1], [0, 1, 3]]).all()


def test_reversed_tie_rules_change_the_picks():
    """The mutation check of the tie rules: a kernel with either rule reversed cannot pass these cases."""
    for name in ("dup", "mirror", "full"):
        assert IC.label_stats(name, False, True)[0].picks != IC.label_stats(name)[0].picks, name
    for name in ("mirror", "far"):
        assert IC.label_stats(name, True, False)[0].picks != IC.label_stats(name)[0].picks, name


def test_lds_cap():
    assert IC.labels_lds_bytes(IC.BIG_A) == IC.LABELS_LDS_CAP == 60000
    assert IC.labels_lds_bytes(IC.BIG_A + 1) == 60004


# ------------------------------------------------------------------ augment
def test_augment_cases_hold_their_edges():
    images, flat, offsets = IC.aug_source()
    assert all(im.size % 2 == 1 for im in images if im.shape[:2] in ((37, 53), (9, 7), (5, 11)))
    g = IC.aug_geom()
    assert {(-65535, 0), (0, -65535)} <= {(int(r[2]), int(r[3])) for r in g}
    assert any(r[2] == r[1] - 1 and r[3] == r[0] - 1 for r in g)                 # one row, one column left
    assert all(((g[:, 2] == dx) & (g[:, 3] == dy) & (g[:, 4] == fl)).any() for _, dx, dy in IC.AUG_GEOMS for fl in (0, 1))
    assert [wd for _, wd in IC.AUG_DSTS] == [261, 262, 259, 5] and {hd for hd, _ in IC.AUG_DSTS} == {7, 12}
    for hd, wd in IC.AUG_DSTS:
        ref, pad = IC.aug_reference(hd, wd)
        assert pad.all(axis=(1, 2)).any() and (~pad).all(axis=(1, 2)).any()
        assert any(0 < p.mean() < 1 for p in pad)                                  # an image whose padding meets its pixels
        assert all((r[p] == 0).all() and (r[~p] != 0).all() for r, p in zip(ref, pad))


def test_augment_restatement_is_the_reference_and_the_check_accepts_it():
    images = IC.aug_source()[0]
    for hd, wd in IC.AUG_DSTS:
        ref, pad = IC.aug_reference(hd, wd)
        for k, (im, (_, dx, dy, fl)) in enumerate(zip(images, IC.AUG_IMAGES)):
            out = IC.augment_restatement(im, dx, dy, fl, hd, wd)
            assert np.array_equal(out, ref[k])
            assert IC.check_augment(out, ref[k], pad[k]) == 0.0
            assert IC.check_augment(out.astype(np.float16).astype(np.float32), ref[k], pad[k], f16=True) <= 1.0


def test_check_augment_rejects_wrong_outputs():
    images = IC.aug_source()[0]
    hd, wd = IC.AUG_DSTS[0]
    ref, pad = IC.aug_reference(hd, wd)
    k = IC.AUG_IMAGES.index(((37, 53), -30, -20, 1))
    im, (_, dx, dy, fl) = images[k], IC.AUG_IMAGES[k]
    for f16 in (False, True):
        h = (lambda a: a.astype(np.float16).astype(np.float32)) if f16 else (lambda a: a)
        with pytest.raises(AssertionError, match="error|equal"):                   # the mirrored pair left in memory order
            IC.check_augment(h(IC.augment_restatement(im, dx, dy, fl, hd, wd, swap_pair=False)), ref[k], pad[k], f16)
        with pytest.raises(AssertionError, match="padding elements are not 0"):    # padding = -mean
            IC.check_augment(h(IC.augment_restatement(im, dx, dy, fl, hd, wd, pad_with_zero=False)), ref[k], pad[k], f16)
    # what the flat 0.07 let through: a float16 padding pixel of 0.05, and a value off by 0.05
    bad = ref[k].copy()
    bad[pad[k]] = 0.05
    with pytest.raises(AssertionError, match="padding elements are not 0"):
        IC.check_augment(bad, ref[k], pad[k], f16=True)
    bad = ref[k].copy()
    bad[~pad[k]] += np.float32(0.05)
    with pytest.raises(AssertionError, match="float16 error"):
        IC.check_augment(bad, ref[k], pad[k], f16=True)
    assert IC.f16_bound(np.float32(0)) < 2.1e-4 and IC.f16_bound(np.float32(152)) < 0.075
    # an unwritten (NaN) cell
    bad = ref[k].copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        IC.check_augment(bad, ref[k], pad[k])


def test_augment_cases_reach_every_load_and_store_branch():
    _, flat, offsets = IC.aug_source()
    flips = np.array([fl for _, _, _, fl in IC.AUG_IMAGES])
    for esize in (4, 2):
        for fl in (0, 1):
            loads, end_of_buffer, stores = set(), False, set()
            for hd, wd in IC.AUG_DSTS:
                for k, (s, dx, dy, f) in enumerate(IC.AUG_IMAGES):
                    if f != fl:
                        continue
                    pair, tail = IC.load_pairs(s[0], s[1], dx, dy, f, hd, wd, int(offsets[k]), flat.size)
                    loads |= {"pair"} if pair.any() else set()
                    loads |= {"bytes"} if (~pair).any() else set()
                    end_of_buffer |= bool(tail.any())
                rows = np.concatenate([np.arange(hd) + k * hd for k in np.flatnonzero(flips == fl)])
                for off in IC.AUG_BASE_OFFSETS:
                    stores |= set(IC.store_classes(esize, wd, rows, off * esize))
            assert loads == {"pair", "bytes"}, (esize, fl, loads)
            assert stores == IC.STORE_CLASSES[esize], (esize, fl, stores)
            assert end_of_buffer == (fl == 1)                                      # the buffer's last image is a mirrored one
    # what the issue says of the widths, at an aligned base: float16 rows of 261 cycle through all three stores, float32 rows
    # alternate; float16 rows of 262 alternate 8-byte and 4-byte stores
    first = lambda esize, wd, row: next(iter(IC.store_classes(esize, wd, [row], 0).keys() - {"scalar_tail"}))
    assert [first(2, 261, r) for r in range(4)] == ["vector", "scalar_full", "h2", "scalar_full"]
    assert [first(4, 261, r) for r in range(4)] == ["vector", "scalar_full", "vector", "scalar_full"]
    assert [first(2, 262, r) for r in range(4)] == ["vector", "h2", "vector", "h2"]
    # one element past an aligned start: float16 is never 4-byte aligned, float32 swaps its rows
    assert set(IC.store_classes(2, 262, range(12), 2)) == {"scalar_full", "scalar_tail"}
    assert [first(4, 261, r) for r in range(2)] != [next(iter(IC.store_classes(4, 261, [r], 4).keys() - {"scalar_tail"})) for r in range(2)]
    assert all(wd > 256 and wd % 4 for _, wd in IC.AUG_DSTS[:3])                   # two workgroups per row, a partial last group
