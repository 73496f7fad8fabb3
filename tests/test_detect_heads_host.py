"""The inputs of tests/test_gpu_detect_heads.py, proven on the CPU oracle alone (tests/detect_head_cases.py): every condition
the GPU tests rely on -- the share of anchors left out of the exact class check, exact zeros of the padding classes, the
planted ties / thresholds / clips doing what they were planted for, and the filter cases keeping, spreading and suppressing
detections -- holds before a kernel ever sees them."""
import numpy as np
import pytest

from oracle import sqdet_oracle as O
from tests import detect_head_cases as H

HEADS = [(n, d) for n in H.DECODE_CASES for d in H.DTYPES]
EDGES = [(n, d) for n in ("voc23_edges", "c3_edges") for d in H.DTYPES]
ids = lambda p: "%s-%s" % p


def test_head_config_sets_the_head_and_distinct_anchors():
    for C, K, gh, gw in ((1, 9, 8, 16), (23, 1, 8, 16), (23, 10, 32, 64), (4, 6, 8, 16)):
        mc = H.head_config(C, K, gh, gw)
        assert (mc.CLASSES, mc.ANCHOR_PER_GRID, mc.ANCHORS) == (C, K, gh * gw * K) and mc.ANCHOR_BOX.shape == (gh * gw * K, 4)
        cell = mc.ANCHOR_BOX[:K]
        assert len({tuple(r) for r in cell}) == K and (cell[:, :2] == cell[0, :2]).all()
        np.testing.assert_array_equal(cell[:min(K, 9), 2:], np.array(O._SQDET_SHAPES)[:min(K, 9)])
    assert H.head_config(23, 10, 32, 64).ANCHORS == 20480 and H.head_config(23, 10, 3, 683).ANCHORS == 20490


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_constant_score_map_overflows_the_fast_filters_candidate_list(dtype):
    mc, preds = H.head_preds("voc23_constant", dtype)
    p = O.interpret_output(preds, mc)["det_probs"]
    assert mc.ANCHORS > 2048 and (p[1] == p[1, 0]).all() and len(np.unique(p[0])) > 2048      # FCAP (filter_body.h) is 2048


@pytest.mark.parametrize("case", HEADS, ids=ids)
def test_inputs_are_storage_values_and_nearly_every_class_is_decided(case):
    name, dtype = case
    mc, preds = H.head_preds(name, dtype)
    C, R, K, gh, gw, B, _ = H.HEAD_CASES[name]
    assert preds.shape == (B, gh, gw, K * (C + 5)) and preds.dtype == np.float32 and np.isfinite(preds).all()
    np.testing.assert_array_equal(preds, H.round_storage(preds, dtype))
    ref = H.head_reference(name, dtype)
    undecided = 1.0 - ref["decided"].mean()
    print("UNDECIDED %-12s %s: %.4f%% of %d anchors" % (name, dtype, 100 * undecided, ref["decided"].size))
    assert undecided <= 0.01
    assert np.isfinite(ref["det_boxes"]).all() and np.isfinite(ref["det_probs"]).all()
    r64 = H.decode_float64(mc, preds)                # the float64 restatement agrees with the float32 oracle to float32 rounding
    for key in r64:
        assert H.max_rel_error(ref[key], r64[key]) < 1e-5
    if C == 1:
        assert (ref["pred_class_probs"] == 1.0).all() and (ref["det_class"] == 0).all()


@pytest.mark.parametrize("case", [c for c in HEADS if H.HEAD_CASES[c[0]][0] == 23], ids=ids)
def test_padding_classes_have_probability_zero_and_never_win(case):
    ref = H.head_reference(*case)
    assert (ref["pred_class_probs"][..., 20:] == 0.0).all()
    assert (ref["det_class"] < 20).all() and (ref["det_probs"] > 0).all()


@pytest.mark.parametrize("case", EDGES, ids=ids)
def test_planted_values_do_what_they_were_planted_for(case):
    name, dtype = case
    mc, preds = H.head_preds(name, dtype)
    ref, plants = H.head_reference(name, dtype), H.head_plants(name, dtype)
    C, R, K = H.HEAD_CASES[name][:3]
    lg = H.class_logits(mc, preds)
    W1, H1 = mc.IMAGE_WIDTH - 1.0, mc.IMAGE_HEIGHT - 1.0
    # ties: bit-equal top logits, the rest >= 8 below, the oracle takes the lowest tied index
    lows = set()
    for b, a, T in plants["ties"]:
        v = lg[b, a, list(T)]
        others = np.delete(lg[b, a, :R], list(T))
        assert (v == v[0]).all() and (others <= v[0] - 8.0).all()
        assert ref["det_class"][b, a] == min(T) and ref["decided"][b, a]
        lows.add((len(T), min(T)))
    assert {(2, 0), (3, 0), (R, 0)} <= lows
    assert ({(2, 7), (2, 18), (3, 9), (3, 17)} if R == 20 else {(2, 1)}) <= lows     # a middle class, and as high as R allows
    # saturated
    assert len(plants["saturated"]) >= 12
    for b, a in plants["saturated"]:
        assert set(np.abs(lg[b, a, :R])) == {30.0}
        assert ref["pred_conf"][b, a] in (np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(s) * 20).astype(np.float32)) for s in (-1, 1))
    # thresholds: the side of EXP_THRESH each delta lands on, and safe_exp's branch there
    thr = np.float32(mc.EXP_THRESH)
    slope = np.float32(np.exp(mc.EXP_THRESH))
    kinds = {}
    for b, a, kind in plants["thresh"]:
        dx, dy, dw, dh = ref["pred_box_delta"][b, a]
        assert dx == 0 and dy == 0
        want = dict(at=(False, False), below=(False, False), below_w=(False, False), above=(True, True), above_8=(True, True), plus8=(True, True))[kind]
        assert (bool(dw > thr), bool(dh > thr)) == want
        if kind == "at":
            assert dw == thr and dh == thr
        if kind.startswith("below"):
            assert dw < thr and dw > thr - np.float32(2e-3)
        if kind.startswith("above"):
            assert dw > thr and dw < thr + np.float32(2e-3)
        for d in (dw, dh):
            e = O.safe_exp(np.array([d]), mc.EXP_THRESH)[0]
            assert e == (slope * (d - thr + np.float32(1.0)) if d > thr else np.exp(d).astype(np.float32))
        if kind != "plus8" and kind != "above_8":      # e * (36x37 or 72x43) stays inside the image: the width is the decoded one
            aw = np.float32(mc.ANCHOR_BOX[a, 2])
            assert abs(ref["det_boxes"][b, a, 2] - (aw * np.exp(np.float64(dw)) + 1.0)) < 0.01
        kinds[kind] = kinds.get(kind, 0) + 1
    assert set(kinds) == {"at", "below", "below_w", "above", "above_8", "plus8"}
    # clips
    sides = set()
    for b, a, side in plants["clip"]:
        cx, cy, w, h = ref["det_boxes"][b, a].astype(np.float64)
        xmin, ymin, xmax, ymax = cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w - 1.0, cy + 0.5 * h - 1.0
        ok = dict(left=abs(xmin) < 1e-3 and 1 < xmax < W1, right=abs(xmax - W1) < 1e-3 and 0 < xmin < W1 - 1,
                  top=abs(ymin) < 1e-3 and 1 < ymax < H1, bottom=abs(ymax - H1) < 1e-3 and 0 < ymin < H1 - 1,
                  out_right=w == 1.0 and abs(xmin - W1) < 1e-3, out_left=w == 1.0 and abs(xmin) < 1e-3,
                  out_bottom=h == 1.0 and abs(ymin - H1) < 1e-3, out_top=h == 1.0 and abs(ymin) < 1e-3)[side]
        assert ok, (side, b, a, ref["det_boxes"][b, a])
        sides.add(side)
    assert len(sides) == 8
    # the last real class
    assert sorted(b for b, _, _ in plants["last_class"]) == list(range(preds.shape[0]))
    for b, a, c in plants["last_class"]:
        assert c == R - 1 and ref["det_class"][b, a] == c and ref["decided"][b, a]


@pytest.mark.parametrize("name", list(H.FILTER_CASES))
def test_filter_cases_keep_spread_and_suppress(name):
    C, A, top_n, _ = H.FILTER_CASES[name]
    mc, boxes, probs, cls, bad = H.filter_case(name)
    rows = H.filter_reference(name)
    assert boxes.shape == (H.FILTER_B, A, 4) and mc.NMS_THRESH == 0.4 and mc.CLASSES == C
    for b in range(H.FILTER_B):
        oi, op, ob, oc, n = rows[b]
        cand = H.candidates(mc, probs[b])
        valid = int(((cls[b, cand] >= 0) & (cls[b, cand] < C)).sum())
        assert len(cand) == (top_n if top_n else int((probs[b] > 0.6).sum())) and len(cand) <= H.filter_max_out(name)
        assert n >= 1                                            # every image keeps a detection
        if C >= 20:
            assert len(set(oc[:n].tolist())) >= 8                # ... in at least 8 classes
        if len(cand) > 1:                                        # (M = 1: a lone candidate has nothing to be suppressed by)
            assert valid - n >= 1, "NMS suppresses nothing"
        else:
            assert name == "c4_a65_top1" and n == 1
        assert (oi[n:] == -1).all() and (oc[n:] == -1).all() and (op[n:] == 0).all() and (ob[n:] == 0).all()
        # class ascending, then descending prob (top-N branch) / ascending anchor (threshold branch)
        key = list(zip(oc[:n].tolist(), (-op[:n]).tolist() if top_n else oi[:n].tolist()))
        assert key == sorted(key)
        # the kernel's documented rule for classes outside [0, C): dropped, while still taking their place in the top-N
        assert (name in H.BAD_CLASS_CASES) == bool(bad[b])
        for a in bad[b]:
            assert a in cand and a not in oi[:n] and not 0 <= cls[b, a] < C
    if name.endswith("_ties"):
        cand = H.candidates(mc, probs[0])
        p = probs[0]
        assert (p == p[cand[-1]]).sum() > (p[cand] == p[cand[-1]]).sum() >= 1      # the top-N boundary cuts through a tie
        tied = cand[p[cand] == p[cand[-1]]]
        assert (np.diff(tied) < 0).all() and tied.min() > np.setdiff1d(np.nonzero(p == p[cand[-1]])[0], tied).max()
    if name == "c2_a300_top256":
        assert (A - 1) >> 16 == 0 and (A - 1) >> 8 != 0                                # index bytes 2 and 3 are zero, byte 1 is not
