"""Inputs for the decode (interpret_output) and filter (filter_prediction) kernels at heads other than KITTI's 9 x (3 + 5)
and at top-N settings other than 64 (test infrastructure, no GPU): shared by tests/test_detect_heads_host.py, which proves
on the oracle alone that every input has the properties the GPU tests rely on, and tests/test_gpu_detect_heads.py.

Heads: head_config / head_preds / head_plants / head_reference.  A case is used at float32 and at float16 STORAGE: the
values are rounded to the storage type here, and the same rounded values go to the kernel and to the oracle.
Filter inputs: filter_case / filter_reference (FILTER_CASES)."""
import functools
import itertools
import zlib

import numpy as np

from oracle import sqdet_oracle as O

IMG_H, IMG_W = 384, 1248          # every head here decodes into a KITTI-sized image (the grid is a free parameter)
PAD_LOGIT = -1.0e4                # a padding class (squeezedet_amd/config.py PAD_CLASS_BIAS): exp(-1e4 - max) == 0
UNDECIDED_REL = 1e-5              # top-2 score products closer than this (relative) are left out of the exact class check

# name: (C, real classes, K, gh, gw, B, planted)
HEAD_CASES = {
    "c1": (1, 1, 9, 8, 16, 3, False),
    "c2": (2, 2, 9, 8, 16, 3, False),
    "c4_k6": (4, 4, 6, 8, 16, 3, False),
    "c20": (20, 20, 9, 8, 16, 3, False),
    "voc23": (23, 20, 9, 8, 16, 3, False),
    "c23_k1": (23, 20, 1, 8, 16, 2, False),
    "voc23_edges": (23, 20, 9, 8, 16, 3, True),
    "c3_edges": (3, 3, 9, 8, 16, 3, True),
    # test_detect_filter_any_head only: all 20 register slots of the fast filter, and one grid it must refuse
    "voc23_k10_32x64": (23, 20, 10, 32, 64, 2, False),
    "voc23_k10_3x683": (23, 20, 10, 3, 683, 2, False),
    # a constant score map on image 1 of a 16x32 grid: all 4608 anchors tie, more than the fast filter's 2048 candidate
    # slots, so it falls back to its radix select
    "voc23_constant": (23, 20, 9, 16, 32, 2, False),
}
DECODE_CASES = ["c1", "c2", "c4_k6", "c20", "voc23", "c23_k1", "voc23_edges", "c3_edges"]
DTYPES = ["fp32", "fp16"]


def anchor_shapes(K):
    """The first K of the nine KITTI shapes; beyond nine they repeat scaled by 1.1, 1.2, ...: no two anchors of a cell are equal."""
    base = np.array(O._SQDET_SHAPES, np.float64)
    return [list(base[i % 9] * (1.0 + 0.1 * (i // 9))) for i in range(K)]


def head_config(C, K, gh, gw, img_h=IMG_H, img_w=IMG_W):
    mc = O.squeezeDet_config_for_input(img_h, img_w)
    mc.CLASSES = C
    mc.ANCHOR_PER_GRID = K
    mc.ANCHOR_BOX = O.set_anchors(mc, gh, gw, anchor_shapes(K))
    mc.ANCHORS = len(mc.ANCHOR_BOX)
    assert mc.ANCHORS == gh * gw * K
    return mc


def storage(dtype):
    return np.float16 if dtype == "fp16" else np.float32


def round_storage(a, dtype):
    return np.asarray(a, np.float32).astype(storage(dtype)).astype(np.float32)


def tie_sets(R):
    """Class sets whose logits are made bit-equal: 2 and 3 tied classes with the lowest tied index at 0, at a middle class and
    as high as R real classes allow (R-2 / R-3: no real class lies above R-1, which the 'last_class' plant covers), and all R."""
    if R >= 6:
        sets = [(0, R // 2 + 1), (R // 3 + 1, R - 1), (R - 2, R - 1),
                (0, R // 4, R - 1), (R // 2 - 1, R // 2, R - 5), (R - 3, R - 2, R - 1)]
    else:
        sets = list(itertools.combinations(range(R), 2)) + [s for s in itertools.combinations(range(R), 3) if len(s) < R]
    return sets + [tuple(range(R))]


@functools.lru_cache(maxsize=None)
def _build(name, dtype):
    C, R, K, gh, gw, B, planted = HEAD_CASES[name]
    mc = head_config(C, K, gh, gw)
    A = mc.ANCHORS
    rs = np.random.RandomState(zlib.crc32(name.encode()) % (2 ** 31))
    preds = (rs.randn(B, gh, gw, K * (C + 5)) * 1.7).astype(np.float32)
    pv = preds.reshape(B, gh * gw, K * (C + 5))
    logits = lambda b, a: pv[b, a // K, (a % K) * C:(a % K) * C + C]
    delta = lambda b, a: pv[b, a // K, K * (C + 1) + 4 * (a % K):K * (C + 1) + 4 * (a % K) + 4]
    if name == "voc23_constant":
        pv[1, :, :K * (C + 1)] = 0.25
    for k in range(K):
        pv[:, :, k * C + R:(k + 1) * C] = PAD_LOGIT
    preds[:] = round_storage(preds, dtype)
    plants = dict(ties=[], saturated=[], thresh=[], clip=[], last_class=[])
    if planted:
        st = storage(dtype)
        thr = st(mc.EXP_THRESH)
        up, dn = np.nextafter(thr, st(2)), np.nextafter(thr, st(0))       # one ulp of the STORAGE type either side
        assert float(up) > float(thr) > float(dn)
        interior = [c for c in range(gh * gw) if 2 <= c // gw < gh - 2 and 3 <= c % gw < gw - 3]
        free = [(b, c * K + k) for b in range(B) for c in interior for k in range(K)]
        order = rs.permutation(len(free))
        it = iter(free[i] for i in order)
        small = iter(free[i] for i in order[::-1] if free[i][1] % K in (0, 8))      # 36x37 / 72x43 anchors: e * shape fits the image
        # exact class ties: the tied logits are one storage value, the other real classes at least 8 below
        for T in tie_sets(R):
            for _ in range(2):
                b, a = next(it)
                top = float(round_storage(rs.uniform(-1.0, 3.0), dtype))
                lg = logits(b, a)
                lg[:R] = round_storage(top - 8.5 - np.abs(rs.randn(R)) * 2.0, dtype)
                lg[list(T)] = top
                plants["ties"].append((b, a, T))
        # saturated logits: classes +-30, confidence +-20
        for j in range(12):
            b, a = next(it)
            logits(b, a)[:R] = np.where(rs.uniform(size=R) < 0.5, -30.0, 30.0)
            pv[b, a // K, K * C + a % K] = 20.0 if j % 2 else -20.0
            plants["saturated"].append((b, a))
        # width / height deltas at EXP_THRESH (centre deltas 0: the box stays inside the image, nothing is clipped away)
        for kind, dw, dh in (("at", thr, thr), ("below", dn, dn), ("below_w", dn, thr), ("above", up, up), ("above_8", up, 8.0),
                             ("plus8", 8.0, 8.0)):
            for _ in range(2):
                b, a = next(small)
                delta(b, a)[:] = (0.0, 0.0, float(dw), float(dh))
                plants["thresh"].append((b, a, kind))
        # centre deltas that clip: over one border from a border cell, and wholly outside from an interior cell
        for b in range(B):
            for side, cell, d, v in (("left", 3 * gw, 0, -0.5), ("right", 4 * gw - 1, 0, 0.5), ("top", 5, 1, -0.5), ("bottom", (gh - 1) * gw + 6, 1, 0.5)):
                a = cell * K + (2, 3, 5)[b]                           # 115x59 / 162x87 / 258x173 anchors: half a shape over the border
                delta(b, a)[:] = (0.0, 0.0, 0.0, 0.0)
                delta(b, a)[d] = v
                plants["clip"].append((b, a, side))
        for side, d, v in (("out_right", 0, 60.0), ("out_left", 0, -60.0), ("out_bottom", 1, 60.0), ("out_top", 1, -60.0)):
            b, a = next(it)
            delta(b, a)[d] = v
            plants["clip"].append((b, a, side))
        # the last real class wins (next to the padding classes), one anchor per image
        for b0 in range(B):
            b, a = next((b_, a_) for b_, a_ in it if b_ == b0)
            lg = logits(b, a)
            lg[:R] = np.minimum(lg[:R], round_storage(2.0, dtype))
            lg[R - 1] = 6.0
            plants["last_class"].append((b, a, R - 1))
        used = [(p[0], p[1]) for v in plants.values() for p in v]
        assert len(used) == len(set(used)), "planted anchors overlap"
        assert np.array_equal(preds, round_storage(preds, dtype)), "a planted value is not a storage value"
    assert np.isfinite(preds).all()
    preds.setflags(write=False)
    return mc, preds, plants


def head_preds(name, dtype="fp32"):
    """(mc, preds float32 [B,gh,gw,K*(C+5)]), seeded by the name; the values are already rounded to `dtype` storage."""
    mc, preds, _ = _build(name, dtype)
    return mc, preds


def head_plants(name, dtype="fp32"):
    """{kind: [(image, anchor, what)]} of the values planted into the *_edges cases (empty lists elsewhere)."""
    return _build(name, dtype)[2]


def real_classes(name):
    return HEAD_CASES[name][1]


@functools.lru_cache(maxsize=None)
def head_reference(name, dtype="fp32"):
    """The oracle's interpret_output of the case, computed once (read-only arrays), plus `decided` [B,A]."""
    mc, preds = head_preds(name, dtype)
    ref = O.interpret_output(preds, mc)
    ref["decided"] = decided_anchors(mc, preds, ref)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def class_logits(mc, preds):
    B, K, C = preds.shape[0], mc.ANCHOR_PER_GRID, mc.CLASSES
    return preds[..., :K * C].reshape(B, mc.ANCHORS, C)


def decided_anchors(mc, preds, ref):
    """An anchor's class is DECIDED -- demanded bit for bit of any correct implementation -- when the largest score product
    class_prob * conf exceeds the next one by more than UNDECIDED_REL relative.  Classes whose logits are bit-equal to the
    largest logit (a planted tie, or two float16-rounded logits that meet) count as ONE contender: equal inputs give equal
    expf outputs everywhere, and the first of them must win; the margin is then taken to the best class outside the tie."""
    lg = class_logits(mc, preds)
    pr = ref["pred_class_probs"].astype(np.float64) * ref["pred_conf"].astype(np.float64)[..., None]
    tied = lg == lg.max(axis=2, keepdims=True)
    top = pr.max(axis=2)
    rest = np.where(tied, -np.inf, pr).max(axis=2)            # -inf: every class is in the tie (or C == 1)
    return (top - rest) > UNDECIDED_REL * top


def decode_float64(mc, preds):
    """interpret_output's class probabilities, confidence and score (nn_skeleton.py:150-170, 274-283) in float64: the yardstick
    for the error lines test_interpret_output_any_head prints (kernel vs float64 beside float32 oracle vs float64)."""
    lg = class_logits(mc, preds).astype(np.float64)
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    pcp = e / e.sum(axis=2, keepdims=True)
    K, C = mc.ANCHOR_PER_GRID, mc.CLASSES
    conf = 1.0 / (1.0 + np.exp(-preds[..., K * C:K * C + K].reshape(preds.shape[0], mc.ANCHORS).astype(np.float64)))
    return dict(pred_class_probs=pcp, pred_conf=conf, det_probs=(pcp * conf[..., None]).max(axis=2))


def max_rel_error(got, ref64):
    """max |got - ref| / ref over the entries whose float64 value is a normal float32 (an underflowed class probability of a
    saturated anchor has no relative error to speak of)."""
    m = ref64 > 1.2e-38
    return float(np.max(np.abs(np.asarray(got, np.float64)[m] - ref64[m]) / ref64[m]))


# ------------------------------------------------------------------------------------------------ filter_prediction inputs
# id: (C, A, top_n, what).  All cases: B = 2, NMS_THRESH 0.4; top_n == 0: the threshold branch (PROB_THRESH 0.6, max_out 512).
# "fast" / "generic": the kernel sqdet_filter_prediction dispatches to (filter_fast.hip: top-N branch, top_n <= 64, A <= 20480).
FILTER_CASES = {
    "c23_a16848_top64": (23, 16848, 64, "fast"),            # 23 placement ballots; bad input classes
    "c20_a20480_top64": (20, 20480, 64, "fast"),            # all 20 register slots
    "c20_a17409_top64": (20, 17409, 64, "fast"),            # first anchor of register slot 17
    "c4_a65_top64": (4, 65, 64, "fast"),                    # smallest fast case
    "c4_a65_top1": (4, 65, 1, "fast"),                      # M = 1
    "c23_a20481_top64": (23, 20481, 64, "generic"),         # radix select, one anchor past the fast limit
    "c23_a16848_top65": (23, 16848, 65, "generic"),         # capacity 128
    "c23_a16848_top1000": (23, 16848, 1000, "generic"),     # capacity 1024
    "c2_a300_top256": (2, 300, 256, "generic"),             # index bytes 2..3 all zero: the select skips them
    "c1_a5000_top200": (1, 5000, 200, "generic"),           # one class: every pair competes; bad input classes
    "c23_a600_thresh": (23, 600, 0, "generic"),             # threshold branch at 23 classes
    "c23_a16848_top100_ties": (23, 16848, 100, "generic"),  # probs rounded to 2 decimals: descending prob, then higher index
}
BAD_CLASS_CASES = ("c23_a16848_top64", "c1_a5000_top200")
FILTER_B = 2


def filter_config(name):
    C, A, top_n, _ = FILTER_CASES[name]
    mc = O.kitti_squeezeDet_config()
    mc.CLASSES, mc.ANCHORS, mc.TOP_N_DETECTION, mc.NMS_THRESH = C, A, top_n, 0.4
    mc.PROB_THRESH = 0.6 if top_n == 0 else 0.005
    return mc


def filter_max_out(name):
    return 512 if FILTER_CASES[name][2] == 0 else FILTER_CASES[name][2]


@functools.lru_cache(maxsize=None)
def filter_case(name):
    """(mc, boxes [B,A,4] f32, probs [B,A] f32, cls [B,A] i64, bad [B] lists of anchors given a class outside [0, C)):
    clusters of boxes and probs = uniform**6, the construction of test_filter_prediction_batched_random_vs_oracle."""
    C, A, top_n, _ = FILTER_CASES[name]
    mc = filter_config(name)
    B = FILTER_B
    rs = np.random.RandomState(zlib.crc32(name.encode()) % (2 ** 31))
    centers = rs.uniform([100, 60, 40, 30], [1100, 320, 250, 150], size=(B, 8, 4))
    which = rs.randint(0, 8, (B, A))
    boxes = np.take_along_axis(centers, which[..., None].repeat(4, 2), 1) + rs.normal(0, 1, (B, A, 4)) * [14, 9, 12, 9]
    boxes[..., 2:] = np.maximum(boxes[..., 2:], 1.0)
    boxes = boxes.astype(np.float32)
    probs = (rs.uniform(0, 1, (B, A)) ** 6).astype(np.float32)
    if name.endswith("_ties"):
        probs = np.round(probs, 2).astype(np.float32)
    cls = rs.randint(0, C, (B, A)).astype(np.int64)
    bad = [[] for _ in range(B)]
    if name in BAD_CLASS_CASES:
        for b in range(B):
            ranked = O.rank_order(probs[b])
            for r, c in ((2, -1), (7, C), (11, -1), (30, C), (41, C + 5)):          # candidates of the top-N, some near its head
                cls[b, ranked[r]] = c
                bad[b].append(int(ranked[r]))
    for a in (boxes, probs, cls):
        a.setflags(write=False)
    return mc, boxes, probs, cls, bad


def oracle_rows(mc, boxes, probs, cls, max_out):
    """O.filter_prediction of one image laid out as the kernel's five outputs: (index i32 [max_out], prob f32, box f32 [max_out,4],
    class i32, count) with the tail rows -1 / 0."""
    fb, fp, fc, fi = O.filter_prediction(mc, boxes, probs, cls, return_index=True)
    n = len(fp)
    assert n <= max_out
    oi, oc = np.full(max_out, -1, np.int32), np.full(max_out, -1, np.int32)
    op, ob = np.zeros(max_out, np.float32), np.zeros((max_out, 4), np.float32)
    oi[:n], oc[:n], op[:n] = fi, fc, fp
    ob[:n] = np.asarray(fb, np.float32).reshape(-1, 4)
    return oi, op, ob, oc, n


def candidates(mc, probs):
    """Anchors that enter NMS (nn_skeleton.py:711-720): the top-N by the repo's total order, or those above PROB_THRESH."""
    if 0 < mc.TOP_N_DETECTION < len(probs):
        return O.rank_order(probs)[:mc.TOP_N_DETECTION]
    return np.nonzero(probs > mc.PROB_THRESH)[0]


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    """Per image: the oracle's rows (oracle_rows) of the case, computed once."""
    mc, boxes, probs, cls, _ = filter_case(name)
    return [oracle_rows(mc, boxes[b], probs[b], cls[b], filter_max_out(name)) for b in range(FILTER_B)]
