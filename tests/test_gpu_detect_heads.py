"""The decode (interpret_kernel, score_kernel, the fused filter's re-decode) and filter kernels (filter_topn_fast, the generic
filter_kernel) against the CPU oracle at heads other than KITTI's 9 x (3 + 5) and at top-N settings other than 64 -- the generic
class loop of decode_score, 1 .. 23 placement ballots, every register slot of the fast filter and its hand-over to the generic
kernel, the generic kernel's radix select, interpret_kernel's grid-stride loop.  The inputs are built, and proven good on the
oracle alone, by tests/detect_head_cases.py and tests/test_detect_heads_host.py.

Bounds: floats as in test_interpret_output_parity (device expf vs NumPy exp: last-ulp differences); classes, picks, order and
every filter output bit for bit."""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O
from tests import detect_head_cases as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ops():
    from squeezedet_amd import ops
    return ops


def _t(a, dtype=None):
    t = torch.tensor(a)
    return (t.to(DEV) if dtype is None else t.to(DEV, dtype)).contiguous()


def _anchors(mc):
    return _t(np.asarray(mc.ANCHOR_BOX).astype(np.float32))


def _tdt(dtype):
    return torch.float16 if dtype == "fp16" else torch.float32


def _close(what, got, ref32, ref64, rtol, atol, saturated):
    """assert_allclose(got, ref32); where that fails ONLY on anchors planted with saturated logits, the rule of
    test_loss_against_float64_within_four_times_the_float32_oracles_error instead: kernel error against float64 at most four times
    the float32 oracle's (+ 1e-9) on those entries."""
    bad = ~np.isclose(got, ref32, rtol=rtol, atol=atol)
    if not bad.any():
        return
    sat = np.zeros(got.shape[:2], bool)
    for b, a in saturated:
        sat[b, a] = True
    assert saturated and not bad[~sat].any(), "%s: %d entries off the float32 oracle beyond rtol %g outside the saturated anchors" % (what, bad[~sat].sum(), rtol)
    eg = np.abs(got.astype(np.float64) - ref64)[bad].max()
    er = np.abs(ref32.astype(np.float64) - ref64)[bad].max()
    print("SATURATED %s: %d entries beyond rtol %g; kernel err %.3e, float32 oracle err %.3e against float64" % (what, bad.sum(), rtol, eg, er))
    assert eg <= 4.0 * er + 1e-9, "%s: kernel error %g, float32 oracle error %g" % (what, eg, er)


def _check_decode(name, mc, preds, ref, got, plants=None, real=None):
    """got: (det_boxes, det_probs, det_class, pred_class_probs, pred_conf) numpy arrays of the kernel."""
    boxes, probs, cls, pcp, pconf = got
    assert boxes.dtype == np.float32 and probs.dtype == np.float32 and cls.dtype == np.int64
    r64 = H.decode_float64(mc, preds)
    errs = []
    for key, g in (("pred_class_probs", pcp), ("pred_conf", pconf), ("det_probs", probs)):
        errs.append("%s %.2e / %.2e" % (key, H.max_rel_error(g, r64[key]), H.max_rel_error(ref[key], r64[key])))
    print("DECODE %-24s max rel err against float64, kernel / float32 oracle: %s; boxes max |kernel - oracle| %.2e"
          % (name, "  ".join(errs), np.abs(boxes.astype(np.float64) - ref["det_boxes"]).max()))
    sat = plants["saturated"] if plants else []
    _close(name + " pred_class_probs", pcp, ref["pred_class_probs"], r64["pred_class_probs"], 2e-6, 1e-9, sat)
    _close(name + " pred_conf", pconf, ref["pred_conf"], r64["pred_conf"], 2e-6, 1e-9, sat)
    _close(name + " det_probs", probs, ref["det_probs"], r64["det_probs"], 3e-6, 1e-9, sat)
    np.testing.assert_allclose(boxes, ref["det_boxes"], rtol=2e-6, atol=1e-3)
    decided = ref["decided"]
    assert decided.mean() >= 0.99
    np.testing.assert_array_equal(cls[decided], ref["det_class"][decided])
    assert (cls >= 0).all() and (cls < mc.CLASSES).all()
    if real is not None and real < mc.CLASSES:
        assert (pcp[..., real:] == 0.0).all() and (cls < real).all()
    if mc.CLASSES == 1:
        assert (pcp == 1.0).all() and np.array_equal(probs, pconf)
    if plants and plants["ties"]:
        for b, a, T in plants["ties"]:
            assert cls[b, a] == min(T), "tie %s at image %d anchor %d -> class %d" % (T, b, a, cls[b, a])
        for b, a, c in plants["last_class"]:
            assert cls[b, a] == c
        above = [(b, a) for b, a, kind in plants["thresh"] if kind in ("above", "above_8", "plus8")]
        assert len(above) >= 6
        for b, a in above:              # no expf on this path: the same float32 operations as the oracle's
            assert boxes[b, a].tobytes() == ref["det_boxes"][b, a].tobytes(), (b, a, boxes[b, a], ref["det_boxes"][b, a])


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("name", H.DECODE_CASES)
def test_interpret_output_any_head(name, dtype):
    """interpret_kernel (decode_score's generic class loop for C != 3, the pred_class_probs / pred_conf loops, decode_box) against
    O.interpret_output at 1, 2, 4, 20 and 23 classes, 1, 6 and 9 anchors per cell; exact classes on every decided anchor, the
    lowest index on planted bit-equal ties, exact zeros on the padding classes, bit-equal boxes above EXP_THRESH."""
    ops = _ops()
    mc, preds = H.head_preds(name, dtype)
    ref = H.head_reference(name, dtype)
    out = ops.interpret_output(_t(preds, _tdt(dtype)), _anchors(mc), mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT,
                               mc.EXP_THRESH, with_class_probs=True)
    torch.cuda.synchronize()
    _check_decode("%s-%s" % (name, dtype), mc, preds, ref, [o.cpu().numpy() for o in out], H.head_plants(name, dtype), H.real_classes(name))


def test_interpret_output_past_the_grid_cap():
    """4 x 256 x 228 x 9 = 2 101 248 anchors: more than the 8192 x 256 threads the launch is capped at, so interpret_kernel's
    grid-stride loop takes a second lap (one class: the 50 MB of preds are the smallest that get there)."""
    ops = _ops()
    C, K, B, gh, gw = 1, 9, 4, 256, 228
    mc = H.head_config(C, K, gh, gw)
    A = mc.ANCHORS
    assert B * A > 8192 * 256
    preds = (np.random.RandomState(2101248).randn(B, gh, gw, K * (C + 5)) * 1.7).astype(np.float32)
    ref = O.interpret_output(preds, mc)
    ref["decided"] = H.decided_anchors(mc, preds, ref)
    out = (torch.full((B, A, 4), float("nan"), device=DEV), torch.full((B, A), float("nan"), device=DEV),
           torch.full((B, A), -1, dtype=torch.int64, device=DEV))
    got = ops.interpret_output(_t(preds), _anchors(mc), C, K, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH, with_class_probs=True, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2]
    got = [o.cpu().numpy() for o in got]
    for g in got:
        assert not np.isnan(g).any()
    assert (got[0].reshape(-1, 4)[-4096:] != 0).all() and (got[2] == 0).all()
    _check_decode("past_the_grid_cap", mc, preds, ref, got)


@pytest.mark.parametrize("name", list(H.FILTER_CASES))
def test_filter_prediction_any_head(name):
    """sqdet_filter_prediction bit for bit against O.filter_prediction: index, prob, box, class, count and the -1 / 0 tail rows.
    H.FILTER_CASES names what each case reaches and which kernel takes it (the dispatch of filter_topn_fast_launch)."""
    ops = _ops()
    C, A, top_n, kernel = H.FILTER_CASES[name]
    mc, boxes, probs, cls, _ = H.filter_case(name)
    assert kernel == ("fast" if 0 < top_n <= 64 and A <= 20480 else "generic") and (top_n == 0 or top_n < A)
    max_out = H.filter_max_out(name)
    ob, op, oc, oi, cnt = [o.cpu().numpy() for o in ops.filter_prediction(_t(boxes), _t(probs), _t(cls), C, top_n, mc.NMS_THRESH, mc.PROB_THRESH,
                                                                          max_out=max_out)]
    assert ob.shape == (H.FILTER_B, max_out, 4) and oi.dtype == np.int32 and oc.dtype == np.int32
    for b, (ri, rp, rb, rc, n) in enumerate(H.filter_reference(name)):
        assert cnt[b] == n, "image %d: %d rows, oracle %d" % (b, cnt[b], n)
        np.testing.assert_array_equal(oi[b], ri)
        np.testing.assert_array_equal(oc[b], rc)
        assert op[b].tobytes() == rp.tobytes() and ob[b].tobytes() == rb.tobytes()


DETECT_CASES = H.DECODE_CASES + ["voc23_k10_32x64", "voc23_constant"]


def _pair_and_oracle(ops, mc, pd, anchors, top_n=64):
    """interpret_output -> filter_prediction on the device, and the oracle's filter_prediction fed the kernel's OWN det_boxes /
    det_probs / det_class: the select + NMS link (test_interpret_output_any_head is the decode link), free of last-ulp expf
    differences at the top-N boundary."""
    C, K = mc.CLASSES, mc.ANCHOR_PER_GRID
    boxes, probs, cls = ops.interpret_output(pd, anchors, C, K, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH)
    want = ops.filter_prediction(boxes, probs, cls, C, top_n, mc.NMS_THRESH, mc.PROB_THRESH)
    torch.cuda.synchronize()
    b_, p_, c_ = boxes.cpu().numpy(), probs.cpu().numpy(), cls.cpu().numpy()
    ob, op, oc, oi, cnt = [w.cpu().numpy() for w in want]
    for i in range(pd.shape[0]):
        ri, rp, rb, rc, n = H.oracle_rows(mc, b_[i], p_[i], c_[i], top_n)
        assert cnt[i] == n and n >= 1
        np.testing.assert_array_equal(oi[i], ri)
        np.testing.assert_array_equal(oc[i], rc)
        assert op[i].tobytes() == rp.tobytes() and ob[i].tobytes() == rb.tobytes()
    return want, p_


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("name", DETECT_CASES)
def test_detect_filter_any_head(name, dtype):
    """sqdet_detect_filter (score_kernel + the fused filter's re-decode of the selected anchors) is EXACTLY interpret_output ->
    filter_prediction at every head, at A = 20480 (all 20 register slots) and on a constant score map (the radix-select
    fallback); and those rows are the oracle's filter_prediction of the kernel's own decode."""
    ops = _ops()
    mc, preds = H.head_preds(name, dtype)
    assert mc.TOP_N_DETECTION == 64 < mc.ANCHORS <= 20480 and mc.NMS_THRESH == 0.4
    pd, anchors = _t(preds, _tdt(dtype)), _anchors(mc)
    want, scores = _pair_and_oracle(ops, mc, pd, anchors)
    got = ops.detect_filter(pd, anchors, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH, 64, mc.NMS_THRESH)
    torch.cuda.synchronize()
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)
    if name == "voc23_constant":
        assert (scores[1] == scores[1, 0]).all() and mc.ANCHORS > 2048         # every anchor of image 1 ties: candidate overflow
        assert got[3][1, :int(got[4][1])].min() >= mc.ANCHORS - 64               # ties -> higher anchor index first
    if H.real_classes(name) < mc.CLASSES:
        assert int(got[2].max()) < H.real_classes(name)


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_detect_filter_refuses_more_than_20480_anchors(dtype):
    """A = 3 x 683 x 10 = 20490: sqdet_detect_filter has no kernel for it and says so; the pair the model falls back to
    (interpret_output -> filter_prediction, here the generic kernel) still gives the oracle's rows."""
    ops = _ops()
    from squeezedet_amd import _lib
    mc, preds = H.head_preds("voc23_k10_3x683", dtype)
    assert mc.ANCHORS == 20490 and not ops.detect_filter_supported(mc.ANCHORS, 64)
    pd, anchors = _t(preds, _tdt(dtype)), _anchors(mc)
    with pytest.raises(_lib.SqdetUnsupported, match="needs the top-N branch"):
        ops.detect_filter(pd, anchors, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH, 64, mc.NMS_THRESH)
    want, _ = _pair_and_oracle(ops, mc, pd, anchors)
    assert int(want[2].max()) < 20
