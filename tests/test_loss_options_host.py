"""The loss with options without a GPU: the hand-derived float64 gradient of
tests/loss_options_reference.py against autograd and against central differences, for every box loss and gamma 0, 0.5 and 2;
the defaults against loss_reference64; the orderings giou <= iou and ciou <= diou <= iou; the direction of the GIoU gradient of a
disjoint pair; the cases' edges and their distance from every tie; mutation checks (each wrong gradient is caught by the
cases); and the flag / config / checkpoint-policy plumbing of train.py."""
import argparse

import numpy as np
import pytest
import torch

from squeezedet_amd.drivers import BOX_LOSSES           # (the names --bbox_loss takes: the restatement must know the same ones)
from tests import loss_options_cases as LC, loss_options_reference as LR

assert BOX_LOSSES == LR.BOX_LOSSES
KINDS = list(BOX_LOSSES)
GAMMAS = [0.0, 0.5, 2.0]
_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = LC.loss_case(name)
    return _CACHE[name]


def ref64(name, kind, gamma, **kw):
    key = (name, kind, gamma, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = LR.loss_options_reference64(*case(name)[:6], box_loss=kind, gamma=gamma, **kw)
    return _CACHE[key]


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("name", list(LC.CASES))
def test_cases_hold_their_edges_and_stay_off_every_tie(name):
    mc, preds, mask, delta, box, labels, planted = case(name)
    gh, gw, K, C, B, extra = LC.CASES[name]
    A = mc.ANCHORS
    assert preds.shape == (B, gh, gw, K * (C + 5)) and A == gh * gw * K
    nobj = int(mask.sum())
    assert nobj == 5 + extra and 1 <= nobj and (name == "kitti_b8" or nobj < A)
    assert LC.min_separation(mc, preds, mask, box) >= LC.MIN_SEPARATION          # every positive anchor: none is excluded
    assert sorted(planted) == ["P1", "P2", "P3", "P4", "P5"]
    w1, h1 = mc.IMAGE_WIDTH - 1.0, mc.IMAGE_HEIGHT - 1.0
    thr = float(np.float32(mc.EXP_THRESH))
    pos = {(b, a): (anc, d, g) for b, a, anc, d, g in LC.positives(mc, preds, mask, box)}
    geo = {}
    for kind, (b, a) in planted.items():
        anc, d, g = pos[(b, a)]
        raw, c = LC._corners_of(mc, anc, d)
        gb = [g[0] - g[2] / 2.0, g[1] - g[3] / 2.0, g[0] + g[2] / 2.0, g[1] + g[3] / 2.0]
        geo[kind] = (raw, c, gb, d)
    raw, c, gb, d = geo["P1"]
    assert raw[0] < 0 and raw[1] < 0 and 0 < raw[2] < w1 and 0 < raw[3] < h1 and d[2] > thr          # left + top clipped, linear branch
    assert c[0] < gb[0] and c[1] < gb[1] and c[2] > gb[2] and c[3] > gb[3]                          # contains its ground truth
    raw, c, gb, d = geo["P2"]
    assert raw[2] > w1 and raw[3] > h1 and 0 < raw[0] < w1 and 0 < raw[1] < h1 and d[3] > thr        # right + bottom clipped
    assert gb[0] < c[0] and gb[1] < c[1] and gb[2] > c[2] and gb[3] > c[3]                          # contained in it
    raw, c, gb, d = geo["P3"]
    assert gb[0] > c[2] and gb[1] > c[3]                                                            # disjoint
    raw, c, gb, d = geo["P4"]
    iw, ih = min(c[2], gb[2]) - max(c[0], gb[0]), min(c[3], gb[3]) - max(c[1], gb[1])
    assert iw > 0 and ih > 0 and not (c[0] < gb[0] and c[2] > gb[2]) and not (gb[0] < c[0] and gb[2] > c[2])      # partial overlap
    raw, c, gb, d = geo["P5"]
    assert max(abs(c[j] - gb[j]) for j in range(4)) < 1.0                                            # equal to within a pixel
    ious = ref64(name, "iou", 0.0)[1]
    b, a = planted["P3"]
    assert ious[b, a] == 0.0
    b, a = planted["P5"]
    assert ious[b, a] > 0.75


def test_case_shapes_cover_what_the_issue_lists():
    small = [LC.CASES[n] for n in LC.SMALL_CASES]
    assert {(c[0], c[1]) for c in small} == {(2, 3), (3, 5)} and {c[2] for c in small} == {1, 9}
    assert {c[3] for c in small} == {1, 3, 20} and {c[4] for c in small} == {1, 3}
    assert LC.CASES["kitti_b8"][:5] == (24, 78, 9, 3, 8)


# ---------------------------------------------------------------- the hand-derived gradient
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("kind", KINDS)
def test_hand_gradient_is_autograds(kind, gamma):
    """float64: hand derivation == torch autograd of the same forward, on every small case; losses and ious agree too."""
    for name in LC.SMALL_CASES:
        got = ref64(name, kind, gamma)
        want = LR.loss_options_torch(*case(name)[:6], box_loss=kind, gamma=gamma, dtype=torch.float64)
        scale = np.abs(want[2]).max()
        np.testing.assert_allclose(got[0], want[0], rtol=1e-12, atol=1e-14, err_msg=name)
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-14, err_msg=name)
        assert np.abs(got[2] - want[2]).max() <= 1e-11 * scale, (name, np.abs(got[2] - want[2]).max(), scale)


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("kind", KINDS)
def test_hand_gradient_is_the_central_difference(kind, gamma):
    """d(class + bbox loss)/dpreds by central differences, h = 1e-6 (the cases stay 1e-3 px off every kink; the anchors are at
    most 366 px wide, so a step of 1e-6 in a delta moves an edge by less than 1e-3 px).  The confidence term is left out: its
    target, the IoU, is a constant of the backward pass by definition but not of a difference quotient.  CIoU's alpha likewise:
    the quotient is compared with the gradient that differentiates alpha too (the `alpha_grad` variant)."""
    for name in ("g2x3_k1_c3_b1", "g3x5_k9_c3_b1"):
        mc, preds, mask, delta, box, labels, _ = case(name)
        kw = dict(box_loss=kind, gamma=gamma)
        total = lambda p: LR.loss_options_reference64(mc, p, mask, delta, box, labels, **kw)[0][[0, 2]].sum()
        full = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, mutate="alpha_grad" if kind == "ciou" else None, **kw)[2]
        K, C, A = mc.ANCHOR_PER_GRID, mc.CLASSES, mc.ANCHORS
        ch = K * (C + 5)
        p64 = preds.astype(np.float64)
        flat = p64.reshape(-1)
        idx = []                                  # the class logits and the deltas of every positive anchor (all others: zero)
        for b, a in np.argwhere(mask[..., 0] > 0):
            base = (b * (A // K) + a // K) * ch
            idx += [base + (a % K) * C + c for c in range(C)] + [base + K * (C + 1) + 4 * (a % K) + d for d in range(4)]
        h = 1e-6
        worst = 0.0
        for i in idx:
            keep = flat[i]
            flat[i] = keep + h
            up = total(p64)
            flat[i] = keep - h
            dn = total(p64)
            flat[i] = keep
            worst = max(worst, abs((up - dn) / (2 * h) - full.reshape(-1)[i]))
        assert worst <= 1e-6 * max(1.0, np.abs(full).max()), (name, worst)


def test_defaults_reproduce_loss_reference64():
    from tests.test_gpu_train_kernels import loss_reference64
    for name in LC.SMALL_CASES:
        mc, preds, mask, delta, box, labels, _ = case(name)
        want = loss_reference64(mc, preds, mask, delta, box, labels)
        got = ref64(name, "delta_l2", 0.0)
        np.testing.assert_allclose(got[0], want[0], rtol=1e-13)
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-15)
        assert np.abs(got[2] - want[2]).max() <= 1e-12 * np.abs(want[2]).max()


def test_measures_are_ordered():
    """giou <= iou and ciou <= diou <= iou elementwise, on 20 000 random box pairs and on every positive of the cases."""
    rs = np.random.RandomState(3)
    lo = rs.uniform(0, 100, (4, 20000))
    a = [lo[0], lo[1], lo[0] + rs.uniform(1, 80, 20000), lo[1] + rs.uniform(1, 80, 20000)]
    b = [lo[2], lo[3], lo[2] + rs.uniform(1, 80, 20000), lo[3] + rs.uniform(1, 80, 20000)]
    iou, giou, diou, ciou = LR.box_measures64(a, b)
    r = 1e-15            # (one rounding of values of size 1)
    assert (giou <= iou + r).all() and (diou <= iou + r).all() and (ciou <= diou + r).all() and (giou >= -1 - r).all() and (iou <= 1 + r).all()
    for name in LC.SMALL_CASES:                       # through the loss: bbox loss ordered the other way round
        l = {k: ref64(name, k, 0.0)[0][2] for k in KINDS[1:]}
        assert l["giou"] >= l["iou"] and l["ciou"] >= l["diou"] >= l["iou"]


def test_giou_gradient_of_a_disjoint_pair_points_towards_the_ground_truth():
    """P3's ground truth lies to the right of and below its prediction: IoU is 0 and its gradient vanishes, GIoU's does not,
    and a descent step (minus the gradient) moves the centre right and down."""
    for name in LC.SMALL_CASES:
        mc, preds, mask, delta, box, labels, planted = case(name)
        b, a = planted["P3"]
        K, C = mc.ANCHOR_PER_GRID, mc.CLASSES
        sl = (b, a // K, slice(K * (C + 1) + 4 * (a % K), K * (C + 1) + 4 * (a % K) + 4))
        g_iou = ref64(name, "iou", 0.0)[2].reshape(preds.shape[0], -1, K * (C + 5))[sl]
        g_giou = ref64(name, "giou", 0.0)[2].reshape(preds.shape[0], -1, K * (C + 5))[sl]
        assert (g_iou == 0).all()
        assert g_giou[0] < 0 and g_giou[1] < 0 and np.isfinite(g_giou).all()


# ---------------------------------------------------------------- mutations
def _caught(name, kind, mutate, gamma=0.0):
    """Largest element difference of the mutated gradient from the right one, in units of 1e-5 of the largest gradient element.
    (The float32 evaluations err by about 1e-7 .. 1e-6 of it -- the tables of the two GPU loss tests -- so a difference of 10
    units, 1e-4, is a hundred times what the GPU test's 4 * e_ref + 1e-7 lets through.)"""
    good = ref64(name, kind, gamma)[2]
    bad = LR.loss_options_reference64(*case(name)[:6], box_loss=kind, gamma=gamma, mutate=mutate)[2]
    return np.abs(good - bad).max() / (1e-5 * np.abs(good).max())


@pytest.mark.parametrize("mutate", ["no_clip_mask", "no_slope", "alpha_grad"])
def test_cases_catch_the_wrong_gradient(mutate):
    kinds = ["ciou"] if mutate == "alpha_grad" else KINDS[1:]
    for name in LC.SMALL_CASES:
        for kind in kinds:
            assert _caught(name, kind, mutate) > 10.0, (name, kind, mutate)


def test_tie_rule_is_invisible_off_ties_and_decides_on_them():
    for name in LC.SMALL_CASES:
        for kind in KINDS[1:]:
            assert _caught(name, kind, "tie_swapped") == 0.0
    mc, preds, mask, delta, box, labels = LC.tie_case()
    for kind in KINDS[1:]:
        good = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss=kind)
        bad = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss=kind, mutate="tie_swapped")
        assert np.isfinite(good[0]).all() and np.isfinite(good[2]).all()
        np.testing.assert_array_equal(good[0], bad[0])                       # the rule is about the gradient only
        assert np.abs(good[2] - bad[2]).max() > 1e-3 * np.abs(good[2]).max()


def test_the_stated_tie_rule_on_the_tie_case():
    """T1 (prediction == ground truth, IoU 1): under the rule no corner owns the intersection, so only the union's growth is
    seen -- the loss rises with the width and height deltas and is flat in the centre.  T2 .. T4 (an edge exactly on the
    border counts as clipped): the delta gradients are those of the one free edge: |dL/dd0| * safe_exp' / 2 == |dL/dd2|."""
    mc, preds, mask, delta, box, labels = LC.tie_case()
    sc = mc.LOSS_COEF_BBOX / 5.0
    g = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss="iou")[2].reshape(6, 8)[:, 4:]
    aw, ah = 40.0, 20.0
    ue = 41.0 * 21.0 + float(np.float32(mc.EPSILON))
    np.testing.assert_allclose(g[0], [0.0, 0.0, sc * 21.0 / ue * aw, sc * 41.0 / ue * ah], rtol=1e-12, atol=1e-15)
    assert g[1][0] != 0 and abs(g[1][2]) == pytest.approx(abs(g[1][0]) / 2)           # T2: only the right edge moves
    assert g[2][0] != 0 and abs(g[2][2]) == pytest.approx(abs(g[2][0]) / 2)           # T3: only the left edge (x) ...
    assert g[2][1] != 0 and abs(g[2][3]) == pytest.approx(abs(g[2][1]) / 2)           # ... and only the bottom edge (y)
    assert g[3][1] != 0 and abs(g[3][3]) == pytest.approx(abs(g[3][1]) / 2)           # T4: only the top edge
    # T5: a width delta exactly at EXP_THRESH is on the exp branch; there both branches have the derivative e, so the rule
    # shows in the value of neither -- only that it is finite and uses e
    assert np.isfinite(g[4]).all() and g[4][2] != 0


# ---------------------------------------------------------------- flags, config, checkpoint policy
def test_config_defaults_and_ops_options():
    from squeezedet_amd import config, drivers
    for mk in (config.kitti_squeezeDet_config, config.kitti_res50_config, config.kitti_vgg16_config, config.kitti_squeezeDetPlus_config):
        mc = mk()
        assert mc.BBOX_LOSS == "delta_l2" and mc.FOCAL_GAMMA == 0.0
    assert config.pad_head_classes(config.voc_squeezeDet_config_for_input(128, 256)).BBOX_LOSS == "delta_l2"
    assert drivers.BOX_LOSSES == LR.BOX_LOSSES
    # ops reads the two fields from any config: one without them (the oracle's, whose missing attribute is a KeyError; a plain
    # namespace) means the reference's loss, and an unknown name is refused before the library is called
    from oracle import sqdet_oracle as O
    from squeezedet_amd import ops
    from squeezedet_amd._lib import SqdetError
    assert ops.BOX_LOSSES == LR.BOX_LOSSES
    assert ops.loss_options(O.kitti_squeezeDet_config()) == ("delta_l2", 0.0)
    assert ops.loss_options(argparse.Namespace(CLASSES=3)) == ("delta_l2", 0.0)
    assert ops.loss_options(config.kitti_squeezeDet_config()) == ("delta_l2", 0.0)
    mc = config.kitti_squeezeDet_config()
    mc.BBOX_LOSS, mc.FOCAL_GAMMA = "ciou", 2
    assert ops.loss_options(mc) == ("ciou", 2.0)
    mc.BBOX_LOSS = "l1"
    with pytest.raises(SqdetError, match="BBOX_LOSS"):
        ops.loss_options(mc)


def test_flags_set_the_config_and_the_recorded_policy():
    import train as T
    from squeezedet_amd import config, drivers
    a = T.parse_args([])
    assert not hasattr(a, "bbox_loss") and not hasattr(a, "focal_gamma") and not hasattr(a, "bbox_loss_coef")
    mc = config.kitti_squeezeDet_config()
    policy, off = drivers.loss_policy(a, mc)
    assert policy == off == dict(bbox_loss="delta_l2", focal_gamma=0.0, bbox_loss_coef=5.0)
    assert (mc.BBOX_LOSS, mc.FOCAL_GAMMA, mc.LOSS_COEF_BBOX) == ("delta_l2", 0.0, 5.0)
    a = T.parse_args(["--bbox_loss", "giou", "--focal_gamma", "2", "--bbox_loss_coef", "2.5"])
    mc = config.kitti_squeezeDet_config()
    policy, off = drivers.loss_policy(a, mc)
    assert policy == dict(bbox_loss="giou", focal_gamma=2.0, bbox_loss_coef=2.5) and off["bbox_loss_coef"] == 5.0
    assert (mc.BBOX_LOSS, mc.FOCAL_GAMMA, mc.LOSS_COEF_BBOX) == ("giou", 2.0, 2.5)
    assert config.pad_head_classes(mc).BBOX_LOSS == "giou"                       # the config a padded net is built with is a copy
    for kind in LR.BOX_LOSSES:
        assert T.parse_args(["--bbox_loss", kind]).bbox_loss == kind
    for bad in (["--bbox_loss", "l1"], ["--focal_gamma", "-1"], ["--focal_gamma", "nan"], ["--bbox_loss_coef", "-2"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_resume_under_another_loss_policy_is_refused():
    import train as T
    from squeezedet_amd import config, drivers
    mc = config.kitti_squeezeDet_config()
    giou, off = drivers.loss_policy(argparse.Namespace(bbox_loss="giou", focal_gamma=2.0), mc)
    base = dict(net="squeezeDet", dtype="fp32", augment=T.AUGMENT_OFF, mosaic=0.0)
    T.check_resume_record(dict(base, loss=giou), dict(base, loss=giou), off)                     # recorded and matching
    T.check_resume_record(dict(base), dict(base, loss=off), off)                                 # absent key: the defaults
    T.check_resume_record(dict(net="squeezeDet", dtype="fp32"), dict(base, loss=off), off)       # (a checkpoint from before any policy key)
    with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with loss .*delta_l2.*this run asks for .*giou"):
        T.check_resume_record(dict(base), dict(base, loss=giou), off)
    with pytest.raises(SystemExit, match="trained with loss .*giou.*asks for .*ciou"):
        T.check_resume_record(dict(base, loss=giou), dict(base, loss=dict(giou, bbox_loss="ciou")), off)
    with pytest.raises(SystemExit, match="loss"):
        T.check_resume_record(dict(base, loss=giou), dict(base, loss=dict(giou, focal_gamma=1.0)), off)
    with pytest.raises(SystemExit, match="loss"):
        T.check_resume_record(dict(base, loss=giou), dict(base, loss=dict(giou, bbox_loss_coef=1.0)), off)
    with pytest.raises(SystemExit, match="mosaic"):                                              # the earlier keys still hold
        T.check_resume_record(dict(base, mosaic=0.5), dict(base, loss=off), off)


def test_checkpoint_extra_keeps_the_loss_policy(tmp_path):
    """The record goes through the checkpoint's `extra` as JSON-able values and comes back equal."""
    import json
    from squeezedet_amd import config, drivers
    policy, _ = drivers.loss_policy(argparse.Namespace(bbox_loss="ciou", focal_gamma=0.5, bbox_loss_coef=3.0), config.kitti_squeezeDet_config())
    assert json.loads(json.dumps(dict(loss=policy)))["loss"] == policy


def test_bench_train_takes_the_flags():
    """tools/bench_train.py: the flags reach the config its trainer is built with, and the line's `loss` record."""
    from tools import bench_train as BT
    mc, policy = BT.make_config(BT.parse_args([]))
    assert (mc.BBOX_LOSS, mc.FOCAL_GAMMA, mc.LOSS_COEF_BBOX) == ("delta_l2", 0.0, 5.0)
    assert policy == dict(bbox_loss="delta_l2", focal_gamma=0.0, bbox_loss_coef=5.0)
    a = BT.parse_args(["--arch", "resnet50", "--bbox_loss", "ciou", "--focal_gamma", "2", "--bbox_loss_coef", "1.5"])
    mc, policy = BT.make_config(a)
    assert (mc.BBOX_LOSS, mc.FOCAL_GAMMA, mc.LOSS_COEF_BBOX, mc.BATCH_SIZE) == ("ciou", 2.0, 1.5, 8)
    assert policy == dict(bbox_loss="ciou", focal_gamma=2.0, bbox_loss_coef=1.5)
    for bad in (["--bbox_loss", "l1"], ["--focal_gamma", "-1"]):
        with pytest.raises(SystemExit):
            BT.parse_args(bad)
