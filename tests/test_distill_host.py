"""Host tests of the distillation feature: the float64 restatement of tests/distill_reference.py against
float64 autograd and central differences, the hand-worked cases, the mutations each caught by a named case, the case table, and the
plumbing that needs no GPU -- options, check_compatible, the flags, the `distill` checkpoint key and the resume refusal."""
import argparse

import numpy as np
import pytest

from tests import distill_cases as DC, distill_reference as DR

_CACHE = {}


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {"ties": DC.tie_case, "extreme": DC.extreme_case}.get(name, lambda: DC.distill_case(name))()
    return _CACHE[name]


def ref64(name, **kw):
    K, C, s, t, opt = case(name)
    opt = kw.pop("opt", opt)
    return DR.distill_reference64(s, t, K, C, opt, **kw)


# ---------------------------------------------------------------- the cases
def test_case_shapes_cover_what_the_issue_lists():
    shapes = {(gh, gw, K, C, B) for gh, gw, K, C, B, _ in DC.CASES.values()}
    assert {(g[0], g[1]) for g in shapes} == {(2, 3), (3, 5), (24, 78)}
    assert {g[2] for g in shapes} == {1, 9} and {g[3] for g in shapes} == {1, 3, 20} and {g[4] for g in shapes} >= {1, 3}
    assert (24, 78, 9, 3, 2) in shapes
    opts = [o for *_, o in DC.CASES.values()]
    assert {o[0] for o in opts} == {0.5, 1.0, 2.0, 4.0}
    for pos in (1, 2, 3):                                       # a zero coefficient in each position
        assert any(o[pos] == 0.0 for o in opts)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_cases_stay_off_the_floor(name):
    K, C, s, t, opt = case(name)
    assert s.dtype == t.dtype == np.float32 and s.shape == t.shape
    assert np.array_equal(s, s.astype(np.float16).astype(np.float32)) and np.array_equal(t, t.astype(np.float16).astype(np.float32))
    assert DC.floor_separation(t, K, C, opt[4]) >= DC.MIN_SEPARATION
    if opt[4] > 0.0:                                            # the floor removes some anchors and keeps some
        ct = DC.sigmoid64(DC.conf_logits(t, K, C))
        assert (ct < opt[4]).any() and (ct >= opt[4]).any()


def test_the_tie_case_sits_on_the_floor():
    K, C, s, t, opt = case("ties")
    assert DC.floor_separation(t, K, C, opt[4]) == 0.0
    assert np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-0.0))) == np.float32(0.5)


# ---------------------------------------------------------------- the restatement against autograd and differences
@pytest.mark.parametrize("name", DC.SMALL_CASES + ["ties"])
def test_hand_gradient_is_autograds(name):
    """To 1e-11 of the largest gradient element (test_loss_options_host.py's bound), the terms to 1e-12 relative."""
    K, C, s, t, opt = case(name)
    for gb in (0, 7):
        terms, grad = DR.distill_reference64(s, t, K, C, opt, global_batch=gb)
        a_terms, a_grad = DR.distill_autograd64(s, t, K, C, opt, global_batch=gb)
        np.testing.assert_allclose(terms, a_terms, rtol=1e-12, atol=1e-15)
        assert np.abs(grad - a_grad).max() <= 1e-11 * max(np.abs(a_grad).max(), 1e-300), name


@pytest.mark.parametrize("T", [0.5, 1.0, 4.0])
def test_hand_gradient_is_the_central_difference(T):
    """Every element of the smallest case and 60 seeded elements of a K = 9, C = 3 case, h = 1e-6: the difference quotient of
    the float64 total agrees to 1e-7 of the largest gradient element (truncation h^2 f''' / 6 ~ 1e-13, rounding eps * L / h ~ 1e-9)."""
    for name, picks in (("g2x3_k1_c3_b1", None), ("g3x5_k9_c3_b1", 60)):
        K, C, s, t, opt = case(name)
        opt = (T, 1.0, 1.0, 1.0, opt[4])
        _, grad = DR.distill_reference64(s, t, K, C, opt)
        flat = np.arange(s.size) if picks is None else np.random.RandomState(3).choice(s.size, picks, replace=False)
        h, scale = 1e-6, np.abs(grad).max()
        for i in flat:
            up, dn = s.astype(np.float64).copy(), s.astype(np.float64).copy()
            up.reshape(-1)[i] += h
            dn.reshape(-1)[i] -= h
            d = (DR.distill_reference64(up, t, K, C, opt)[0].sum() - DR.distill_reference64(dn, t, K, C, opt)[0].sum()) / (2 * h)
            assert abs(d - grad.reshape(-1)[i]) <= 1e-7 * scale, (name, T, int(i), d, grad.reshape(-1)[i])


def test_global_batch_divides_every_term_and_gradient():
    K, C, s, t, opt = case("g3x5_k9_c20_b3")
    a, b = DR.distill_reference64(s, t, K, C, opt), DR.distill_reference64(s, t, K, C, opt, global_batch=6)
    assert np.array_equal(a[0], 2.0 * b[0]) and np.array_equal(a[1], 2.0 * b[1])


# ---------------------------------------------------------------- hand-worked cases
def test_one_class_has_no_class_term():
    K, C, s, t, opt = case("g2x3_k9_c1_b3")
    assert C == 1 and opt[1] > 0.0
    terms, grad = DR.distill_reference64(s, t, K, C, opt)
    gz = DR.split(grad, K, C)[0]
    assert terms[0] == 0.0 and not gz.any()
    assert terms[1] > 0.0 and terms[2] > 0.0


@pytest.mark.parametrize("name", list(DC.CASES))
def test_teacher_equal_to_student_gives_exact_zeros(name):
    K, C, s, _, opt = case(name)
    terms, grad = DR.distill_reference64(s, s.copy(), K, C, opt)
    assert not terms.any() and not grad.any()


def test_uniform_teacher_logits_give_q_one_over_c():
    """With q = 1/C the class term is c T^2 / Bg * sum w (-log C - mean_j lp_j) and the gradient c T w (p_j - 1/C) / Bg."""
    K, C, s, t, _ = case("g3x5_k9_c3_b1")
    t = t.copy()
    tv = t.reshape(t.shape[0], -1, K * (C + 5))                   # (a view: split returns copies)
    tv[..., :K * C] = 0.75
    T = 2.0
    terms, grad = DR.distill_reference64(s, t, K, C, (T, 1.5, 0.0, 0.0, 0.0))
    zs, _, _ = DR.split(s.astype(np.float64), K, C)
    ct = DC.sigmoid64(DR.split(t, K, C)[1])
    lp = DR.log_softmax(zs / T)
    want = 1.5 * T * T * (ct * (-np.log(C) - lp.mean(-1))).sum() / s.shape[0]
    assert abs(terms[0] - want) <= 1e-12 * abs(want) and terms[1] == 0.0 and terms[2] == 0.0
    gz = DR.split(grad, K, C)[0]
    np.testing.assert_allclose(gz, 1.5 * T * ct[..., None] * (np.exp(lp) - 1.0 / C) / s.shape[0], rtol=1e-12, atol=1e-18)


def test_the_floor_is_inclusive_on_the_tie_case():
    """ut = 0 under conf_floor 0.5: the anchor is kept with weight exactly 0.5 -- its class and box gradients are those of weight 0.5,
    not 0; the anchor below the floor gets none; the confidence gradient ignores the floor."""
    K, C, s, t, opt = case("ties")
    terms, grad = DR.distill_reference64(s, t, K, C, opt)
    gz, gu, gd = DR.split(grad, K, C)
    zs, us, ds = DR.split(s.astype(np.float64), K, C)
    zt, ut, dt = DR.split(t.astype(np.float64), K, C)
    for a in (0, 1):
        assert ut[0, a] == 0.0
        np.testing.assert_allclose(gd[0, a], 2.0 * 0.5 * (ds[0, a] - dt[0, a]), rtol=1e-15)
        assert np.abs(gz[0, a]).max() > 0.0
    assert not gz[0, 2].any() and not gd[0, 2].any() and gu[0, 2] != 0.0
    assert gz[0, 3:].any() and gd[0, 3:].all()


def test_a_floor_that_removes_all_anchors_leaves_only_the_confidence_term():
    K, C, s, t, _ = case("g3x5_k9_c3_b1")
    t = t.copy()
    tv = t.reshape(t.shape[0], -1, K * (C + 5))
    tv[..., K * C:K * (C + 1)] = np.minimum(tv[..., K * C:K * (C + 1)], 2.0)          # every teacher confidence <= sigmoid(2) < 0.9
    terms, grad = DR.distill_reference64(s, t, K, C, (1.0, 1.0, 1.0, 1.0, 0.9))
    gz, gu, gd = DR.split(grad, K, C)
    assert terms[0] == 0.0 and terms[2] == 0.0 and terms[1] > 0.0
    assert not gz.any() and not gd.any() and gu.all()
    A = gu.shape[1]
    np.testing.assert_allclose(gu, (DC.sigmoid64(DR.split(s, K, C)[1]) - DC.sigmoid64(DR.split(t, K, C)[1])) / (s.shape[0] * A), rtol=1e-13)


def test_extreme_logits_stay_finite():
    K, C, s, t, opt = case("extreme")
    assert opt[0] == 0.5 and np.abs(s).max() == 60000.0 and np.isfinite(s.astype(np.float16)).all()
    terms, grad = DR.distill_reference64(s, t, K, C, opt)
    assert np.isfinite(terms).all() and np.isfinite(grad).all()
    a_terms, a_grad = DR.distill_autograd64(s, t, K, C, opt)
    np.testing.assert_allclose(terms, a_terms, rtol=1e-12)
    assert np.abs(grad - a_grad).max() <= 1e-11 * np.abs(a_grad).max()
    # anchor 0: the teacher is certain of class 1, the student of class 0, 240000 apart in tempered logits: KL = 240000 exactly
    ct0 = DC.sigmoid64(-30.0)
    assert ct0 > 0.0
    f32_terms, f32_grad = DR.distill_torch32(s, t, K, C, opt)
    assert np.isfinite(f32_terms).all() and np.isfinite(f32_grad).all()


# ---------------------------------------------------------------- mutations: each caught by a named case
# (mutation, the case that catches it, what must move: index into terms or "grad")
CAUGHT_BY = [("drop_T2", "kitti_b2", 0), ("drop_T2", "g3x5_k1_c20_b3", "grad"), ("student_weight", "g3x5_k9_c3_b1", "grad"),
             ("student_weight", "g2x3_k1_c3_b1", 2), ("conf_no_A", "g2x3_k1_c3_b1", 1), ("conf_no_A", "g3x5_k9_c20_b3", "grad"),
             ("kl_reversed", "g3x5_k9_c3_b1", 0), ("kl_reversed", "g3x5_k1_c20_b3", "grad"), ("exclusive_floor", "ties", "grad"),
             ("exclusive_floor", "ties", 2)]


@pytest.mark.parametrize("mutate,name,what", CAUGHT_BY)
def test_cases_catch_the_mutation(mutate, name, what):
    """The mutated restatement differs from the stated one by more than 1e-3 of the quantity's size on the named case: a thousand
    times the GPU tests' allowance at these magnitudes."""
    good, bad = ref64(name), ref64(name, mutate=mutate)
    if what == "grad":
        assert np.abs(good[1] - bad[1]).max() > 1e-3 * np.abs(good[1]).max(), (mutate, name)
    else:
        assert abs(good[0][what] - bad[0][what]) > 1e-3 * abs(good[0][what]) > 0.0, (mutate, name)


def test_every_mutation_is_caught_and_only_the_floor_needs_the_tie():
    assert {m for m, _, _ in CAUGHT_BY} == set(DR.MUTATIONS)
    for name in DC.CASES:                                         # off the floor the exclusive comparison is invisible
        good, bad = ref64(name), ref64(name, mutate="exclusive_floor")
        assert np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])


# ---------------------------------------------------------------- options, compatibility
def test_config_default_and_the_options_record():
    from squeezedet_amd import config, distill
    from squeezedet_amd._lib import SqdetError
    assert config.kitti_squeezeDet_config().DISTILL is None and config.base_model_config("PASCAL_VOC").DISTILL is None
    assert distill.is_default(None) and distill.is_default({}) and not distill.is_default(dict(teacher_net="vgg16"))
    o = distill.distill_options()
    assert tuple(o) == (1.0, 1.0, 1.0, 1.0, 0.0)
    assert distill.from_dict(dict(distill.as_dict(o), teacher_net="vgg16", teacher_checkpoint="")) == o
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(class_coef=-0.1), dict(conf_coef=float("nan")), dict(bbox_coef=float("inf")),
                dict(class_coef=0.0, conf_coef=0.0, bbox_coef=0.0), dict(conf_floor=-0.01), dict(conf_floor=1.01), dict(conf_floor=float("nan"))):
        with pytest.raises(SqdetError):
            distill.distill_options(**bad)
    distill.distill_options(class_coef=0.0, conf_coef=0.0, bbox_coef=0.5, conf_floor=1.0)


def test_check_compatible_refuses_what_does_not_line_up():
    from squeezedet_amd import config, distill
    from squeezedet_amd._lib import SqdetError
    s = config.kitti_squeezeDet_config()
    # at 1248 x 384 the ResNet50 and VGG16 nets give the student's 24 x 78 grid; the teacher takes the student's anchor shapes
    for net in ("squeezeDet", "resnet50", "vgg16"):
        tmc = distill.teacher_config(net, s)
        assert config.anchor_grid(tmc) == (24, 78) and not tmc.IS_TRAINING
        distill.check_compatible(s, tmc)
    small = config.kitti_squeezeDet_config_for_input(128, 256)
    for net in ("squeezeDet", "resnet50", "vgg16"):
        distill.check_compatible(small, distill.teacher_config(net, small))
    # SqueezeDet+'s VALID convolution and pools give 22 x 76 there: refused, and the text carries both records
    plus = distill.teacher_config("squeezeDet+", s)
    assert config.anchor_grid(plus) == (22, 76) == config.anchor_grid(config.kitti_squeezeDetPlus_config())
    with pytest.raises(SqdetError, match=r"grid differs.*student.*\[24, 78\].*teacher.*\[22, 76\]"):
        distill.check_compatible(s, plus)
    other = type(s)(s)
    other.CLASSES = 4
    with pytest.raises(SqdetError, match="class count.*'classes': 3.*'classes': 4"):
        distill.check_compatible(s, other)
    fewer = config.with_anchor_shapes(s, config.SQUEEZEDET_ANCHOR_SHAPES[:8])
    with pytest.raises(SqdetError, match="number of anchors per cell"):
        distill.check_compatible(s, fewer)
    shapes = config.SQUEEZEDET_ANCHOR_SHAPES.copy()
    shapes[3, 0] += 1.0
    with pytest.raises(SqdetError, match="anchor boxes"):
        distill.check_compatible(s, config.with_anchor_shapes(s, shapes))
    with pytest.raises(SqdetError, match="anchor boxes"):           # the ResNet50 config's own shapes are not SqueezeDet's
        distill.check_compatible(s, config.kitti_res50_config_for_input(384, 1248))
    with pytest.raises(SqdetError, match="padded"):
        distill.teacher_config("vgg16", config.pad_head_classes(config.voc_squeezeDet_config_for_input(128, 256)))


# ---------------------------------------------------------------- flags, checkpoint key, resume
FLAGS = ["--teacher_net", "vgg16", "--teacher_checkpoint", "logs/vgg16", "--teacher_dtype", "fp16", "--distill_temperature", "2",
         "--distill_class_coef", "0.5", "--distill_conf_coef", "0.25", "--distill_bbox_coef", "3", "--distill_conf_floor", "0.3"]
POLICY = dict(teacher_net="vgg16", teacher_checkpoint="logs/vgg16", teacher_dtype="fp16", temperature=2.0, class_coef=0.5,
              conf_coef=0.25, bbox_coef=3.0, conf_floor=0.3)


def test_flags_absent_leave_everything_as_it_was():
    import train as T
    from squeezedet_amd import config, drivers
    a = T.parse_args([])
    assert not any(hasattr(a, k) for k in ("teacher_net",) + drivers.DISTILL_FLAGS)
    mc = config.kitti_squeezeDet_config()
    assert drivers.distill_policy(a, mc) == (None, None) and mc.DISTILL is None
    assert drivers.make_teacher(None, mc, 0) is None
    # the trainer's keyword defaults to None, and a step's outputs gain nothing
    import inspect
    from squeezedet_amd.train import _TrainerBase
    assert inspect.signature(_TrainerBase.__init__).parameters["teacher"].default is None


def test_flags_set_the_recorded_policy():
    import train as T
    from squeezedet_amd import config, drivers
    mc = config.kitti_squeezeDet_config()
    policy, off = drivers.distill_policy(T.parse_args(FLAGS), mc)
    assert policy == POLICY and off is None and mc.DISTILL == POLICY
    assert all(isinstance(policy[k], str) for k in ("teacher_net", "teacher_checkpoint", "teacher_dtype"))
    a = T.parse_args(["--synthetic", "8", "--dtype", "fp16", "--teacher_net", "resnet50"])
    policy, _ = drivers.distill_policy(a)
    assert policy == dict(teacher_net="resnet50", teacher_checkpoint="", teacher_dtype="fp16", temperature=1.0, class_coef=1.0,
                          conf_coef=1.0, bbox_coef=1.0, conf_floor=0.0)
    for bad in (["--teacher_net", "alexnet"], ["--distill_temperature", "2"], ["--teacher_checkpoint", "x.npz"],
                ["--teacher_net", "vgg16"],                                          # a dataset run needs the teacher's checkpoint
                ["--synthetic", "8", "--teacher_net", "vgg16", "--distill_temperature", "0"],
                ["--synthetic", "8", "--teacher_net", "vgg16", "--distill_conf_floor", "1.5"],
                ["--synthetic", "8", "--teacher_net", "vgg16", "--distill_bbox_coef", "-1"],
                ["--synthetic", "8", "--teacher_net", "vgg16", "--distill_class_coef", "0", "--distill_conf_coef", "0", "--distill_bbox_coef", "0"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)


def test_checkpoint_extra_keeps_the_policy_and_resume_refuses_another(tmp_path):
    import json
    import train as T
    from squeezedet_amd import config, drivers
    off = drivers.loss_policy(argparse.Namespace(), config.kitti_squeezeDet_config())[1]
    assert json.loads(json.dumps(dict(distill=POLICY)))["distill"] == POLICY
    base = dict(net="squeezeDet", dtype="fp32", augment=T.AUGMENT_OFF, mosaic=0.0, loss=off)
    T.check_resume_record(dict(base, distill=POLICY), dict(base, distill=POLICY), off)           # recorded and matching
    T.check_resume_record(dict(base), dict(base), off)                                           # neither: trained without a teacher
    with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with distill None, this run asks for .*vgg16"):
        T.check_resume_record(dict(base), dict(base, distill=POLICY), off)
    with pytest.raises(SystemExit, match="trained with distill .*vgg16.*this run asks for None"):
        T.check_resume_record(dict(base, distill=POLICY), dict(base), off)
    for key, v in (("temperature", 4.0), ("teacher_net", "resnet50"), ("conf_floor", 0.0), ("teacher_checkpoint", "elsewhere")):
        with pytest.raises(SystemExit, match="distill"):
            T.check_resume_record(dict(base, distill=POLICY), dict(base, distill=dict(POLICY, **{key: v})), off)
    with pytest.raises(SystemExit, match="mosaic"):                                              # the earlier keys still hold
        T.check_resume_record(dict(base, mosaic=0.5), dict(base), off)
    # a train dir as --teacher_checkpoint: its newest model file
    for step in (3, 12, 7):
        (tmp_path / ("model.ckpt-%d.npz" % step)).write_bytes(b"")
    assert drivers.teacher_checkpoint_file(str(tmp_path)) == str(tmp_path / "model.ckpt-12.npz")
    assert drivers.teacher_checkpoint_file(str(tmp_path / "model.ckpt-3.npz")) == str(tmp_path / "model.ckpt-3.npz")
    with pytest.raises(SystemExit):
        drivers.teacher_checkpoint_file(str(tmp_path / "nothing"))


def test_bench_train_takes_the_flags():
    from tools import bench_train as BT
    assert not hasattr(BT.parse_args([]), "teacher_net")
    a = BT.parse_args(["--teacher_net", "vgg16", "--distill_temperature", "2"])
    assert a.teacher_net == "vgg16" and a.distill_temperature == 2.0
    for bad in (["--distill_temperature", "2"], ["--teacher_net", "vgg16", "--distill_temperature", "-2"]):
        with pytest.raises(SystemExit):
            BT.parse_args(bad)
