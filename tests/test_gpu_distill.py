"""GPU tests of distillation (sqdet_distill_fwd_bwd, distill_kernel in squeezedet_amd/csrc/loss.hip) against
the float64 restatement of tests/distill_reference.py on the cases of tests/distill_cases.py.

The metric and the bound are those of tests/test_gpu_loss_options.py: the error of a quantity -- the three terms, the gradient -- is
its largest absolute element error against float64; e_ref is that error of the float32 torch-CPU evaluation of the same formulas
(distill_torch32) on the same inputs; the kernel's must be at most 4 * e_ref + 1e-7.  The cases' values are exact in float16, so the
four dtype pairs (student x teacher in float32 / float16) read the same numbers and share one reference per case.

Measured on an MI355X (kernel error / e_ref; the four dtype pairs give the same figures, to the bit):

  case              terms {class, conf, box}            terms                  gradient               max |g|
  g2x3_k1_c3_b1     0.5272   0.10144  17.0681           2.90e-07 / 2.90e-07    3.09e-07 / 3.09e-07    3.79
  g2x3_k9_c1_b3     0        0.05770  242.980           8.11e-06 / 2.34e-05    1.59e-07 / 3.67e-07    4.29
  g3x5_k1_c20_b3    2.43679  0        39.68864          1.43e-06 / 1.34e-06    1.28e-07 / 1.28e-07    2.2
  g3x5_k9_c3_b1     11.19705 0.11952  0                 3.80e-08 / 3.80e-08    9.34e-08 / 1.51e-07    0.594
  g3x5_k9_c20_b3    0        0.33783  297.06931         1.31e-06 / 1.31e-06    1.63e-07 / 2.61e-07    2.02
  kitti_b2          2364.02  0.12019  29422.3           4.43e-04 / 1.51e-03    3.30e-07 / 3.30e-07    4.39

(The terms' error is that of the largest term; at the full grid the box term is 2.9e4, so 4.4e-4 is 1.5e-8 of it.)

Beyond that: run onto zeros the kernel writes g, run onto a loss's dpreds exactly float32(dp + g), and the float16 copy is
convert_scale's expression of that sum; two runs give the same bits; global_batch = 2 * batch halves every output exactly; every
refusal returns SQDET_EINVAL with the canaries around dpreds, distill3 and the workspace intact (they are intact after a good run
too); the hand-worked cases hold on the device; and a SqueezeDet student with a VGG16+ConvDet teacher trains to the same bits eager,
graphed and resumed, in float32 and mixed precision, with the teacher's variables untouched.  (The entry point exposes no grid size,
as the loss's does not: there is no one-workgroup variant to compare.)  SqueezeDet+ cannot teach SqueezeDet: its grid is 22 x 76
where the other three nets' is 24 x 78, and the pair is refused.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import distill_cases as DC, distill_reference as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float16, torch.float32), (torch.float16, torch.float16)]
PAIR_IDS = ["s32_t32", "s32_t16", "s16_t32", "s16_t16"]
CANARY = -123.456
_CACHE = {}


def _ops():
    from squeezedet_amd import ops
    return ops


def _opt(o):
    from squeezedet_amd.distill import DistillOptions
    return DistillOptions(*[float(v) for v in o])


def case(name):
    if name not in _CACHE:
        _CACHE[name] = {"ties": DC.tie_case, "extreme": DC.extreme_case}.get(name, lambda: DC.distill_case(name))()
    return _CACHE[name]


def refs(name):
    """(float64 reference, the float32 torch-CPU evaluation's error against it), once per case."""
    key = ("ref", name)
    if key not in _CACHE:
        K, C, s, t, opt = case(name)
        ref = DR.distill_reference64(s, t, K, C, opt)
        f32 = DR.distill_torch32(s, t, K, C, opt)
        _CACHE[key] = (ref, [float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(f32, ref)])
    return _CACHE[key]


def dev(name, sdt, tdt):
    key = ("dev", name, sdt, tdt)
    if key not in _CACHE:
        _, _, s, t, _ = case(name)
        _CACHE[key] = (torch.from_numpy(s).to(DEV, sdt), torch.from_numpy(t).to(DEV, tdt))
    return _CACHE[key]


def run_kernel(name, sdt=torch.float32, tdt=torch.float32, onto=None, loss_scale=1.0, global_batch=0, opt=None):
    """(g16 or None, dpreds, distill3) of one call onto `onto` (default zeros)."""
    ops = _ops()
    K, C, _, _, o = case(name)
    s, t = dev(name, sdt, tdt)
    dp = torch.zeros(s.shape, dtype=torch.float32, device=DEV) if onto is None else onto.clone()
    g16 = torch.full(s.shape, float("nan"), dtype=torch.float16, device=DEV) if sdt == torch.float16 else None
    d3 = ops.distill_fwd_bwd(s, t, dp, K, C, _opt(o if opt is None else opt), g16=g16, loss_scale=loss_scale, global_batch=global_batch)
    torch.cuda.synchronize()
    return g16, dp, d3


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(view), b.view(view)), "%s: bits differ" % what


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", list(DC.CASES))
def test_distill_against_float64_within_four_times_the_float32_evaluations_error(name):
    (ref_terms, ref_grad), e_ref = refs(name)
    failures = []
    for (sdt, tdt), pid in zip(PAIRS, PAIR_IDS):
        _, dp, d3 = run_kernel(name, sdt, tdt)
        got = (d3.cpu().numpy(), dp.cpu().numpy())
        assert all(np.isfinite(g).all() for g in got), (name, pid)
        e_gpu = [float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, (ref_terms, ref_grad))]
        print("DISTILL %-16s %-8s terms %s | kernel err / e_ref: terms %.2e / %.2e  gradient %.2e / %.2e (max |g| %.3g)"
              % (name, pid, np.array2string(ref_terms, precision=5), e_gpu[0], e_ref[0], e_gpu[1], e_ref[1], np.abs(ref_grad).max()))
        for what, eg, er in zip(("terms", "gradient"), e_gpu, e_ref):
            if not eg <= 4.0 * er + 1e-7:
                failures.append("%s %s %s: kernel error %g, float32 evaluation's error %g" % (name, pid, what, eg, er))
    assert not failures, "\n".join(failures)


def test_dtype_pairs_agree_bit_for_bit_on_float16_exact_values():
    """The arithmetic is float32 on the stored values, whatever the storage: the four pairs give the same float32 bits."""
    name = "g3x5_k9_c20_b3"
    want = run_kernel(name)
    for sdt, tdt in PAIRS[1:]:
        _, dp, d3 = run_kernel(name, sdt, tdt)
        _same(dp, want[1], "gradient")
        _same(d3, want[2], "terms")


# ---------------------------------------------------------------- hand-worked cases on the device
def test_one_class_and_equal_teacher_give_exact_zeros():
    K, C, s, t, opt = case("g2x3_k9_c1_b3")
    _, dp, d3 = run_kernel("g2x3_k9_c1_b3")
    gz = DR.split(dp.cpu().numpy(), K, C)[0]
    assert float(d3[0]) == 0.0 and not gz.any() and float(d3[1]) > 0.0 and float(d3[2]) > 0.0
    ops = _ops()
    for name in ("g3x5_k9_c20_b3", "kitti_b2"):
        K, C, _, _, opt = case(name)
        for sdt, tdt in PAIRS:
            s = dev(name, sdt, tdt)[0]
            dp = torch.zeros(s.shape, dtype=torch.float32, device=DEV)
            g16 = torch.empty_like(s) if sdt == torch.float16 else None
            d3 = ops.distill_fwd_bwd(s, s.to(tdt), dp, K, C, _opt(opt), g16=g16, loss_scale=64.0)
            assert not bool(d3.any()) and not bool(dp.any()) and (g16 is None or not bool(g16.any())), (name, sdt, tdt)


def test_the_floor_is_inclusive_and_extreme_logits_stay_finite():
    K, C, s, t, opt = case("ties")
    ref_terms, ref_grad = DR.distill_reference64(s, t, K, C, opt)
    excl = DR.distill_reference64(s, t, K, C, opt, mutate="exclusive_floor")
    _, dp, d3 = run_kernel("ties")
    got = dp.cpu().numpy()
    scale = np.abs(ref_grad).max()
    assert np.abs(got - ref_grad).max() <= 1e-5 * scale and np.abs(got - excl[1]).max() > 1e-2 * scale
    np.testing.assert_allclose(d3.cpu().numpy(), ref_terms, rtol=1e-5)
    K, C, s, t, opt = case("extreme")
    ref_terms, ref_grad = DR.distill_reference64(s, t, K, C, opt)
    for sdt, tdt in PAIRS:
        g16, dp, d3 = run_kernel("extreme", sdt, tdt)
        assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(d3).all()) and (g16 is None or bool(torch.isfinite(g16).all()))
        np.testing.assert_allclose(d3.cpu().numpy(), ref_terms, rtol=1e-5)
        assert np.abs(dp.cpu().numpy() - ref_grad).max() <= 1e-5 * np.abs(ref_grad).max()


# ---------------------------------------------------------------- bitwise properties
@pytest.mark.parametrize("name", ["g3x5_k1_c20_b3", "kitti_b2"])
def test_adds_onto_dpreds_and_writes_convert_scales_float16_copy(name):
    ops = _ops()
    rs = torch.Generator(device="cpu").manual_seed(5)
    K, C, s, _, _ = case(name)
    onto = (torch.randn(s.shape, generator=rs) * 0.01).to(DEV)
    _, g, d3 = run_kernel(name)
    assert bool(g.any())
    _, dp, d3b = run_kernel(name, onto=onto)
    _same(dp, onto + g, "dpreds = float32(dp + g)")
    _same(d3b, d3, "terms do not depend on dpreds")
    for scale in (512.0, 65536.0):
        for tdt in (torch.float32, torch.float16):
            g16, dp16, d3c = run_kernel(name, torch.float16, tdt, onto=onto, loss_scale=scale)
            _same(dp16, dp, "float32 dpreds of the float16 student")
            # (sqdet_convert_scale takes multiples of four elements; the smaller case has 1125: padded for the call)
            flat = torch.cat([dp.reshape(-1), torch.zeros((-dp.numel()) % 4, device=DEV)])
            want = ops.convert_scale(flat, torch.float16, scale)[:dp.numel()].reshape(dp.shape).contiguous()
            _same(g16, want, "float16 copy at scale %g" % scale)
            _same(d3c, d3, "terms")
    again = run_kernel(name, onto=onto)
    _same(again[1], dp, "second run: dpreds")
    _same(again[2], d3, "second run: terms")


@pytest.mark.parametrize("name", ["g3x5_k9_c3_b1", "g3x5_k9_c20_b3", "kitti_b2"])
def test_twice_the_global_batch_halves_everything_exactly(name):
    B = case(name)[2].shape[0]
    for sdt, tdt in (PAIRS[0], PAIRS[3]):
        _, g1, t1 = run_kernel(name, sdt, tdt, global_batch=B)
        _, g0, t0 = run_kernel(name, sdt, tdt)
        _, g2, t2 = run_kernel(name, sdt, tdt, global_batch=2 * B)
        _same(g0, g1, "global_batch = batch is the default")
        _same(g2 * 2.0, g1, "gradient")
        _same(t2 * 2.0, t1, "terms")
        assert bool(g1.any()) and bool(t1.any())


def _guarded(n, dtype=torch.float32, pad=256):
    """A tensor of n elements with `pad` canary elements on either side: (whole buffer, the view in the middle)."""
    buf = torch.full((n + 2 * pad,), CANARY, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + n]


def _raw_call(name, o, sdt=torch.float32, tdt=torch.float32, preds_code=None, teacher_code=None, g16=True, loss_scale=8.0):
    """sqdet_distill_fwd_bwd itself on guarded buffers; returns (rc, the guarded buffers, the middles)."""
    ops = _ops()
    from squeezedet_amd._lib import dtype_code, lib
    K, C, s_np, _, _ = case(name)
    s, t = dev(name, sdt, tdt)
    B, gh, gw, ch = s.shape
    bufs = [_guarded(s.numel()), _guarded(3), _guarded(int(lib().sqdet_distill_workspace_bytes()) // 4), _guarded(s.numel(), torch.float16)]
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib().sqdet_distill_fwd_bwd(ptr(s), dtype_code(sdt) if preds_code is None else preds_code, ptr(t),
                                     dtype_code(tdt) if teacher_code is None else teacher_code, ptr(bufs[0][1]),
                                     ptr(bufs[3][1]) if g16 else None, float(loss_scale), ptr(bufs[1][1]), ptr(bufs[2][1]), B, gh, gw, K, C, 0,
                                     ctypes.cast(ctypes.pointer(o), ctypes.c_void_p), ops.stream_ptr())
    torch.cuda.synchronize()
    return rc, bufs


NAN, INF = float("nan"), float("inf")
BAD = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=NAN), dict(temperature=INF), dict(class_coef=-1.0),
       dict(conf_coef=NAN), dict(bbox_coef=INF), dict(class_coef=0.0, conf_coef=0.0, bbox_coef=0.0), dict(conf_floor=-0.5),
       dict(conf_floor=1.5), dict(conf_floor=NAN), dict(preds_code=2), dict(teacher_code=-1), dict(sdt=torch.float16, g16=False),
       dict(sdt=torch.float16, loss_scale=0.0)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_refusals_return_einval_and_leave_the_canaries(bad):
    ops = _ops()
    fields = dict(temperature=1.0, class_coef=1.0, conf_coef=1.0, bbox_coef=1.0, conf_floor=0.0)
    call = {k: bad[k] for k in bad if k not in fields}
    fields.update({k: bad[k] for k in bad if k in fields})
    rc, bufs = _raw_call("g3x5_k9_c3_b1", ops._DistillOptions(**fields), **call)
    assert rc == -1                                               # SQDET_EINVAL
    for whole, _ in bufs:
        assert bool((whole == CANARY).all())


def test_a_good_run_stays_inside_its_buffers():
    ops = _ops()
    for name in ("g2x3_k1_c3_b1", "kitti_b2"):
        rc, bufs = _raw_call(name, ops._DistillOptions(2.0, 1.0, 1.0, 1.0, 0.3), sdt=torch.float16, tdt=torch.float16)
        assert rc == 0
        for (whole, mid), pad in zip(bufs, (256,) * 4):
            assert bool((whole[:pad] == CANARY).all()) and bool((whole[-pad:] == CANARY).all())
        assert not bool((bufs[1][1] == CANARY).any()) and not bool((bufs[3][1] == CANARY).any())
    from squeezedet_amd._lib import SqdetError
    K, C, _, _, o = case("g2x3_k1_c3_b1")
    s, t = dev("g2x3_k1_c3_b1", torch.float32, torch.float32)
    with pytest.raises(SqdetError):                               # through ops: a wrong shape, a wrong head
        ops.distill_fwd_bwd(s, t[:, :1].contiguous(), torch.zeros_like(s), K, C, _opt(o))
    with pytest.raises(SqdetError):
        ops.distill_fwd_bwd(s, t, torch.zeros_like(s), K, C + 1, _opt(o))


# ---------------------------------------------------------------- the trainers
def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TERMS = ("distill_class_loss", "distill_conf_loss", "distill_bbox_loss")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_squeezedet_with_a_vgg16_teacher_is_bitwise_eager_graphed_and_resumed(tmp_path, dtype):
    """SqueezeDet at the trainers' small shape (2 x 128 x 256) with a VGG16+ConvDet teacher (the same 8 x 16 grid; synthetic variables),
    temperature 2, floor 0.3: three steps graphed == three steps eager, bit for bit (the teacher's forward runs ahead of the replay and
    the captured step holds the distill launch); a run resumed from the checkpoint of step 2 computes step 3's bits; the teacher's
    variables never change; the reported terms and dpreds are the kernel's on the step's tensors; the checkpoint refuses another
    policy and a run without a teacher; SqueezeDet+ is refused for its grid."""
    T = _load("train")
    ops = _ops()
    flags = ["--dtype", dtype, "--teacher_net", "vgg16", "--distill_temperature", "2", "--distill_conf_floor", "0.3"]
    args = lambda d, *more: T.parse_args(["--synthetic", "12", "--seed", "3", "--train_dir", str(d), "--summary_step", "0",
                                          "--image_size", "128", "256", "--batch_size", "2"] + list(more))

    def state(run):
        run.tr.flush()
        torch.cuda.synchronize()
        return run.tr.flat_params.clone().view(torch.int32), run.tr.flat_accum.clone().view(torch.int32), run.tr.global_step

    a_args = args(tmp_path / "graphed", *flags)
    os.makedirs(a_args.train_dir)
    a = T.Run(a_args)
    assert a.stepper is not None and a.tr.teacher is a.teacher and a.teacher.net == "vgg16" and a.extra["distill"]["temperature"] == 2.0
    assert a.teacher.model.keep_prob == 1.0 and a.teacher.model.dtype == a.model.dtype
    before = {n: p.clone() for n, p in a.teacher.model.params.items()}
    for s in range(3):
        out = a.step(s)
    terms = [float(out[k]) for k in TERMS]
    assert np.isfinite(terms).all() and all(v > 0.0 for v in terms)
    assert abs(a.total_loss(out) - sum(float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss") + TERMS)) < 1.0      # (+ the weight decay)
    after3 = state(a)
    a.save(2)
    a.step(3)
    after4 = state(a)
    for n, p in a.teacher.model.params.items():
        assert torch.equal(p, before[n]), n
    a.close()
    del a
    b = T.Run(args(tmp_path / "eager", "--no_graph", *flags))
    assert b.stepper is None
    for s in range(3):
        b.step(s)
    got3 = state(b)
    assert got3[2] == after3[2] == 3 and torch.equal(got3[0], after3[0]) and torch.equal(got3[1], after3[1])
    # one more eager step by hand: its dpreds and terms are the loss launch's followed by the kernel's on the same tensors
    tr, mc = b.tr, b.mc
    batch = b.reader.read_batch()
    labels = ops.build_labels(b.anchors, batch.gt_boxes, batch.gt_classes, batch.gt_counts, mc.CLASSES, anchors_per_grid=int(mc.ANCHOR_PER_GRID))
    out = tr.step(batch.image_input, *labels[:4], apply_update=False)
    mask, delta, box, lab = [x.to(DEV, torch.float32).contiguous() for x in labels[:4]]
    mask = mask.reshape(2, -1)
    tp = b.teacher.preds(batch.image_input)
    if dtype == "fp16":
        g16, dp0, _, _ = ops.loss_fwd_bwd_mixed(out["preds"], b.model.anchors_f32(), mask, delta, box, lab, mc, out["num_objects"], tr.loss_scale)
    else:
        g16, (dp0, _, _) = None, ops.loss_fwd_bwd(out["preds"], b.model.anchors_f32(), mask, delta, box, lab, mc, out["num_objects"])
    d3 = ops.distill_fwd_bwd(out["preds"], tp, dp0, mc.ANCHOR_PER_GRID, mc.CLASSES, b.teacher.options, g16=g16, loss_scale=tr.loss_scale)
    torch.cuda.synchronize()
    _same(out["dpreds"], dp0, "the step's dpreds")
    for k, v in zip(TERMS, d3):
        assert float(out[k]) == float(v), k
    b.close()
    del b
    c = T.Run(a_args, resume_step=2)
    assert c.first == 3
    c.step(3)
    got4 = state(c)
    c.close()
    del c
    assert got4[2] == after4[2] and torch.equal(got4[0], after4[0]) and torch.equal(got4[1], after4[1])
    assert not torch.equal(after4[0], after3[0])
    with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with distill"):
        T.Run(args(tmp_path / "graphed", *(flags[:-1] + ["0.5"])), resume_step=2)
    with pytest.raises(SystemExit, match="trained with distill .*this run asks for None"):
        T.Run(args(tmp_path / "graphed", "--dtype", dtype), resume_step=2)
    if dtype == "fp32":
        with pytest.raises(SystemExit, match="--teacher_net: distill: the teacher's grid differs"):
            T.Run(args(tmp_path / "plus", "--teacher_net", "squeezeDet+"))


def test_a_run_without_a_teacher_is_what_it_was(tmp_path):
    """No --teacher_net: no teacher is built, the step's outputs and the checkpoint's record have no distillation key, the result
    does not depend on the feature (two such runs agree bit for bit) -- and a teacher does change the weights."""
    T = _load("train")
    args = lambda d, *more: T.parse_args(["--synthetic", "12", "--seed", "3", "--train_dir", str(d), "--summary_step", "0",
                                          "--image_size", "128", "256", "--batch_size", "2"] + list(more))
    params = []
    for d, more in (("plain", ()), ("plain2", ("--no_graph",)), ("taught", ("--teacher_net", "squeezeDet", "--summary_step", "1"))):
        run = T.Run(args(tmp_path / d, *more))
        assert (run.teacher is None) == (d != "taught") and (run.tr.teacher is None) == (d != "taught")
        assert ("distill" in run.extra) == (d == "taught") and run.mc.DISTILL == run.extra.get("distill")
        for s in range(2):
            out = run.step(s)
        assert all((k in out) == (d == "taught") for k in TERMS)
        run.tr.flush()
        torch.cuda.synchronize()
        params.append(run.tr.flat_params.clone().view(torch.int32))
        run.close()
        if d == "taught":                                         # the summaries' line carries the three terms and adds them to `loss`
            line = run.summary.last
            assert [line[k] for k in TERMS] == [float(out[k]) for k in TERMS]
            parts = [line[k] for k in ("class_loss", "conf_loss", "bbox_loss") + TERMS] + [line["weight_decay_loss"]]
            assert abs(line["loss"] - sum(parts)) <= 1e-9 * abs(line["loss"])
        del run
    assert torch.equal(params[0], params[1]) and not torch.equal(params[0], params[2])
