"""GPU tests of the loss with options (sqdet_loss_fwd_bwd_opt, loss_kernel<PT, true> in squeezedet_amd/csrc/loss.hip; DESIGN.md
section 3.16): IoU / GIoU / DIoU / CIoU box terms and the focal class term, against the float64 restatement of
tests/loss_options_reference.py on the cases of tests/loss_options_cases.py.

The metric and the bound are those of test_loss_against_float64_within_four_times_the_float32_oracles_error
(tests/test_gpu_train_kernels.py): the error of a quantity -- the three losses, ious, dpreds -- is its largest absolute element
error against float64; e_ref is that error of the float32 torch-CPU evaluation of the same formulas (loss_options_torch) on
the same inputs; the kernel's must be at most 4 * e_ref + 1e-7 (a different but equally valid float32 order, expf / logf / atanf /
powf an ulp apart).  Measured on an MI355X, the worst option pair of each case (kernel error / e_ref):

  case              worst pair      losses                 ious                   dpreds
  g2x3_k1_c3_b1     delta_l2 g=0.5  3.12e-06 / 4.08e-06    4.68e-07 / 4.68e-07    3.17e-06 / 3.17e-06
  g2x3_k9_c1_b3     giou g=0        2.28e-06 / 2.28e-06    2.96e-07 / 2.96e-07    2.05e-07 / 1.48e-07
  g3x5_k1_c20_b3    delta_l2 g=0.5  1.59e-06 / 5.70e-07    1.44e-07 / 1.44e-07    3.77e-07 / 4.37e-07
  g3x5_k9_c3_b1     delta_l2 g=0.5  7.97e-07 / 4.61e-06    8.28e-07 / 8.28e-07    1.69e-06 / 1.65e-06
  g3x5_k9_c20_b3    iou g=0         2.82e-06 / 9.90e-07    1.08e-06 / 1.08e-06    2.43e-07 / 2.43e-07
  kitti_b8          delta_l2 g=0.5  5.26e-06 / 5.26e-06    1.87e-06 / 1.87e-06    2.32e-07 / 2.45e-07

("Worst" is the pair whose kernel error comes closest to its allowance.  Over all 75 case / option pairs the kernel's error is
within 4 * e_ref + 1e-7 everywhere; for ious and, in most pairs, dpreds the two float32 evaluations err by the same amount to
the digit: the decode is the same float32 expression.)

Beyond that: the defaults through the new entry are the bits of the three existing entries; the mixed form is bitwise convert ->
loss -> convert; num_objects from the device gives the host's bits; global_batch shares add up to the full batch; bad options
are refused with dpreds untouched; the tie case follows the stated rule; and a SqueezeDet run with giou + gamma 2 is bitwise
the same eager, graphed and resumed.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from squeezedet_amd.ops import BOX_LOSSES               # (sqdet_loss_options_t.box_loss by index)
from tests import loss_options_cases as LC, loss_options_reference as LR

assert BOX_LOSSES == LR.BOX_LOSSES
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = list(BOX_LOSSES)
GAMMAS = [0.0, 0.5, 2.0]
ALL_OPTIONS = [(k, g) for k in KINDS for g in GAMMAS if (k, g) != ("delta_l2", 0.0)]
# the full grid's float64 and float32 CPU evaluations take a second each: five option pairs that between them run every kind and gamma
KITTI_OPTIONS = [("ciou", 2.0), ("giou", 0.5), ("diou", 0.0), ("iou", 2.0), ("delta_l2", 0.5)]
_CACHE = {}


def _ops():
    from squeezedet_amd import ops
    return ops


def case(name):
    if name not in _CACHE:
        _CACHE[name] = LC.tie_case() if name == "ties" else LC.loss_case(name)[:6]
    return _CACHE[name]


def with_options(mc, kind, gamma):
    mc = type(mc)(mc)
    mc.BBOX_LOSS, mc.FOCAL_GAMMA = kind, gamma
    return mc


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_args(name):
    """(preds, (anchors, mask, delta, box, labels)) on the device, once per case."""
    key = ("dev", name)
    if key not in _CACHE:
        mc, preds, mask, delta, box, labels = case(name)
        B = preds.shape[0]
        _CACHE[key] = (t(preds), (t(np.asarray(mc.ANCHOR_BOX).astype(np.float32)), t(mask.reshape(B, -1)), t(delta), t(box), t(labels)))
    return _CACHE[key]


def run_kernel(name, kind, gamma, nobj=None, global_batch=0):
    ops = _ops()
    mc, preds, mask = case(name)[:3]
    p, args = device_args(name)
    nobj = float(mask.sum()) if nobj is None else nobj
    dp, ious, losses = ops.loss_fwd_bwd(p, *args, with_options(mc, kind, gamma), nobj, global_batch=global_batch)
    torch.cuda.synchronize()
    return dp, ious, losses


def loss_errors(got, ref):
    return [float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, ref)]


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    assert torch.equal(a.view(view), b.view(view)), "%s: bits differ" % what


# ---------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", list(LC.CASES))
def test_loss_options_against_float64_within_four_times_the_float32_evaluations_error(name):
    mc, preds, mask, delta, box, labels = case(name)
    worst = None
    failures = []
    for kind, gamma in (KITTI_OPTIONS if name == "kitti_b8" else ALL_OPTIONS):
        ref = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss=kind, gamma=gamma)
        e_ref = loss_errors(LR.loss_options_torch(mc, preds, mask, delta, box, labels, box_loss=kind, gamma=gamma, dtype=torch.float32), ref)
        dp, ious, losses = run_kernel(name, kind, gamma)
        got = (losses.cpu().numpy(), ious.cpu().numpy(), dp.cpu().numpy())
        e_gpu = loss_errors(got, ref)
        print("LOSSOPT %-16s %-8s g=%-3g losses %s | kernel err / e_ref: losses %.2e / %.2e  ious %.2e / %.2e  dpreds %.2e / %.2e (max |dpreds| %.3g)"
              % (name, kind, gamma, np.array2string(ref[0], precision=5), e_gpu[0], e_ref[0], e_gpu[1], e_ref[1], e_gpu[2], e_ref[2], np.abs(ref[2]).max()))
        assert all(np.isfinite(g).all() for g in got), (name, kind, gamma)
        for what, eg, er in zip(("losses", "ious", "dpreds"), e_gpu, e_ref):
            if not eg <= 4.0 * er + 1e-7:
                failures.append("%s %s g=%g %s: kernel error %g, float32 evaluation's error %g" % (name, kind, gamma, what, eg, er))
        ratio = max(eg / (4.0 * er + 1e-7) for eg, er in zip(e_gpu, e_ref))
        if worst is None or ratio > worst[0]:
            worst = (ratio, kind, gamma, e_gpu, e_ref)
    print("LOSSOPT-WORST %-16s %-5s g=%-3g  %.2e / %.2e    %.2e / %.2e    %.2e / %.2e"
          % ((name, worst[1], worst[2]) + tuple(v for pair in zip(worst[3], worst[4]) for v in pair)))
    assert not failures, "\n".join(failures)


def test_tie_case_follows_the_stated_rule():
    """On exact ties (tests/loss_options_cases.py tie_case: small integers, exact in float32) the kernel's gradient is the
    restatement's under the stated rule -- to 1e-5 of the largest gradient, far inside the gap to the swapped rule's -- and the
    losses are finite and the restatement's."""
    mc, preds, mask, delta, box, labels = case("ties")
    for kind in KINDS[1:]:
        ref = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss=kind)
        swapped = LR.loss_options_reference64(mc, preds, mask, delta, box, labels, box_loss=kind, mutate="tie_swapped")
        dp, ious, losses = run_kernel("ties", kind, 0.0)
        got = (losses.cpu().numpy(), ious.cpu().numpy(), dp.cpu().numpy())
        assert all(np.isfinite(g).all() for g in got)
        np.testing.assert_allclose(got[0], ref[0], rtol=1e-5)
        np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=1e-6)
        scale = np.abs(ref[2]).max()
        assert np.abs(got[2] - ref[2]).max() <= 1e-5 * scale, kind
        assert np.abs(got[2] - swapped[2]).max() > 1e-3 * scale, kind


# ---------------------------------------------------------------- the contracts of the entry point
def _opt_call(name, kind, gamma, nobj, half=False, loss_scale=1.0, global_batch=0, dpreds=None):
    """sqdet_loss_fwd_bwd_opt itself (ops._loss_fwd_bwd_opt: no dispatch on the defaults in Python)."""
    ops = _ops()
    from squeezedet_amd._lib import lib
    mc = case(name)[0]
    p, args = device_args(name)
    if half:
        p = p.to(torch.float16)
    B, A = p.shape[0], mc.ANCHORS
    dpreds = torch.empty(p.shape, dtype=torch.float32, device=DEV) if dpreds is None else dpreds
    g16 = torch.empty_like(p) if half else None
    ious, losses = torch.empty((B, A), dtype=torch.float32, device=DEV), torch.empty(3, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib().sqdet_loss_workspace_bytes()) // 4 + 16, dtype=torch.float32, device=DEV)
    ops._loss_fwd_bwd_opt((kind, gamma), p, *args, mc, nobj, dpreds, g16, loss_scale, ious, losses, ws, global_batch)
    torch.cuda.synchronize()
    return g16, dpreds, ious, losses


@pytest.mark.parametrize("name", ["g3x5_k9_c20_b3", "kitti_b8"])
def test_defaults_through_the_new_entry_are_the_bits_of_the_existing_entries(name):
    ops = _ops()
    mc, preds, mask = case(name)[:3]
    p, args = device_args(name)
    host, dev = float(mask.sum()), ops.sum_f32(t(mask))
    for nobj in (host, dev):                                     # sqdet_loss_fwd_bwd and sqdet_loss_fwd_bwd_dev
        want = ops.loss_fwd_bwd(p, *args, mc, nobj, global_batch=11)
        _, dp, ious, losses = _opt_call(name, "delta_l2", 0.0, nobj, global_batch=11)
        for g, w, what in zip((dp, ious, losses), want, ("dpreds", "ious", "losses")):
            _same(g, w, what)
        want = ops.loss_fwd_bwd_mixed(p.to(torch.float16), *args, mc, nobj, 512.0)      # sqdet_loss_fwd_bwd_mixed
        got = _opt_call(name, "delta_l2", 0.0, nobj, half=True, loss_scale=512.0)
        for g, w, what in zip(got, want, ("g16", "dpreds", "ious", "losses")):
            _same(g, w, what)


@pytest.mark.parametrize("loss_scale", [512.0, 65536.0])
def test_mixed_form_is_convert_loss_convert(loss_scale):
    """At the full grid with B = 8 (the grid-stride loop, 512 workgroups, eight laps of loss_finish_kernel), ciou + gamma 2, the
    host and the device num_objects: float16 preds in, float32 dpreds and their loss-scaled float16 copy out, bit for bit."""
    ops = _ops()
    mc, preds, mask = case("kitti_b8")[:3]
    mc = with_options(mc, "ciou", 2.0)
    p, args = device_args("kitti_b8")
    p16 = p.to(torch.float16)
    for nobj in (float(mask.sum()), ops.sum_f32(t(mask))):
        dp, ious, losses = ops.loss_fwd_bwd(ops.convert_scale(p16, torch.float32), *args, mc, nobj)
        want = ops.convert_scale(dp, torch.float16, loss_scale)
        g16, dp2, ious2, losses2 = ops.loss_fwd_bwd_mixed(p16, *args, mc, nobj, loss_scale)
        torch.cuda.synchronize()
        _same(g16, want, "g16 at scale %g" % loss_scale)
        _same(dp2, dp, "dpreds")
        _same(ious2, ious, "ious")
        _same(losses2, losses, "losses")
        assert bool(torch.isfinite(dp).all())


@pytest.mark.parametrize("name", ["g2x3_k1_c3_b1", "kitti_b8"])
def test_num_objects_from_the_device_gives_the_hosts_bits(name):
    ops = _ops()
    mask = case(name)[2]
    for kind, gamma in (("giou", 2.0), ("ciou", 0.0), ("delta_l2", 0.5)):
        a = run_kernel(name, kind, gamma)
        b = run_kernel(name, kind, gamma, nobj=ops.sum_f32(t(mask)))
        for x, y, what in zip(a, b, ("dpreds", "ious", "losses")):
            _same(x, y, what)
        c = run_kernel(name, kind, gamma)                         # and again: deterministic
        for x, y, what in zip(a, c, ("dpreds", "ious", "losses")):
            _same(x, y, what)


@pytest.mark.parametrize("name", ["g3x5_k1_c20_b3", "kitti_b8"])
def test_global_batch_shares_add_up_to_the_full_batch(name):
    """Each image as its own replica's batch, with the GLOBAL num_objects and global_batch = B: every replica's dpreds and ious
    are the full batch's rows bit for bit (an anchor's terms depend on nothing else), and the losses add up to the full batch's
    (to float32 summation: 1e-5)."""
    ops = _ops()
    mc, preds, mask = case(name)[:3]
    B = preds.shape[0]
    mc = with_options(mc, "diou", 2.0)
    p, args = device_args(name)
    nobj = float(mask.sum())
    full = ops.loss_fwd_bwd(p, *args, mc, nobj)
    total = torch.zeros(3, dtype=torch.float64)
    for b in range(B):
        dp, ious, losses = ops.loss_fwd_bwd(p[b:b + 1].contiguous(), args[0], *[x[b:b + 1].contiguous() for x in args[1:]], mc, nobj, global_batch=B)
        _same(dp, full[0][b:b + 1].contiguous(), "dpreds of image %d" % b)
        _same(ious, full[1][b:b + 1].contiguous(), "ious of image %d" % b)
        total += losses.double().cpu()
    np.testing.assert_allclose(total.numpy(), full[2].double().cpu().numpy(), rtol=1e-5)


@pytest.mark.parametrize("bad", [("box_loss", 5), ("box_loss", -1), ("gamma", -0.5), ("gamma", float("nan")), ("gamma", float("inf"))])
def test_bad_options_are_refused_and_dpreds_stays_untouched(bad):
    ops = _ops()
    from squeezedet_amd._lib import SqdetError, lib
    name = "g2x3_k1_c3_b1"
    mc, preds, mask = case(name)[:3]
    p, args = device_args(name)
    o = ops._LossOptions(bad[1] if bad[0] == "box_loss" else 2, bad[1] if bad[0] == "gamma" else 0.0)
    dpreds = torch.full(p.shape, -123.456, dtype=torch.float32, device=DEV)
    ious, losses = torch.full((1, mc.ANCHORS), -1.0, device=DEV), torch.full((3,), -1.0, device=DEV)
    ws = torch.empty(int(lib().sqdet_loss_workspace_bytes()) // 4 + 16, dtype=torch.float32, device=DEV)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = lib().sqdet_loss_fwd_bwd_opt(ptr(p), 0, *[ptr(x) for x in args], ptr(dpreds), None, 1.0, ptr(ious), ptr(losses), ptr(ws),
                                      1, 2, 3, 1, 3, float(mc.IMAGE_WIDTH), float(mc.IMAGE_HEIGHT), float(mc.EXP_THRESH), float(mc.EPSILON),
                                      1.0, 75.0, 100.0, 5.0, float(mask.sum()), None, 0, ctypes.cast(ctypes.pointer(o), ctypes.c_void_p),
                                      ops.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1                                               # SQDET_EINVAL
    assert bool((dpreds == -123.456).all()) and bool((ious == -1.0).all()) and bool((losses == -1.0).all())
    with pytest.raises(SqdetError):                               # and through ops: an unknown name, a negative gamma
        ops.loss_fwd_bwd(p, *args, with_options(mc, "l1", 0.0), 5.0)
    with pytest.raises(SqdetError):
        ops.loss_fwd_bwd(p, *args, with_options(mc, "giou", -1.0), 5.0)


# ---------------------------------------------------------------- the trainers
def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_squeezedet_giou_focal_is_bitwise_eager_graphed_and_resumed(tmp_path):
    """SqueezeDet at the trainers' small shape (2 x 128 x 256), --bbox_loss giou --focal_gamma 2: three steps graphed == three
    steps eager, bit for bit (the captured step holds the new launch); a run resumed from the checkpoint of step 2 computes step
    3's bits; and the same checkpoint refuses --bbox_loss ciou."""
    T = _load("train")
    flags = ["--bbox_loss", "giou", "--focal_gamma", "2"]
    args = lambda d, *more: T.parse_args(["--synthetic", "12", "--seed", "3", "--train_dir", str(d), "--summary_step", "0",
                                          "--image_size", "128", "256", "--batch_size", "2"] + list(more))

    def state(run):
        run.tr.flush()
        torch.cuda.synchronize()
        return run.tr.flat_params.clone().view(torch.int32), run.tr.flat_accum.clone().view(torch.int32), run.tr.global_step

    a_args = args(tmp_path / "graphed", *flags)
    os.makedirs(a_args.train_dir)
    a = T.Run(a_args)
    assert a.mc.BBOX_LOSS == "giou" and a.model.mc.FOCAL_GAMMA == 2.0 and a.stepper is not None
    for s in range(3):
        out = a.step(s)
    losses = [float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")]
    assert np.isfinite(losses).all() and 0.0 < losses[2] <= 2.0 * a.mc.LOSS_COEF_BBOX       # 1 - GIoU lies in [0, 2]
    after3 = state(a)
    a.save(2)
    a.step(3)
    after4 = state(a)
    a.close()
    del a
    b = T.Run(args(tmp_path / "eager", "--no_graph", *flags))
    assert b.stepper is None
    for s in range(3):
        b.step(s)
    got3 = state(b)
    b.close()
    del b
    assert got3[2] == after3[2] == 3 and torch.equal(got3[0], after3[0]) and torch.equal(got3[1], after3[1])
    c = T.Run(a_args, resume_step=2)
    assert c.first == 3
    c.step(3)
    got4 = state(c)
    c.close()
    del c
    assert got4[2] == after4[2] and torch.equal(got4[0], after4[0]) and torch.equal(got4[1], after4[1])
    assert not torch.equal(after4[0], after3[0])
    with pytest.raises(SystemExit, match="--resume: the checkpoint was trained with loss"):
        T.Run(args(tmp_path / "graphed", "--bbox_loss", "ciou", "--focal_gamma", "2"), resume_step=2)
