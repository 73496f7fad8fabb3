"""Generates tests/golden/train_step_bits.npz: the BITS the loss, distillation and optimizer entry points give on an MI355X, for
tests/test_gpu_train_step_bits.py to compare against.  The other tests of these kernels compare one path with another or with a
float64 restatement; two paths that drift together pass them all.  This file pins every path to a recording.

Inputs come from the case generators the other tests use (tests/loss_options_cases.py, tests/distill_cases.py,
tests/optimizer_cases.py).  What is recorded:

  loss       cases g2x3_k1_c3_b1 (6 anchors: one partly filled workgroup), g3x5_k9_c20_b3 (K = 9, C = 20) and kitti_b8 (134 784
             anchors: the grid-stride loop and a second lap of loss_finish_kernel).  Calls: the defaults through sqdet_loss_fwd_bwd,
             _dev and _mixed (loss scale 512), the five option pairs of KITTI_OPTIONS in float32, and ciou / gamma 2 mixed.
  distill    the smallest case and g3x5_k9_c20_b3 with a float32 and a float16 student against a float32 teacher, and the
             smallest case once with a float16 teacher; onto zeros.
  optimizer  the layout of tests/optimizer_cases.py (aligned and odd offsets, tails, a variable past the 64-block cap): three steps
             of sqdet_optimizer_step, and of sqdet_optimizer_step_opt for every rule x clip x EMA off / on, with max_norm 1, 50, 1;
             sqdet_optimizer_step and every rule (with an EMA) again with every base pointer one float off 16-byte alignment; one
             overflowed step.  After every step: each buffer in use (params, grads, accum; accum2 under AdamW; ema with one), found_inf
             and the state.

The inputs of the loss calls hold the same option pairs as KITTI_OPTIONS of tests/test_gpu_loss_options.py; they are restated here
(LOSS_OPTIONS) so that what is compared with the file depends on this module and the case modules alone.

An array of at most FULL elements is stored as it is; a larger one as the SHA-256 of its bytes and its first HEAD elements.  The
optimizer's buffers (137 k floats each, some 200 of them) are stored per run: the digests of every step, the first HEAD elements --
the first three variables: an aligned offset, an odd one, a tail -- after the last.  The file stays below tests/golden/augment.npz
(212 KB) that way: it is 148 KB, and one optimizer buffer stored in full would add 550 KB that do not compress.  The price: a
difference in an optimizer buffer beyond its first elements is reported as a digest that differs, without a position or a distance.

    python tests/golden/make_train_step_bits.py [out.npz]          (on the GPU)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import distill_cases as DC, loss_options_cases as LC, optimizer_cases as OC  # noqa: E402

# Everything the recording depends on besides the case modules stands here: an edit elsewhere cannot change what is compared.
DEV = "cuda:0"
FULL, HEAD = 16384, 128
LOSS_CASES = ["g2x3_k1_c3_b1", "g3x5_k9_c20_b3", "kitti_b8"]
LOSS_OPTIONS = [("ciou", 2.0), ("giou", 0.5), ("diou", 0.0), ("iou", 2.0), ("delta_l2", 0.5)]      # every box kind, every gamma
LOSS_SCALE = 512.0
DISTILL_CALLS = [("g2x3_k1_c3_b1", torch.float32, torch.float32, "s32_t32"), ("g2x3_k1_c3_b1", torch.float16, torch.float32, "s16_t32"),
                 ("g3x5_k9_c20_b3", torch.float32, torch.float32, "s32_t32"), ("g3x5_k9_c20_b3", torch.float16, torch.float32, "s16_t32"),
                 ("g2x3_k1_c3_b1", torch.float32, torch.float16, "s32_t16")]
EMAS = ((0.0, False), (0.99, False))                  # off / on
_CACHE = {}


def ordered(a):
    """The bits of a float array as integers in the floats' order (so that a difference is a distance in ulps)."""
    i = a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize]).astype(np.int64)
    return np.where(i < 0, np.int64(-(1 << (8 * a.itemsize - 1))) - i, i)


def record(out, key, a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    if a.size <= FULL:
        out[key] = a
    else:
        out[key + ".sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8)
        out[key + ".head"] = a.reshape(-1)[:HEAD].copy()


def _loss_inputs(name):
    """(mc, num_objects, preds, (anchors, mask, delta, box, labels)) of a case of tests/loss_options_cases.py, the tensors on the device."""
    if name not in _CACHE:
        mc, preds, mask, delta, box, labels = LC.loss_case(name)[:6]
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        _CACHE[name] = (mc, float(mask.sum()), t(preds), (t(np.asarray(mc.ANCHOR_BOX).astype(np.float32)), t(mask.reshape(preds.shape[0], -1)),
                                                           t(delta), t(box), t(labels)))
    return _CACHE[name]


def _with_options(mc, kind, gamma):
    mc = type(mc)(mc)
    mc.BBOX_LOSS, mc.FOCAL_GAMMA = kind, gamma
    return mc


def loss_bits(name):
    from squeezedet_amd import ops
    mc, nobj, p, args = _loss_inputs(name)
    out = {}

    def rec(call, res):             # (dpreds, ious, losses), or (g16, dpreds, ious, losses) of the mixed form
        torch.cuda.synchronize()
        for what, a in zip(("g16", "dpreds", "ious", "losses")[4 - len(res):], res):
            record(out, "loss/%s/%s/%s" % (name, call, what), a)

    rec("default", ops.loss_fwd_bwd(p, *args, mc, nobj))
    rec("default_dev", ops.loss_fwd_bwd(p, *args, mc, torch.tensor([nobj], dtype=torch.float32, device=DEV)))
    rec("default_mixed", ops.loss_fwd_bwd_mixed(p.half(), *args, mc, nobj, LOSS_SCALE))
    for kind, gamma in LOSS_OPTIONS:
        rec("%s_g%g" % (kind, gamma), ops.loss_fwd_bwd(p, *args, _with_options(mc, kind, gamma), nobj))
    rec("ciou_g2_mixed", ops.loss_fwd_bwd_mixed(p.half(), *args, _with_options(mc, "ciou", 2.0), nobj, LOSS_SCALE))
    return out


def distill_bits():
    from squeezedet_amd import ops
    from squeezedet_amd.distill import DistillOptions
    out = {}
    for name, sdt, tdt, pid in DISTILL_CALLS:
        K, C, student, teacher, o = DC.distill_case(name)
        s, t = torch.from_numpy(student).to(DEV, sdt), torch.from_numpy(teacher).to(DEV, tdt)
        dp = torch.zeros(s.shape, dtype=torch.float32, device=DEV)
        g16 = torch.zeros(s.shape, dtype=torch.float16, device=DEV) if sdt == torch.float16 else None
        d3 = ops.distill_fwd_bwd(s, t, dp, K, C, DistillOptions(*[float(v) for v in o]), g16=g16, loss_scale=LOSS_SCALE)
        torch.cuda.synchronize()
        for what, a in (("g16", g16), ("dpreds", dp), ("distill3", d3)):
            if a is not None:
                record(out, "distill/%s/%s/%s" % (name, pid, what), a)
    return out


def _shifted(a, shift):
    """The array on the device, its base pointer `shift` floats off the allocation's (so off 16-byte alignment)."""
    t = torch.zeros(a.size + shift, dtype=torch.float32, device=DEV)
    t[shift:].copy_(torch.from_numpy(a))
    return t[shift:]


def _optimizer_run(out, key, options, shift=0, steps=3, overflow=False):
    """options None: sqdet_optimizer_step with momentum 0.9; else sqdet_optimizer_step_opt."""
    from squeezedet_amd import ops
    offs, cnts, decs, total = OC.layout()
    dev = [_shifted(b, shift) for b in OC.buffers(offs, cnts, total, 20)]
    adamw, ema = bool(options) and options.get("rule") == "adamw", bool(options) and options.get("ema_decay", 0.0) > 0.0
    used = [True, True, True, adamw, ema]
    opt = ops.MomentumOptimizer(offs, cnts, decs, DEV) if options is None else ops.Optimizer(offs, cnts, decs, DEV, options)
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    digests, flags, states = [], [], []
    for k in range(steps):
        G = OC.gradients(offs, cnts, total, 21 + k)
        if overflow:
            G[offs[-1] + cnts[-1] - 1] = np.inf
        dev[1] = _shifted(G, shift)
        max_norm = (1.0, 50.0)[k % 2]
        if options is None:
            opt.step(dev[0], dev[1], dev[2], 0.01, 0.9, max_norm, 0.5, found_inf=flag)
        else:
            opt.step(dev[0], dev[1], dev[2], 0.01, max_norm, 0.5, accum2=dev[3] if adamw else None, ema=dev[4] if ema else None,
                     found_inf=flag)
        torch.cuda.synchronize()
        host = [d.cpu().numpy() for d, u in zip(dev, used) if u]
        digests.append([np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8) for a in host])
        flags.append(int(flag.item()))
        states.append(opt.state.cpu().numpy() if options is not None else np.zeros(4))
    # per run: the digests [steps, buffers in use, 32], the last step's first HEAD elements [buffers in use, HEAD], found_inf and state
    out["optimizer/%s/sha256" % key] = np.array(digests, np.uint8)
    out["optimizer/%s/head" % key] = np.stack([a[:HEAD] for a in host])
    out["optimizer/%s/found_inf" % key] = np.array(flags, np.int32)
    out["optimizer/%s/state" % key] = np.stack(states)


def optimizer_bits():
    out = {}
    _optimizer_run(out, "legacy", None)
    _optimizer_run(out, "legacy_unaligned", None, shift=1)
    for rule in OC.RULES:
        for clip in OC.CLIPS:
            for decay, warm in EMAS:
                _optimizer_run(out, "%s_%s_ema%g" % (rule, clip, decay), dict(rule=rule, clip=clip, ema_decay=decay, ema_warmup=warm))
        _optimizer_run(out, "%s_unaligned" % rule, dict(rule=rule, ema_decay=0.99), shift=1)
    _optimizer_run(out, "overflow", dict(rule="adamw", clip="global", ema_decay=0.99, ema_warmup=True), steps=1, overflow=True)
    _optimizer_run(out, "legacy_overflow", None, steps=1, overflow=True)
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "train_step_bits.npz")
    out = {}
    for name in LOSS_CASES:
        out.update(loss_bits(name))
    out.update(distill_bits())
    out.update(optimizer_bits())
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
