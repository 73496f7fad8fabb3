#!/usr/bin/env python
"""Times the update step's three launches with device events on the real segment tables of the SqueezeDet
and the ResNet50+ConvDet trainers: sqdet_optimizer_step (the path of a run without optimizer flags: the baseline), then
sqdet_optimizer_step_opt under momentum, nesterov and adamw, each without and with the EMA of the weights.

    python tools/optimizer_bench.py [--out profiles/optimizer_bench.txt] [--calls 100] [--rounds 5]

A window is `calls` back-to-back steps between two events, issued from Python as the trainers issue them (the step runs eagerly
behind the graph replay: two table copies and three launches per step); the figure is the window over `calls`, the median and the
fastest of `rounds` windows, the variants alternating inside every round.  Beside each: the float32 streams the apply pass
moves (reads + writes; pass 1 reads w and g and writes g for every rule) and the rate they imply over the whole step's time.  The
box's own clock and MFMA / copy rates (ops.box_calibration) are printed with the numbers: a time without its box says little."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("sqdet_optimizer_step", None, False)] + [("step_opt " + r + (" + ema" if e else ""), r, e)
                                                     for r in ("momentum", "nesterov", "adamw") for e in (False, True)]


def segment_table(arch, dev):
    """(offsets, counts, decays, total) as the trainer of `arch` hands them to the optimizer."""
    import torch
    import squeezedet_amd as S
    from squeezedet_amd import nets, synthetic
    from squeezedet_amd.train import ResNet50ConvDetTrainer, SqueezeDetTrainer
    mc = {"squeezeDet": S.kitti_squeezeDet_config, "resnet50": S.kitti_res50_config}[arch]()
    mc.LOAD_PRETRAINED_MODEL, mc.IS_TRAINING, mc.BATCH_SIZE = False, True, 1
    cls, trainer = {"squeezeDet": (nets.SqueezeDet, SqueezeDetTrainer), "resnet50": (nets.ResNet50ConvDet, ResNet50ConvDetTrainer)}[arch]
    model = cls(mc, gpu_id=str(dev.index), dtype=torch.float32)
    model.load_params(synthetic.synthetic_params(model, seed=0))
    tr = trainer(model)
    base = tr.flat_params.data_ptr()
    offs = [(tr.view[n].data_ptr() - base) // 4 for n in tr.names]
    cnts = [int(tr.view[n].numel()) for n in tr.names]
    decs = [mc.WEIGHT_DECAY if n.endswith("/kernels") else 0.0 for n in tr.names]
    return offs, cnts, decs, int(tr.total), tr.flat_params.clone()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.txt"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--archs", nargs="+", default=["squeezeDet", "resnet50"], choices=["squeezeDet", "resnet50"])
    a = ap.parse_args(argv)
    import torch
    from squeezedet_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench: no HIP device -- times are measured on the GPU or not at all")
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    box = ops.box_calibration(dev)
    say("optimizer_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s" % (
        torch.cuda.get_device_name(dev), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")))
    say("windows of %d steps (2 table copies + 3 launches each, issued from Python), %d rounds, variants alternating; us per step: "
        "median (fastest)" % (a.calls, a.rounds))
    for arch in a.archs:
        offs, cnts, decs, total, params = segment_table(arch, dev)
        elements = int(sum(cnts))
        say("%s: %d variables, %d elements (%d with the padding to 64)" % (arch, len(cnts), elements, total))
        runs = []
        for name, rule, ema in VARIANTS:
            g = torch.Generator(device=dev).manual_seed(1)
            buf = dict(p=params.clone(), g=torch.randn(total, device=dev, generator=g) * 1e-3, m=torch.zeros(total, device=dev))
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            if rule is None:
                opt = ops.MomentumOptimizer(offs, cnts, decs, dev)
                step = lambda opt=opt, b=buf, flag=flag: opt.step(b["p"], b["g"], b["m"], 1e-6, 0.9, 1.0, 1.0, found_inf=flag)
                streams = 3 + 5
            else:
                opt = ops.Optimizer(offs, cnts, decs, dev, dict(rule=rule, ema_decay=0.999 if ema else 0.0))
                buf["v"] = torch.zeros(total, device=dev) if rule == "adamw" else None
                buf["e"] = params.clone() if ema else None
                step = lambda opt=opt, b=buf, flag=flag: opt.step(b["p"], b["g"], b["m"], 1e-6, 1.0, 1.0, accum2=b["v"], ema=b["e"], found_inf=flag)
                streams = (2 if rule == "adamw" else 3) + 5 + (2 if rule == "adamw" else 0) + (2 if ema else 0)   # (adamw's pass 1 reads no w)
            runs.append((name, step, streams, flag, []))
        for r in range(a.rounds + 1):
            for name, step, streams, flag, times in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    step()
                e1.record()
                torch.cuda.synchronize()
                if int(flag.item()):
                    raise SystemExit("optimizer_bench: %s skipped a step (non-finite gradient norm): the window timed nothing" % name)
                if r:                                              # (round 0 warms every variant up)
                    times.append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for name, step, streams, flag, times in runs:
            med = float(np.median(times))
            say("  %-28s %8.2f (%8.2f) us   %2d float32 streams, %6.1f GB/s over the step" % (name, med, min(times), streams,
                                                                                             streams * 4.0 * elements / med * 1e-3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
