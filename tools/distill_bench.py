"""Times the distillation launch beside the loss launch, and the SqueezeDet training step with and without a teacher (DESIGN.md
section 3.20).

    python tools/distill_bench.py [--out profiles/distill_bench.txt] [--no_steps]

Kernel part: SqueezeDet's KITTI head, batch 20 (24 x 78 x 9 anchors x 20 images, 3 classes).  Events around 200 back-to-back calls,
warm, the variants alternating for seven rounds in ONE process; microseconds per call, median (min - max) of the seven, and the
ratio of each median to the default loss launch of the same student dtype in the same run.  A distill call is distill_kernel +
loss_finish_kernel onto an existing dpreds; a loss call is the loss kernel + loss_finish_kernel (outputs from torch's caching
allocator, as the trainers').  The four dtype pairs are student x teacher in float32 / float16.

Step part: tools/bench_train.py (SqueezeDet, batch 20, 1248 x 384; eager steps) in child processes, without a teacher and with a
VGG16+ConvDet and a ResNet50+ConvDet teacher (synthetic variables), float32 and mixed precision, alternating twice.  (SqueezeDet+
cannot teach SqueezeDet: its grid is 22 x 76.)  The teacher's inference forward is expected to be most of the difference."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS, LAUNCHES, BATCH = 7, 200, 20
STEP_VARIANTS = [("no teacher", []), ("vgg16 teacher", ["--teacher_net", "vgg16"]), ("resnet50 teacher", ["--teacher_net", "resnet50"])]


def kernel_part(out):
    import torch
    import squeezedet_amd as S
    from squeezedet_amd import distill, ops
    from tools.bench_train import synthetic_ground_truth
    dev = torch.device("cuda", 0)
    mc = S.kitti_squeezeDet_config()
    anchors64 = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(dev)
    anchors = anchors64.float()
    gt, gcls, gcnt = [torch.from_numpy(x).to(dev) for x in synthetic_ground_truth(mc, BATCH, seed=200)]
    mask, delta, box, labels = ops.build_labels(anchors64, gt, gcls, gcnt, mc.CLASSES)[:4]
    nobj = ops.sum_f32(mask)
    gen = torch.Generator(dev).manual_seed(1)
    preds = (torch.randn(BATCH, 24, 78, 72, device=dev, generator=gen) * 1.2).contiguous()
    teach = (0.6 * preds + torch.randn(BATCH, 24, 78, 72, device=dev, generator=gen)).contiguous()
    p = {"float32": preds, "float16": preds.half()}
    t = {"float32": teach, "float16": teach.half()}
    dpreds, g16 = torch.zeros_like(preds), torch.empty_like(p["float16"])
    d3, ws = torch.empty(3, device=dev), ops.distill_workspace(dev)
    opt = distill.distill_options(temperature=2.0, conf_floor=0.3)
    calls = [("loss    float32", lambda: ops.loss_fwd_bwd(preds, anchors, mask, delta, box, labels, mc, nobj)),
             ("loss    mixed", lambda: ops.loss_fwd_bwd_mixed(p["float16"], anchors, mask, delta, box, labels, mc, nobj, 1024.0))]
    for sd in ("float32", "float16"):
        for td in ("float32", "float16"):
            calls.append(("distill student %s teacher %s" % (sd, td),
                          lambda sd=sd, td=td: ops.distill_fwd_bwd(p[sd], t[td], dpreds, mc.ANCHOR_PER_GRID, mc.CLASSES, opt,
                                                                   g16=g16 if sd == "float16" else None, loss_scale=1024.0, distill3=d3, ws=ws)))
    times = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        for name, fn in calls:
            dpreds.zero_()
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    print("batch %d, 24 x 78 x 9 anchors, 3 classes; %d rounds of %d calls, microseconds per call (kernel + finish): median (min - max), "
          "ratio to the default loss launch of the student's dtype" % (BATCH, ROUNDS, LAUNCHES), file=out)
    med = {name: float(np.median(v)) for name, v in times.items()}
    for name, _ in calls:
        v = times[name]
        base = med["loss    mixed"] if "student float16" in name or "mixed" in name else med["loss    float32"]
        print("%-44s %7.2f (%.2f - %.2f)   x %.2f" % (name, med[name], min(v), max(v), med[name] / base), file=out, flush=True)


def step_part(out, steps, warmup):
    print("tools/bench_train.py --arch squeezeDet (batch 20, 1248 x 384, eager steps), %d steps after %d: ms per step" % (steps, warmup), file=out)
    rows = {}
    for rnd in range(2):
        for dt in ("f32", "f16"):
            for name, flags in STEP_VARIANTS:
                cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_train.py"), "--arch", "squeezeDet", "--dtype", dt,
                       "--steps", str(steps), "--warmup", str(warmup)] + flags
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("distill_bench: %s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr[-2000:]))
                line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                rows.setdefault((dt, name), []).append(line)
                print("distill_bench: round %d %s %s: %.3f ms per step" % (rnd, dt, name, line["ms_per_step"]), file=sys.stderr, flush=True)
    for dt in ("f32", "f16"):
        base = float(np.median([l["ms_per_step"] for l in rows[(dt, "no teacher")]]))
        for name, _ in STEP_VARIANTS:
            ls = rows[(dt, name)]
            ms = [l["ms_per_step"] for l in ls]
            print("%s %-18s %s ms per step (median %.3f, %+.3f ms over no teacher)%s"
                  % (dt, name, " / ".join("%.3f" % v for v in ms), float(np.median(ms)), float(np.median(ms)) - base,
                     "" if "distill_losses" not in ls[-1] else "   distill terms %s" % json.dumps(ls[-1]["distill_losses"])), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--no_steps", action="store_true", help="the kernel part only")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench: needs a HIP device (nothing is measured without one)")
    out = open(a.out, "w") if a.out else sys.stdout
    from squeezedet_amd import ops
    box = ops.box_calibration(torch.device("cuda", 0))
    print("distill_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s"
          % (torch.cuda.get_device_name(0), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")), file=out, flush=True)
    kernel_part(out)
    if not a.no_steps:
        step_part(out, a.steps, a.warmup)


if __name__ == "__main__":
    main()
