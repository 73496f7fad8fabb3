"""Times the loss launch pair (loss kernel + loss_finish_kernel) with and without the loss options.

    python tools/loss_options_bench.py [--out profiles/loss_options_bench.txt]

SqueezeDet's KITTI head, batch 20 (134 784 anchors x 20 images, 3 classes), float32 preds and -- the mixed form -- float16
preds; ground truth from tools/bench_train.py's generator through sqdet_build_labels; num_objects on the device.  Events around
200 back-to-back calls of ops.loss_fwd_bwd / ops.loss_fwd_bwd_mixed (each: the loss kernel, then loss_finish_kernel), warm, the
variants alternating for seven rounds in ONE process; microseconds per call, median (min - max) of the seven.  The calls allocate
their outputs from torch's caching allocator, as the trainers' do."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, LAUNCHES, BATCH = 7, 200, 20
VARIANTS = [("delta_l2", 0.0), ("delta_l2", 2.0), ("iou", 0.0), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0), ("giou", 2.0), ("ciou", 2.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import squeezedet_amd as S
    from squeezedet_amd import ops
    from tools.bench_train import synthetic_ground_truth
    dev = torch.device("cuda", 0)
    base = S.kitti_squeezeDet_config()
    anchors64 = torch.from_numpy(np.asarray(base.ANCHOR_BOX, np.float64)).to(dev)
    anchors = anchors64.float()
    gt, gcls, gcnt = [torch.from_numpy(x).to(dev) for x in synthetic_ground_truth(base, BATCH, seed=200)]
    mask, delta, box, labels = ops.build_labels(anchors64, gt, gcls, gcnt, base.CLASSES)[:4]
    nobj = ops.sum_f32(mask)
    preds = (torch.randn(BATCH, 24, 78, 72, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 1.2).contiguous()
    p16 = preds.half()
    calls = []
    for kind, gamma in VARIANTS:
        mc = type(base)(base)
        mc.BBOX_LOSS, mc.FOCAL_GAMMA = kind, gamma
        calls.append(("float32 %-8s gamma %g" % (kind, gamma), lambda mc=mc: ops.loss_fwd_bwd(preds, anchors, mask, delta, box, labels, mc, nobj)))
        calls.append(("mixed   %-8s gamma %g" % (kind, gamma), lambda mc=mc: ops.loss_fwd_bwd_mixed(p16, anchors, mask, delta, box, labels, mc, nobj, 1024.0)))
    times = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        for name, fn in calls:
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    out = open(a.out, "w") if a.out else sys.stdout
    print("batch %d, 24 x 78 x 9 anchors, 3 classes; %d rounds of %d calls, microseconds per call (loss kernel + finish): median (min - max)"
          % (BATCH, ROUNDS, LAUNCHES), file=out)
    for name, _ in calls:
        t = times[name]
        print("%-32s %7.2f (%.2f - %.2f)" % (name, np.median(t), min(t), max(t)), file=out, flush=True)


if __name__ == "__main__":
    main()
