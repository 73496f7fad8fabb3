"""Times the second suppression stage (sqdet_suppress_rows) beside the filter launch, and the serving step
with and without a suppression option.

    python tools/nms_options_bench.py [--out profiles/nms_options_bench.txt]

1. The launches: 32 images of 16848 random-score anchors with KITTI-like random boxes, 3 classes, TOP_N 64.  Events around 200
   back-to-back calls, warm, the variants alternating for seven rounds in ONE process; microseconds per call, median (min - max):
   filter_prediction at the config's threshold (today's one launch), at a threshold of inf (the first stage), and the first
   stage followed by suppress_rows for every method (the second stage works in place, so it is timed behind the launch that
   refills its rows; its own time is the difference to the first stage alone).
2. The serving step: float16 SqueezeDet at 375 x 1242, batch 32, seeded synthetic weights and images,
   detect_filter_pipelined(to_host=True, defer=True) on the model's default lanes: the default policy (riders in the forward's
   fire_chain launches -- the parent's path) against NMS_METHOD = greedy (no riders: filter + second stage + row copy on the side
   stream).  Host clock around 100 steps ending in flush_pipeline() + a device synchronisation, seven alternating rounds;
   milliseconds per step, median (min - max)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, LAUNCHES, STEPS, N, A, ROWS, BATCH = 7, 200, 100, 32, 16848, 64, 32
VARIANTS = [("nongreedy", "iou", False), ("greedy", "iou", False), ("greedy", "diou", False), ("greedy", "iou", True),
            ("soft_linear", "iou", False), ("soft_gaussian", "iou", False)]


def launches(out):
    import torch
    import squeezedet_amd as S
    from squeezedet_amd import ops
    dev = torch.device("cuda", 0)
    mc = S.kitti_squeezeDet_config()
    rs = np.random.RandomState(1)
    boxes = torch.from_numpy(np.stack([rs.uniform(0, 1242, (N, A)), rs.uniform(0, 375, (N, A)), rs.uniform(20, 300, (N, A)),
                                       rs.uniform(20, 200, (N, A))], -1).astype(np.float32)).to(dev)
    probs = torch.from_numpy((rs.uniform(0, 1, (N, A)) ** 4).astype(np.float32)).to(dev)
    cls = torch.from_numpy(rs.randint(0, mc.CLASSES, (N, A)).astype(np.int64)).to(dev)
    rows = ops.filter_prediction(boxes, probs, cls, mc.CLASSES, ROWS, float("inf"), mc.PROB_THRESH)
    first = lambda t: ops.filter_prediction(boxes, probs, cls, mc.CLASSES, ROWS, t, mc.PROB_THRESH, out=rows)
    calls = [("filter_prediction, nms_thresh %g" % mc.NMS_THRESH, lambda: first(mc.NMS_THRESH)),
             ("filter_prediction, nms_thresh inf", lambda: first(float("inf")))]
    for method, overlap, agn in VARIANTS:
        o = dict(method=method, overlap=overlap, class_agnostic=agn, nms_thresh=mc.NMS_THRESH, sigma=0.5, score_floor=0.001)
        calls.append(("  + suppress_rows %s %s%s" % (method, overlap, " agnostic" if agn else ""),
                      lambda o=o: ops.suppress_rows(first(float("inf")), mc.CLASSES, o)))
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
    print("%d images x %d anchors, %d classes, top %d; %d rounds of %d calls, microseconds per call: median (min - max)"
          % (N, A, mc.CLASSES, ROWS, ROUNDS, LAUNCHES), file=out)
    base = np.median(times[calls[1][0]])
    for name, _ in calls:
        t = times[name]
        extra = "   second stage alone: %6.2f" % (np.median(t) - base) if name.startswith("  +") else ""
        print("%-44s %7.2f (%.2f - %.2f)%s" % (name, np.median(t), min(t), max(t), extra), file=out, flush=True)


def serving(out):
    import torch
    import squeezedet_amd as S
    from squeezedet_amd import nets, synthetic
    mc = S.kitti_squeezeDet_config_for_input(375, 1242)
    mc.LOAD_PRETRAINED_MODEL, mc.BATCH_SIZE = False, BATCH
    m = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float16)
    m.load_params(synthetic.synthetic_params(m, seed=0))
    x = synthetic.synthetic_images(BATCH, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, seed=100).to(m.device, torch.float16)
    policies = [("default policy (riders)", None), ("NMS_METHOD greedy (side stream + second stage)", "greedy")]
    times = {name: [] for name, _ in policies}

    def loop(k):
        for _ in range(k):
            m.detect_filter_pipelined(x, to_host=True, defer=True)
        m.flush_pipeline()
        torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, method in policies:
            mc.pop("NMS_METHOD", None)
            if method:
                mc.NMS_METHOD = method
            loop(10)
            t0 = time.perf_counter()
            loop(STEPS)
            times[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
    mc.pop("NMS_METHOD", None)
    print("serving step, float16 SqueezeDet 375 x 1242, batch %d, deferred, to_host; %d rounds of %d steps, milliseconds per step: median (min - max)"
          % (BATCH, ROUNDS, STEPS), file=out)
    for name, _ in policies:
        t = times[name]
        print("%-48s %7.4f (%.4f - %.4f)" % (name, np.median(t), min(t), max(t)), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nms_options_bench: needs a HIP device (nothing is measured without one)")
    out = open(a.out, "w") if a.out else sys.stdout
    from squeezedet_amd import ops
    box = ops.box_calibration(torch.device("cuda", 0))
    print("nms_options_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s"
          % (torch.cuda.get_device_name(0), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")), file=out, flush=True)
    launches(out)
    serving(out)


if __name__ == "__main__":
    main()
