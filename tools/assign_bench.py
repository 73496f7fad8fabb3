"""Times the label build under the assignment options (sqdet_build_labels_opt) beside sqdet_build_labels at
the same shape on the same box -- the yardstick is that ratio, not an absolute time.

    python tools/assign_bench.py [--out profiles/assign_bench.txt]

KITTI anchors (16848, 9 per cell), 3 classes, batch 20.  Two shapes: M = 32 with 1..8 boxes per image (the training benchmark's
ground truth) and M = 128 with 8..40 boxes per image (a mosaic's density); boxes w in [20, 300], h in [20, 200], centres uniform in
the image.  The C entries are called on preallocated outputs (no allocation inside the timed loop), four input sets rotating from
call to call.  Events around 200 back-to-back calls, warm, the variants alternating for seven rounds in ONE process; microseconds
per call, median (min - max), and the ratio of the medians to sqdet_build_labels."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, LAUNCHES, BATCH, SETS = 7, 200, 20, 4
SHAPES = [(32, 1, 8), (128, 8, 40)]            # (M, fewest, most boxes per image)
VARIANTS = [("sqdet_build_labels (3 launches)", None), ("  _opt iou 0.5, at most 16 (5 launches)", ("iou", 0.5, 16, 9)),
            ("  _opt iou 0.5, at most 64", ("iou", 0.5, 64, 9)), ("  _opt atss, topk 9 (5 launches)", ("atss", 0.5, 16, 9)),
            ("  _opt atss, topk 32", ("atss", 0.5, 16, 32))]


def ground_truth(mc, M, lo, hi, seed, dev):
    import torch
    rs = np.random.RandomState(seed)
    cnt = rs.randint(lo, hi + 1, BATCH).astype(np.int32)
    gt = np.stack([rs.uniform(0, mc.IMAGE_WIDTH, (BATCH, M)), rs.uniform(0, mc.IMAGE_HEIGHT, (BATCH, M)), rs.uniform(20, 300, (BATCH, M)),
                   rs.uniform(20, 200, (BATCH, M))], 2)
    cls = rs.randint(0, mc.CLASSES, (BATCH, M)).astype(np.int32)
    return torch.from_numpy(gt).to(dev), torch.from_numpy(cls).to(dev), torch.from_numpy(cnt).to(dev)


def shape(out, mc, M, lo, hi):
    import torch
    from squeezedet_amd import _lib, assign, ops
    dev = torch.device("cuda", 0)
    lib, A, C, apg = _lib.lib(), int(mc.ANCHORS), int(mc.CLASSES), int(mc.ANCHOR_PER_GRID)
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(dev)
    sets = [ground_truth(mc, M, lo, hi, 500 + s, dev) for s in range(SETS)]
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    outs = [f(BATCH, A), f(BATCH, A, 4), f(BATCH, A, 4), f(BATCH, A, C), i(BATCH, M), i(BATCH, A), i(BATCH, M)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    calls, positives = [], {}
    for name, o in VARIANTS:
        if o is None:
            def fn(k, name=name):
                gt, cls, cnt = sets[k % SETS]
                _lib.check(lib.sqdet_build_labels(ptr(anchors), ptr(gt), ptr(cls), ptr(cnt), *[ptr(t) for t in outs[:5]], BATCH, A, M, C,
                                                  _lib.stream_ptr()), name)
        else:
            rec = ops._AssignOptions(assign.ASSIGN_MODES.index(o[0]), o[1], o[2], o[3])
            po = ctypes.cast(ctypes.pointer(rec), ctypes.c_void_p)
            ws = torch.empty(int(lib.sqdet_build_labels_opt_workspace_bytes(BATCH, A, M, apg, po)), dtype=torch.uint8, device=dev)

            def fn(k, name=name, po=po, ws=ws, rec=rec):
                gt, cls, cnt = sets[k % SETS]
                _lib.check(lib.sqdet_build_labels_opt(ptr(anchors), ptr(gt), ptr(cls), ptr(cnt), *[ptr(t) for t in outs], ptr(ws), BATCH, A, M, C,
                                                      apg, po, _lib.stream_ptr()), name)
            fn(0)
            torch.cuda.synchronize()
            positives[name] = assign.positives_summary(outs[6], sets[0][2])
        calls.append((name, fn))
    times = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        for name, fn in calls:
            for k in range(20):
                fn(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(LAUNCHES):
                fn(k)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    mean_n = float(np.mean([s[2].float().mean().item() for s in sets]))
    print("batch %d x %d anchors, M = %d, %d..%d boxes per image (mean %.1f); %d rounds of %d calls, microseconds per call: median (min - max)"
          % (BATCH, A, M, lo, hi, mean_n, ROUNDS, LAUNCHES), file=out)
    base = np.median(times[calls[0][0]])
    for name, _ in calls:
        t = times[name]
        note = "   x%.2f   positives per object min / mean / max: %d / %.1f / %d" % ((np.median(t) / base,) + positives[name]) if name in positives else ""
        print("%-42s %8.2f (%.2f - %.2f)%s" % (name, np.median(t), min(t), max(t), note), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench: needs a HIP device (nothing is measured without one)")
    out = open(a.out, "w") if a.out else sys.stdout
    import squeezedet_amd as S
    from squeezedet_amd import ops
    box = ops.box_calibration(torch.device("cuda", 0))
    print("assign_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s"
          % (torch.cuda.get_device_name(0), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")), file=out, flush=True)
    mc = S.kitti_squeezeDet_config()
    for M, lo, hi in SHAPES:
        shape(out, mc, M, lo, hi)


if __name__ == "__main__":
    main()
