#!/usr/bin/env python
"""Times Tracker.update (sqdet_track_update) with device events at the three shapes a user runs -- a camera bank (S=32, F=1), a
video batch (S=1, F=32), a large bank (S=256, F=1) -- and, beside each, the filter launch that feeds it (ops.filter_prediction, KITTI's
16848 anchors, top 64) at the same number of images, alternating in the same run.

    python tools/track_bench.py [--out profiles/track_bench.txt] [--calls 200] [--rounds 5]

Steady state: every stream carries 20 objects on closed paths (high rows: 20 live, confirmed tracks) and 20 low-prob clutter
rows (valid, candidates of stage two, never born): 40 valid rows of 64.  Ten warm-up frames per stream come first.  A window is
`calls` back-to-back launches between two events, issued from Python ("eager": launch-to-launch time on one stream, the host's
enqueue included, which is what a Python serving loop pays) and replayed as one captured graph ("graph": the device alone); the
figure is the window over `calls`, the median and the fastest of `rounds` windows.  The box's own clock and MFMA / copy rates
(ops.box_calibration) are printed with the numbers: a time without its box says little."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, OBJECTS, CLUTTER, WARMUP = 64, 20, 20, 10
ANCHORS, CLASSES, TOP_N, NMS_THRESH, PROB_THRESH = 16848, 3, 64, 0.4, 0.005


def make_frames(rs, S, frames, period):
    """boxes [frames, S, 64, 4], probs, cls, counts [frames, S] for S streams: row order shuffled per stream, fixed over time;
    the objects' paths close after `period` frames, so the timed frames can be cycled."""
    x0, y0 = rs.uniform(60, 1180, (S, OBJECTS)), rs.uniform(40, 340, (S, OBJECTS))
    w, h = rs.uniform(30, 90, (S, OBJECTS)), rs.uniform(25, 70, (S, OBJECTS))
    phase, klass = rs.uniform(0, 2 * np.pi, (S, OBJECTS)), rs.randint(0, CLASSES, (S, OBJECTS))
    boxes = np.zeros((frames, S, ROWS, 4), np.float32)
    probs = np.zeros((frames, S, ROWS), np.float32)
    cls = np.zeros((frames, S, ROWS), np.int32)
    perm = np.stack([rs.permutation(OBJECTS + CLUTTER) for _ in range(S)])
    for f in range(frames):
        a = 2 * np.pi * f / float(period) + phase
        obj = np.stack([x0 + 30 * np.sin(a), y0 + 10 * np.cos(a), w, h], -1) + rs.uniform(-1, 1, (S, OBJECTS, 4))
        clutter = np.stack([rs.uniform(0, 1248, (S, CLUTTER)), rs.uniform(0, 384, (S, CLUTTER)), rs.uniform(20, 80, (S, CLUTTER)),
                            rs.uniform(20, 60, (S, CLUTTER))], -1)
        b = np.concatenate([obj, clutter], 1)
        p = np.concatenate([rs.uniform(0.6, 0.99, (S, OBJECTS)), rs.uniform(0.15, 0.45, (S, CLUTTER))], 1)
        c = np.concatenate([klass, rs.randint(0, CLASSES, (S, CLUTTER))], 1)
        for s in range(S):
            boxes[f, s, :OBJECTS + CLUTTER] = b[s, perm[s]]
            probs[f, s, :OBJECTS + CLUTTER] = p[s, perm[s]]
            cls[f, s, :OBJECTS + CLUTTER] = c[s, perm[s]]
    return boxes, probs, cls, np.full((frames, S), OBJECTS + CLUTTER, np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from squeezedet_amd import ops, track
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: no HIP device -- times are measured on the GPU or not at all")
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    box = ops.box_calibration(dev)
    say("track_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s" % (
        torch.cuda.get_device_name(dev), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")))
    say("windows of %d launches, %d rounds, track and filter alternating; us per launch: median (fastest); eager = issued from Python, "
        "graph = the window replayed as one captured graph" % (a.calls, a.rounds))
    rs = np.random.RandomState(0)
    for S, F in ((32, 1), (1, 32), (256, 1)):
        n = S * F
        distinct = 40                                              # calls' worth of distinct inputs, cycled
        frames = (WARMUP + distinct) * F
        boxes, probs, cls, counts = make_frames(rs, S, frames, distinct * F)
        # call k of a stream takes its frames [k*F, (k+1)*F): image s*F + f
        def call_arrays(k):
            sl = slice(k * F, (k + 1) * F)
            return [torch.from_numpy(np.ascontiguousarray(np.swapaxes(v[sl], 0, 1)).reshape((n,) + v.shape[2:])).to(dev)
                    for v in (boxes, probs, cls, counts)]
        inputs = [call_arrays(k) for k in range(frames // F)]
        trk = track.Tracker(S, dev)
        for k in range(WARMUP):
            trk.update(*inputs[k], frames_per_stream=F)
        torch.cuda.synchronize()
        live = sum(len(trk.tracks(s)) for s in range(min(S, 8))) / float(min(S, 8))
        det = (torch.rand((n, ANCHORS, 4), device=dev) * 300 + 20, torch.rand((n, ANCHORS), device=dev) ** 8,
               torch.randint(0, CLASSES, (n, ANCHORS), device=dev, dtype=torch.int64))
        fout = ops.filter_prediction(*det, CLASSES, TOP_N, NMS_THRESH, PROB_THRESH)
        torch.cuda.synchronize()
        def run_track():
            for k in range(a.calls):
                trk.update(*inputs[WARMUP + k % distinct], frames_per_stream=F)

        def run_filter():
            for k in range(a.calls):
                ops.filter_prediction(*det, CLASSES, TOP_N, NMS_THRESH, PROB_THRESH, out=fout)

        def captured(fn):
            """The window as ONE graph: its replay has no host between the launches."""
            g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(g, stream=side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            return g.replay

        times = {}
        for mode, (do_track, do_filter) in (("eager", (run_track, run_filter)), ("graph", (captured(run_track), captured(run_filter)))):
            t_track, t_filter = [], []
            for r in range(a.rounds + 1):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                do_track()
                e[1].record()
                do_filter()
                e[2].record()
                torch.cuda.synchronize()
                if r:                                              # (round 0 warms both up at this shape)
                    t_track.append(e[0].elapsed_time(e[1]) * 1e3 / a.calls)
                    t_filter.append(e[1].elapsed_time(e[2]) * 1e3 / a.calls)
            times[mode] = (float(np.median(t_track)), min(t_track), float(np.median(t_filter)), min(t_filter))
        live_after = sum(len(trk.tracks(s)) for s in range(min(S, 8))) / float(min(S, 8))
        for mode in ("eager", "graph"):
            say("S=%-3d F=%-2d n=%-3d %s  update %8.2f (%8.2f) us   filter_prediction %8.2f (%8.2f) us" % ((S, F, n, mode) + times[mode]))
        say("    live tracks per stream %.1f -> %.1f, dropped %d" % (live, live_after, int(trk.dropped.sum().cpu())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
