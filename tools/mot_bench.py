#!/usr/bin/env python
"""Times MotAccumulator.update (sqdet_mot_update) beside Tracker.update (sqdet_track_update) in the same run, with device events,
at the three shapes of tools/track_bench.py -- a camera bank (S=32, F=1), a video batch (S=1, F=32), a large bank (S=256, F=1) --
and MotAccumulator.evaluate (sqdet_mot_evaluate) at 64 x 128 and 256 x 1024 identities.

    python tools/mot_bench.py [--out profiles/mot_bench.txt] [--calls 200] [--rounds 5]

The scene is track_bench's: per stream 20 objects on closed paths and 20 low-prob clutter rows, 40 valid rows of 64; the labelled
objects are the 20 object rows themselves (ids by row), so a frame has 20 objects, about 20 hypotheses, continuity matches nearly
all of them and the assignment sees what is left.  A window is `calls` back-to-back launches between two events -- issued from
Python ("eager") and replayed as one captured graph ("graph") -- tracker and accumulator alternating; the figure is the window over
`calls`, the median and the fastest of `rounds` windows.  evaluate() is timed alone, a call between two events (its launch, its
three copies and its synchronisation), on random sparse overlap tables, one stream.  No speed target is set: the numbers are a
record, printed with the box's own clock."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.track_bench import CLASSES, OBJECTS, WARMUP, make_frames  # noqa: E402


def sparse_tables(rs, mot, G, T, per_row=6):
    """A table state of G object and T hypothesis identities with a few overlaps per row."""
    import torch
    d = {f: torch.zeros(shape, dtype=getattr(torch, dtype)) for f, (shape, dtype) in mot.table_shapes(1, CLASSES).items()}
    d["n_obj"][0], d["n_hyp"][0] = G, T
    d["obj_id"][0, :G] = torch.arange(1, G + 1, dtype=torch.int32)
    d["hyp_id"][0, :T] = torch.arange(1, T + 1, dtype=torch.int32)
    d["obj_cls"][0, :G] = torch.from_numpy(rs.randint(CLASSES, size=G).astype(np.int32))
    d["hyp_cls"][0, :T] = torch.from_numpy(rs.randint(CLASSES, size=T).astype(np.int32))
    ov = np.zeros((G, T), np.int32)
    for g in range(G):
        ov[g, rs.choice(T, size=min(per_row, T), replace=False)] = rs.randint(1, 200, size=min(per_row, T))
    d["overlap"][0, :G, :T] = torch.from_numpy(ov)
    d["obj_present"][0, :G] = torch.from_numpy(ov.max(1) + 10)
    d["obj_tracked"][0, :G] = torch.from_numpy(ov.max(1))
    d["hyp_frames"][0, :T] = torch.from_numpy(ov.max(0))
    return d


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mot_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    from squeezedet_amd import mot, ops, track
    if not torch.cuda.is_available():
        raise SystemExit("mot_bench: no HIP device -- times are measured on the GPU or not at all")
    dev = torch.device("cuda", a.gpu)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    box = ops.box_calibration(dev)
    say("mot_bench: %s; box: effective clock %s MHz, box_mfma_tflops %s, box_copy_gbs %s" % (
        torch.cuda.get_device_name(dev), box.get("effective_clock_mhz"), box.get("box_mfma_tflops"), box.get("box_copy_gbs")))
    say("windows of %d launches, %d rounds, tracker and accumulator alternating; us per launch: median (fastest); eager = issued from "
        "Python, graph = the window replayed as one captured graph" % (a.calls, a.rounds))
    rs = np.random.RandomState(0)
    for S, F in ((32, 1), (1, 32), (256, 1)):
        n = S * F
        distinct = 40
        frames = (WARMUP + distinct) * F
        boxes, probs, cls, counts = make_frames(rs, S, frames, distinct * F)
        # the labelled objects: the rows above 0.5 (the 20 objects; their row is fixed over time), id = row + 1
        is_obj = probs[0] > 0.5                                     # [S, 64]
        assert (is_obj.sum(1) == OBJECTS).all()
        gt_box = np.zeros((frames, S, OBJECTS, 4), np.float64)
        gt_id, gt_cls = np.zeros((frames, S, OBJECTS), np.int32), np.zeros((frames, S, OBJECTS), np.int32)
        for s in range(S):
            r = np.nonzero(is_obj[s])[0]
            gt_box[:, s], gt_id[:, s], gt_cls[:, s] = boxes[:, s, r], r + 1, cls[:, s, r]
        gt_flags, gt_count = np.zeros_like(gt_id), np.full((frames, S), OBJECTS, np.int32)

        def call_arrays(k, arrays):
            sl = slice(k * F, (k + 1) * F)
            return [torch.from_numpy(np.ascontiguousarray(np.swapaxes(v[sl], 0, 1)).reshape((n,) + v.shape[2:])).to(dev) for v in arrays]
        inputs = [call_arrays(k, (boxes, probs, cls, counts)) for k in range(frames // F)]
        labels = [tuple(call_arrays(k, (gt_box, gt_id, gt_cls, gt_flags, gt_count))) for k in range(frames // F)]
        trk, acc = track.Tracker(S, dev), mot.MotAccumulator(S, dev, CLASSES)
        for k in range(WARMUP):
            trk.update(*inputs[k], frames_per_stream=F)
        # the tracker's outputs of the timed calls, kept: the accumulator's window reads what the tracker's window would write
        outs = []
        for k in range(distinct):
            i, s_ = trk.update(*inputs[WARMUP + k], frames_per_stream=F)
            outs.append((i.clone(), s_.clone()))
            acc.update(inputs[WARMUP + k][0], inputs[WARMUP + k][2], inputs[WARMUP + k][3], i, s_, labels[WARMUP + k], frames_per_stream=F)
        torch.cuda.synchronize()
        first = acc.evaluate()["overall"]

        def run_track():
            for k in range(a.calls):
                trk.update(*inputs[WARMUP + k % distinct], frames_per_stream=F)

        def run_mot():
            for k in range(a.calls):
                b = inputs[WARMUP + k % distinct]
                acc.update(b[0], b[2], b[3], outs[k % distinct][0], outs[k % distinct][1], labels[WARMUP + k % distinct], frames_per_stream=F)

        def captured(fn):
            g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(g, stream=side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            return g.replay

        times = {}
        for mode, (do_track, do_mot) in (("eager", (run_track, run_mot)), ("graph", (captured(run_track), captured(run_mot)))):
            t_track, t_mot = [], []
            for r in range(a.rounds + 1):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                do_track()
                e[1].record()
                do_mot()
                e[2].record()
                torch.cuda.synchronize()
                if r:                                              # (round 0 warms both up at this shape)
                    t_track.append(e[0].elapsed_time(e[1]) * 1e3 / a.calls)
                    t_mot.append(e[1].elapsed_time(e[2]) * 1e3 / a.calls)
            times[mode] = (float(np.median(t_track)), min(t_track), float(np.median(t_mot)), min(t_mot))
        for mode in ("eager", "graph"):
            say("S=%-3d F=%-2d n=%-3d %s  Tracker.update %8.2f (%8.2f) us   MotAccumulator.update %8.2f (%8.2f) us" % ((S, F, n, mode) + times[mode]))
        m = acc.evaluate()["overall"]
        say("    first pass: tp %d fn %d fp %d idsw %d; after the windows: MOTA %.4f MOTP %.4f IDF1 %.4f, identities %d objects %d hypotheses" % (
            first["tp"], first["fn"], first["fp"], first["idsw"], m["mota"], m["motp"], m["idf1"], m["gt_ids"], m["hyp_ids"]))
    for G, T in ((64, 128), (256, 1024)):
        acc = mot.MotAccumulator(1, dev, CLASSES)
        acc.load_state_dict(sparse_tables(rs, mot, G, T))
        ts = []
        for r in range(a.rounds + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            table, _ = acc.evaluate_raw()
            e[1].record()
            torch.cuda.synchronize()
            if r:
                ts.append(e[0].elapsed_time(e[1]) * 1e3)
        say("evaluate  %3d x %4d identities, 1 stream: %9.1f (%9.1f) us   idtp %d" % (G, T, float(np.median(ts)), min(ts), int(table[0, :, 9].sum())))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
