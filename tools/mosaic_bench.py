"""Times sqdet_augment_bgr_mosaic beside sqdet_augment_bgr_window and sqdet_augment_bgr, and the host
half of BatchReader with the mosaic on.

    python tools/mosaic_bench.py [--parent squeezedet_amd/libsqdet_hip_alt.so] [--out profiles/mosaic_bench.txt]
    python tools/mosaic_bench.py --host            # next_plan only, no GPU

Kernel: batch 20, the four KITTI sizes -> 384 x 1248 float16, geometry uploaded once; events around 200 back-to-back launches,
warm, the variants alternating for seven rounds in ONE process; median (min - max) of the seven.  The mosaic is a centre split on
every image, each part a centred crop at 1.25 x the zoom that fills its pane (the middle of the policy's U[1, 1.5]; 1.6 source
pixels per output pixel) or at 2 x (one source pixel per output pixel, the sampling density of the whole-image window), every second
part mirrored; split (W, H) is the layout's own cost on the whole-image window's work; a cut at W / 2 + 1 puts the right-hand panes
on the element store path.  --parent names a library with the parent commit's augment.hip, its objects linked in the build's own
order: its sqdet_augment_bgr and sqdet_augment_bgr_window are timed in the same alternation.
Host: milliseconds of next_plan per batch of 20 under the reference policy, `ssd` and the mosaic at probability 1."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, LAUNCHES, BATCH = 7, 200, 20


def host(out):
    import squeezedet_amd as S
    from squeezedet_amd.synthetic import synthetic_dataset
    rows = []
    for name, setup in (("reference (drift / flip)", {}), ("ssd, zoom-out 2, colour", dict(AUG_GEOMETRY="ssd", AUG_ZOOM_OUT_MAX=2.0, AUG_COLOR=True)),
                        ("reference + mosaic 1", dict(AUG_MOSAIC_PROB=1.0)), ("reference + mosaic 1 + colour", dict(AUG_MOSAIC_PROB=1.0, AUG_COLOR=True))):
        mc = S.kitti_squeezeDet_config()
        mc.BATCH_SIZE = BATCH
        for k, v in setup.items():
            mc[k] = v
        r = S.BatchReader(mc, *synthetic_dataset(mc, 2 * BATCH, seed=300), seed=0)
        for _ in range(5):
            r.next_plan()
        ts = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(20):
                r.next_plan()
            ts.append((time.perf_counter() - t0) / 20 * 1e3)
        rows.append("next_plan  %-30s %7.2f ms per batch of %d  (%.2f - %.2f over %d rounds of 20)" % (name, np.median(ts), BATCH, min(ts), max(ts), ROUNDS))
    for row in rows:
        print(row, file=out, flush=True)


def kernel(out, parent):
    import torch
    from squeezedet_amd import _lib, ops
    from squeezedet_amd.synthetic import KITTI_SIZES
    dev = torch.device("cuda", 0)
    H, W = 384, 1248
    rs = np.random.RandomState(1)
    sizes = np.array([KITTI_SIZES[i % 4] for i in range(BATCH)], np.int64)
    nbytes = sizes[:, 0] * sizes[:, 1] * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    src = torch.from_numpy(rs.randint(0, 256, size=int(nbytes.sum())).astype(np.uint8)).to(dev)
    dx, dy, fl = rs.randint(-150, 151, BATCH), rs.randint(-100, 101, BATCH), rs.randint(0, 2, BATCH)
    g5 = np.stack([sizes[:, 0], sizes[:, 1], dx, dy, fl], 1)
    g7 = np.stack([sizes[:, 0], sizes[:, 1], dx, dy, sizes[:, 1] - dx, sizes[:, 0] - dy, fl], 1)
    whole = np.stack([sizes[:, 0], sizes[:, 1], 0 * dx, 0 * dy, sizes[:, 1], sizes[:, 0], fl], 1)
    color = rs.uniform(-0.5, 1.5, (BATCH, 12)).astype(np.float32)
    color4 = rs.uniform(-0.5, 1.5, (BATCH, 4, 12)).astype(np.float32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    def mosaic(xc, yc, zoom):
        """(part_offsets, geom, split) on the device and the source bytes inside the windows: every image cut at (xc, yc), each pane a
        centred crop at `zoom` x the zoom that fills it (None: the whole image), every second part mirrored."""
        split = np.tile(np.array([xc, yc], np.int64), (BATCH, 1))
        part_off, gm = np.zeros((BATCH, 4), np.int64), np.zeros((BATCH, 4, 7), np.int64)
        for i in range(BATCH):
            for p, (pw, ph) in enumerate([(xc, yc), (W - xc, yc), (xc, H - yc), (W - xc, H - yc)]):
                s = (i + 5 * p) % BATCH                                            # four different images per output
                h, w = sizes[s]
                cw, ch = w, h
                if zoom is not None and pw > 0 and ph > 0:
                    z = max(pw / float(w), ph / float(h)) * zoom
                    cw, ch = min(w, int(pw / z)), min(h, int(ph / z))
                part_off[i, p], gm[i, p] = offsets[s], (h, w, (w - cw) // 2, (h - ch) // 2, cw, ch, fl[i] if zoom is None else (i + p) & 1)
        po, gmc, sp, _ = ops.check_augment_mosaic_geometry(part_off, gm, split, src.numel(), H, W, color4)
        live = (np.array([xc, W - xc, xc, W - xc]) > 0) & (np.array([yc, yc, H - yc, H - yc]) > 0)
        return (up(po, np.int64), up(gmc, np.int32), up(sp, np.int32)), int((gmc[:, live, 4].astype(np.int64) * gmc[:, live, 5] * 3).sum())

    ops.check_augment_geometry(g5, offsets, src.numel())
    ops.check_augment_window_geometry(np.concatenate([g7, whole]), np.concatenate([offsets, offsets]), src.numel())
    d = dict(off=up(offsets, np.int64), g5=up(g5, np.int32), g7=up(g7, np.int32), whole=up(whole, np.int32), color=up(color, np.float32),
             color4=up(color4, np.float32))
    d["one"], bytes_one = mosaic(W, H, None)
    d["policy"], bytes_policy = mosaic(W // 2, H // 2, 1.25)
    d["unit"], bytes_unit = mosaic(W // 2, H // 2, 2.0)
    d["odd"], _ = mosaic(W // 2 + 1, H // 2, 1.25)
    dst = torch.empty((BATCH, H, W, 3), dtype=torch.float16, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    means = [103.939, 116.779, 123.68]
    tail = [BATCH, H, W] + means + [_lib.dtype_code(torch.float16)]
    here = _lib.lib()
    variants = [("sqdet_augment_bgr, first timing of a round", here, "bgr", None),
                ("sqdet_augment_bgr_window, the same drifts as windows", here, "win", ("g7", None)),
                ("sqdet_augment_bgr_window, the whole image", here, "win", ("whole", None)),
                ("sqdet_augment_bgr_mosaic, split (W, H): the whole image in pane 0", here, "mosaic", ("one", None)),
                ("sqdet_augment_bgr_mosaic, centre split, crops at 2 x fill (1 : 1 sampling)", here, "mosaic", ("unit", None)),
                ("sqdet_augment_bgr_mosaic, centre split, crops at 1.25 x fill (1.6 : 1)", here, "mosaic", ("policy", None)),
                ("sqdet_augment_bgr_mosaic, the same cut at W / 2 + 1", here, "mosaic", ("odd", None)),
                ("sqdet_augment_bgr, second timing of the same round", here, "bgr", None),
                ("sqdet_augment_bgr_window, the whole image, with matrices", here, "win", ("whole", "color")),
                ("sqdet_augment_bgr_mosaic, centre split, crops at 1.25 x fill, with matrices", here, "mosaic", ("policy", "color4"))]
    if parent:
        old = C.CDLL(os.path.abspath(parent))
        for name in ("sqdet_augment_bgr", "sqdet_augment_bgr_window"):
            getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
        variants[1:1] = [("parent build: sqdet_augment_bgr", old, "bgr", None)]
        variants.insert(5, ("parent build: sqdet_augment_bgr_window, the whole image", old, "win", ("whole", None)))
        variants.append(("parent build: sqdet_augment_bgr_window, the whole image, with matrices", old, "win", ("whole", "color")))

    def launch(lib, kind, arg):
        st = _lib.stream_ptr()
        if kind == "bgr":
            return lib.sqdet_augment_bgr(p(src), src.numel(), p(d["off"]), p(d["g5"]), p(dst), *tail, st)
        if kind == "win":
            return lib.sqdet_augment_bgr_window(p(src), src.numel(), p(d["off"]), p(d[arg[0]]), None if arg[1] is None else p(d[arg[1]]), p(dst), *tail, st)
        po, gm, sp = d[arg[0]]
        return lib.sqdet_augment_bgr_mosaic(p(src), src.numel(), p(po), p(gm), p(sp), None if arg[1] is None else p(d[arg[1]]), p(dst), *tail, st)

    for _, lib, kind, arg in variants:                                             # warm
        for _ in range(20):
            assert launch(lib, kind, arg) == 0
    torch.cuda.synchronize()
    times = [[] for _ in variants]
    for _ in range(ROUNDS):
        for k, (_, lib, kind, arg) in enumerate(variants):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LAUNCHES):
                launch(lib, kind, arg)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / LAUNCHES * 1e3)
    cal = ops.box_calibration(dev)
    print("device %s; box calibration %s" % (torch.cuda.get_device_name(0), cal), file=out)
    print("batch %d, KITTI sizes -> %d x %d float16; %d rounds of %d launches, microseconds per launch: median (min - max)" % (BATCH, H, W, ROUNDS, LAUNCHES), file=out)
    print("source bytes inside the windows: whole image %d (mosaic with one pane: %d), mosaic at 2 x fill %d, at 1.25 x fill %d; output bytes %d"
          % (int(nbytes.sum()), bytes_one, bytes_unit, bytes_policy, dst.numel() * 2), file=out)
    for (name, _, _, _), t in zip(variants, times):
        print("%-80s %7.2f (%.2f - %.2f)" % (name, np.median(t), min(t), max(t)), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a library built from the parent commit, timed in the same alternation")
    ap.add_argument("--host", action="store_true", help="time next_plan only (no GPU)")
    ap.add_argument("--out", default="", help="append the report to this file as well")
    a = ap.parse_args()
    outs = [sys.stdout] + ([open(a.out, "a")] if a.out else [])

    class Tee:
        def write(self, s):
            for o in outs:
                o.write(s)

        def flush(self):
            for o in outs:
                o.flush()
    if a.host:
        host(Tee())
    else:
        kernel(Tee(), a.parent)
        host(Tee())


if __name__ == "__main__":
    main()
