#!/usr/bin/env python
"""bench.py -- the SqueezeDet hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W [--config NAME]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

--config (default sqdet_infer = BASELINE.json configs[1], the headline):
  sqdet_infer        SqueezeDet float16 inference, batch 32 per GPU, synthetic 1242x375 images.  One step = one pass of
                     the whole hot path over one batch already resident in HBM: sqdet_net_forward (conv1 .. conv12) ->
                     sqdet_interpret_output -> sqdet_filter_prediction -> the <= 64 filtered rows per image copied to
                     pinned host memory (what the reference's sess.run + filter_prediction hand the caller).
  sqdetplus_infer    configs[3]: SqueezeDet+ float16 inference, batch 8 per GPU (64 over 8 GPUs), same step.
  sqdet_train_fp32   configs[2]: SqueezeDet float32 training, batch 20 per GPU, 1248x384: GPU label build + forward
                     (dropout on) + loss + backward + flat-bucket gradient all-reduce (RCCL) + clipped Momentum update.
  res50_train_fp16   configs[4]: ResNet50+ConvDet mixed-precision (float16 activations) training, batch 8 per GPU.
  sqdet_infer_384    configs[1] at the reference's TRUE input size (kitti_squeezeDet_config.py:13-14: 1248x384), batch 32.
  sqdet_sample_b1    configs[0]: the reference's data/sample.png (tests/golden/sample.png) -> sqdet_preprocess_bgr (resize to
                     1248x384, BGR mean subtraction: demo.py:186-190) -> the same step at batch 1; also reports the
                     synchronous per-image latency in float16 and float32 and the CPU oracle's latency beside them.
Inference shards by image (weak scaling, no data-path collective); training all-reduces one float32 gradient bucket.
--gpus N > 1 without a torchrun environment re-launches this script under torch.distributed.run with N local ranks.
--dry-run: no kernels, no GPU: the launcher, rendezvous (gloo), barrier and max-over-ranks timing only (CI on a CPU box).
A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, ms_per_step, ...).  --full adds
everything else the benchmark measures: the per-launch survey and roofline objects, box calibration, clocks, latencies,
forward-only diagnostics, the training losses and the CPU baseline (--no-cpu-baseline drops the last one).
--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step handed its caller as DIR/<name>.npy
(float32 / float64); the inputs are seeded, so two builds can be compared output for output.
Every step reads a DIFFERENT input batch from a rotation larger than the 256 MiB Infinity Cache.
Inference steps keep TWO batches in flight (consecutive steps alternate between two HIP streams / plans; SQDET_SERVE_LANES=1: one):
all K batches' work is inside the timed region, which ends with flush_pipeline() + a device-wide synchronize.
Rank 0 prints ONE JSON line.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SHARE_DEVICE = os.environ.get("SQDET_SHARE_DEVICE") == "1"
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16/bf16 MFMA peak
MFMA_F32_PEAK_TFLOPS = 157.3   # f32-input MFMA (= the f32 vector rate)
MALL_BYTES = 256 << 20

CONFIGS = {
    "sqdet_infer": dict(kind="infer", arch="squeezeDet", batch=32, height=375, width=1242, dtype="fp16",
                        metric="images/sec SqueezeDet 1242x375 inference", steps=200, warmup=20),
    "sqdet_infer_384": dict(kind="infer", arch="squeezeDet", batch=32, height=384, width=1248, dtype="fp16",
                            metric="images/sec SqueezeDet 1248x384 inference", steps=200, warmup=20),
    "sqdet_sample_b1": dict(kind="infer", arch="squeezeDet", batch=1, height=384, width=1248, dtype="fp16", sample=True,
                            # (a batch-1 forward leaves most of the chip idle: THREE images in flight -- 11.1-11.8 k img/s against 8.3 k
                            # with two on the same box, host-bound from there; four read 8.4 k)
                            lanes=3,
                            metric="images/sec SqueezeDet single sample.png (1242x375 -> 1248x384) inference, batch 1", steps=500, warmup=20),
    "sqdetplus_infer": dict(kind="infer", arch="squeezeDet+", batch=8, height=375, width=1242, dtype="fp16",
                            metric="images/sec SqueezeDet+ 1242x375 inference", steps=100, warmup=10),
    "sqdet_train_fp32": dict(kind="train", arch="squeezeDet", batch=20, height=384, width=1248, dtype="fp32",
                             metric="images/sec SqueezeDet 1248x384 fp32 training", steps=20, warmup=3),
    "res50_train_fp16": dict(kind="train", arch="resnet50", batch=8, height=375, width=1242, dtype="fp16",
                             metric="images/sec ResNet50+ConvDet 1242x375 fp16 (mixed precision) training", steps=20, warmup=3),
    # (not a BASELINE.json config: configs[2] in mixed precision, for the fp32 / fp16 comparison DESIGN.md quotes)
    "sqdet_train_fp16": dict(kind="train", arch="squeezeDet", batch=20, height=384, width=1248, dtype="fp16",
                             metric="images/sec SqueezeDet 1248x384 fp16 (mixed precision) training", steps=20, warmup=3),
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--config", default="sqdet_infer", choices=sorted(CONFIGS))
    # defaults per config (sqdet_infer: 200 steps ~ 0.14 s of GPU time; short runs reproduce it within a few %)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: the config's)")
    ap.add_argument("--warmup", type=int, default=-1)
    ap.add_argument("--full", action="store_true",
                    help="also the diagnostics: per-launch survey, roofline, box calibration, clocks, latencies, losses, CPU baseline")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64, <= 64 MB; rank 0)")
    ap.add_argument("--spinup-ms", type=float, default=250.0, help="untimed steps for this long before the timed region (clock settle)")
    ap.add_argument("--batch", type=int, default=0, help="images per GPU per step (default: the config's)")
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--dtype", default="", choices=["", "fp16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="run decode + NMS on the forward's stream (no side stream)")
    ap.add_argument("--no-graph", action="store_true", help="training configs: issue the step from Python instead of replaying a hipGraph")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=26.0)
    ap.add_argument("--layer-table", default="", help="write the per-launch table (json) here")
    ap.add_argument("--opt", action="append", default=[], help="A/B diagnostics: tuning knob name=value (sqdet_set_option), repeatable")
    ap.add_argument("--dry-run", action="store_true", help="launcher / rendezvous / timing reduction only: gloo on CPU, no kernels")
    a = ap.parse_args(argv)
    c = CONFIGS[a.config]
    a.kind, a.arch, a.metric, a.sample = c["kind"], c["arch"], c["metric"], bool(c.get("sample"))
    a.steps = c["steps"] if a.steps is None else a.steps
    if a.steps < 1:
        fail("--steps must be >= 1, got %d" % a.steps)
    if a.layer_table and not a.full:
        fail("--layer-table needs --full (the per-launch survey runs only there)")
    a.warmup = a.warmup if a.warmup >= 0 else c["warmup"]
    a.batch = a.batch or c["batch"]
    a.height = a.height or c["height"]
    a.width = a.width or c["width"]
    a.dtype = a.dtype or c["dtype"]
    return a


def dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def _dist_on():
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


_RANK_SECONDS = None     # every rank's elapsed seconds of the last timed region (rank order), for the line's "rank_ms_per_step"


def max_over_ranks(value, world, device, own=None):
    """Timing rule of the bench contract: the job's time is the MAX over ranks.  `own` = this rank's seconds up to its own device
    synchronisation, BEFORE the closing barrier: kept for every rank (all-gather) -- the line reports their min / max, so a straggling
    rank or GPU shows up in the record instead of hiding inside the maximum."""
    global _RANK_SECONDS
    own = value if own is None else own
    if not _dist_on():
        _RANK_SECONDS = [float(own)]
        return value
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.float64, device=device)
    o = torch.tensor([own], dtype=torch.float64, device=device)
    every = [torch.zeros_like(o) for _ in range(dist.get_world_size())]
    dist.all_gather(every, o)
    _RANK_SECONDS = [float(e.item()) for e in every]
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def barrier(world, device):
    if _dist_on():
        import torch.distributed as dist
        if device.type == "cuda" and dist.get_backend() == "nccl":
            dist.barrier(device_ids=[device.index])
        else:
            dist.barrier()


def aggregate_throughput(images_per_rank_step, steps, world, seconds_max):
    """value = the units ALL ranks processed / the max-over-ranks time."""
    return images_per_rank_step * steps * world / seconds_max


def gpu_state(device_index=0):
    """Clock / power / temperature of this rank's GPU right now (amdsmi; None where a field is unavailable): recorded
    before and after the timed region so a slow box (round 2 saw one with every kernel 33 % slower) is identifiable from
    the JSON line alone.  Costs ~1 ms, outside the timed region."""
    out = {}
    try:
        import amdsmi
        global _AMDSMI_READY
        if not globals().get("_AMDSMI_READY"):
            amdsmi.amdsmi_init()
            _AMDSMI_READY = True
        hs = amdsmi.amdsmi_get_processor_handles()
        vis = os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES") or ""
        phys = device_index
        if vis:
            try:
                phys = int(vis.split(",")[device_index])
            except (ValueError, IndexError):
                phys = device_index
        h = hs[min(phys, len(hs) - 1)]
        try:
            m = amdsmi.amdsmi_get_gpu_metrics_info(h)
            for k_out, k_in in (("gfxclk_mhz", "current_gfxclk"), ("uclk_mhz", "current_uclk"), ("socclk_mhz", "current_socclk"),
                                ("socket_power_w", "current_socket_power"), ("temp_hotspot_c", "temperature_hotspot"),
                                ("temp_mem_c", "temperature_mem"), ("gfx_activity", "average_gfx_activity"),
                                ("throttle_status", "throttle_status")):
                v = m.get(k_in)
                if isinstance(v, (list, tuple)):
                    v = [x for x in v if isinstance(x, (int, float)) and 0 <= x < 65535][:8] or None
                    if v and k_out.endswith("_mhz"):
                        v = max(v)
                out[k_out] = v if not (isinstance(v, str) and v == "N/A") else None
        except Exception as e:  # noqa: BLE001 -- a monitoring read-out must never break the bench
            out["metrics_error"] = repr(e)[:120]
        for k_out, typ in (("sclk", "GFX"), ("mclk", "MEM")):
            try:
                c = amdsmi.amdsmi_get_clock_info(h, getattr(amdsmi.AmdSmiClkType, typ))
                out[k_out + "_mhz"] = c.get("clk")
                out[k_out + "_max_mhz"] = c.get("max_clk")
            except Exception:  # noqa: BLE001
                pass
        try:
            pw = amdsmi.amdsmi_get_power_info(h)
            out["power_w"] = pw.get("current_socket_power", pw.get("average_socket_power"))
            out["power_limit_w"] = pw.get("power_limit")
        except Exception:  # noqa: BLE001
            pass
    except Exception as e:  # noqa: BLE001
        out["error"] = "amdsmi unavailable: " + repr(e)[:120]
    return out


def rank_census(rank, local_rank, world, device):
    """What the process group ACTUALLY is: world size as torch.distributed sees it and every rank's device -- a launcher
    that silently ran fewer ranks (or two ranks on one GPU) shows up in the JSON line."""
    mine = {"rank": rank, "local_rank": local_rank, "device": str(device), "pid": os.getpid()}
    if device.type == "cuda":
        pr = torch.cuda.get_device_properties(device)
        mine.update(name=pr.name, cus=pr.multi_processor_count, uuid=str(getattr(pr, "uuid", "")),
                    pci_bus_id=getattr(pr, "pci_bus_id", None))
    if not _dist_on():
        return 1, [mine]
    import torch.distributed as dist
    seen = [None] * dist.get_world_size()
    dist.all_gather_object(seen, mine)
    return dist.get_world_size(), seen


def build_fingerprint():
    """sha256 over the kernel sources the loaded library was built from: a PMC traffic profile is only attached to
    the roofline object when it was taken on THIS build (profiles/*_hbm_traffic_pmc.json carries the fingerprint)."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "squeezedet_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(csrc, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(config_name, layer):
    """HBM (fabric) bytes per launch of `layer` from the newest committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
    of this command whose build fingerprint matches the loaded kernels; None otherwise (stale profiles are refused)."""
    prof = os.path.join(ROOT, "profiles")
    fp = build_fingerprint()
    best = None
    for f in sorted(os.listdir(prof)) if os.path.isdir(prof) else []:
        if not f.endswith("_hbm_traffic_pmc.json"):
            continue
        try:
            with open(os.path.join(prof, f)) as fh:
                d = json.load(fh)
        except (OSError, ValueError):
            continue
        if d.get("build_fingerprint") == fp and d.get("config", "sqdet_infer") == config_name and layer in d.get("by_layer", {}):
            best = (d["by_layer"][layer], f)
    return best


def rocprof_launch_ms(traffic_profile, layer, stats_suffix="_kernel_stats.txt"):
    """Average duration of `layer`'s kernel in the rocprofv3 --kernel-trace --stats summary committed beside the fingerprinted
    PMC profile (same collection: profiles/<tag>_kernel_stats.txt next to profiles/<tag>_hbm_traffic_pmc.json), or None.  The
    summary must carry the same build fingerprint in its header; the layer -> kernel name map is the PMC profile's."""
    prof = os.path.join(ROOT, "profiles")
    try:
        with open(os.path.join(prof, traffic_profile)) as fh:
            d = json.load(fh)
        kname = next(k["kernel"] for k in d["kernels"] if k["layer"] == layer)
        shared_layers = [k["layer"] for k in d["kernels"] if k["kernel"] == kname]
        shared = len(shared_layers)
        stats = traffic_profile.replace("_hbm_traffic_pmc.json", stats_suffix)
        fp_ok, avg = False, None
        with open(os.path.join(prof, stats)) as fh:
            for line in fh:
                if line.startswith("# build_fingerprint:"):
                    fp_ok = line.split(":", 1)[1].strip() == d.get("build_fingerprint")
                elif not line.startswith(("#", "kernel ")) and line[:88].rstrip() == kname[:88].rstrip():
                    avg = float(line[90:].split()[2]) * 1e-3            # columns: calls, total_us, avg_us, %
        if not fp_ok or avg is None:
            return None
        return {"ms": round(avg, 5), "profile": stats, "kernel_shared_by_launches": shared, "shared_layers": shared_layers}
    except (OSError, ValueError, KeyError, StopIteration, IndexError):
        return None


def dominant_kernel_from_stats(config_name):
    """The kernel with the largest total time in the committed rocprofv3 --kernel-trace --stats summary of this config and THIS build
    (profiles/*_kernel_stats_<config>.txt, fingerprint in its header), with its average launch and its share of the profiled time;
    None when no summary of this build is committed.  (Training lines: `roofline` itself stays the whole step -- forward + loss +
    backward + update are ~300 launches of ~40 kernels; this names the one to look at first.)"""
    prof = os.path.join(ROOT, "profiles")
    fp = build_fingerprint()
    best = None
    for f in sorted(os.listdir(prof)) if os.path.isdir(prof) else []:
        if not f.endswith("_kernel_stats_%s.txt" % config_name):
            continue
        rows, fp_ok = [], False
        try:
            with open(os.path.join(prof, f)) as fh:
                for line in fh:
                    if line.startswith("# build_fingerprint:"):
                        fp_ok = line.split(":", 1)[1].strip() == fp
                    elif not line.startswith(("#", "kernel ")) and len(line) > 92:
                        c = line[90:].split()
                        rows.append((line[:88].rstrip(), int(c[0]), float(c[1]), float(c[2]), float(c[3])))
        except (OSError, ValueError, IndexError):
            continue
        rows = [r for r in rows if "calib_" not in r[0] and "rocclr" not in r[0] and "at::native" not in r[0]]
        if fp_ok and rows:
            top = max(rows, key=lambda r: r[2])
            best = {"kernel": top[0], "launches_profiled": top[1], "avg_launch_us": round(top[3], 2), "share_of_profiled_time": round(top[4] / 100.0, 4),
                    "profile": f}
    return best


def pmc_kernels(config_name):
    """The committed per-kernel PMC summary of this config ON THIS BUILD (profiles/*_pmc_kernels_<config>.json, profiles/pmc_kernels.py), or
    None."""
    prof = os.path.join(ROOT, "profiles")
    fp = build_fingerprint()
    best = None
    for f in sorted(os.listdir(prof)) if os.path.isdir(prof) else []:
        if not f.endswith("_pmc_kernels_%s.json" % config_name):
            continue
        try:
            with open(os.path.join(prof, f)) as fh:
                d = json.load(fh)
        except (OSError, ValueError):
            continue
        if d.get("build_fingerprint") == fp and d.get("config") == config_name:
            d["profile"] = f
            best = d
    return best


def kernel_roofline(dom, pk, dtype):
    """A kernel's OWN roofline position from the committed profiles of this build: its average launch (kernel trace) against its fabric
    bytes per launch (PMC FETCH_SIZE / WRITE_SIZE) and the matrix instructions it issued (PMC SQ_INSTS_MFMA x the flops of one
    instruction of the config's dtype: 16x16x32 f16 = 16384, 16x16x4 f32 = 2048 -- issued flops, padding lanes included)."""
    if not dom or not pk:
        return dom
    e = next((v for k, v in pk["kernels"].items() if k[:88].rstrip() == dom["kernel"][:88].rstrip()), None)
    if e is None:
        return dom
    sec = dom["avg_launch_us"] * 1e-6
    out = dict(dom)
    out["pmc_profile"] = pk["profile"]
    if e.get("hbm_bytes_per_launch_corrected") is not None:
        out["traffic_bytes_per_launch"] = e["hbm_bytes_per_launch_corrected"]
        out["hbm_gbs"] = round(e["hbm_bytes_per_launch_corrected"] / sec / 1e9, 1)
        out["hbm_frac"] = round(out["hbm_gbs"] / HBM_PEAK_GBS, 4)
    if e.get("SQ_INSTS_MFMA") is not None:
        per = 16384.0 if dtype == "fp16" else 2048.0
        peak = MFMA_F16_PEAK_TFLOPS if dtype == "fp16" else MFMA_F32_PEAK_TFLOPS
        out["mfma_issued_flops_per_launch"] = e["SQ_INSTS_MFMA"] * per
        out["mfma_tflops"] = round(e["SQ_INSTS_MFMA"] * per / sec / 1e12, 1)
        out["mfma_frac"] = round(out["mfma_tflops"] / peak, 4)
    if "hbm_frac" in out and "mfma_frac" in out:
        out["bound"] = "hbm" if out["hbm_frac"] >= out["mfma_frac"] else "mfma"
        out["frac"] = max(out["hbm_frac"], out["mfma_frac"])
    return out


def rotation_count(batch_bytes):
    """distinct input batches to rotate through: at least 4, and more than the Infinity Cache holds"""
    return max(4, int(np.ceil(1.3 * MALL_BYTES / float(batch_bytes))))


DUMP_LIMIT_BYTES = 64 << 20
DUMP_MAX_PARAMS = 1 << 22       # a larger parameter vector is dumped as a fixed, seeded sample of this many values


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy (float32 or float64 only), DUMP_LIMIT_BYTES at most in all."""
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT_BYTES, "outputs of %d bytes exceed the dump limit" % total
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def infer_outputs(out):
    """What the last timed inference step hands its caller: filter_prediction_batch's rows (boxes [B,M,4], probs [B,M], classes
    [B,M], anchor indices [B,M], counts [B]).  Rows past an image's count carry no result and are written as zeros."""
    boxes, probs, cls, idx, cnt = [torch.as_tensor(t).cpu().numpy() for t in out[:5]]
    cnt = cnt.astype(np.int64)
    valid = np.arange(probs.shape[1])[None, :] < cnt[:, None]
    return {"boxes": np.where(valid[..., None], boxes, 0).astype(np.float32),
            "probs": np.where(valid, probs, 0).astype(np.float32),
            "classes": np.where(valid, cls, 0).astype(np.float32),
            "anchor_index": np.where(valid, idx, 0).astype(np.float64),
            "count": cnt.astype(np.float32)}


def train_outputs(out, trainer):
    """What the last timed training step leaves its caller: the step's losses and the updated float32 parameter vector (a fixed,
    seeded sample of DUMP_MAX_PARAMS values, with their indices, when the vector is longer)."""
    res = {k: v.detach().float().cpu().numpy() for k, v in out.items() if isinstance(v, torch.Tensor) and v.numel() == 1}
    flat = trainer.flat_params.detach().float().cpu().numpy()
    if flat.size > DUMP_MAX_PARAMS:
        idx = np.sort(np.random.RandomState(0).choice(flat.size, DUMP_MAX_PARAMS, replace=False))
        res["params_sample_index"] = idx.astype(np.float64)
        flat = flat[idx]
    res["params"] = flat
    return res


# ------------------------------------------------------------------------------------------------ inference
def build_infer_model(args, device_index):
    import squeezedet_amd as S
    from squeezedet_amd import nets, synthetic
    if args.arch == "squeezeDet":
        mc = S.kitti_squeezeDet_config_for_input(args.height, args.width)
        cls = nets.SqueezeDet
    else:
        mc = S.kitti_squeezeDetPlus_config()
        assert (args.height, args.width) == (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH)
        cls = nets.SqueezeDetPlus
    mc.LOAD_PRETRAINED_MODEL = False
    mc.BATCH_SIZE = args.batch
    tdt = torch.float16 if args.dtype == "fp16" else torch.float32
    model = cls(mc, gpu_id=str(device_index), dtype=tdt)
    model.load_params(synthetic.synthetic_params(model, seed=0))
    esz = 2 if args.dtype == "fp16" else 4
    nrot = rotation_count(args.batch * args.height * args.width * 3 * esz)
    if args.sample:
        # configs[0]: the reference's one input fixture through demo.py:186-190's preparation (cv2.imread's BGR uint8 ->
        # resize to the network input -> BGR mean subtraction), done by sqdet_preprocess_bgr on the device; the rotation
        # holds `nrot` resident COPIES of the prepared image at distinct addresses so that every step still reads HBM
        x0 = sample_image_input(model, mc, tdt)
        xs = [x0.clone() for _ in range(nrot)]
        return model, mc, xs
    xs = [synthetic.synthetic_images(args.batch, args.height, args.width, seed=1000 * device_index + 100 + k).to(model.device, tdt).contiguous()
          for k in range(nrot)]
    return model, mc, xs


SAMPLE_PNG = os.path.join(ROOT, "tests", "golden", "sample.png")     # = the reference's data/sample.png (1242x375 RGB)


def sample_bgr_u8():
    from PIL import Image
    rgb = np.asarray(Image.open(SAMPLE_PNG).convert("RGB"))
    return np.ascontiguousarray(rgb[:, :, ::-1])                      # what cv2.imread returns (demo.py:187)


def sample_image_input(model, mc, tdt):
    from squeezedet_amd import ops
    bgr = torch.from_numpy(sample_bgr_u8()).to(model.device)
    return ops.preprocess_bgr(bgr[None], mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, tdt).contiguous()


def sync_latency_ms(model, x, iters=60):
    """Per-image latency of the full step issued synchronously (forward + decode + filter + rows in pinned host memory,
    device idle before and after): median over `iters`."""
    ts = []
    for i in range(iters + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.detect_filter_pipelined(x, to_host=True)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[5:]))


def batch_latency(model, step, lanes, x, n=24):
    """Result latency of a batch beside the throughput (untimed pass).  `steady_state`: in the free-running serving loop with
    `lanes` batches in flight, from the start of a batch's device work (event on its lane's stream ahead of its forward) to the end
    of the call that carries its decode + filter (the next call of its lane; an upper bound: the riders finish inside that
    forward's fire_chain launches) -- median over the loop.  `synchronous`: one batch issued on an idle device, flush_pipeline(),
    synchronize: forward + decode + filter + rows in pinned host memory, host-timed."""
    model.flush_pipeline()
    torch.cuda.synchronize()
    model._latency_probe = probe = []
    try:
        for i in range(n):
            step(i)
        model.flush_pipeline()
        torch.cuda.synchronize()
    finally:
        model._latency_probe = None
    lat = []
    for i, (which, evs) in enumerate(probe):
        nxt = [e for (w, e) in probe[i + 1:] if w == which]
        if nxt and i >= lanes:
            lat.append(evs[0].elapsed_time(nxt[0][1]))
    ts = []
    for i in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.detect_filter_pipelined(x, to_host=True, defer=True)
        model.flush_pipeline()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"steady_state": round(float(np.median(lat)), 4) if lat else None, "batches_in_flight": lanes,
            "synchronous": round(float(np.median(ts[2:])), 4),
            "note": "steady_state: start of a batch's forward -> end of the next call of its lane (which carries its decode + filter), "
                    "device events, median; synchronous: one batch on an idle device incl. flush, host-timed"}


def cpu_thread_candidates():
    n = os.cpu_count() or 8
    c = sorted({t for t in (4, 8, 16, 32, 64, 128, n) if t <= n})
    return c or [n]


def cpu_baseline_infer(args, seconds):
    """The oracle (CPU restatement of the reference path: PyTorch-CPU fp32 convs with TF padding + NumPy
    interpret_output + the restated filter_prediction) timed on this box's host cores on a bounded sample.  The host's
    BEST configuration is reported: a short sweep over torch.set_num_threads x images per call picks it (round 2 ran 128
    threads at batch 4 and got HALF the images/s of 8 threads -- oneDNN oversubscription on small maps), then the rest
    of the time budget measures it."""
    from oracle import sqdet_oracle as O
    if args.arch == "squeezeDet":
        mc = O.squeezeDet_config_for_input(args.height, args.width)
    else:
        mc = O.kitti_squeezeDetPlus_config()
    p32 = O.init_params(args.arch, seed=0, storage="fp32")
    if args.sample:
        from oracle import preproc_oracle as PO
        x_all = torch.from_numpy(PO.preprocess_bgr(sample_bgr_u8(), mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS)[None])
        batches = [1]
    else:
        x_all = O.synthetic_images(4, args.height, args.width, seed=7)
        batches = [1, 4]
    prev_threads = torch.get_num_threads()
    O.detect(args.arch, mc, p32, x_all[:1])  # warm-up

    def rate_of(th, nb, min_s):
        torch.set_num_threads(th)
        x = x_all[:nb]
        O.detect(args.arch, mc, p32, x)
        t0 = time.perf_counter()
        n = 0
        while n < 2 * nb or time.perf_counter() - t0 < min_s:
            O.detect(args.arch, mc, p32, x)
            n += nb
        return n / (time.perf_counter() - t0), n

    # 1. a short sweep RANKS the (threads x images per call) candidates (0.4 s each: noisy, used for the ranking only)
    sweep = []
    t_sweep = time.perf_counter()
    for th in cpu_thread_candidates():
        for nb in batches:
            r, _ = rate_of(th, nb, 0.4)
            sweep.append({"threads": th, "images_per_call": nb, "images_per_s": round(r, 2)})
        if time.perf_counter() - t_sweep > 0.3 * seconds:
            break
    # 2. the two best are measured properly: three runs of >= `per_run` seconds each, the MEDIAN is the candidate's rate (round 3
    # reported single 0.4-second samples: 20.9-74.3 images/s for one box class); the better median is the baseline
    ranked = sorted(sweep, key=lambda e: -e["images_per_s"])[:2]
    per_run = max(3.0, (seconds - (time.perf_counter() - t_sweep)) / (3.0 * len(ranked)))
    finals = []
    for e in ranked:
        runs, imgs = [], 0
        for _ in range(3):
            r, n = rate_of(e["threads"], e["images_per_call"], per_run)
            runs.append(r)
            imgs += n
        med = float(np.median(runs))
        finals.append({"threads": e["threads"], "images_per_call": e["images_per_call"], "runs_images_per_s": [round(r, 2) for r in runs],
                       "median": round(med, 3), "spread": round((max(runs) - min(runs)) / med, 3), "images": imgs})
    best = max(finals, key=lambda f: f["median"])
    th, nb, n = best["threads"], best["images_per_call"], best["images"]
    torch.set_num_threads(prev_threads)
    return {"value": best["median"], "unit": "images/s", "cores": int(th), "kind": "port", "ms_per_image": round(1e3 / best["median"], 2),
            "spread": best["spread"], "runs": best["runs_images_per_s"],
            "sample": "%d %s %dx%d images (%d per call): median of three >= %.1f-second runs of the better of the two best "
                      "(threads x images-per-call) candidates of a ranking sweep, fp32: PyTorch-CPU convs with TF SAME padding + NumPy "
                      "interpret_output + restated filter_prediction; host has %d logical cores, one process; oneDNN is faster than "
                      "TF-1.0 Eigen, so this over-estimates the reference's own CPU path"
                      % (n, "copies of sample.png at" if args.sample else "synthetic", args.width, args.height, nb, per_run, os.cpu_count()),
            "candidates": finals, "sweep": sweep}


def box_calibration(device):
    """`box_mfma_tflops` / `box_copy_gbs`: a fixed ~1 ms MFMA microkernel and a 1 GiB device copy run right before the timed region
    (ops.box_calibration -> sqdet_calib_mfma / sqdet_calib_copy).  Round 3 met boxes that ran every MFMA-heavy launch 20-27 % slower
    while reporting the same clock and power (profiles/r03_slowbox_*): with these two numbers in the line such a box is
    identifiable from the JSON alone.  SQDET_BENCH_NO_CALIB=1 skips it."""
    if os.environ.get("SQDET_BENCH_NO_CALIB") == "1":
        return None
    from squeezedet_amd import ops
    try:
        return ops.box_calibration(device)
    except Exception as e:  # noqa: BLE001 -- a calibration failure must not void the bench line
        return {"error": repr(e)[:160]}


def spin_up(step, ms, flush=None):
    """Untimed steps for a fixed wall time right before the timed region: the W warm-up steps of a short run (the
    driver's 5) end ~3 ms after the per-launch survey's synchronisations, before the clocks have settled -- 20-step runs
    read 8 % below 200-step runs of the same binary without it.  Setup, not measurement: the timed region is still
    exactly K steps between barrier + synchronize pairs."""
    if ms <= 0:
        return
    t0 = time.perf_counter()
    i = 0
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(8):
            step(i)
            i += 1
        if flush is not None:
            flush()
        torch.cuda.synchronize()


def launch_roofline(flops, nbytes, ms, dtype):
    """Roofline entry of one launch: MFMA-bound when its algorithmic intensity exceeds the ridge (fp16 only: the peak the
    guide gives is the dense fp16 one), else HBM-bound; achieved = algorithmic flops (bytes) / measured duration."""
    intensity = flops / nbytes if nbytes else 0.0
    ridge = MFMA_F16_PEAK_TFLOPS * 1e12 / (HBM_PEAK_GBS * 1e9)
    if dtype == "fp16" and intensity > ridge:
        roof = {"bound": "mfma", "achieved": round(flops / (ms * 1e-3) / 1e12, 3), "peak": MFMA_F16_PEAK_TFLOPS, "unit": "TFLOP/s"}
    else:
        roof = {"bound": "hbm", "achieved": round(nbytes / (ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s"}
    roof["frac"] = round(roof["achieved"] / roof["peak"], 4)
    return roof


def run_infer(args, rank, local_rank, world, device):
    model, mc, xs = build_infer_model(args, local_rank)
    # forwards in flight (serving lanes of detect_filter_pipelined): the library's default is 2; a config may name its own
    cfg_lanes = CONFIGS[args.config].get("lanes")
    lanes = 1 if args.no_pipeline else max(1, int(os.environ.get("SQDET_SERVE_LANES", cfg_lanes or 2)))
    model.serve_lanes = lanes                 # (explicit: the completion contract of a deferred call depends on it)
    plan = model._native_plan(args.batch)
    layers = plan.layer_table()
    # the benchmarked step runs ConvDet's SCORE form (interpret_output's det_probs written by its epilogue: one float32 per anchor):
    # those bytes are part of what the launch must write
    score_epilogue = bool(plan.scores_supported() and os.environ.get("SQDET_SCORE_EPILOGUE") != "0" and not args.no_pipeline)
    score_bytes = args.batch * plan.gh * plan.gw * mc.ANCHOR_PER_GRID * 4 if score_epilogue else 0
    if score_bytes:
        n_, f_, b_ = layers[-1]
        layers = list(layers[:-1]) + [(n_, f_, b_ + score_bytes)]
    nrot = len(xs)

    def step(i):
        # forward on this stream; interpret_output + filter_prediction + the copy of the filtered rows to pinned host
        # memory on a side HIP stream behind an event (two-stage pipeline: the next batch's forward overlaps this batch's
        # decode + NMS + D2H).  Every step does all of its work inside the timed region: the closing
        # torch.cuda.synchronize() is device-wide.
        x = xs[i % nrot]
        if args.no_pipeline:
            boxes, probs, cls = model.detect(x)
            out = model.filter_prediction_batch(boxes, probs, cls)
            return [t.cpu() for t in out]
        # defer=True: the side work of step k is enqueued by step k+1, beside that forward's fire_chain launches (which leave 16
        # CUs idle) instead of beside its stem; flush_pipeline() below enqueues the last step's INSIDE the timed region
        return model.detect_filter_pipelined(x, to_host=os.environ.get("SQDET_BENCH_NO_D2H") != "1", defer=True)   # (the env knob: A/B diagnostics only)

    for i in range(max(args.warmup, 1)):
        out = step(i)
    model.flush_pipeline()
    torch.cuda.synchronize()

    if args.full:
        # untimed per-launch survey to find the dominant kernel (HIP events on the launch stream)
        _, ms0 = plan.forward_timed(xs[0])
        for k in range(1, 3):
            _, ms = plan.forward_timed(xs[k % nrot])
            ms0 = [min(a, b) for a, b in zip(ms0, ms)]
        dom = int(np.argmax(ms0))
    spin_up(step, args.spinup_ms, model.flush_pipeline)
    box = clocks = None
    if args.full:
        box = box_calibration(device)                     # ~6 ms of fixed microkernels: what THIS box sustains (untimed)
        # (the clock read-out sits AHEAD of the last spin-up: its first call loads and initialises amdsmi, tens of milliseconds with
        # the GPU idle, and a 20-step timed region that starts behind such a gap reads up to 10 % below a 200-step one)
        clocks = {"before": gpu_state(local_rank)}
    spin_up(step, min(args.spinup_ms, 20.0), model.flush_pipeline)
    if args.full and os.environ.get("SQDET_BENCH_NO_PROBE") != "1":     # (A/B knob: what the live event pairs cost the step)
        plan.set_probe(dom, args.steps)

    # ---- timed region: EXACTLY `steps` steps between barrier+synchronize pairs ----
    barrier(world, device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = step(i)
    model.flush_pipeline()                   # the last step's decode + filter + row copy
    t_issued = time.perf_counter() - t0      # host side done enqueueing (diagnostic: host-bound if ~ elapsed)
    torch.cuda.synchronize()
    own = time.perf_counter() - t0           # this rank's own time (before the barrier): the line's rank_ms_per_step
    barrier(world, device)
    elapsed = time.perf_counter() - t0
    if args.full:
        clocks["after"] = gpu_state(local_rank)
    elapsed = max_over_ranks(elapsed, world, device, own)
    ranks_seen, devices = rank_census(rank, local_rank, world, device)
    # (the rows of the last timed step, read before any later step can reuse its pipeline slot)
    counts = np.asarray(out[4].cpu() if isinstance(out[4], torch.Tensor) else out[4])
    assert (counts >= 0).all() and (counts <= 64).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, infer_outputs(out))

    def head():
        res = result_head(args, aggregate_throughput(args.batch, args.steps, world, elapsed), world, elapsed, ranks_seen, devices, clocks)
        res["config"] = {"workload": "%s %s inference, batch=%d per GPU, synthetic %dx%d images (%d distinct batches in rotation), full hot "
                                     "path (forward + interpret_output + filter_prediction + filtered rows to pinned host memory), inputs "
                                     "resident in HBM%s" % (args.arch, args.dtype, args.batch, args.width, args.height, nrot,
                                                         "; %d batches in flight (consecutive steps alternate between %d HIP streams)" % (lanes, lanes) if lanes >= 2 else ""),
                         "name": args.config, "global_batch": args.batch * world,
                         "parallelism": "dp%d (independent image shards, no collective)" % world}
        return res

    if not args.full:
        return head() if rank == 0 else None

    probe_ms = plan.read_probe(args.steps)
    plan.set_probe(-1, 0)
    single = None
    if lanes >= 2 and os.environ.get("SQDET_BENCH_NO_PROBE") != "1":
        # the SAME dominant launch with ONE forward in flight (untimed second pass of the same K steps): under two lanes a launch
        # shares the chip with the other lane's launches, so its wall-clock duration above is not the time the kernel needs
        # (two sub-passes: the step time WITHOUT the probe's event pair in the stream -- the one-lane serving loop itself, each call's
        #  decode + filter riding in the next forward -- then the probed launch; round-5 review: the probed, flushed pass read 0.54 ms
        #  where SQDET_SERVE_LANES=1 runs 0.44)
        model.serve_lanes = 1
        for i in range(8):
            step(i)
        model.flush_pipeline()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        model.flush_pipeline()
        torch.cuda.synchronize()
        single_step_ms = (time.perf_counter() - t1) / args.steps * 1e3
        plan.set_probe(dom, args.steps)
        for i in range(args.steps):
            step(i)
        model.flush_pipeline()
        torch.cuda.synchronize()
        sp = plan.read_probe(args.steps)
        plan.set_probe(-1, 0)
        model.serve_lanes = lanes
        if sp:
            single = (float(np.mean(sp)), single_step_ms)
    latency = batch_latency(model, step, lanes, xs[0])
    if rank != 0:
        return None
    name, flops, nbytes = layers[dom]
    avg_ms = float(np.mean(probe_ms)) if probe_ms else float(ms0[dom])
    roof = launch_roofline(flops, nbytes, avg_ms, args.dtype)
    # HBM bytes per launch from the PMC counters: not measurable inside this process; taken from the committed
    # rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command ON THIS BUILD (fingerprint-checked), else null
    tr = pmc_traffic(args.config, name) if (args.batch, args.height, args.width) == tuple(CONFIGS[args.config][k] for k in ("batch", "height", "width")) else None
    roof["traffic"] = tr[0] if tr else None
    if tr:
        roof["traffic_profile"] = tr[1]
        # the same launch as rocprofv3's kernel trace timed it in the committed collection of THIS build (the live event pair
        # below brackets the launch on its stream and reads ~4 us more than the kernel's own duration)
        rp = rocprof_launch_ms(tr[1], name)
        roof["rocprof_avg_launch_ms"] = rp["ms"] if rp else None
        # (a kernel instantiation that serves SEVERAL launches of the forward has ONE average in the trace summary: the fraction is then
        #  the launches' MEAN work over that mean duration, and the line says so)
        def rocprof_frac_of(rp_):
            sh = [l for l in layers if l[0] in (rp_.get("shared_layers") or [])] or [(name, flops, nbytes)]
            return launch_roofline(float(np.mean([l[1] for l in sh])), float(np.mean([l[2] for l in sh])), rp_["ms"], args.dtype)["frac"]
        if rp:
            roof["rocprof_profile"] = rp["profile"]
            roof["rocprof_frac"] = rocprof_frac_of(rp)
            if rp["kernel_shared_by_launches"] > 1:
                roof["rocprof_note"] = ("the kernel instantiation serves %d launches of the forward (%s): rocprof_avg_launch_ms is their mean "
                                        "duration, rocprof_frac their mean work over it" % (rp["kernel_shared_by_launches"], ", ".join(rp["shared_layers"])))
    roof["kernel"] = name
    roof["avg_launch_ms"] = round(avg_ms, 5)
    roof["algorithmic_bytes_per_launch"] = nbytes
    roof["algorithmic_flops_per_launch"] = flops
    roof["concurrent_forwards"] = lanes
    if lanes >= 2:
        roof["note"] = ("measured live in the timed region, where %s forwards are in flight on as many HIP streams: the launch shares the "
                        "chip with the other lanes' launches, its duration is wall time -- `single_lane` is the same launch with one forward "
                        "in flight (second, untimed pass of the same steps), `pipeline` the chip-level rate of the timed steps"
                        % {2: "TWO", 3: "THREE"}.get(lanes, str(lanes)))
        if single:
            sl = launch_roofline(flops, nbytes, single[0], args.dtype)
            sl.update(avg_launch_ms=round(single[0], 5), ms_per_step=round(single[1], 4))
            rp1 = rocprof_launch_ms(tr[1], name, "_kernel_stats_1lane.txt") if tr else None
            if rp1:      # the committed SQDET_SERVE_LANES=1 kernel trace of this build
                sl.update(rocprof_avg_launch_ms=rp1["ms"], rocprof_profile=rp1["profile"], rocprof_frac=rocprof_frac_of(rp1))
            roof["single_lane"] = sl
    # the next largest launches (several are within a microsecond of each other, so which one is "dominant" can change from
    # run to run): durations from the untimed survey = one forward at a time, nothing else on the chip
    order = [int(k) for k in np.argsort(ms0)[::-1] if int(k) != dom][:3]
    roof["next_largest_launches"] = [dict(launch_roofline(layers[k][1], layers[k][2], float(ms0[k]), args.dtype), kernel=layers[k][0],
                                          survey_launch_ms=round(float(ms0[k]), 5)) for k in order]
    table = [{"layer": n, "ms": round(m, 5), "GB/s": round(b / (m * 1e-3) / 1e9, 1) if m > 0 else None,
              "TFLOP/s": round(f / (m * 1e-3) / 1e12, 2) if m > 0 else None, "bytes": b, "flops": f}
             for (n, f, b), m in zip(layers, ms0)]
    if args.layer_table:
        with open(args.layer_table, "w") as fh:
            json.dump({"layers": table, "forward_ms_sum": sum(ms0), "step_ms": elapsed / args.steps * 1e3,
                       "build_fingerprint": build_fingerprint()}, fh, indent=1)
    res = head()
    res["roofline"] = roof
    # chip-level view of the timed steps: the forward's algorithmic flops over the step time, and the composite roofline -- the sum over
    # the launches of max(bytes / 8 TB/s, flops / 2.5 PF/s) -- over the step time
    fl_sum = float(sum(f for _, f, _ in layers))
    comp = sum(max(b / (HBM_PEAK_GBS * 1e9), (f / (MFMA_F16_PEAK_TFLOPS * 1e12)) if args.dtype == "fp16" else 0.0) for _, f, b in layers)
    step_s = elapsed / args.steps
    res["pipeline"] = {"forwards_in_flight": lanes, "forward_gflop": round(fl_sum / 1e9, 2), "achieved_tflops": round(fl_sum / step_s / 1e12, 1),
                       "frac_of_mfma_peak": round(fl_sum / step_s / 1e12 / MFMA_F16_PEAK_TFLOPS, 4) if args.dtype == "fp16" else None,
                       "composite_roofline_ms": round(comp * 1e3, 4), "composite_roofline_frac": round(comp / step_s, 4)}
    res["box"] = box
    if getattr(model, "_lane_check", None):
        res["pipeline"]["lane_stream_check"] = json.loads(json.dumps(model._lane_check), parse_float=lambda v: round(float(v), 4))
    res["latency_ms_per_batch"] = latency
    res["host_issue_ms_per_step"] = round(t_issued / args.steps * 1e3, 4)
    res["forward_launches_ms_sum"] = round(float(sum(ms0)), 4)
    # diagnostic, outside the timed region: the same K forwards back to back WITHOUT decode / filter / D2H -- what the
    # post-processing costs the step is ms_per_step minus this
    torch.cuda.synchronize()
    pre = torch.empty((args.batch, plan.gh, plan.gw, plan.out_ch), dtype=xs[0].dtype, device=device)
    t1 = time.perf_counter()
    for i in range(args.steps):
        plan.forward(xs[i % nrot], pre)
    torch.cuda.synchronize()
    res["forward_only_ms_per_step"] = round((time.perf_counter() - t1) / args.steps * 1e3, 4)   # ONE forward in flight
    if lanes == 2:
        plans2 = [plan, model._native_plan(args.batch, 1)]
        pres = [pre, torch.empty_like(pre)]
        strs = [ln["stream"] for ln in model._serving_lanes(True, 2)]          # (the serving lanes' own streams: idle here)
        for i in range(2):
            with torch.cuda.stream(strs[i]):
                plans2[i].forward(xs[i], pres[i])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.steps):
            with torch.cuda.stream(strs[i & 1]):
                plans2[i & 1].forward(xs[i % nrot], pres[i & 1])
        torch.cuda.synchronize()
        res["forward_only_ms_per_step_two_lanes"] = round((time.perf_counter() - t1) / args.steps * 1e3, 4)
    res["score_epilogue"] = score_epilogue
    if score_bytes:
        res["roofline"]["score_bytes_in_conv12"] = score_bytes
    mode = os.environ.get("SQDET_POST_DEFER", "ride")
    res["post_processing"] = ("riders of the next forward's fire_chain launches (same stream, rows written to pinned host memory)"
                              if res["score_epilogue"] and mode == "ride" and plan.rider_capacity() >= args.batch else
                              "side stream behind a mid-forward event of the next forward" if res["score_epilogue"] and mode == "signal" and plan.overlap_layer() >= 0
                              else "side stream behind the forward")
    if args.sample:
        # configs[0] is a LATENCY case: one image, device idle before and after (the timed region above is the pipelined
        # throughput of the same step).  float32 = the reference's dtype, float16 = the benchmark's.
        lat = {args.dtype: round(sync_latency_ms(model, xs[0]), 4)}
        other = "fp32" if args.dtype == "fp16" else "fp16"
        a2 = argparse.Namespace(**vars(args))
        a2.dtype = other
        m2, _, xs2 = build_infer_model(a2, local_rank)
        lat[other] = round(sync_latency_ms(m2, xs2[0]), 4)
        res["latency_ms_per_image_sync"] = lat
    if not args.no_cpu_baseline and world == 1:
        res["cpu_baseline"] = cpu_baseline_infer(args, args.cpu_baseline_seconds)
    return res


# ------------------------------------------------------------------------------------------------ training
def training_flops_per_image(model):
    """2*MAC of the step: every conv forward; backward-filter of every trainable conv; backward-data of every trainable
    conv except the lowest one (nothing below it needs a gradient)."""
    fwd = bwd = 0.0
    convs = []
    seen = set()

    def walk(n):
        if n in seen:
            return
        seen.add(n)
        for i in n.inputs:
            walk(i)
        if n.op in ("conv", "conv_bn"):
            convs.append(n)
    walk(model.preds)
    first = True
    for n in convs:
        cin = int(n.inputs[0].get_shape()[3])
        _, ho, wo, cout = n.get_shape()
        f = 2.0 * n.attrs["size"] ** 2 * cin * cout * ho * wo
        fwd += f
        if model.trainable[n.name + "/kernels"]:
            bwd += f if first else 2.0 * f
            first = False
    return fwd, bwd


def cpu_baseline_train(args, seconds):
    """The training oracle (PyTorch-CPU float32 autograd restatement of forward + loss + backward) on a bounded sample."""
    from oracle import sqdet_oracle as O
    from oracle import train_oracle as TO
    nb = 2
    if args.arch == "squeezeDet":
        mc = O.squeezeDet_config_for_input(args.height, args.width)
        params = O.init_params("squeezeDet", seed=0)
        x = O.synthetic_images(nb, args.height, args.width, seed=7)
        mask, delta, box, labels = TO.synthetic_labels(mc, nb, seed=3)
        dm = torch.ones((nb, 24, 78, 768))
        fn = lambda: TO.loss_and_grads("squeezeDet", mc, params, x, dm, mask, delta, box, labels)
    else:
        from oracle import resnet_oracle as RO
        mc = O.kitti_res50_config()
        params = RO.init_params(seed=0)
        x = O.synthetic_images(nb, args.height, args.width, seed=7)
        mask, delta, box, labels = TO.synthetic_labels(mc, nb, seed=3)
        dm = torch.ones((nb, 24, 78, 1024))
        fn = lambda: RO.loss_and_grads(mc, params, x, dm, mask, delta, box, labels)
    fn()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += nb
        if time.perf_counter() - t0 >= seconds:
            break
    dt = time.perf_counter() - t0
    return {"value": round(n / dt, 3), "unit": "images/s", "cores": int(torch.get_num_threads()), "kind": "port",
            "sample": "%d synthetic %dx%d images (batches of %d): PyTorch-CPU float32 autograd restatement of forward + loss + "
                      "backward (no optimizer step); host has %d logical cores" % (n, args.width, args.height, nb, os.cpu_count())}


def run_train(args, rank, local_rank, world, device):
    import squeezedet_amd as S
    from squeezedet_amd import nets, ops, synthetic
    from squeezedet_amd.train import GraphedStep, ResNet50ConvDetTrainer, SqueezeDetTrainer
    from tools.bench_train import synthetic_ground_truth
    mc = S.kitti_squeezeDet_config() if args.arch == "squeezeDet" else S.kitti_res50_config()
    assert (args.height, args.width) == (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH), "training configs run at the config's own input size"
    mc.LOAD_PRETRAINED_MODEL = False
    mc.IS_TRAINING = True
    mc.BATCH_SIZE = args.batch
    cls, trainer = (nets.SqueezeDet, SqueezeDetTrainer) if args.arch == "squeezeDet" else (nets.ResNet50ConvDet, ResNet50ConvDetTrainer)
    tdt = torch.float32 if args.dtype == "fp32" else torch.float16
    model = cls(mc, gpu_id=str(local_rank), dtype=tdt)
    model.load_params(synthetic.synthetic_params(model, seed=0))      # same weights on every rank
    tr = trainer(model, lazy_overflow_check=True)
    nrot = 4
    xs = [synthetic.synthetic_images(args.batch, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, seed=100 + 10 * rank + k).to(device) for k in range(nrot)]
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(device)
    gts = [[torch.from_numpy(a).to(device) for a in synthetic_ground_truth(mc, args.batch, seed=200 + 10 * rank + k)] for k in range(nrot)]
    use_graph = not args.no_graph
    stepper = GraphedStep(tr, anchors, mc.CLASSES) if use_graph else None

    def step(i):
        x, (gt, gcls, gcnt) = xs[i % nrot], gts[i % nrot]
        if stepper is not None:
            return stepper.step(x, gt, gcls, gcnt)
        return tr.step(x, *ops.build_labels(anchors, gt, gcls, gcnt, mc.CLASSES)[:4])

    for i in range(max(args.warmup, 1)):
        out = step(i)
    torch.cuda.synchronize()
    spin_up(step, args.spinup_ms)
    box = clocks = None
    if args.full:
        box = box_calibration(device)
        clocks = {"before": gpu_state(local_rank)}        # (ahead of the last spin-up: see run_infer)
    spin_up(step, min(args.spinup_ms, 20.0))
    barrier(world, device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = step(i)
    t_issued = time.perf_counter() - t0
    torch.cuda.synchronize()
    tr.flush()
    own = time.perf_counter() - t0
    barrier(world, device)
    elapsed = time.perf_counter() - t0
    if args.full:
        clocks["after"] = gpu_state(local_rank)
    elapsed = max_over_ranks(elapsed, world, device, own)
    ranks_seen, devices = rank_census(rank, local_rank, world, device)
    if rank != 0:
        return None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, train_outputs(out, tr))
    value = aggregate_throughput(args.batch, args.steps, world, elapsed)
    res = result_head(args, value, world, elapsed, ranks_seen, devices, clocks)
    res["config"] = {"workload": "%s %s training, batch=%d per GPU, synthetic %dx%d images + KITTI-like ground truth (%d distinct batches "
                                 "in rotation): GPU label build + forward + loss + backward + gradient all-reduce + clipped Momentum"
                                 % (args.arch, "float32" if args.dtype == "fp32" else "mixed-precision (float16 activations)", args.batch,
                                    args.width, args.height, nrot),
                     "name": args.config, "global_batch": args.batch * world,
                     "parallelism": "dp%d (one flat float32 gradient bucket all-reduced over RCCL per step)" % world}
    res["hipgraph"] = bool(use_graph)
    res["skipped_steps"] = tr.skipped_steps
    if not args.full:
        return res
    fwd, bwd = training_flops_per_image(model)
    step_ms = elapsed / args.steps * 1e3
    peak = MFMA_F32_PEAK_TFLOPS if args.dtype == "fp32" else MFMA_F16_PEAK_TFLOPS
    flops = (fwd + bwd) * args.batch
    roof = {"bound": "mfma", "achieved": round(flops / (step_ms * 1e-3) / 1e12, 3), "peak": peak, "unit": "TFLOP/s"}
    roof["frac"] = round(roof["achieved"] / roof["peak"], 4)
    pk = pmc_kernels(args.config)
    roof["traffic"] = pk["hbm_bytes_per_step"] if pk else None      # fabric bytes of ONE step: every kernel's PMC bytes x its launches / steps
    if pk:
        roof["traffic_profile"] = pk["profile"]
    roof["kernel"] = "whole training step (forward + loss + backward + update; ~300 launches%s)" % (", replayed as one hipGraph" if use_graph else "")
    roof["avg_launch_ms"] = round(step_ms, 4)
    roof["algorithmic_flops_per_launch"] = flops
    roof["dominant_kernel"] = kernel_roofline(dominant_kernel_from_stats(args.config), pk, args.dtype)
    res["roofline"] = roof
    res["box"] = box
    res["host_issue_ms_per_step"] = round(t_issued / args.steps * 1e3, 4)
    res["losses"] = {k: float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")}
    if not args.no_cpu_baseline and world == 1:
        res["cpu_baseline"] = cpu_baseline_train(args, args.cpu_baseline_seconds)
    return res


def result_head(args, value, world, elapsed, ranks_seen=1, devices=None, clocks=None):
    return {
        "metric": args.metric,
        "value": round(value, 2),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "spinup_ms": args.spinup_ms,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f16" if args.dtype == "fp16" else "f32",
        "data": "reference data/sample.png (tests/golden/sample.png), random-init weights" if getattr(args, "sample", False) else "synthetic",
        # per-rank step time (the timed region of every rank / K): ms_per_step above is the max; a wide min..max = a straggler
        "rank_ms_per_step": None if not _RANK_SECONDS else {"min": round(min(_RANK_SECONDS) / args.steps * 1e3, 4),
                                                            "max": round(max(_RANK_SECONDS) / args.steps * 1e3, 4),
                                                            "per_rank": [round(v / args.steps * 1e3, 4) for v in _RANK_SECONDS]},
        "ranks_seen": ranks_seen,          # dist.get_world_size() as the process group reports it (== n_gpus or the run is void)
        "devices": devices,                # one entry per rank: device index, name, uuid / PCI id
        "clocks": clocks,                  # rank 0's GPU right before / after the timed region (amdsmi)
    }


def fail(msg, **extra):
    """A failure is ONE JSON line on stdout (the driver parses stdout) and a non-zero exit code -- never a usage string."""
    d = {"error": msg, "metric": None, "value": None}
    d.update(extra)
    print(json.dumps(d), flush=True)
    sys.exit(2)


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, argv):
    """`python bench.py --gpus N` (N > 1) outside a torchrun environment: re-launch this script as N local ranks under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1), forward rank 0's JSON line and the exit code.
    The reference is single-process / single-device (src/train.py:107, nets/squeezeDet.py:21): nothing to mirror."""
    import subprocess
    if not args.dry_run:
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if n < args.gpus and not (SHARE_DEVICE and n >= 1):
            fail("--gpus %d but only %d HIP device(s) are visible" % (args.gpus, n), n_gpus=args.gpus, devices_visible=n)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    sys.stderr.write(r.stderr[-6000:] if r.returncode != 0 else "")
    if r.returncode != 0 or not lines:
        fail("the %d-rank launch failed (exit code %d)" % (args.gpus, r.returncode), n_gpus=args.gpus,
             stderr_tail=r.stderr[-1500:], stdout_tail=r.stdout[-500:])
    print(lines[-1], flush=True)


def run_dry(args, rank, local_rank, world, device):
    """--dry-run: everything around the kernels -- rendezvous, barrier, the exactly-K-steps timed loop, max-over-ranks,
    the rank census, the JSON line -- with a no-op step on CPU tensors (gloo)."""
    step = lambda i: None
    for i in range(max(args.warmup, 1)):
        step(i)
    barrier(world, device)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    time.sleep(0.01 * (1 + rank))                      # ranks finish at different times: the MAX must win
    own = time.perf_counter() - t0
    barrier(world, device)
    elapsed = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed, world, device, own)
    ranks_seen, devices = rank_census(rank, local_rank, world, device)
    if rank != 0:
        return None
    res = result_head(args, aggregate_throughput(args.batch, args.steps, world, elapsed), world, elapsed, ranks_seen, devices, None)
    res.update(dry_run=True, value=None, ms_per_step=None, data="none (dry run: no kernels executed)")
    res["config"] = {"workload": "DRY RUN of %s: launcher + rendezvous + timing reduction only" % args.config, "name": args.config,
                     "global_batch": args.batch * world, "parallelism": "dp%d" % world}
    return res


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    rank, local_rank, world = dist_env()
    in_torchrun = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if world > 1 and world != args.gpus:
        fail("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world), n_gpus=args.gpus)
    if args.gpus > 1 and not in_torchrun:
        return self_launch(args, argv)
    if args.dry_run:
        import torch.distributed as dist
        device = torch.device("cpu")
        if in_torchrun:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
        res = run_dry(args, rank, local_rank, world, device)
    else:
        if not torch.cuda.is_available():
            fail("bench.py needs a HIP device (there is no CPU fallback); --dry-run exercises the launcher without one", n_gpus=args.gpus)
        ndev = torch.cuda.device_count()
        if local_rank >= ndev and not SHARE_DEVICE:
            fail("rank %d: local rank %d but only %d HIP device(s) are visible" % (rank, local_rank, ndev), n_gpus=args.gpus)
        # SQDET_SHARE_DEVICE=1 (tests on a one-GPU box): ranks beyond the visible devices share them, and the process group is
        # gloo (RCCL refuses two ranks on one device) -- the launcher / rendezvous / timing path with real kernels, NOT a
        # multi-GPU measurement: the line carries `shared_device`
        local_rank = local_rank % ndev
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
        # (SQDET_FORCE_DIST=1 under torch.distributed.run with one process: exercises the RCCL path on a single-GPU box)
        if world > 1 or (os.environ.get("SQDET_FORCE_DIST") == "1" and in_torchrun):
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if SHARE_DEVICE and world > ndev:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        if args.opt:
            from squeezedet_amd import ops
            for o in args.opt:
                k, v = o.split("=")
                ops.set_option(k, int(v))
        res = run_infer(args, rank, local_rank, world, device) if args.kind == "infer" else run_train(args, rank, local_rank, world, device)
        if args.opt and res is not None:
            res["options"] = list(args.opt)           # (a line measured with non-default knobs says so)
    if rank == 0:
        if SHARE_DEVICE and not args.dry_run and world > torch.cuda.device_count():
            res["shared_device"] = True
        if res.get("ranks_seen") != args.gpus:
            res["error"] = "ranks_seen %s != --gpus %d" % (res.get("ranks_seen"), args.gpus)
        print(json.dumps(res), flush=True)
    if _dist_on():
        import torch.distributed as dist
        dist.destroy_process_group()
    if rank == 0 and "error" in res:
        sys.exit(2)


if __name__ == "__main__":
    main()
