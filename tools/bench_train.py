#!/usr/bin/env python
"""Training throughput of SqueezeDet on MI355X: BASELINE.json configs[2], "SqueezeDet fp32 training
batch=20/GPU, RCCL grad all-reduce, synthetic KITTI labels" (network input 1248x384, the reference's
training size).  One step = GPU label build + forward (dropout on) + loss + backward + flat-bucket gradient all-reduce
+ clipped Momentum update.  Launch with torch.distributed.run for N > 1 (one process per GPU).

    python tools/bench_train.py --steps 10 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_ground_truth(mc, batch, seed, max_objects=8):
    """Seeded KITTI-like ground truth: n~U{1..8} boxes per image, w in [20,300], h in [20,200],
    centre uniform in the image, class U{0..C-1} -- as padded arrays for sqdet_build_labels."""
    rs = np.random.RandomState(seed)
    gt = np.zeros((batch, max_objects, 4), np.float64)
    cls = rs.randint(0, mc.CLASSES, size=(batch, max_objects)).astype(np.int32)
    cnt = rs.randint(1, max_objects + 1, size=batch).astype(np.int32)
    gt[..., 0] = rs.uniform(0, mc.IMAGE_WIDTH, (batch, max_objects))
    gt[..., 1] = rs.uniform(0, mc.IMAGE_HEIGHT, (batch, max_objects))
    gt[..., 2] = rs.uniform(20, 300, (batch, max_objects))
    gt[..., 3] = rs.uniform(20, 200, (batch, max_objects))
    return gt, cls, cnt


from squeezedet_amd.synthetic import KITTI_SIZES, synthetic_dataset  # noqa: E402,F401  (lives in the package: train.py --synthetic reads it too)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0,
                    help="images per GPU per step (default: 20 squeezeDet, 8 resnet50, 5 vgg16 -- the reference's BATCH_SIZE)")
    ap.add_argument("--arch", default="squeezeDet", choices=["squeezeDet", "resnet50", "vgg16"],
                    help="squeezeDet = BASELINE.json configs[2]; resnet50 = configs[4] (ResNet50+ConvDet, 1242x375, in float32); "
                         "vgg16 = VGG16+ConvDet, 1242x375")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f16"],
                    help="f32 = the reference's training dtype; f16 = mixed precision (float16 activations / activation gradients, "
                         "float32 master weights, weight gradients and optimizer, dynamic loss scale) -- configs[4] is resnet50 + f16")
    ap.add_argument("--augment", nargs="?", const="reference", default="", choices=["reference", "ssd"],
                    help="read every batch inside the timed step through a resident BatchReader from synthetic uint8 images of the "
                         "four KITTI sizes, rois in original pixels.  reference (also the bare flag): the reference's drift / flip "
                         "augmentation, imdb.read_batch; ssd: crop windows, zoom-out up to 2x and colour jitter (train.py --augment ssd "
                         "--zoom_out 2 --color_jitter)")
    ap.add_argument("--mosaic", type=float, default=0.0, metavar="P",
                    help="with --augment: a batch image is a mosaic of four images with probability P (train.py --mosaic P)")
    from squeezedet_amd import drivers
    drivers.add_loss_args(ap)             # --bbox_loss, --focal_gamma, --bbox_loss_coef as train.py takes them
    drivers.add_optim_args(ap)            # --optimizer ... --ema_warmup as train.py takes them
    drivers.add_assign_flags(ap)          # --assign ... --assign_topk as train.py takes them
    drivers.add_distill_args(ap)          # --teacher_net ... --distill_conf_floor as train.py takes them
    args = ap.parse_args(argv)
    drivers.check_distill_args(ap, args)
    drivers.check_loss_args(ap, args)
    drivers.check_optim_args(ap, args)
    drivers.check_assign_args(ap, args)
    if not 0.0 <= args.mosaic <= 1.0 or (args.mosaic > 0.0 and not args.augment):
        ap.error("--mosaic P needs 0 <= P <= 1 and --augment")
    if args.batch <= 0:
        args.batch = {"squeezeDet": 20, "resnet50": 8, "vgg16": 5}[args.arch]
    return args


def make_config(args):
    """(mc of --arch with the batch size and the loss flags applied, the loss policy as train.py records it)."""
    import squeezedet_amd as S
    from squeezedet_amd import drivers
    mc = {"squeezeDet": S.kitti_squeezeDet_config, "resnet50": S.kitti_res50_config, "vgg16": S.kitti_vgg16_config}[args.arch]()
    mc.LOAD_PRETRAINED_MODEL = False
    mc.IS_TRAINING = True
    mc.BATCH_SIZE = args.batch
    loss_policy, _ = drivers.loss_policy(args, mc)
    return mc, loss_policy


def make_optim(args, mc):
    """The optimizer policy as train.py records it (sets mc.WEIGHT_DECAY), or None without any of its flags: the trainer's own
    update.  cosine / linear without --lr_total_steps run over this benchmark's own length, as train.py's over --max_steps."""
    from squeezedet_amd.optim import optim_policy
    if not hasattr(args, "max_steps"):
        args.max_steps = args.warmup + args.steps
    optim, optim_off = optim_policy(args, mc)
    return None if optim == optim_off else optim


def main():
    args = parse_args()
    rank, local_rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import squeezedet_amd as S
    from squeezedet_amd import drivers, nets, synthetic
    from squeezedet_amd.train import ResNet50ConvDetTrainer, SqueezeDetTrainer, VGG16ConvDetTrainer
    mc, loss_policy = make_config(args)
    optim = make_optim(args, mc)
    cls, trainer = {"squeezeDet": (nets.SqueezeDet, SqueezeDetTrainer), "resnet50": (nets.ResNet50ConvDet, ResNet50ConvDetTrainer),
                    "vgg16": (nets.VGG16ConvDet, VGG16ConvDetTrainer)}[args.arch]
    model = cls(mc, gpu_id=str(local_rank), dtype=torch.float32 if args.dtype == "f32" else torch.float16)
    model.load_params(synthetic.synthetic_params(model, seed=0))      # same weights on every rank
    from squeezedet_amd import assign as assign_mod
    assign_policy, _ = drivers.assign_policy(args, mc)
    assign = assign_mod.from_dict(assign_policy)
    assign = None if assign_mod.is_default(assign) else assign
    # --teacher_net: a second, inference-only model at the step's batch and size (synthetic variables of seed 1 without a checkpoint)
    if hasattr(args, "teacher_net") and not hasattr(args, "teacher_dtype"):
        args.teacher_dtype = "fp32" if args.dtype == "f32" else "fp16"
    distill_policy, _ = drivers.distill_policy(args, mc)
    teacher = drivers.make_teacher(distill_policy, mc, local_rank, seed=0)
    tr = trainer(model, lazy_overflow_check=True, optim=optim, assign=assign, **({} if teacher is None else {"teacher": teacher}))
    x = synthetic.synthetic_images(args.batch, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, seed=100 + rank).to(dev)
    # ground truth lives on the device; the anchor assignment + dense label build (imdb.py:195-239,
    # train.py:163-224) runs on the GPU inside every step, like the reference's per-batch _load_data
    from squeezedet_amd import ops
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(dev)
    gt, gcls, gcnt = [torch.from_numpy(a).to(dev) for a in synthetic_ground_truth(mc, args.batch, seed=200 + rank)]
    nobj = float(gcnt.sum().item())      # known to the host: no per-step device -> host sync for sum(input_mask)
    # (under --assign iou / atss the normaliser is the number of positives, sum(input_mask): the trainer sums it on the device)
    build = lambda g, c, n: ops.build_labels(anchors, g, c, n, mc.CLASSES, assign=assign, anchors_per_grid=int(mc.ANCHOR_PER_GRID))[:4]
    one_step = lambda: tr.step(x, *build(gt, gcls, gcnt), num_objects=nobj if assign is None else None)
    if args.augment:
        if args.augment == "ssd":
            mc.AUG_GEOMETRY, mc.AUG_ZOOM_OUT_MAX, mc.AUG_COLOR = "ssd", 2.0, True
        mc.AUG_MOSAIC_PROB = args.mosaic
        reader = S.BatchReader(mc, *synthetic_dataset(mc, 2 * args.batch, seed=300 + rank), seed=rank, device=dev,
                               dtype=model.dtype, resident=True)

        def one_step():
            b = reader.read_batch()
            return tr.step(b.image_input, *build(b.gt_boxes, b.gt_classes, b.gt_counts),
                           num_objects=float(sum(len(l) for l in b.label_per_batch)) if assign is None else None)
    for _ in range(args.warmup):
        out = one_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier(device_ids=[local_rank])
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one_step()
    t_issued = time.perf_counter() - t0          # host done enqueueing (diagnostic: launch-bound if ~ the step time)
    torch.cuda.synchronize()
    tr.flush()
    if world > 1:
        dist.barrier(device_ids=[local_rank])
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    if rank == 0:
        label = {"squeezeDet": "SqueezeDet 1248x384", "resnet50": "ResNet50+ConvDet 1242x375", "vgg16": "VGG16+ConvDet 1242x375"}[args.arch]
        prec = "fp32" if args.dtype == "f32" else "fp16 (mixed precision)"
        print(json.dumps({"metric": "images/sec %s %s training" % (label, prec), "value": round(args.batch * world * args.steps / el, 2),
                          "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(el / args.steps * 1e3, 3),
                          "host_issue_ms_per_step": round(t_issued / args.steps * 1e3, 3), "dtype": args.dtype,
                          "data": ("synthetic uint8 + BatchReader " + {"reference": "drift/flip", "ssd": "ssd windows/zoom-out 2/colour"}[args.augment]
                                   + (" + mosaic %g" % args.mosaic if args.mosaic > 0.0 else "")) if args.augment else "synthetic",
                          "config": {"workload": "%s %s training, batch=%d per GPU, forward+loss+backward+"
                                                 "all-reduce+clipped Momentum" % (label, prec, args.batch), "parallelism": "dp%d" % world},
                          "loss": loss_policy, **({"assign": assign_policy} if assign is not None else {}), **({"optim": optim} if optim is not None else {}), **({"distill": distill_policy, "distill_losses": {k: float(out[k]) for k in ("distill_class_loss", "distill_conf_loss", "distill_bbox_loss")}} if teacher is not None else {}), "skipped_steps": tr.skipped_steps, "loss_scale": tr.loss_scale,
                          "losses": {k: float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")}}))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
