#!/usr/bin/env python
"""Trains SqueezeDet / SqueezeDet+ / ResNet50+ConvDet / VGG16+ConvDet on KITTI (the reference's src/train.py): resumable,
with on-device summaries.

    python train.py --data_path KITTI --image_set train --train_dir logs/train --net squeezeDet [--pretrained_model_path w.npz]
    python train.py --dataset PASCAL_VOC --data_path VOCdevkit --year 2007 --image_set trainval --train_dir logs/voc
    python train.py --synthetic 40 --train_dir /tmp/run --max_steps 100          # seeded synthetic data, no dataset needed
    python train.py ... --resume                                                  # continue from the newest checkpoint
    python train.py ... --anchor_shapes anchors.json --anchor_report             # shapes from tools/fit_anchors.py; coverage report
    python train.py ... --bbox_loss giou --focal_gamma 2                          # a GIoU box term and a focal class term
    python train.py ... --optimizer adamw --lr_schedule cosine --warmup_steps 500 --ema_decay 0.999   # AdamW, warm-up + cosine, EMA weights
    python train.py ... --teacher_net vgg16 --teacher_checkpoint logs/vgg16 --distill_temperature 2   # train towards a bigger net's output

Per step as the reference (train.py:266-330): a summary step (step % summary_step == 0) runs the eager trainer step with the
activations kept and hands it to squeezedet_amd.summary.TrainSummary (-> <train_dir>/summaries.jsonl, in place of TF event
files) and, with --image_summary N, the first N images of its batch with ground truth and detections drawn on the device to
squeezedet_amd.viz.ImageSummary (-> <train_dir>/images/step-<step>/<i>.png); every other step is a hipGraph replay
(squeezedet_amd.train.GraphedStep) unless --no_graph.  A checkpoint -- written at step % checkpoint_step == 0 and at the last
step, named by the step -- is the pair model.ckpt-<step>.npz (what eval.py polls for and demo.py --weights reads) +
state/step-<step>.npz (squeezedet_amd.checkpoint); --resume continues from the newest pair bit for bit.  <train_dir>/model_metrics.txt is the reference's (train.py:137-159).

The reference deletes --train_dir at start (train.py:338-340).  Here a non-empty --train_dir is refused unless --resume
or --overwrite (delete, as the reference does).  --dataset PASCAL_VOC trains SqueezeDet with the 20-class config
(config.voc_squeezeDet_config_for_input, at --image_size or 384 x 1248) on <data_path>/VOC<year>, read by
squeezedet_amd.voc.load_voc; the images may differ in size.  (Its ConvDet head is padded to 23 classes: DESIGN.md section 3.9.)
--anchor_shapes FILE (tools/fit_anchors.py writes it) replaces the config's anchor shapes (config.with_anchor_shapes, before the
head is padded); the file is copied to <train_dir>/anchor_shapes.json, where eval.py and demo.py find it, and the shapes are
recorded in every checkpoint: --resume refuses other shapes and, without the flag, uses the recorded ones.  --augment ssd
[--zoom_out MAX] and --color_jitter switch on BatchReader's crop-window / zoom-out and colour augmentation (squeezedet_amd.imdb);
the policy is recorded in every checkpoint and --resume under another one is refused.  --mosaic P makes a batch image, with
probability P, a mosaic of four training images (one sqdet_augment_bgr_mosaic launch per batch); P is recorded under its own key,
`mosaic`, and --resume under another P is refused (a checkpoint without the key was trained with 0).  --bbox_loss
{delta_l2,iou,giou,diou,ciou}, --focal_gamma G and --bbox_loss_coef X choose the box term, the class term's focal exponent and
mc.LOSS_COEF_BBOX (the defaults are the reference's loss); the three are recorded under the key `loss`, and
--resume under another loss policy is refused (a checkpoint without the key was trained with the defaults).  --optimizer
{momentum,nesterov,adamw} (--adam_beta1, --adam_beta2, --adam_eps), --weight_decay, --clip_norm {per_variable,global}, --lr,
--lr_schedule {staircase,constant,cosine,linear} (--warmup_steps, --warmup_factor, --min_lr_ratio, --lr_total_steps) and --ema_decay D
(--ema_warmup) choose the update rule, the clip, the learning-rate schedule and an exponential moving average of the weights (DESIGN.md
section 3.18; the defaults are the reference's update, and a run without any of them launches what it always launched).  A policy that
differs from the defaults is recorded under the key `optim`, and --resume under another one -- --lr_total_steps included -- is refused.
With --ema_decay every checkpoint adds <train_dir>/ema/model.ckpt-<step>.npz, the model file with the averaged weights, which eval.py
--ema reads.  --teacher_net NET [--teacher_checkpoint PATH --teacher_dtype D --distill_temperature T --distill_class_coef X
--distill_conf_coef X --distill_bbox_coef X --distill_conf_floor F] adds a teacher: a second, inference-only
model whose ConvDet output for the step's images is a further target of the loss -- its grid, anchors and classes must be the
student's, which SqueezeDet+'s are not.  The policy is recorded under the key `distill` (the checkpoint's path as a string only), and
--resume with another one, or with none, is refused; a checkpoint without the key was trained without a teacher.  --anchor_report writes
<train_dir>/anchor_coverage.json (squeezedet_amd.anchors.dataset_coverage of the training set) once, before the first step.
Under torch.distributed.run every rank trains its own batches (reader seeded seed + rank) and rank 0 writes the files.
"""
import argparse
import datetime
import os
import shutil
import sys
import time

import numpy as np

from squeezedet_amd import drivers

RESIDENT_BYTES = 4 << 30       # a dataset whose uint8 images fit this budget lives on the device (BatchReader resident=True)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[1], formatter_class=argparse.RawDescriptionHelpFormatter)
    drivers.add_dataset_args(ap, image_set_default="train")
    drivers.add_model_args(ap, dtype_default="fp32")
    ap.add_argument("--train_dir", default="/tmp/squeezeDet/train", help="Directory where to write summaries and checkpoints.")
    ap.add_argument("--max_steps", type=int, default=1000000, help="Maximum number of batches to run.")
    ap.add_argument("--pretrained_model_path", default="", help="Path to the pretrained model (.npz, or the backbone pickle).")
    ap.add_argument("--summary_step", type=int, default=10, help="Number of steps to save summary (0: never).")
    ap.add_argument("--checkpoint_step", type=int, default=1000, help="Number of steps to save a checkpoint.")
    ap.add_argument("--batch_size", type=int, default=0, help="images per GPU per step (default: the config's BATCH_SIZE)")
    ap.add_argument("--seed", type=int, default=0, help="seeds the batch order, the augmentation, the dropout and --synthetic")
    ap.add_argument("--resume", action="store_true", help="continue from the newest checkpoint of --train_dir")
    ap.add_argument("--overwrite", action="store_true", help="delete a non-empty --train_dir first, as the reference does")
    ap.add_argument("--keep_checkpoints", type=int, default=0, help="keep only the newest N checkpoints (0: all)")
    ap.add_argument("--no_graph", action="store_true", help="eager steps only (no hipGraph replay)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="train on N seeded synthetic KITTI-sized images")
    ap.add_argument("--loss_scale", type=float, default=1024.0, help="fp16: the initial loss scale")
    ap.add_argument("--image_summary", type=int, default=0, metavar="N",
                    help="at summary steps, write the first N images of the batch with ground truth and detections drawn (0: none)")
    ap.add_argument("--anchor_shapes", default="", metavar="FILE", help="anchor shapes fitted by tools/fit_anchors.py (default: the config's)")
    ap.add_argument("--anchor_report", action="store_true",
                    help="write <train_dir>/anchor_coverage.json, how the anchors cover the training set, before the first step")
    # (the three augmentation flags leave no attribute behind when they are not given: augment_policy supplies the defaults, and
    # the namespace of a command line without them stays what every earlier checkpoint's driver saw)
    ap.add_argument("--augment", default=argparse.SUPPRESS, choices=["reference", "ssd"],
                    help="reference (default): the drift and mirror of the reference; ssd: zoom-out and IoU-constrained crop windows "
                         "(squeezedet_amd.imdb)")
    ap.add_argument("--zoom_out", type=float, default=argparse.SUPPRESS, metavar="MAX",
                    help="--augment ssd: with probability 1/2 place the image on a canvas U[1, MAX] times its size (default 1: never)")
    ap.add_argument("--color_jitter", action="store_true", default=argparse.SUPPRESS,
                    help="random brightness, contrast, saturation and hue, one 3x4 matrix per image")
    ap.add_argument("--mosaic", type=float, default=argparse.SUPPRESS, metavar="P",
                    help="with probability P a batch image is a mosaic: four training images, each cropped into its own pane of the "
                         "network input (default 0: never)")
    drivers.add_loss_args(ap)
    drivers.add_optim_args(ap)
    drivers.add_assign_flags(ap)
    drivers.add_distill_args(ap)
    a = ap.parse_args(argv)
    drivers.check_dataset_args(ap, a)
    drivers.check_loss_args(ap, a)
    drivers.check_optim_args(ap, a)
    drivers.check_assign_args(ap, a)
    drivers.check_distill_args(ap, a)
    if not 0.0 <= getattr(a, "mosaic", 0.0) <= 1.0:
        ap.error("--mosaic P needs 0 <= P <= 1")
    if a.resume and a.overwrite:
        ap.error("--resume and --overwrite exclude each other")
    policy = augment_policy(a)
    if policy["zoom_out"] < 1.0 or (policy["zoom_out"] > 1.0 and policy["geometry"] != "ssd"):
        ap.error("--zoom_out MAX needs MAX >= 1 and --augment ssd")
    return a


AUGMENT_OFF = dict(geometry="reference", zoom_out=1.0, color_jitter=False)      # what a checkpoint without the record was trained with


def augment_policy(a, mc=None):
    """The policy of --augment / --zoom_out / --color_jitter as the checkpoint records it; sets mc's augmentation fields when given."""
    policy = dict(geometry=getattr(a, "augment", AUGMENT_OFF["geometry"]), zoom_out=float(getattr(a, "zoom_out", AUGMENT_OFF["zoom_out"])),
                  color_jitter=bool(getattr(a, "color_jitter", AUGMENT_OFF["color_jitter"])))
    if mc is not None:
        mc.AUG_GEOMETRY = "ssd" if policy["geometry"] == "ssd" else "drift"
        mc.AUG_ZOOM_OUT_MAX, mc.AUG_COLOR = policy["zoom_out"], policy["color_jitter"]
    return policy


DISTILL_TERMS = ("distill_class_loss", "distill_conf_loss", "distill_bbox_loss")      # a step's extra outputs under --teacher_net
ASSIGN_OFF = dict(mode="reference")      # what a checkpoint without the `assign` record was trained with (drivers.assign_policy's)


def check_resume_record(saved, extra, loss_off, optim_off=None):
    """--resume: what the checkpoint records (`saved`) against what this run asks for (`extra`); SystemExit on the first key that
    differs.  A checkpoint from before a key existed was trained with that key's defaults (`loss_off`: drivers.loss_policy's;
    `optim_off`: optim.optim_policy's; `assign`: the reference's one anchor per object; `distill`: no teacher -- a key a run
    without a teacher does not record either, so it is compared in both directions)."""
    saved, extra = dict(saved), dict(extra)
    saved.setdefault("distill", None)
    extra.setdefault("distill", None)
    saved.setdefault("assign", ASSIGN_OFF)
    saved.setdefault("augment", AUGMENT_OFF)
    saved.setdefault("mosaic", 0.0)
    saved.setdefault("loss", loss_off)
    if optim_off is not None:             # (a run without the optimizer flags records no `optim` key: its state file is what it was)
        saved.setdefault("optim", optim_off)
        extra.setdefault("optim", optim_off)
    for key, now in extra.items():
        if saved.get(key) != now:
            raise SystemExit("--resume: the checkpoint was trained with %s %r, this run asks for %r" % (key, saved.get(key), now))


def make_trainer(a, mc, local_rank=0):
    """(model, trainer) of --net in training mode."""
    mc.IS_TRAINING = True
    mc.PRETRAINED_MODEL_PATH = a.pretrained_model_path
    return drivers.build_model(mc, a.net, str(local_rank), a.dtype, a.batch_size), drivers.trainer_class(a.net)


def initial_params(a, model):
    from squeezedet_amd.config import pin_padding_classes
    params = _initial_params(a, model)
    if model.mc.get("HEAD_PAD_CLASSES", 0):         # a padded ConvDet head (PASCAL_VOC): its padding classes get probability 0
        for name in ("conv12/kernels", "conv12/biases"):
            params.setdefault(name, model.params[name])          # (a backbone pickle does not cover the head)
        params = pin_padding_classes(model.mc, params)
    return params


def _initial_params(a, model):
    from squeezedet_amd import synthetic, weights
    p = a.pretrained_model_path
    if not p:
        return synthetic.synthetic_params(model, seed=a.seed)
    if p.endswith(".npz"):
        return weights.load_params(p)
    import joblib                       # the reference's ImageNet backbones are joblib pickles (nn_skeleton.py:397-412)
    return weights.from_caffe_weights(joblib.load(p), model)


def load_dataset(a, mc):
    """(images: list of uint8 BGR arrays, rois)."""
    if a.synthetic:
        return drivers.synthetic_data(mc, a.synthetic, a.seed)
    data = drivers.load_index(a.dataset, a.data_path, a.year, a.image_set, mc)
    return [drivers.read_bgr(p) for p in data.image_paths], data.rois


def write_model_metrics(path, model):
    """train.py:137-159."""
    with open(path, "w") as f:
        for k, (title, counter) in enumerate((("Number of parameter by layer:", model.model_size_counter),
                                              ("Activation size by layer:", model.activation_counter),
                                              ("Number of flops by layer:", model.flop_counter))):
            f.write(("\n" if k else "") + title + "\n")
            count = 0
            for c in counter:
                f.write("\t{}: {}\n".format(c[0], c[1]))
                count += c[1]
            f.write("\ttotal: {}\n".format(count))


def resolve_anchor_shapes(a, resume_step=None):
    """The anchor shapes of this run, [k,2] or None (the config's): --anchor_shapes, checked against what the checkpoint to resume
    from records; without the flag, what it records."""
    from squeezedet_amd import anchors, checkpoint
    shapes = anchors.load_for_driver(a.anchor_shapes) if a.anchor_shapes else None
    if resume_step is not None:
        rec = checkpoint.read_extra(a.train_dir, resume_step).get("anchor_shapes")
        if shapes is not None and (rec is None or not anchors.same_shapes(rec, shapes)):
            raise SystemExit("--resume: the checkpoint was trained with anchor shapes %s, --anchor_shapes %s gives %s"
                             % ("of its config" if rec is None else rec, a.anchor_shapes, shapes.tolist()))
        if shapes is None and rec is not None:
            shapes = np.array(rec, np.float64)
    return shapes


def write_anchor_report(path, mc, reader, device):
    """--anchor_report: how mc's anchors cover the training set (no augmentation), as JSON."""
    import json
    from squeezedet_amd import anchors, config
    rep = anchors.dataset_coverage(mc, reader.rois, reader.sizes, device=device)
    with open(path, "w") as f:
        json.dump(dict(rep.summary(), anchor_shapes=config.anchor_shapes_of(mc).tolist(),
                       image_size=[int(mc.IMAGE_HEIGHT), int(mc.IMAGE_WIDTH)]), f, indent=1)
        f.write("\n")
    return rep


def prepare_train_dir(a, rank):
    """The train_dir policy; returns the step to resume from, or None."""
    from squeezedet_amd import checkpoint
    used = os.path.isdir(a.train_dir) and bool(os.listdir(a.train_dir))
    if a.resume:
        step = checkpoint.latest(a.train_dir) if used else None
        if step is None:
            raise SystemExit("--resume: no checkpoint (model.ckpt-<step>.npz with state/step-<step>.npz) in %s" % a.train_dir)
        return step
    if used and not a.overwrite:
        raise SystemExit("%s is not empty: pass --resume to continue its run or --overwrite to delete it" % a.train_dir)
    if rank == 0:
        if used:
            shutil.rmtree(a.train_dir)
        os.makedirs(a.train_dir, exist_ok=True)
    return None


class Run:
    """Everything one process of a run holds: config, model, trainer, reader, the graphed stepper and the summaries.
    ``Run(a)`` builds it (and restores the checkpoint of ``resume_step``); ``step(k)`` is the body of one training step,
    ``save(k)`` writes the checkpoint pair, ``close()`` settles the trainer and the summaries."""

    def __init__(self, a, rank=0, local_rank=0, world=1, resume_step=None):
        import torch
        import squeezedet_amd as S
        from squeezedet_amd import checkpoint
        from squeezedet_amd.summary import TrainSummary
        from squeezedet_amd.train import GraphedStep
        self.a, self.rank = a, rank
        self.dev = dev = torch.device("cuda", local_rank)
        self.anchor_shapes = resolve_anchor_shapes(a, resume_step)
        self.mc = mc = drivers.make_config(a.net, a.image_size, a.dataset, self.anchor_shapes)
        policy = augment_policy(a, mc)
        mc.AUG_MOSAIC_PROB = mosaic = float(getattr(a, "mosaic", 0.0))
        if mosaic > 0.0 and not mc.DATA_AUGMENTATION:
            raise SystemExit("--mosaic needs a config with DATA_AUGMENTATION on")
        loss, loss_off = drivers.loss_policy(a, mc)         # (before the model is built: a padded head's config is a copy of mc)
        from squeezedet_amd.optim import optim_policy
        optim, optim_off = optim_policy(a, mc)              # (sets mc.WEIGHT_DECAY: before the trainer reads it)
        from squeezedet_amd import assign as assign_mod
        assign, _ = drivers.assign_policy(a, mc)
        self.assign = assign_mod.from_dict(assign)
        distill, _ = drivers.distill_policy(a, mc)          # (None without --teacher_net: nothing below changes then)
        self.model, trainer_cls = make_trainer(a, mc, local_rank)
        self.model.load_params(initial_params(a, self.model))
        # (every rank builds its own teacher, from the same file or seed: a second, inference-only model on this rank's device)
        from squeezedet_amd._lib import SqdetError
        try:
            self.teacher = drivers.make_teacher(distill, self.model.mc, local_rank, seed=a.seed)
        except SqdetError as e:
            raise SystemExit("--teacher_net: %s" % e)
        more = {} if self.teacher is None else dict(teacher=self.teacher)
        # (a run without any of the optimizer flags takes the trainer's own path: the launches and state keys of every run before)
        self.tr = trainer_cls(self.model, seed=a.seed, loss_scale=a.loss_scale, optim=None if optim == optim_off else optim,
                              assign=None if assign_mod.is_default(self.assign) else self.assign, **more)
        images, rois = load_dataset(a, mc)
        resident = int(sum(im.nbytes for im in images)) <= RESIDENT_BYTES
        self.reader = S.BatchReader(mc, images, rois, seed=a.seed + rank, device=dev, dtype=self.model.dtype, resident=resident)
        self.extra = dict(image_size=[int(mc.IMAGE_HEIGHT), int(mc.IMAGE_WIDTH)], net=a.net, dtype=a.dtype, batch_size=int(mc.BATCH_SIZE),
                          anchor_shapes=None if self.anchor_shapes is None else self.anchor_shapes.tolist(), augment=policy, mosaic=mosaic, loss=loss,
                          assign=assign)
        if optim != optim_off:
            self.extra["optim"] = optim
        if distill is not None:
            self.extra["distill"] = distill
        self.first = 0
        if resume_step is not None:
            check_resume_record(checkpoint.read_extra(a.train_dir, resume_step), self.extra, loss_off, optim_off)
            checkpoint.load(a.train_dir, resume_step, self.model, self.tr, self.reader)
            self.first = resume_step + 1
        self.anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(dev)
        self.stepper = None if a.no_graph else GraphedStep(self.tr, self.anchors, mc.CLASSES)
        self.summary = TrainSummary(self.tr, a.train_dir, write=(rank == 0)) if a.summary_step > 0 else None
        # (reads the summary step's batch and preds, nothing of the trainer or the reader: a run with it is bitwise the run without)
        self.images = None
        if a.image_summary > 0 and a.summary_step > 0 and rank == 0:
            from squeezedet_amd.viz import ImageSummary
            self.images = ImageSummary(mc, a.train_dir, a.image_summary, device=dev)
        self._wd_plan = None

    def total_loss(self, out):
        """loss = the three terms + the weight decay of the 'losses' collection (one statistics call over the flat variables:
        sumsq per kernel); a synchronisation: print steps only."""
        from squeezedet_amd.summary import StatsPlan, decode
        tr = self.tr
        if self._wd_plan is None:
            self._wd_plan = StatsPlan([(tr.view[n].data_ptr() - tr.flat_params.data_ptr()) // 4 for n in tr.names],
                                      [int(tr.view[n].numel()) for n in tr.names], tr.total, self.dev)
        rec = decode(self._wd_plan.run(tr.flat_params).cpu(), self._wd_plan.n_bins)
        wd = sum(float(r["sumsq"]) for n, r in zip(tr.names, rec) if n.endswith("/kernels")) * self.mc.WEIGHT_DECAY / 2
        terms = ("class_loss", "conf_loss", "bbox_loss") + (() if self.teacher is None else DISTILL_TERMS)
        return sum(float(out[k]) for k in terms) + wd

    def positives_note(self, labels, b):
        """The summaries line's tail under --assign iou / atss: the mean number of positive anchors per object of this batch."""
        if len(labels) < 7:
            return ""
        from squeezedet_amd.assign import positives_summary
        return ", positives per object: {:.2f}".format(positives_summary(labels[6], b.gt_counts)[1])

    def step(self, step):
        """train.py:273-325 for one step."""
        from squeezedet_amd import ops
        a, tr, mc, summary = self.a, self.tr, self.mc, self.summary
        start_time = time.time()
        is_summary = summary is not None and step % a.summary_step == 0
        lr = tr.learning_rate()
        b = self.reader.read_batch()
        if is_summary or self.stepper is None:
            labels = ops.build_labels(self.anchors, b.gt_boxes, b.gt_classes, b.gt_counts, mc.CLASSES, assign=tr.assign,
                                      anchors_per_grid=int(mc.ANCHOR_PER_GRID))
            out = tr.step(b.image_input, *labels[:4], keep_activations=is_summary)
        else:
            out = self.stepper.step(b.image_input, b.gt_boxes, b.gt_classes, b.gt_counts)
        if is_summary:
            summary.record(step, out, lr)
            if self.images is not None:
                self.images.record(step, b, out["preds"])
            if self.rank == 0:
                print("conf_loss: {}, bbox_loss: {}, class_loss: {}".format(float(out["conf_loss"]), float(out["bbox_loss"]),
                                                                           float(out["class_loss"])) + self.positives_note(labels, b)
                      + ("" if self.teacher is None else "".join(", {}: {}".format(k, float(out[k])) for k in DISTILL_TERMS)))
        elif summary is not None:
            summary.poll()
            if self.images is not None:
                self.images.poll()
        if step % 10 == 0:
            loss_value = self.total_loss(out)               # (reads the device: the step has finished)
            duration = time.time() - start_time
            # the reference asserts on the loss every step (train.py:313); here the trainer raises FloatingPointError on a
            # non-finite float32 gradient (at the latest at the next step / flush), so the loss is read on print steps only
            assert not np.isnan(loss_value), \
                "Model diverged. Total loss: {}, conf_loss: {}, bbox_loss: {}, class_loss: {}".format(
                    loss_value, float(out["conf_loss"]), float(out["bbox_loss"]), float(out["class_loss"]))
            if self.rank == 0:
                print("%s: step %d, loss = %.2f (%.1f images/sec; %.3f sec/batch)" % (
                    datetime.datetime.now(), step, loss_value, mc.BATCH_SIZE / duration, float(duration)))
                sys.stdout.flush()
        return out

    def save(self, step):
        """(state_dict() flushes the trainer first: a diverged step raises before anything is written)"""
        from squeezedet_amd import checkpoint
        if self.rank == 0:
            return checkpoint.save(self.a.train_dir, step, self.model, self.tr, self.reader, extra=self.extra, keep=self.a.keep_checkpoints)
        self.tr.flush()

    def close(self):
        try:
            self.tr.flush()
        finally:
            try:
                if self.summary is not None:
                    self.summary.close()
            finally:
                if self.images is not None:
                    self.images.close()


def train(a):
    rank, local_rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    resume_step = prepare_train_dir(a, rank)
    import torch
    if world == 1:
        local_rank = int(a.gpu)
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        dist.barrier(device_ids=[local_rank])          # rank 0 has prepared the directory
    run = Run(a, rank, local_rank, world, resume_step)
    if rank == 0:
        if resume_step is not None:
            print("Resuming from step {} of {}".format(resume_step, a.train_dir))
        write_model_metrics(os.path.join(a.train_dir, "model_metrics.txt"), run.model)
        print("Model statistics saved to {}.".format(os.path.join(a.train_dir, "model_metrics.txt")))
        beside = os.path.join(a.train_dir, "anchor_shapes.json")
        if a.anchor_shapes and os.path.abspath(a.anchor_shapes) != os.path.abspath(beside):
            shutil.copyfile(a.anchor_shapes, beside)
        if a.anchor_report and resume_step is None:
            rep = write_anchor_report(os.path.join(a.train_dir, "anchor_coverage.json"), run.mc, run.reader, run.dev)
            print("Anchor coverage of the training set ({}):".format(os.path.join(a.train_dir, "anchor_coverage.json")))
            print("\n".join("  {}: {}".format(k, v) for k, v in rep.lines()))
    try:
        for step in range(run.first, a.max_steps):
            run.step(step)
            if (a.checkpoint_step > 0 and step % a.checkpoint_step == 0) or step + 1 == a.max_steps:
                run.save(step)
    finally:
        try:
            run.close()
        finally:
            if world > 1:
                torch.distributed.destroy_process_group()


def main(argv=None):
    train(parse_args(argv))


if __name__ == "__main__":
    main()
