"""What train.py, eval.py, demo.py and tools/fit_anchors.py decide the same way, once: the table of nets, the order in which a
config is built, the model constructor call, the image read, the dataset choice, the anchor-shape lookup and the shared flags.
Importing this needs neither torch nor a GPU; the nets and trainer classes are looked up when asked for."""
import numpy as np

from . import config

NETS = ("squeezeDet", "squeezeDet+", "resnet50", "vgg16")
DATASETS = ("KITTI", "PASCAL_VOC")
VOC_IMAGE_SIZE = (384, 1248)        # PASCAL_VOC without --image_size: SqueezeDet's KITTI input

# net -> (default config, config for an input size or None, class in squeezedet_amd.nets, class in squeezedet_amd.train)
# (SqueezeDetTrainer walks any conv / fire / pool chain: it trains SqueezeDet+ too, tests/test_gpu_train.py)
NET_TABLE = {
    "squeezeDet": (config.kitti_squeezeDet_config, config.kitti_squeezeDet_config_for_input, "SqueezeDet", "SqueezeDetTrainer"),
    "squeezeDet+": (config.kitti_squeezeDetPlus_config, None, "SqueezeDetPlus", "SqueezeDetTrainer"),
    "resnet50": (config.kitti_res50_config, config.kitti_res50_config_for_input, "ResNet50ConvDet", "ResNet50ConvDetTrainer"),
    "vgg16": (config.kitti_vgg16_config, config.kitti_vgg16_config_for_input, "VGG16ConvDet", "VGG16ConvDetTrainer"),
}


def model_class(net):
    from . import nets
    return getattr(nets, NET_TABLE[net][2])


def trainer_class(net):
    """(looked up here, not in the table: eval.py and demo.py never import squeezedet_amd.train)"""
    from . import train
    return getattr(train, NET_TABLE[net][3])


def torch_dtype(name):
    import torch
    return torch.float16 if name == "fp16" else torch.float32


def base_config(net, image_size=None, dataset="KITTI"):
    """The config of --net at --image_size (None: the net's own size), its head not padded: the classes are the real ones."""
    default, sized = NET_TABLE[net][:2]
    if dataset == "PASCAL_VOC":
        h, w = image_size if image_size is not None else VOC_IMAGE_SIZE
        return config.voc_squeezeDet_config_for_input(int(h), int(w))
    if image_size is None:
        return default()
    if sized is None:
        raise SystemExit("--image_size: no sized config for --net %s (squeezeDet, resnet50 and vgg16 have one)" % net)
    return sized(int(image_size[0]), int(image_size[1]))


def make_config(net, image_size=None, dataset="KITTI", anchor_shapes=None):
    """The config a driver runs: anchor_shapes ([k,2], None: the config's own) go in before the head is padded, because the
    padding depends on their count (PASCAL_VOC: 20 classes -> a head of 23, 3 of them padding)."""
    mc = base_config(net, image_size, dataset)
    if anchor_shapes is not None:
        mc = config.with_anchor_shapes(mc, anchor_shapes)
    return config.pad_head_classes(mc) if dataset == "PASCAL_VOC" else mc


def build_model(mc, net, gpu, dtype, batch_size=0):
    """The nets class of --net on mc; its parameters are loaded by the caller."""
    if batch_size:
        mc.BATCH_SIZE = int(batch_size)
    mc.LOAD_PRETRAINED_MODEL = False
    return model_class(net)(mc, gpu, dtype=torch_dtype(dtype))


def read_bgr(path):
    """uint8 BGR [H, W, 3], what cv2.imread returns."""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])


def load_index(dataset, data_path, year, image_set, mc):
    """The image paths, rois and ground truth of the set: what voc.load_voc / kitti_ap.load_kitti return."""
    if dataset == "PASCAL_VOC":
        from .voc import load_voc
        return load_voc(data_path, year, image_set, mc)
    from .kitti_ap import load_kitti
    return load_kitti(data_path, image_set, mc)


def synthetic_data(mc, n, seed):
    """--synthetic N --seed S: (images, rois), the same for every driver."""
    from .synthetic import synthetic_dataset
    return synthetic_dataset(mc, int(n), seed=300 + seed)


def driver_anchor_shapes(flag_path, checkpoint_path):
    """[k,2] from --anchor_shapes, else from an anchor_shapes.json beside the checkpoint, else None (the config's shapes)."""
    from . import anchors
    path = flag_path or (checkpoint_path and anchors.beside_checkpoint(checkpoint_path))
    if not path:
        return None
    print("Anchor shapes from {}".format(path))
    return anchors.load_for_driver(path)


def add_dataset_args(ap, image_set_default):
    ap.add_argument("--dataset", default="KITTI", help="KITTI or PASCAL_VOC")
    ap.add_argument("--year", default="2007", help="PASCAL_VOC: the VOC<year> directory under --data_path; before 2010 the 11-point AP is reported")
    ap.add_argument("--data_path", default="", help="root directory of the KITTI data (PASCAL_VOC: the directory that holds VOC<year>)")
    ap.add_argument("--image_set", default=image_set_default, help="ImageSets/<image_set>.txt (PASCAL_VOC: ImageSets/Main/<image_set>.txt)")


def add_model_args(ap, dtype_default):
    """--net, --image_size, --gpu and, unless dtype_default is None, --dtype."""
    ap.add_argument("--net", default="squeezeDet", choices=NETS, help="neural net architecture")
    ap.add_argument("--image_size", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="network input size (default: the net's; PASCAL_VOC: %d %d)" % VOC_IMAGE_SIZE)
    ap.add_argument("--gpu", default="0", help="gpu id")
    if dtype_default:
        ap.add_argument("--dtype", default=dtype_default, choices=["fp32", "fp16"], help="fp32: the reference's; fp16: half-precision storage")


def check_dataset_args(ap, a):
    assert a.dataset in DATASETS, "Currently only supports KITTI dataset (and PASCAL_VOC)"
    if a.dataset == "PASCAL_VOC" and a.net != "squeezeDet":
        ap.error("--dataset PASCAL_VOC: only --net squeezeDet has a VOC config")


BOX_LOSSES = ("delta_l2", "iou", "giou", "diou", "ciou")       # sqdet_loss_options_t.box_loss by index; the one list (ops imports it)


def add_loss_args(ap):
    """--bbox_loss, --focal_gamma, --bbox_loss_coef (train.py, tools/bench_train.py).  A flag that is not given leaves no
    attribute behind: loss_policy supplies the defaults."""
    import argparse
    ap.add_argument("--bbox_loss", default=argparse.SUPPRESS, choices=BOX_LOSSES,
                    help="the box term: delta_l2 (default), the reference's squared error on the four deltas; iou, giou, diou, ciou: "
                         "1 - that measure of the decoded box and the ground truth (DESIGN.md section 3.16)")
    ap.add_argument("--focal_gamma", type=float, default=argparse.SUPPRESS, metavar="G",
                    help="G > 0: the class term is weighted by (1 - p)^G on the labelled class and p^G on the others (default 0: the reference's)")
    ap.add_argument("--bbox_loss_coef", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="overrides the config's LOSS_COEF_BBOX (default: the config's)")


def check_loss_args(ap, a):
    g, x = float(getattr(a, "focal_gamma", 0.0)), float(getattr(a, "bbox_loss_coef", 0.0))
    if not (0.0 <= g < float("inf")):
        ap.error("--focal_gamma G needs a finite G >= 0")
    if not (0.0 <= x < float("inf")):
        ap.error("--bbox_loss_coef X needs a finite X >= 0")


def loss_policy(a, mc):
    """(the loss policy of --bbox_loss / --focal_gamma / --bbox_loss_coef as a checkpoint records it, the policy of a run without
    the flags -- what a checkpoint without the record was trained with); sets mc.BBOX_LOSS, mc.FOCAL_GAMMA and mc.LOSS_COEF_BBOX."""
    off = dict(bbox_loss="delta_l2", focal_gamma=0.0, bbox_loss_coef=float(mc.LOSS_COEF_BBOX))
    policy = dict(bbox_loss=str(getattr(a, "bbox_loss", off["bbox_loss"])), focal_gamma=float(getattr(a, "focal_gamma", off["focal_gamma"])),
                  bbox_loss_coef=float(getattr(a, "bbox_loss_coef", off["bbox_loss_coef"])))
    mc.BBOX_LOSS, mc.FOCAL_GAMMA, mc.LOSS_COEF_BBOX = policy["bbox_loss"], policy["focal_gamma"], policy["bbox_loss_coef"]
    return policy, off


def add_assign_args(ap):
    """--assign, --assign_iou, --assign_max, --assign_topk (train.py, tools/bench_train.py).  A flag that
    is not given leaves no attribute behind: assign_policy supplies the defaults."""
    import argparse
    from .assign import ASSIGN_MODES, MAX_PER_BOX, MAX_TOPK
    S = argparse.SUPPRESS
    ap.add_argument("--assign", default=S, choices=ASSIGN_MODES,
                    help="which anchors are trained as positives: reference (default), the one anchor per object the reference picks; "
                         "iou: also every unclaimed anchor with IoU >= --assign_iou, at most --assign_max per object; atss: also the "
                         "anchors ATSS selects (mean + std of the IoUs of the --assign_topk nearest anchors per shape)")
    ap.add_argument("--assign_iou", type=float, default=S, metavar="T", help="--assign iou: the IoU threshold (default 0.5)")
    ap.add_argument("--assign_max", type=int, default=S, metavar="K", help="--assign iou: at most K more positives per object, 1..%d (default 16)" % MAX_PER_BOX)
    ap.add_argument("--assign_topk", type=int, default=S, metavar="K", help="--assign atss: candidates per anchor shape, 1..%d (default 9)" % MAX_TOPK)


add_assign_flags = add_assign_args


def check_assign_args(ap, a):
    from ._lib import SqdetError
    from .assign import assign_options
    mode = getattr(a, "assign", "reference")
    for key, needs in (("assign_iou", "iou"), ("assign_max", "iou"), ("assign_topk", "atss")):
        if hasattr(a, key) and mode != needs:
            ap.error("--%s needs --assign %s" % (key, needs))
    try:
        assign_options(mode, getattr(a, "assign_iou", 0.5), getattr(a, "assign_max", 16), getattr(a, "assign_topk", 9))
    except SqdetError as e:
        ap.error(str(e))


def assign_policy(a, mc=None):
    """(the assignment policy of --assign ... as a checkpoint records it, the policy of a run without the flags -- what a
    checkpoint without the record was trained with).  assign.from_dict(policy) is the record the trainers take."""
    from .assign import as_dict, assign_options
    off = dict(mode="reference")
    opt = assign_options(getattr(a, "assign", "reference"), getattr(a, "assign_iou", 0.5), getattr(a, "assign_max", 16), getattr(a, "assign_topk", 9))
    return as_dict(opt), off


def add_distill_args(ap):
    """--teacher_net ... --distill_conf_floor (train.py, tools/bench_train.py).  A flag that is not given
    leaves no attribute behind: distill_policy supplies the defaults, and without --teacher_net there is no policy at all."""
    import argparse
    S = argparse.SUPPRESS
    ap.add_argument("--teacher_net", default=S, choices=NETS,
                    help="train towards this net's ConvDet output as well as the labels: a second, inference-only model on the same "
                         "device, whose grid, anchors and classes must be the student's (default: no teacher)")
    ap.add_argument("--teacher_checkpoint", default=S, metavar="PATH",
                    help="the teacher's variables: an .npz, or a train dir, whose newest checkpoint is used (synthetic data without "
                         "it: seeded synthetic variables, seed + 1)")
    ap.add_argument("--teacher_dtype", default=S, choices=["fp32", "fp16"], help="the teacher's storage dtype (default: the run's)")
    ap.add_argument("--distill_temperature", type=float, default=S, metavar="T", help="softens both class distributions, T > 0 (default 1)")
    ap.add_argument("--distill_class_coef", type=float, default=S, metavar="X", help="weight of the class term, the tempered KL (default 1)")
    ap.add_argument("--distill_conf_coef", type=float, default=S, metavar="X", help="weight of the confidence term, a Bernoulli KL (default 1)")
    ap.add_argument("--distill_bbox_coef", type=float, default=S, metavar="X", help="weight of the box term, squared error on the deltas (default 1)")
    ap.add_argument("--distill_conf_floor", type=float, default=S, metavar="F",
                    help="anchors whose teacher confidence is below F take no part in the class and box terms, 0 <= F <= 1 (default 0)")


DISTILL_FLAGS = ("teacher_checkpoint", "teacher_dtype", "distill_temperature", "distill_class_coef", "distill_conf_coef",
                 "distill_bbox_coef", "distill_conf_floor")


def _distill_options_of(a):
    from .distill import distill_options
    return distill_options(getattr(a, "distill_temperature", 1.0), getattr(a, "distill_class_coef", 1.0), getattr(a, "distill_conf_coef", 1.0),
                           getattr(a, "distill_bbox_coef", 1.0), getattr(a, "distill_conf_floor", 0.0))


def check_distill_args(ap, a):
    from ._lib import SqdetError
    if not hasattr(a, "teacher_net"):
        for key in DISTILL_FLAGS:
            if hasattr(a, key):
                ap.error("--%s needs --teacher_net" % key)
        return
    if not getattr(a, "teacher_checkpoint", "") and not getattr(a, "synthetic", 1):      # (tools/bench_train.py is always synthetic)
        ap.error("--teacher_net needs --teacher_checkpoint (only --synthetic runs may draw the teacher's variables)")
    try:
        _distill_options_of(a)
    except SqdetError as e:
        ap.error(str(e))


def distill_policy(a, mc=None):
    """(the distillation policy of --teacher_net ... as a checkpoint records it under `distill` -- the teacher net, its dtype,
    the five options and the teacher checkpoint's path, as a string only -- or None without --teacher_net; None: what a checkpoint
    without the record was trained with).  Sets mc.DISTILL when mc is given."""
    from .distill import as_dict
    policy = None
    if hasattr(a, "teacher_net"):
        policy = dict(teacher_net=str(a.teacher_net), teacher_checkpoint=str(getattr(a, "teacher_checkpoint", "")),
                      teacher_dtype=str(getattr(a, "teacher_dtype", getattr(a, "dtype", "fp32"))), **as_dict(_distill_options_of(a)))
    if mc is not None:
        mc.DISTILL = policy
    return policy, None


def teacher_checkpoint_file(path):
    """--teacher_checkpoint: the .npz itself, or the newest model.ckpt-<step>.npz of a train dir."""
    import glob
    import os
    from . import checkpoint
    if os.path.isdir(path):
        found = sorted(checkpoint._steps(glob.glob(os.path.join(path, "model.ckpt-*.npz"))))
        if not found:
            raise SystemExit("--teacher_checkpoint: no model.ckpt-<step>.npz in %s" % path)
        return os.path.join(path, checkpoint.MODEL_FMT % found[-1])
    if not os.path.isfile(path):
        raise SystemExit("--teacher_checkpoint: %s is neither a file nor a directory" % path)
    return path


def make_teacher(policy, mc, gpu, seed=0):
    """The distill.Teacher of a policy beside a student on mc, or None without one.  Its variables: the checkpoint's, or --
    no path recorded -- synthetic ones of seed + 1 (the student's are of `seed`)."""
    from . import distill, weights
    if distill.is_default(policy):
        return None
    params = None
    if policy["teacher_checkpoint"]:
        path = teacher_checkpoint_file(policy["teacher_checkpoint"])
        print("Teacher {} from {}".format(policy["teacher_net"], path))
        params = weights.load_params(path)
    return distill.Teacher(policy["teacher_net"], mc, gpu=gpu, dtype=policy["teacher_dtype"], params=params, seed=int(seed) + 1,
                           options=distill.from_dict(policy))


def add_optim_args(ap):
    """The update step's flags (train.py, tools/bench_train.py).  A flag that is not given leaves no
    attribute behind: optim.optim_policy supplies the defaults."""
    import argparse
    from .optim import CLIP_MODES, RULES, SCHEDULES
    S = argparse.SUPPRESS
    ap.add_argument("--optimizer", default=S, choices=RULES,
                    help="momentum (default): the reference's MomentumOptimizer; nesterov: with the look-ahead; adamw: Adam with bias "
                         "correction and decoupled weight decay")
    ap.add_argument("--adam_beta1", type=float, default=S, metavar="B", help="adamw: decay of the first moment (default 0.9)")
    ap.add_argument("--adam_beta2", type=float, default=S, metavar="B", help="adamw: decay of the second moment (default 0.999)")
    ap.add_argument("--adam_eps", type=float, default=S, metavar="E", help="adamw: added to the root of the second moment (default 1e-8)")
    ap.add_argument("--weight_decay", type=float, default=S, metavar="X", help="overrides the config's WEIGHT_DECAY (kernels only)")
    ap.add_argument("--clip_norm", default=S, choices=CLIP_MODES,
                    help="per_variable (default): tf.clip_by_norm on every variable; global: tf.clip_by_global_norm over all of them")
    ap.add_argument("--lr", type=float, default=S, metavar="X", help="the base learning rate (default: the config's LEARNING_RATE)")
    ap.add_argument("--lr_schedule", default=S, choices=SCHEDULES,
                    help="staircase (default): the reference's LR_DECAY_FACTOR every DECAY_STEPS; constant; cosine, linear: from the base "
                         "rate down to base * --min_lr_ratio over --lr_total_steps")
    ap.add_argument("--warmup_steps", type=int, default=S, metavar="N",
                    help="the first N updates run at --warmup_factor .. 1 times the schedule, linearly (default 0)")
    ap.add_argument("--warmup_factor", type=float, default=S, metavar="F", help="the multiplier of update 0 under --warmup_steps (default 0.001)")
    ap.add_argument("--min_lr_ratio", type=float, default=S, metavar="R", help="cosine, linear: the final rate over the base rate (default 0)")
    ap.add_argument("--lr_total_steps", type=int, default=S, metavar="T", help="cosine, linear: the update at which the final rate is reached (default --max_steps)")
    ap.add_argument("--ema_decay", type=float, default=S, metavar="D",
                    help="D > 0: keep an exponential moving average of the trainable variables, e += (1 - D) * (w - e) after every update; "
                         "checkpoints add ema/model.ckpt-<step>.npz, which eval.py --ema reads (default 0: none)")
    ap.add_argument("--ema_warmup", action="store_true", default=S, help="--ema_decay: use min(D, (1 + t) / (10 + t)) at update t")


def check_optim_args(ap, a):
    import math
    given = lambda key: hasattr(a, key)
    rule, sched = getattr(a, "optimizer", "momentum"), getattr(a, "lr_schedule", "staircase")
    for key in ("adam_beta1", "adam_beta2", "adam_eps"):
        if given(key) and rule != "adamw":
            ap.error("--%s needs --optimizer adamw" % key)
    for key in ("min_lr_ratio", "lr_total_steps"):
        if given(key) and sched not in ("cosine", "linear"):
            ap.error("--%s needs --lr_schedule cosine or linear" % key)
    fin = lambda key, default: float(getattr(a, key, default)) if math.isfinite(float(getattr(a, key, default))) else float("nan")
    for key in ("adam_beta1", "adam_beta2"):
        if not (0.0 <= fin(key, 0.9) < 1.0):
            ap.error("--%s B needs 0 <= B < 1" % key)
    if not (fin("adam_eps", 1e-8) > 0.0):
        ap.error("--adam_eps E needs a finite E > 0")
    if not (fin("weight_decay", 0.0) >= 0.0):
        ap.error("--weight_decay X needs a finite X >= 0")
    if not (fin("lr", 1.0) > 0.0):
        ap.error("--lr X needs a finite X > 0")
    if getattr(a, "warmup_steps", 0) < 0:
        ap.error("--warmup_steps N needs N >= 0")
    if not (0.0 <= fin("warmup_factor", 0.001) <= 1.0):
        ap.error("--warmup_factor F needs 0 <= F <= 1")
    if not (0.0 <= fin("min_lr_ratio", 0.0) <= 1.0):
        ap.error("--min_lr_ratio R needs 0 <= R <= 1")
    if getattr(a, "lr_total_steps", 1) < 1:
        ap.error("--lr_total_steps T needs T >= 1")
    if not (0.0 <= fin("ema_decay", 0.0) < 1.0):
        ap.error("--ema_decay D needs 0 <= D < 1")
    if getattr(a, "ema_warmup", False) and not fin("ema_decay", 0.0) > 0.0:
        ap.error("--ema_warmup needs --ema_decay D with D > 0")


def add_nms_args(ap):
    """--nms, --nms_overlap, --nms_sigma, --nms_score_floor, --nms_class_agnostic (eval.py, demo.py).  A flag that is not given
    leaves no attribute behind: nms_policy supplies the defaults."""
    import argparse
    from .nms import NMS_METHODS, NMS_OVERLAPS
    ap.add_argument("--nms", default=argparse.SUPPRESS, choices=NMS_METHODS,
                    help="the suppression rule over the top-N rows: reference (default), a row is dropped when ANY higher-scored row of its "
                         "class overlaps it; greedy, only a kept row suppresses; soft_linear, soft_gaussian: Soft-NMS, overlapped rows "
                         "lose score instead (DESIGN.md section 3.17)")
    ap.add_argument("--nms_overlap", default=argparse.SUPPRESS, choices=NMS_OVERLAPS,
                    help="what the config's NMS_THRESH is compared with: iou (default), or diou = IoU minus the squared centre distance "
                         "over the squared enclosing diagonal (reference and greedy only)")
    ap.add_argument("--nms_sigma", type=float, default=argparse.SUPPRESS, metavar="S", help="soft_gaussian: scores decay by exp(-iou^2 / S) (default 0.5)")
    ap.add_argument("--nms_score_floor", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="soft methods: rows whose decayed score falls below X are dropped (default 0.001)")
    ap.add_argument("--nms_class_agnostic", action="store_true", default=argparse.SUPPRESS, help="rows of different classes suppress each other too")


def check_nms_args(ap, a):
    soft = str(getattr(a, "nms", "reference")).startswith("soft")
    if getattr(a, "nms_overlap", "iou") == "diou" and soft:
        ap.error("--nms_overlap diou goes with --nms reference or greedy, not with a soft method")
    if not (0.0 < float(getattr(a, "nms_sigma", 0.5)) < float("inf")):
        ap.error("--nms_sigma S needs a finite S > 0")
    if not (abs(float(getattr(a, "nms_score_floor", 0.0))) < float("inf")):
        ap.error("--nms_score_floor X needs a finite X")
    if hasattr(a, "nms_sigma") and getattr(a, "nms", "reference") != "soft_gaussian":
        ap.error("--nms_sigma needs --nms soft_gaussian")
    if hasattr(a, "nms_score_floor") and not soft:
        ap.error("--nms_score_floor needs --nms soft_linear or soft_gaussian")


def nms_policy(a, mc):
    """The suppression policy of the --nms flags as a dict (what eval.py prints and records); sets mc.NMS_METHOD, mc.NMS_OVERLAP,
    mc.NMS_SIGMA, mc.NMS_SCORE_FLOOR and mc.NMS_CLASS_AGNOSTIC, which every filtering call site reads through nms.nms_options."""
    from . import nms
    d = nms.DEFAULTS
    mc.NMS_METHOD = str(getattr(a, "nms", d["NMS_METHOD"]))
    mc.NMS_OVERLAP = str(getattr(a, "nms_overlap", d["NMS_OVERLAP"]))
    mc.NMS_SIGMA = float(getattr(a, "nms_sigma", d["NMS_SIGMA"]))
    mc.NMS_SCORE_FLOOR = float(getattr(a, "nms_score_floor", d["NMS_SCORE_FLOOR"]))
    mc.NMS_CLASS_AGNOSTIC = bool(getattr(a, "nms_class_agnostic", d["NMS_CLASS_AGNOSTIC"]))
    opt = nms.nms_options(mc)
    if not nms.is_default(opt) and not (0 < int(mc.TOP_N_DETECTION) <= nms.MAX_ROWS):
        raise SystemExit("--nms / --nms_overlap / --nms_class_agnostic work on the top-N rows: the config needs 0 < TOP_N_DETECTION <= %d, "
                         "it has %d" % (nms.MAX_ROWS, int(mc.TOP_N_DETECTION)))
    return config_nms_policy(mc)


def config_nms_policy(mc):
    """The suppression policy a config holds, as a dict: what the model built on it filters with."""
    from . import nms
    opt = nms.nms_options(mc)
    return dict(opt._asdict(), nms_thresh=float(mc.NMS_THRESH), default=nms.is_default(opt))


def format_nms_policy(policy):
    return "{method}, {overlap} > {nms_thresh:g}, {scope}{soft}".format(
        scope="class-agnostic" if policy["class_agnostic"] else "per class",
        soft=(", sigma {sigma:g}".format(**policy) if policy["method"] == "soft_gaussian" else "")
        + (", score floor {score_floor:g}".format(**policy) if policy["method"].startswith("soft") else ""), **policy)
