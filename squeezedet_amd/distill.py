"""Knowledge distillation (OURS): a teacher net's ConvDet output as a second target of the loss.

The student trains as ever; after the loss launch one more launch (sqdet_distill_fwd_bwd, squeezedet_amd/csrc/loss.hip) adds the
gradient of three terms -- a tempered KL on the class logits, a Bernoulli KL on the confidence logit, a squared error on the box
deltas, the first and the last weighted by the teacher's confidence -- onto dpreds.  The teacher is a second model of the run in
inference mode on the same device; it gets no gradient and its parameters never change.  The definition stands in
include/sqdet.h and, sequentially, in tests/distill_reference.py.
Importing this needs neither torch nor a GPU (drivers.py and the host tests use it); Teacher looks both up when it is built."""
import math
from collections import namedtuple

import numpy as np

from . import config
from ._lib import SqdetError

DistillOptions = namedtuple("DistillOptions", "temperature class_coef conf_coef bbox_coef conf_floor")       # sqdet_distill_options_t


def distill_options(temperature=1.0, class_coef=1.0, conf_coef=1.0, bbox_coef=1.0, conf_floor=0.0):
    """The validated record.  A temperature that is not a finite number > 0, a negative or non-finite coefficient, three zero
    coefficients and a floor outside [0, 1] are refused here, before anything is launched (the library refuses them too)."""
    opt = DistillOptions(float(temperature), float(class_coef), float(conf_coef), float(bbox_coef), float(conf_floor))
    if not (math.isfinite(opt.temperature) and opt.temperature > 0.0):
        raise SqdetError("distill temperature must be a finite number > 0, got %r" % (temperature,))
    for name in ("class_coef", "conf_coef", "bbox_coef"):
        v = getattr(opt, name)
        if not (math.isfinite(v) and v >= 0.0):
            raise SqdetError("distill %s must be a finite number >= 0, got %r" % (name, v))
    if opt.class_coef == 0.0 and opt.conf_coef == 0.0 and opt.bbox_coef == 0.0:
        raise SqdetError("distill: the three coefficients are all zero (nothing to distil: train without a teacher instead)")
    if not 0.0 <= opt.conf_floor <= 1.0:
        raise SqdetError("distill conf_floor must lie in [0, 1], got %r" % (conf_floor,))
    return opt


def is_default(policy):
    """True for a run without a teacher: None (config.DISTILL's default), or a record that names no teacher net."""
    return policy is None or not dict(policy).get("teacher_net")


def as_dict(opt):
    return dict(opt._asdict())


def from_dict(d):
    return distill_options(**{k: d[k] for k in DistillOptions._fields if k in d})


def _record(mc):
    """What check_compatible compares, as the error text carries it."""
    try:
        grid = list(config.anchor_grid(mc))
    except ValueError:
        grid = None
    return dict(image_size=[int(mc.IMAGE_HEIGHT), int(mc.IMAGE_WIDTH)], grid=grid, anchors_per_grid=int(mc.ANCHOR_PER_GRID),
                classes=int(mc.CLASSES), anchors=int(mc.ANCHORS), anchor_shapes=config.anchor_shapes_of(mc).tolist())


def check_compatible(student_mc, teacher_mc):
    """Refuses (SqdetError carrying both records) a teacher whose preds do not line up with the student's channel for channel and
    cell for cell: another grid, number of anchors per cell, class count or set of anchor boxes."""
    s, t = _record(student_mc), _record(teacher_mc)
    what = None
    if s["grid"] is None or s["grid"] != t["grid"]:
        what = "grid"
    elif s["anchors_per_grid"] != t["anchors_per_grid"]:
        what = "number of anchors per cell"
    elif s["classes"] != t["classes"]:
        what = "class count"
    elif not np.array_equal(np.asarray(student_mc.ANCHOR_BOX, np.float64), np.asarray(teacher_mc.ANCHOR_BOX, np.float64)):
        what = "anchor boxes"
    if what is not None:
        raise SqdetError("distill: the teacher's %s differs from the student's -- student %r, teacher %r" % (what, s, t))


def _native_grid(net, h, w):
    """The grid --net produces on an h x w input, from the layers of squeezedet_amd.nets."""
    if net == "squeezeDet+":              # conv1 7x7/s2 VALID, then three 3x3/s2 VALID pools (nets.SqueezeDetPlus)
        g = []
        for n in (int(h), int(w)):
            n = (n - 7) // 2 + 1
            for _ in range(3):
                n = (n - 3) // 2 + 1
            g.append(n)
        return tuple(g)
    sized = {"squeezeDet": config.kitti_squeezeDet_config_for_input, "resnet50": config.kitti_res50_config_for_input,
             "vgg16": config.kitti_vgg16_config_for_input}[net]
    return tuple(config.anchor_grid(sized(int(h), int(w))))


def teacher_config(net, student_mc, batch_size=None):
    """The config a teacher of `net` is built with beside a student on student_mc: the student's image size, class count and
    anchor shapes on the grid the TEACHER's layers produce at that size, inference mode.  check_compatible decides whether the
    two line up (at 1248 x 384 SqueezeDet, ResNet50+ConvDet and VGG16+ConvDet share the 24 x 78 grid; SqueezeDet+'s VALID
    convolution and pools give 22 x 76)."""
    if int(student_mc.get("HEAD_PAD_CLASSES", 0)):
        raise SqdetError("distill: a student with a padded ConvDet head (PASCAL_VOC) is not supported")
    h, w = int(student_mc.IMAGE_HEIGHT), int(student_mc.IMAGE_WIDTH)
    gh, gw = _native_grid(net, h, w)
    if gh < 1 or gw < 1:
        raise SqdetError("distill: --teacher_net %s has no output cell on a %d x %d input" % (net, h, w))
    mc = type(student_mc)(student_mc)
    mc.ANCHOR_BOX = config.set_anchors(mc, gh, gw, config.anchor_shapes_of(student_mc))
    mc.ANCHORS = len(mc.ANCHOR_BOX)
    mc.IS_TRAINING, mc.LOAD_PRETRAINED_MODEL, mc.PRETRAINED_MODEL_PATH = False, False, ""
    if batch_size:
        mc.BATCH_SIZE = int(batch_size)
    return mc


class Teacher:
    """A model of any of the four nets in inference mode (keep_prob 1: model.run([model.preds], ...) goes through the native plan)
    at the student's batch, image size, class count and anchors.  preds(images) is its ConvDet output for a batch -- no gradient,
    no state: the parameters are loaded once and never written."""

    def __init__(self, net, student_mc, gpu=0, dtype="fp32", params=None, seed=0, options=None):
        from . import drivers
        if net not in drivers.NETS:
            raise SqdetError("distill: teacher net %r is not one of %s" % (net, ", ".join(drivers.NETS)))
        self.net, self.options = net, options if options is not None else distill_options()
        self.mc = teacher_config(net, student_mc)
        check_compatible(student_mc, self.mc)
        import torch
        tdt = dtype if isinstance(dtype, torch.dtype) else drivers.torch_dtype(dtype)
        self.model = drivers.model_class(net)(self.mc, str(gpu), dtype=tdt)
        assert self.model.keep_prob == 1.0
        if params is None:
            from .synthetic import synthetic_params
            params = synthetic_params(self.model, seed=seed)
        self.model.load_params(params)
        self.dtype = self.model.dtype

    def preds(self, images):
        """[B,gh,gw,K*(C+5)] in the teacher's dtype for images [B,H,W,3] (device float32 / float16, or a host array)."""
        return self.model.run([self.model.preds], {self.model.image_input: images})[0]
