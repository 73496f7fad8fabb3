"""The suppression policy of a config (OURS): which rule thins the top-N rows, read in ONE place by every
call site that filters for a model (ModelSkeleton.filter_prediction_batch, the serving step, viz.ImageSummary).

The default -- the reference's non-greedy NMS on the IoU, per class -- is the filter kernels' own rule: nothing here launches
anything then, and the filter is called with mc.NMS_THRESH as ever.  Any other policy runs as a second, small launch
(sqdet_suppress_rows) over the rows of a filter that was called with a threshold of +inf, which suppresses nothing.
Importing this needs neither torch nor a GPU (drivers.py and the host tests use it); apply() imports ops when called."""
from collections import namedtuple

from ._lib import SqdetError

NMS_METHODS = ("reference", "greedy", "soft_linear", "soft_gaussian")
NMS_OVERLAPS = ("iou", "diou")                                          # sqdet_nms_options_t.overlap by index
KERNEL_METHODS = ("nongreedy", "greedy", "soft_linear", "soft_gaussian")  # sqdet_nms_options_t.method by index
MAX_ROWS = 64                                                           # sqdet_suppress_rows: one wave's lanes

DEFAULTS = dict(NMS_METHOD="reference", NMS_OVERLAP="iou", NMS_SIGMA=0.5, NMS_SCORE_FLOOR=0.001, NMS_CLASS_AGNOSTIC=False)

NmsOptions = namedtuple("NmsOptions", "method overlap sigma score_floor class_agnostic")
_DEFAULT = NmsOptions(DEFAULTS["NMS_METHOD"], DEFAULTS["NMS_OVERLAP"], DEFAULTS["NMS_SIGMA"], DEFAULTS["NMS_SCORE_FLOOR"], DEFAULTS["NMS_CLASS_AGNOSTIC"])
_FIELDS = frozenset(DEFAULTS)


def nms_options(mc):
    """The policy of a config; a config without the fields (the reference's) means the reference's rule.  Unknown names, diou
    with a soft method, a sigma that is not > 0 and a non-finite floor are refused here, before anything is launched."""
    if isinstance(mc, dict) and _FIELDS.isdisjoint(mc):      # (a config without the fields, read once per serving step: no work)
        return _DEFAULT

    def field(key):                   # (mc may be any attribute dict: one whose __getattr__ raises KeyError included)
        try:
            return mc[key] if isinstance(mc, dict) else getattr(mc, key)
        except (KeyError, AttributeError):
            return DEFAULTS[key]
    opt = NmsOptions(str(field("NMS_METHOD")), str(field("NMS_OVERLAP")), float(field("NMS_SIGMA")), float(field("NMS_SCORE_FLOOR")),
                     bool(field("NMS_CLASS_AGNOSTIC")))
    if opt.method not in NMS_METHODS:
        raise SqdetError("mc.NMS_METHOD %r is not one of %s" % (opt.method, ", ".join(NMS_METHODS)))
    if opt.overlap not in NMS_OVERLAPS:
        raise SqdetError("mc.NMS_OVERLAP %r is not one of %s" % (opt.overlap, ", ".join(NMS_OVERLAPS)))
    if opt.overlap == "diou" and opt.method.startswith("soft"):
        raise SqdetError("mc.NMS_OVERLAP diou goes with the hard methods only (reference, greedy), not %s" % opt.method)
    if not (0.0 < opt.sigma < float("inf")):
        raise SqdetError("mc.NMS_SIGMA must be a finite number > 0, got %r" % (opt.sigma,))
    if not (abs(opt.score_floor) < float("inf")):
        raise SqdetError("mc.NMS_SCORE_FLOOR must be finite, got %r" % (opt.score_floor,))
    return opt


def is_default(opt):
    """True only for the rule the filter kernels run themselves: reference + iou + per class."""
    return opt.method == "reference" and opt.overlap == "iou" and not opt.class_agnostic


def first_stage_thresh(opt, mc):
    """The nms_thresh the filter call gets: the config's, or +inf (no row suppresses another) ahead of a second stage."""
    return mc.NMS_THRESH if is_default(opt) else float("inf")


def kernel_method(opt):
    """sqdet_nms_options_t.method: `reference` with diou or class-agnostic is the second stage's nongreedy rule."""
    return "nongreedy" if opt.method == "reference" else opt.method


def apply(opt, mc, out):
    """The second stage, in place on a filter call's five outputs (on the current stream); `out` is returned."""
    from . import ops
    rows = int(out[1].shape[1])
    if rows > MAX_ROWS:
        raise SqdetError("NMS_METHOD %s / NMS_OVERLAP %s%s work on the top-N rows of an image, at most %d: the filter emitted %d per image "
                         "(TOP_N_DETECTION %s, %d anchors) -- set 0 < TOP_N_DETECTION <= %d"
                         % (opt.method, opt.overlap, " / class-agnostic" if opt.class_agnostic else "", MAX_ROWS, rows,
                            getattr(mc, "TOP_N_DETECTION", "?"), int(getattr(mc, "ANCHORS", 0)), MAX_ROWS))
    return ops.suppress_rows(out, mc.CLASSES, dict(method=kernel_method(opt), overlap=opt.overlap, class_agnostic=opt.class_agnostic,
                                                   nms_thresh=float(mc.NMS_THRESH), sigma=opt.sigma, score_floor=opt.score_floor))
