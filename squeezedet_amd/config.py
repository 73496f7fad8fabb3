"""`mc` model configurations with the reference's field names (reference
src/config/config.py:10-142, src/config/kitti_*_config.py).  `mc.ANCHOR_BOX` is built
with the closed form  ANCHOR_BOX[(h*W+w)*B+k] = [(w+1)*IMG_W/(W+1), (h+1)*IMG_H/(H+1), aw_k, ah_k]
(float64), which is bit-identical to the reference's reshape/transpose construction
(kitti_squeezeDet_config.py:45-79; checked in tests against vectors produced by the reference).
"""
import numpy as np


class EasyDict(dict):
    """Attribute-access dict (what easydict.EasyDict gives the reference)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


edict = EasyDict


def base_model_config(dataset="PASCAL_VOC"):
    """config/config.py:10-142."""
    assert dataset.upper() == "PASCAL_VOC" or dataset.upper() == "KITTI", \
        "Currently only support PASCAL_VOC or KITTI dataset"
    cfg = edict()
    cfg.DATASET = dataset.upper()
    if cfg.DATASET == "PASCAL_VOC":
        cfg.CLASS_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
                           "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa",
                           "train", "tvmonitor")
    elif cfg.DATASET == "KITTI":
        cfg.CLASS_NAMES = ("car", "pedestrian", "cyclist")
    cfg.CLASSES = len(cfg.CLASS_NAMES)
    cfg.GRID_POOL_WIDTH = 7
    cfg.GRID_POOL_HEIGHT = 7
    cfg.LEAKY_COEF = 0.1
    cfg.KEEP_PROB = 0.5
    cfg.IMAGE_WIDTH = 224
    cfg.IMAGE_HEIGHT = 224
    cfg.ANCHOR_BOX = []
    cfg.ANCHORS = len(cfg.ANCHOR_BOX)
    cfg.ANCHOR_PER_GRID = -1
    cfg.BATCH_SIZE = 20
    cfg.PROB_THRESH = 0.005
    cfg.PLOT_PROB_THRESH = 0.5
    cfg.NMS_THRESH = 0.2
    cfg.BGR_MEANS = np.array([[[103.939, 116.779, 123.68]]])
    cfg.LOSS_COEF_CONF = 1.0
    cfg.LOSS_COEF_CLASS = 1.0
    cfg.LOSS_COEF_BBOX = 10.0
    # OURS (the reference has neither): what the box term is, and the class term's focal exponent
    cfg.BBOX_LOSS = "delta_l2"                  # "delta_l2": the reference's squared delta error; "iou", "giou", "diou", "ciou"
    cfg.FOCAL_GAMMA = 0.0                       # 0.0: the reference's unweighted log loss
    # OURS: the distillation policy of a run trained towards a teacher net's output (drivers.distill_policy's
    # record: the teacher net, its checkpoint's path, the options of squeezedet_amd.distill); None: no teacher
    cfg.DISTILL = None
    cfg.DECAY_STEPS = 10000
    cfg.LR_DECAY_FACTOR = 0.1
    cfg.LEARNING_RATE = 0.005
    cfg.MOMENTUM = 0.9
    cfg.WEIGHT_DECAY = 0.0005
    cfg.LOAD_PRETRAINED_MODEL = True
    cfg.PRETRAINED_MODEL_PATH = ""
    cfg.DEBUG_MODE = False
    cfg.EPSILON = 1e-16
    cfg.EXP_THRESH = 1.0
    cfg.MAX_GRAD_NORM = 10.0
    cfg.DATA_AUGMENTATION = False
    cfg.DRIFT_X = 0
    cfg.DRIFT_Y = 0
    # BatchReader's augmentation beyond the reference's drift / flip (imdb.py; all off by default)
    cfg.AUG_GEOMETRY = "drift"                  # "drift": the reference's; "ssd": zoom-out + IoU-constrained crop windows
    cfg.AUG_ZOOM_OUT_MAX = 1.0                  # "ssd": canvas ratio U[1, max] with probability 1/2 (1.0: never)
    cfg.AUG_CROP_MIN_SCALE = 0.3                # "ssd": a trial window's width and height, U[min, 1] of the canvas
    cfg.AUG_CROP_ASPECT = (0.5, 2.0)            # "ssd": the aspect ratio a trial window must keep
    cfg.AUG_CROP_TRIALS = 50
    cfg.AUG_COLOR = False
    cfg.AUG_BRIGHTNESS = 32.0                   # offset U[-b, b]
    cfg.AUG_CONTRAST = (0.5, 1.5)               # gain
    cfg.AUG_SATURATION = (0.5, 1.5)             # about the BT.601 luma
    cfg.AUG_HUE_DEGREES = 18.0                  # rotation U[-h, h] in YIQ
    cfg.AUG_MOSAIC_PROB = 0.0                   # probability that a batch image is a mosaic of four dataset images (0.0: never)
    cfg.AUG_MOSAIC_CENTER = (0.3, 0.7)          # the split (xc, yc), U[range] of the input's width and height
    cfg.AUG_MOSAIC_ZOOM_MAX = 1.5               # per part an extra zoom U[1, max] beyond the one that fills its pane
    cfg.AUG_MOSAIC_MIN_BOX = 2.0                # a box narrower or lower than this, in network-input pixels, is dropped
    cfg.EXCLUDE_HARD_EXAMPLES = True
    cfg.BATCH_NORM_EPSILON = 1e-5
    cfg.NUM_THREAD = 4
    cfg.QUEUE_CAPACITY = 100
    cfg.IS_TRAINING = False
    return cfg


SQUEEZEDET_ANCHOR_SHAPES = np.array([[36., 37.], [366., 174.], [115., 59.], [162., 87.], [38., 90.],
                                     [258., 173.], [224., 108.], [78., 170.], [72., 43.]])
RES50_ANCHOR_SHAPES = np.array([[94., 49.], [225., 161.], [170., 91.], [390., 181.], [41., 32.],
                                [128., 64.], [298., 164.], [232., 99.], [65., 42.]])


def set_anchors(mc, H=24, W=78, anchor_shapes=SQUEEZEDET_ANCHOR_SHAPES):
    """kitti_squeezeDet_config.py:45-79 in closed form; returns float64 [H*W*B, 4]."""
    B = len(anchor_shapes)
    cx = np.arange(1, W + 1) * float(mc.IMAGE_WIDTH) / (W + 1)
    cy = np.arange(1, H + 1) * float(mc.IMAGE_HEIGHT) / (H + 1)
    out = np.empty((H, W, B, 4), np.float64)
    out[..., 0] = cx[None, :, None]
    out[..., 1] = cy[:, None, None]
    out[..., 2:] = np.asarray(anchor_shapes, np.float64)[None, None, :, :]
    return out.reshape(-1, 4)


def _kitti_common(mc):
    mc.BATCH_SIZE = 20
    mc.WEIGHT_DECAY = 0.0001
    mc.LEARNING_RATE = 0.01
    mc.DECAY_STEPS = 10000
    mc.MAX_GRAD_NORM = 1.0
    mc.MOMENTUM = 0.9
    mc.LR_DECAY_FACTOR = 0.5
    mc.LOSS_COEF_BBOX = 5.0
    mc.LOSS_COEF_CONF_POS = 75.0
    mc.LOSS_COEF_CONF_NEG = 100.0
    mc.LOSS_COEF_CLASS = 1.0
    mc.PLOT_PROB_THRESH = 0.4
    mc.NMS_THRESH = 0.4
    mc.PROB_THRESH = 0.005
    mc.TOP_N_DETECTION = 64
    mc.DATA_AUGMENTATION = True
    mc.DRIFT_X = 150
    mc.DRIFT_Y = 100
    mc.EXCLUDE_HARD_EXAMPLES = False
    return mc


def _finish(mc, H, W, shapes):
    mc.ANCHOR_BOX = set_anchors(mc, H, W, shapes)
    mc.ANCHORS = len(mc.ANCHOR_BOX)
    mc.ANCHOR_PER_GRID = 9
    return mc


def kitti_squeezeDet_config():
    """config/kitti_squeezeDet_config.py:9-43 (network input 1248x384)."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = 1248, 384
    return _finish(_kitti_common(mc), 24, 78, SQUEEZEDET_ANCHOR_SHAPES)


def kitti_squeezeDetPlus_config():
    """config/kitti_squeezeDetPlus_config.py:9-43 (1242x375, 22x76 grid)."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = 1242, 375
    return _finish(_kitti_common(mc), 22, 76, SQUEEZEDET_ANCHOR_SHAPES)


def kitti_res50_config():
    """config/kitti_res50_config.py:9-43."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = 1242, 375
    return _finish(_kitti_common(mc), 24, 78, RES50_ANCHOR_SHAPES)


def kitti_vgg16_config():
    """config/kitti_vgg16_config.py:9-43."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = 1242, 375
    _kitti_common(mc)
    mc.BATCH_SIZE = 5
    return _finish(mc, 24, 78, SQUEEZEDET_ANCHOR_SHAPES)


def kitti_squeezeDet_config_for_input(image_height, image_width):
    """SqueezeDet on another input size (BASELINE.json quotes the metric on 1242x375): the
    grid is what conv1/s2 + three SAME 3x3/s2 pools give, anchors follow the same formula."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = int(image_width), int(image_height)
    gh, gw = int(image_height), int(image_width)
    for _ in range(4):
        gh, gw = -(-gh // 2), -(-gw // 2)
    return _finish(_kitti_common(mc), gh, gw, SQUEEZEDET_ANCHOR_SHAPES)


def kitti_res50_config_for_input(image_height, image_width):
    """ResNet50+ConvDet on another input size: the grid is what conv1 7x7/s2 SAME, pool1 3x3/s2 VALID
    and the stride-2 res3a / res4a blocks give (nets/resnet50_convDet.py:41-99); 375x1242 -> 24x78."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = int(image_width), int(image_height)
    g = []
    for n in (int(image_height), int(image_width)):
        n = -(-n // 2)            # conv1
        n = (n - 3) // 2 + 1      # pool1 VALID
        n = -(-n // 2)            # res3a
        n = -(-n // 2)            # res4a
        g.append(n)
    return _finish(_kitti_common(mc), g[0], g[1], RES50_ANCHOR_SHAPES)


def kitti_vgg16_config_for_input(image_height, image_width):
    """VGG16+ConvDet on another input size: the grid is what the four 2x2/s2 SAME pools give (nets/vgg16_convDet.py:44-78, every
    conv 3x3/s1/SAME); 375x1242 -> 24x78, the grid of kitti_vgg16_config."""
    mc = base_model_config("KITTI")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = int(image_width), int(image_height)
    _kitti_common(mc)
    mc.BATCH_SIZE = 5
    gh, gw = int(image_height), int(image_width)
    for _ in range(4):
        gh, gw = -(-gh // 2), -(-gw // 2)
    return _finish(mc, gh, gw, SQUEEZEDET_ANCHOR_SHAPES)


def voc_squeezeDet_config_for_input(image_height, image_width):
    """SqueezeDet on Pascal VOC's 20 classes at a given input size.  OURS: the reference ships no VOC net config
    (config/ has KITTI ones only); this is base_model_config("PASCAL_VOC") with the hyperparameters, the grid and the
    anchor construction of kitti_squeezeDet_config_for_input, so that eval.py and train.py can run on VOC XML datasets.
    The anchor shapes are KITTI's, not tuned for VOC.
    A net for it is built on pad_head_classes(mc): 9 * (20 + 5) = 225 ConvDet channels are not a multiple of 4."""
    mc = base_model_config("PASCAL_VOC")
    mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT = int(image_width), int(image_height)
    gh, gw = int(image_height), int(image_width)
    for _ in range(4):
        gh, gw = -(-gh // 2), -(-gw // 2)
    return _finish(_kitti_common(mc), gh, gw, SQUEEZEDET_ANCHOR_SHAPES)


def anchor_grid(mc):
    """(H, W) of the grid mc.ANCHOR_BOX was built on, read back from its centres (set_anchors' closed form)."""
    ab = np.asarray(mc.ANCHOR_BOX, np.float64).reshape(-1, int(mc.ANCHOR_PER_GRID), 4)
    W = len(np.unique(ab[:, 0, 0]))
    H = len(np.unique(ab[:, 0, 1]))
    if H * W != len(ab):
        raise ValueError("anchor_grid: mc.ANCHOR_BOX is not a grid of %d anchors per cell" % int(mc.ANCHOR_PER_GRID))
    return H, W


def check_anchor_shapes(shapes):
    """float64 [k,2] of finite, strictly positive (w, h); ValueError otherwise."""
    a = np.array(shapes, np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or len(a) < 1:
        raise ValueError("anchor shapes must be [k,2] (w, h) with k >= 1, got an array of shape %s" % (a.shape,))
    if not np.isfinite(a).all() or not (a > 0).all():
        raise ValueError("anchor shapes must be finite and strictly positive, got %s" % a.tolist())
    return a


def with_anchor_shapes(mc, shapes):
    """A copy of mc whose ANCHOR_BOX, ANCHORS and ANCHOR_PER_GRID are rebuilt for `shapes` ([k,2] of (w, h) in network-input
    pixels, e.g. anchors.fit_anchor_shapes' result) on mc's own grid through set_anchors:
    ANCHOR_BOX[(h*W+w)*k+j] = [(w+1)*IMG_W/(W+1), (h+1)*IMG_H/(H+1), shapes[j,0], shapes[j,1]].  OURS: the reference's shapes are
    literals in its configs.  Apply it BEFORE pad_head_classes, which depends on ANCHOR_PER_GRID; a config that is already
    padded is refused."""
    if int(mc.get("HEAD_PAD_CLASSES", 0)):
        raise ValueError("with_anchor_shapes: apply it before pad_head_classes (the padding depends on ANCHOR_PER_GRID)")
    shapes = check_anchor_shapes(shapes)
    H, W = anchor_grid(mc)
    mc = type(mc)(mc)
    mc.ANCHOR_BOX = set_anchors(mc, H, W, shapes)
    mc.ANCHORS = len(mc.ANCHOR_BOX)
    mc.ANCHOR_PER_GRID = len(shapes)
    return mc


def anchor_shapes_of(mc):
    """The [ANCHOR_PER_GRID, 2] shapes mc.ANCHOR_BOX carries (its first cell's)."""
    return np.array(np.asarray(mc.ANCHOR_BOX, np.float64)[:int(mc.ANCHOR_PER_GRID), 2:4])


PAD_CLASS_BIAS = -1.0e4      # the ConvDet bias of a padding class: exp(-1e4 - max) is exactly 0 in float32 and float16


def pad_head_classes(mc):
    """The config a net is BUILT with when ANCHOR_PER_GRID * (CLASSES + 5) is not a multiple of 4 (the conv kernels store
    output channels four at a time): a copy of mc whose CLASSES is the next count that is -- 20 -> 23, a ConvDet layer of
    252 channels -- with HEAD_PAD_CLASSES = the classes added (0: nothing to do).  CLASS_NAMES keeps the real names: class
    indices >= len(CLASS_NAMES) are padding.  With pin_padding_classes on its parameters a padding class has probability
    exactly 0, so the net computes what the unpadded one would: softmax over the real classes, no detection of a padding
    class, and a zero gradient into the padding channels."""
    mc = type(mc)(mc)
    c = int(mc.CLASSES)
    while (mc.ANCHOR_PER_GRID * (c + 1 + 4)) % 4:
        c += 1
    mc.HEAD_PAD_CLASSES = c - int(mc.CLASSES)
    mc.CLASSES = c
    return mc


def pin_padding_classes(mc, params, layer="conv12"):
    """params ({name: array / tensor}) with the ConvDet layer's padding-class channels pinned: kernels 0, biases
    PAD_CLASS_BIAS.  The class logits are channels a * CLASSES + c (anchor a, class c; nn_skeleton.py:250-258); c >=
    len(CLASS_NAMES) is padding.  Returns params itself when mc has no padding."""
    pad = int(mc.get("HEAD_PAD_CLASSES", 0))
    if not pad:
        return params
    C, real = int(mc.CLASSES), int(mc.CLASSES) - pad
    ch = np.array([a * C + c for a in range(int(mc.ANCHOR_PER_GRID)) for c in range(real, C)])
    out = dict(params)
    host = lambda v: np.array(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)
    k, b = host(out[layer + "/kernels"]), host(out[layer + "/biases"])
    k[..., ch] = 0.0
    b[ch] = PAD_CLASS_BIAS
    out[layer + "/kernels"], out[layer + "/biases"] = k, b
    return out
