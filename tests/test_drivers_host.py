"""squeezedet_amd.drivers, the one module under train.py, eval.py, demo.py and tools/fit_anchors.py: its configs against the
config functions called by hand, its table, the four scripts' argument defaults and refusals, the image read, the seed rule.
No GPU."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import squeezedet_amd as S
from squeezedet_amd import config, drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES9 = np.array([[20.5, 31.], [44., 40.], [61., 120.25], [90., 70.], [130., 95.], [150., 210.], [240., 130.], [300., 260.], [410., 300.]])
DIRECT = {"squeezeDet": (S.kitti_squeezeDet_config, S.kitti_squeezeDet_config_for_input), "squeezeDet+": (S.kitti_squeezeDetPlus_config, None),
          "resnet50": (S.kitti_res50_config, S.kitti_res50_config_for_input), "vgg16": (S.kitti_vgg16_config, S.kitti_vgg16_config_for_input)}


def _load(path):
    spec = importlib.util.spec_from_file_location("_drivers_host_" + os.path.basename(path)[:-3], os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scripts():
    return {p: _load(p) for p in ("train.py", "eval.py", "demo.py", "tools/fit_anchors.py")}


def _same_config(got, want):
    assert np.array_equal(got.ANCHOR_BOX, want.ANCHOR_BOX)
    assert (got.CLASSES, got.IMAGE_HEIGHT, got.IMAGE_WIDTH, got.BATCH_SIZE) == (want.CLASSES, want.IMAGE_HEIGHT, want.IMAGE_WIDTH, want.BATCH_SIZE)


# ------------------------------------------------------------------------------------------------- config equivalence --
def test_nets_and_datasets():
    assert drivers.NETS == ("squeezeDet", "squeezeDet+", "resnet50", "vgg16") == tuple(drivers.NET_TABLE)
    assert drivers.DATASETS == ("KITTI", "PASCAL_VOC")


@pytest.mark.parametrize("net", drivers.NETS)
def test_make_config_is_the_nets_config_function(net):
    default, sized = DIRECT[net]
    _same_config(drivers.make_config(net), default())
    _same_config(drivers.base_config(net), default())
    if sized is None:
        with pytest.raises(SystemExit, match="--image_size: no sized config for --net squeezeDet\\+"):
            drivers.make_config(net, (128, 256))
    else:
        _same_config(drivers.make_config(net, (128, 256)), sized(128, 256))
        _same_config(drivers.make_config(net, [128, 256], "KITTI", None), sized(128, 256))


@pytest.mark.parametrize("size", [None, (128, 256)])
@pytest.mark.parametrize("shapes", [None, SHAPES9])
def test_make_config_pascal_voc(size, shapes):
    """by hand: voc_squeezeDet_config_for_input -> with_anchor_shapes -> pad_head_classes, in that order"""
    want = S.voc_squeezeDet_config_for_input(*(size or (384, 1248)))
    if shapes is not None:
        want = config.with_anchor_shapes(want, shapes)
    want = config.pad_head_classes(want)
    got = drivers.make_config("squeezeDet", size, "PASCAL_VOC", shapes)
    _same_config(got, want)
    assert got.CLASSES == 23 and got.HEAD_PAD_CLASSES == want.HEAD_PAD_CLASSES == 3 and len(got.CLASS_NAMES) == 20
    if shapes is not None:
        assert np.array_equal(config.anchor_shapes_of(got), shapes)
    base = drivers.base_config("squeezeDet", size, "PASCAL_VOC")              # (what fit_anchors.py fits on: the head not padded)
    assert base.CLASSES == 20 and "HEAD_PAD_CLASSES" not in base


# ---------------------------------------------------------------------------------------------------- table integrity --
def test_table_names_the_classes_the_scripts_named():
    from squeezedet_amd import nets, train
    assert [drivers.model_class(n) for n in drivers.NETS] == [nets.SqueezeDet, nets.SqueezeDetPlus, nets.ResNet50ConvDet, nets.VGG16ConvDet]
    assert [drivers.trainer_class(n) for n in drivers.NETS] == [train.SqueezeDetTrainer, train.SqueezeDetTrainer,
                                                                 train.ResNet50ConvDetTrainer, train.VGG16ConvDetTrainer]
    import torch
    assert drivers.torch_dtype("fp16") is torch.float16 and drivers.torch_dtype("fp32") is torch.float32


def test_eval_and_demo_do_not_import_the_trainers():
    code = ("import sys; sys.path.insert(0, %r); from squeezedet_amd import drivers; import demo; import eval as E;"
            " drivers.make_config('vgg16'); drivers.make_config('squeezeDet', (128, 256), 'PASCAL_VOC'); drivers.model_class('resnet50');"
            " assert 'squeezedet_amd.drivers' in sys.modules and 'squeezedet_amd.train' not in sys.modules, sorted(sys.modules)" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ arguments, refusals --
# vars(parse_args([])) of the four scripts as they were before squeezedet_amd.drivers existed, recorded from that commit
DEFAULTS = {
    "train.py": {"dataset": "KITTI", "year": "2007", "data_path": "", "image_set": "train", "train_dir": "/tmp/squeezeDet/train",
                 "max_steps": 1000000, "net": "squeezeDet", "pretrained_model_path": "", "summary_step": 10, "checkpoint_step": 1000,
                 "gpu": "0", "dtype": "fp32", "batch_size": 0, "seed": 0, "resume": False, "overwrite": False, "keep_checkpoints": 0,
                 "no_graph": False, "synthetic": 0, "image_size": None, "loss_scale": 1024.0, "image_summary": 0, "anchor_shapes": "",
                 "anchor_report": False},
    "eval.py": {"dataset": "KITTI", "data_path": "", "image_set": "test", "year": "2007", "image_size": None,
                "eval_dir": "/tmp/squeezeDet/eval", "checkpoint_path": "/tmp/squeezeDet/train", "eval_interval_secs": 60, "run_once": False,
                "net": "squeezeDet", "gpu": "0", "batch_size": 0, "dtype": "fp32", "eval_tool": "", "synthetic_weights": False,
                "visualize": 0, "seed": 0, "anchor_shapes": ""},
    "demo.py": {"mode": "image", "input_path": "./data/sample.png", "out_dir": "./data/out/", "demo_net": "squeezeDet", "weights": "",
                "anchor_shapes": "", "gpu": "0", "dtype": "fp16", "draw": "pil", "crop": [500, 205, 239, 439], "batch": 1},
    "tools/fit_anchors.py": {"dataset": "KITTI", "year": "2007", "data_path": "", "image_set": "train", "net": "squeezeDet",
                             "image_size": None, "synthetic": 0, "k": 9, "seed": 0, "restarts": 8, "max_iter": 100, "gpu": "0",
                             "out": "anchors.json"},
}


@pytest.mark.parametrize("script", sorted(DEFAULTS))
def test_argument_defaults(scripts, script):
    assert vars(scripts[script].parse_args([])) == DEFAULTS[script]


def test_refusals(scripts, capsys):
    T, E, F = scripts["train.py"], scripts["eval.py"], scripts["tools/fit_anchors.py"]
    for mod in (T, E, F):
        with pytest.raises(SystemExit):
            mod.parse_args(["--dataset", "PASCAL_VOC", "--net", "resnet50"])
        assert "--dataset PASCAL_VOC: only --net squeezeDet has a VOC config" in capsys.readouterr().err
        assert mod.parse_args(["--dataset", "PASCAL_VOC"]).net == "squeezeDet"
    with pytest.raises(SystemExit):
        T.parse_args(["--resume", "--overwrite"])
    assert "--resume and --overwrite exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit, match="--image_size is for --dataset PASCAL_VOC"):
        E.main(["--run_once", "--image_size", "128", "256"])
    with pytest.raises(SystemExit, match="--visualize is KITTI-only"):
        E.main(["--dataset", "PASCAL_VOC", "--run_once", "--visualize", "1"])
    for mod in (T, E):                                                   # the reference's assert
        with pytest.raises(AssertionError, match="Currently only supports KITTI dataset"):
            mod.parse_args(["--dataset", "COCO"])
    with pytest.raises(SystemExit):                                      # the tool's own: a usage error
        F.parse_args(["--dataset", "COCO"])
    assert "--dataset must be KITTI or PASCAL_VOC" in capsys.readouterr().err
    for mod in (T, E, F):
        with pytest.raises(SystemExit):
            mod.parse_args(["--net", "alexnet"])
    with pytest.raises(SystemExit):
        scripts["demo.py"].parse_args(["--demo_net", "alexnet"])


# ------------------------------------------------------------------------------------------------ image read, seed rule --
def test_read_bgr(golden_dir):
    from PIL import Image
    path = os.path.join(golden_dir, "sample.png")
    rgb = np.asarray(Image.open(path).convert("RGB"))
    bgr = drivers.read_bgr(path)
    assert bgr.dtype == np.uint8 and bgr.flags["C_CONTIGUOUS"] and bgr.shape == rgb.shape and bgr.ndim == 3 and bgr.shape[2] == 3
    assert np.array_equal(bgr, rgb[:, :, ::-1]) and not np.array_equal(bgr, rgb)


def test_synthetic_data_seed_rule():
    from squeezedet_amd import synthetic
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    got_images, got_rois = drivers.synthetic_data(mc, 4, seed=2)
    want_images, want_rois = synthetic.synthetic_dataset(mc, 4, seed=302)
    assert len(got_images) == len(want_images) == 4 and len(got_rois) == len(want_rois) == 4
    for g, w in zip(list(got_images) + list(got_rois), list(want_images) + list(want_rois)):
        assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(np.asarray(g), np.asarray(w))
    assert not np.array_equal(got_images[0], synthetic.synthetic_dataset(mc, 4, seed=2)[0][0])
