"""CPU-side checks of the Pascal VOC path (squeezedet_amd/voc.py, the drivers' arguments, the C-ABI section): the XML
reader against hand-written files, the detection-file text against the reference's (tests/golden/voc_ap.npz), the config
and -- where the reference tree is present -- one golden case regenerated."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import squeezedet_amd as S
from squeezedet_amd import _lib, drivers, voc as V
from squeezedet_amd import build as sqbuild
from tests.golden import voc_ap_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xml(objects):
    """objects: (name, xmin, ymin, xmax, ymax, difficult) with the coordinates as text."""
    body = "".join("<object><name>%s</name><pose>Left</pose><truncated>1</truncated><difficult>%d</difficult>"
                   "<bndbox><xmin>%s</xmin><ymin>%s</ymin><xmax>%s</xmax><ymax>%s</ymax></bndbox></object>" % (n, d, a, b, c, e)
                   for n, a, b, c, e, d in objects)
    return "<annotation><filename>x.jpg</filename><size><width>500</width><height>375</height></size>%s</annotation>" % body


def _tree(root, files, year="2007", image_set="val"):
    voc = os.path.join(root, "VOC" + year)
    os.makedirs(os.path.join(voc, "Annotations"))
    os.makedirs(os.path.join(voc, "ImageSets", "Main"))
    for idx, objects in files:
        with open(os.path.join(voc, "Annotations", idx + ".xml"), "w") as f:
            f.write(_xml(objects))
    with open(os.path.join(voc, "ImageSets", "Main", image_set + ".txt"), "w") as f:
        f.write("".join(" %s \n" % idx for idx, _ in files))          # (the reference strips each line)
    return voc


def test_load_voc_reads_rois_and_ground_truth(tmp_path):
    mc = S.base_model_config("PASCAL_VOC")
    files = [("2008_000001", [("dog", "48", "240", "195", "371", 0), ("person", "8", "12", "352", "498", 1),
                              (" Car\n", "1", "1", "1", "1", 0), ("giraffe", "5", "6", "7", "8", 1)]),
             ("2008_000002", []),
             ("2008_000003", [("tvmonitor", "100", "50", "300", "200", 0)])]
    _tree(str(tmp_path), files)
    data = V.load_voc(str(tmp_path), "2007", "val", mc)
    assert data.image_idx == ["2008_000001", "2008_000002", "2008_000003"]
    assert data.image_paths[2] == os.path.join(str(tmp_path), "VOC2007", "JPEGImages", "2008_000003.jpg")
    dog, car, tv = mc.CLASS_NAMES.index("dog"), mc.CLASS_NAMES.index("car"), mc.CLASS_NAMES.index("tvmonitor")
    # rois: non-difficult objects, 1-based -> 0-based, bbox_transform_inv (w = xmax - xmin + 1), name.lower().strip()
    assert data.rois == [[[47 + 0.5 * 148, 239 + 0.5 * 132, 148.0, 132.0, dog], [0.5, 0.5, 1.0, 1.0, car]], [],
                         [[99 + 0.5 * 201, 49 + 0.5 * 151, 201.0, 151.0, tv]]]
    # gt: every object, the raw integers, the difficult flag, exact name match or -1
    gt = data.gt
    assert gt.num_images == 3 and gt.offsets.tolist() == [0, 4, 4, 5] and gt.offsets.dtype == np.int32
    assert gt.cls.tolist() == [dog, mc.CLASS_NAMES.index("person"), -1, -1, tv]
    assert gt.difficult.tolist() == [0, 1, 0, 1, 0]
    assert gt.box.dtype == np.float64 and gt.box.tolist()[:2] == [[48, 240, 195, 371], [8, 12, 352, 498]]


def test_load_voc_keeps_the_references_asserts_and_errors(tmp_path):
    mc = S.base_model_config("PASCAL_VOC")
    for k, (objects, exc, text) in enumerate([([("dog", "0", "5", "9", "9", 0)], AssertionError, "x-coord xmin -1.0"),
                                              ([("dog", "5", "9", "9", "8", 0)], AssertionError, "y-coord ymin 8.0 or ymax 7.0 at a.xml"),
                                              ([("giraffe", "5", "6", "7", "8", 0)], KeyError, "giraffe")]):
        root = str(tmp_path / str(k))
        _tree(root, [("a", objects)])
        with pytest.raises(exc, match=text):
            V.load_voc(root, "2007", "val", mc)
    with pytest.raises(FileNotFoundError, match="File does not exist"):
        V.load_voc(str(tmp_path / "0"), "2007", "test", mc)
    with pytest.raises(_lib.SqdetUnsupported, match="129 objects"):
        V.GroundTruth([[(0, 1, 1, 5, 5, 0)] * 129])


@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_detection_file_text_is_the_references(name, tmp_path, golden_dir):
    """The case's rows through the host formula of the table values (voc_ap_cases.table_rows) and voc.write_detection_files:
    the files' sha256 is that of the files pascal_voc.evaluate_detections wrote; parsed again they give the same rows."""
    g = np.load(os.path.join(golden_dir, "voc_ap.npz"))
    case = VC.make_case(name)
    voc = VC.write_tree(case, str(tmp_path))
    assert VC.digest_dir(os.path.join(voc, "Annotations")) == str(g[name + ":annotations_sha256"])
    det = str(tmp_path / "det")
    rows = VC.table_rows(case)
    V.write_detection_files(det, case["names"], case["image_idx"], rows)
    assert sorted(os.listdir(det)) == sorted(c + ".txt" for c in case["names"])
    assert VC.digest_dir(det) == str(g[name + ":detections_sha256"])
    for c, cls in enumerate(case["names"]):
        back = V.parse_detection_file(os.path.join(det, cls + ".txt"))
        want = [(idx, r[5]) + r[1:5] for idx, per in zip(case["image_idx"], rows) for r in per if r[0] == c]
        assert back == want


def test_use_07_metric_for():
    assert V.use_07_metric_for("2007") is True and V.use_07_metric_for("2009") is True
    assert V.use_07_metric_for("2010") is False and V.use_07_metric_for(2012) is False


def test_voc_config_fields():
    mc = S.voc_squeezeDet_config_for_input(128, 256)
    k = S.kitti_squeezeDet_config_for_input(128, 256)
    assert mc.DATASET == "PASCAL_VOC" and mc.CLASSES == 20 and len(mc.CLASS_NAMES) == 20 and mc.CLASS_NAMES[14] == "person"
    assert (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH) == (128, 256) and mc.ANCHOR_PER_GRID == 9
    assert mc.ANCHORS == 8 * 16 * 9 == len(mc.ANCHOR_BOX) and np.array_equal(mc.ANCHOR_BOX, k.ANCHOR_BOX)
    for f in ("BATCH_SIZE", "WEIGHT_DECAY", "LEARNING_RATE", "NMS_THRESH", "PROB_THRESH", "TOP_N_DETECTION", "LOSS_COEF_CONF_POS", "DRIFT_X"):
        assert mc[f] == k[f], f
    big = S.voc_squeezeDet_config_for_input(384, 1248)
    assert big.ANCHORS == 24 * 78 * 9
    from squeezedet_amd import config
    assert S.voc_squeezeDet_config_for_input is config.voc_squeezeDet_config_for_input


def test_head_padding_config_and_pinned_parameters():
    """9 * (20 + 5) = 225 ConvDet channels are not a multiple of 4: the net is built with 23 classes, 3 of them pinned."""
    import torch
    from squeezedet_amd import config
    mc = S.voc_squeezeDet_config_for_input(128, 256)
    p = config.pad_head_classes(mc)
    assert (mc.CLASSES, p.CLASSES, p.HEAD_PAD_CLASSES) == (20, 23, 3) and "HEAD_PAD_CLASSES" not in mc
    assert p.CLASS_NAMES == mc.CLASS_NAMES and (9 * (p.CLASSES + 5)) % 4 == 0 and p.ANCHORS == mc.ANCHORS
    k = config.pad_head_classes(S.kitti_squeezeDet_config())
    assert (k.CLASSES, k.HEAD_PAD_CLASSES) == (3, 0)
    params = {"conv12/kernels": torch.ones(3, 3, 8, 252), "conv12/biases": np.full(252, 0.5, np.float32), "conv1/biases": np.ones(4)}
    assert config.pin_padding_classes(k, params) is params
    out = config.pin_padding_classes(p, params)
    pad = sorted(a * 23 + c for a in range(9) for c in (20, 21, 22))
    real = sorted(set(range(252)) - set(pad))
    assert len(pad) == 27 and max(pad) == 9 * 23 - 1                             # class logits only: conf and box channels untouched
    assert np.all(out["conv12/kernels"][..., pad] == 0) and np.all(out["conv12/kernels"][..., real] == 1)
    assert np.all(out["conv12/biases"][pad] == config.PAD_CLASS_BIAS) and np.all(out["conv12/biases"][real] == 0.5)
    assert out["conv1/biases"] is params["conv1/biases"] and float(params["conv12/kernels"].min()) == 1.0     # the input is not modified
    assert np.exp(np.float32(config.PAD_CLASS_BIAS)) == 0.0 and np.float16(config.PAD_CLASS_BIAS) == config.PAD_CLASS_BIAS


def test_drivers_accept_pascal_voc_and_refuse_other_datasets():
    sys.path.insert(0, ROOT)
    import eval as E
    import train as T
    a = E.parse_args(["--dataset", "PASCAL_VOC", "--year", "2012", "--image_size", "128", "256", "--run_once"])
    assert (a.dataset, a.year, a.image_size) == ("PASCAL_VOC", "2012", [128, 256])
    d = E.parse_args([])
    assert (d.dataset, d.year, d.image_size) == ("KITTI", "2007", None)
    t = T.parse_args(["--dataset", "PASCAL_VOC", "--year", "2012", "--image_size", "128", "256"])
    assert (t.dataset, t.year, t.image_size) == ("PASCAL_VOC", "2012", [128, 256]) and T.parse_args([]).year == "2007"
    for mod in (E, T):
        for bad in ("VOC", "pascal_voc", "COCO"):
            with pytest.raises(AssertionError, match="Currently only supports KITTI dataset"):
                mod.parse_args(["--dataset", bad])
    with pytest.raises(SystemExit):
        T.parse_args(["--dataset", "PASCAL_VOC", "--net", "vgg16"])
    tc = drivers.make_config("squeezeDet", [128, 256], "PASCAL_VOC")
    assert len(tc.CLASS_NAMES) == 20 and (tc.CLASSES, tc.HEAD_PAD_CLASSES) == (23, 3)        # the padded head (config.pad_head_classes)
    assert drivers.make_config("squeezeDet", None, "PASCAL_VOC").ANCHORS == 24 * 78 * 9
    assert drivers.make_config("squeezeDet", [128, 256]).CLASSES == 3
    # --eval_tool / --visualize are KITTI-only: refused before anything is loaded
    for extra in (["--eval_tool", "/bin/true"], ["--visualize", "3"]):
        with pytest.raises(SystemExit, match="KITTI-only"):
            E.main(["--dataset", "PASCAL_VOC", "--run_once"] + extra)
    with pytest.raises(SystemExit, match="--image_size is for --dataset PASCAL_VOC"):
        E.main(["--run_once", "--image_size", "128", "256"])


def test_library_exports_the_voc_entry_points_and_validates_arguments():
    sqbuild.build(verbose=False)
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sqdet.h")).read()
    for name in ("sqdet_voc_ingest", "sqdet_voc_eval_workspace_bytes", "sqdet_voc_evaluate"):
        assert name + "(" in header and hasattr(lib, name) and name in _lib.SIGNATURES
    for enum, value in (("SQDET_VOC_MAX_DETECTIONS", V.MAX_DETECTIONS), ("SQDET_VOC_MAX_GROUNDTRUTH", V.MAX_GROUNDTRUTH),
                        ("SQDET_VOC_MAX_CLASSES", V.MAX_CLASSES)):
        assert "%s = %d" % (enum, value) in header
    assert "TIE RULE" in header
    # argument checks only: nothing is launched
    one = C.c_void_p(8)
    assert lib.sqdet_voc_ingest(None, None, None, None, None, 1, 64, 20, None, None, None, None, None, 0, 1, 64, None) == -1
    assert b"null" in lib.sqdet_last_error()
    assert lib.sqdet_voc_ingest(one, one, one, one, None, 1, 64, 65, one, one, one, one, one, 0, 1, 64, None) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_voc_ingest(one, one, one, one, None, 1, 600, 20, one, one, one, one, one, 0, 1, 600, None) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_voc_ingest(one, one, one, one, None, 1, 64, 20, one, one, one, one, one, 0, 1, 32, None) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_voc_ingest(one, one, one, one, None, 2, 64, 20, one, one, one, one, one, 0, 1, 64, None) == -1
    assert lib.sqdet_voc_evaluate(one, one, one, one, one, 4, 513, 20, one, one, one, one, 1, one, one, one, one, one, -1, None, None,
                                  None) == _lib.SQDET_EUNSUPPORTED
    assert lib.sqdet_voc_evaluate(one, one, one, one, one, 4, 64, 20, one, one, one, one, 1, one, one, one, one, one, 20, one, one,
                                  None) == -1
    small, big = lib.sqdet_voc_eval_workspace_bytes(4, 64, 20), lib.sqdet_voc_eval_workspace_bytes(4952, 64, 20)
    assert 0 < small < big and big >= 4952 * 64 * (2 * 8 + 3 * 4) and lib.sqdet_voc_eval_workspace_bytes(0, 64, 20) == 0


def test_golden_case_regenerates_from_the_reference(golden_dir):
    """Where the reference tree is present: its evaluator run again on one case gives the committed fixture."""
    from tests.golden import make_voc_ap_golden as M
    if not M.available():
        pytest.skip("the reference tree is not present")
    g = np.load(os.path.join(golden_dir, "voc_ap.npz"))
    new = M.run_reference("greedy")
    assert sorted(k for k in g.files if k.startswith("greedy:")) == sorted(new)
    for k, v in new.items():
        assert np.array_equal(np.asarray(v), g[k], equal_nan=v.dtype.kind == "f"), k
    # what the case is built to show (voc_ap_cases._greedy): car = tp, fp (exactly 0.5), fp (taken), neither, fp with npos 2
    assert g["greedy:car:rec"].tolist() == [0.5, 0.5, 0.5, 0.5, 0.5]
    assert g["greedy:car:prec"].tolist() == [1.0, 0.5, 1 / 3.0, 1 / 3.0, 0.25]
