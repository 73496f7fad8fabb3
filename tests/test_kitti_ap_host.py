"""Host half of the GPU KITTI evaluator (squeezedet_amd/kitti_ap.py, eval.py): label / image-set parsing, the evaluator's
number formatting, checkpoint steps, eval.py's command line.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABELS = """Car 0.00 0 -1.58 587.01 173.33 614.12 200.12 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59
van 0.15 1 1.85 387.63 181.54 423.81 203.12 1.67 1.87 3.69 -16.53 2.39 58.49 1.57
Pedestrian 0.30 2 -0.20 712.40 143.00 810.73 307.92 1.89 0.48 1.20 1.84 1.47 8.41 0.01
Person_sitting 0.50 3 -0.20 100.00 100.00 140.00 140.00 1.89 0.48 1.20 1.84 1.47 8.41 0.01
CYCLIST 0.00 0 -0.20 300.00 100.00 330.00 125.00 1.89 0.48 1.20 1.84 1.47 8.41 0.01
DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10
Truck 0.00 0 -1.58 10.00 20.00 30.00 40.00 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59
"""


def _write(tmp_path, text=LABELS):
    p = tmp_path / "000001.txt"
    p.write_text(text)
    return str(p)


def test_label_parsing_type_codes(tmp_path):
    from squeezedet_amd import kitti_ap as KA
    rows = KA.parse_label_file(_write(tmp_path))
    assert [r[0] for r in rows] == [0, 3, 1, 4, 2, 5, 6]           # case-insensitive; Truck -> other
    assert rows[0][1:5] == (587.01, 173.33, 614.12, 200.12)
    assert [r[5] for r in rows] == [0.0, 0.15, 0.30, 0.50, 0.0, -1.0, 0.0]
    assert [r[6] for r in rows] == [0, 1, 2, 3, 0, -1, 0]
    assert rows[3][4] - rows[3][2] == 40.0                            # an exact 40.00 height stays exact
    # parsing stops at the first object that does not parse, like fscanf
    assert len(KA.parse_label_file(_write(tmp_path, LABELS.replace("0.30 2", "x.30 2")))) == 2


def test_rois_follow_load_kitti_annotation(tmp_path):
    from squeezedet_amd import kitti_ap as KA
    from squeezedet_amd.util import bbox_transform_inv
    fn = _write(tmp_path)
    rois = KA.parse_rois(fn)
    assert [r[4] for r in rois] == [0, 1, 2]                          # car, pedestrian, cyclist; others dropped
    assert rois[0][:4] == bbox_transform_inv([587.01, 173.33, 614.12, 200.12])
    # EXCLUDE_HARD_EXAMPLES: level 4 = height + 1 < 25, or truncation > 0.5, or occlusion > 2
    hard = KA.parse_rois(fn, exclude_hard=True)
    assert [r[4] for r in hard] == [0, 1, 2]
    lab = LABELS.replace("Pedestrian 0.30 2", "Pedestrian 0.51 2").replace("CYCLIST 0.00 0 -0.20 300.00 100.00 330.00 125.00",
                                                                           "CYCLIST 0.00 0 -0.20 300.00 100.00 330.00 124.00")
    assert [r[4] for r in KA.parse_rois(_write(tmp_path, lab), exclude_hard=True)] == [0, 2]   # 24 + 1 >= 25 kept
    lab = lab.replace("330.00 124.00", "330.00 123.99")
    assert [r[4] for r in KA.parse_rois(_write(tmp_path, lab), exclude_hard=True)] == [0]
    assert len(KA.parse_rois(_write(tmp_path, lab), exclude_hard=False)) == 3


def test_load_kitti_and_ground_truth_tables(tmp_path):
    from squeezedet_amd import config, kitti_ap as KA
    root = tmp_path / "KITTI"
    (root / "training" / "label_2").mkdir(parents=True)
    (root / "ImageSets").mkdir()
    (root / "training" / "label_2" / "000001.txt").write_text(LABELS)
    (root / "training" / "label_2" / "000002.txt").write_text("")
    (root / "ImageSets" / "val.txt").write_text("000001\n000002\n")
    mc = config.kitti_squeezeDet_config()
    d = KA.load_kitti(str(root), "val", mc)
    assert d.image_idx == ["000001", "000002"]
    assert d.image_paths[0].endswith(os.path.join("training", "image_2", "000001.png"))
    assert list(d.gt.offsets) == [0, 7, 7] and list(d.gt.roi_offsets) == [0, 3, 3]
    assert d.gt.box.shape == (7, 4) and d.gt.type.tolist() == [0, 3, 1, 4, 2, 5, 6]
    assert d.gt.roi_cls.tolist() == [0, 1, 2] and d.gt.roi_box.dtype == np.float64
    from squeezedet_amd._lib import SqdetUnsupported
    with pytest.raises(SqdetUnsupported):
        KA.GroundTruth([[(0, 0.0, 0.0, 1.0, 1.0, 0.0, 0)] * 129], [[]])


def test_stats_formatting_matches_cpp_ostream():
    from squeezedet_amd import kitti_ap as KA
    assert KA.cpp_float_g(1.0) == "1" and KA.cpp_float_g(0.0) == "0"
    assert KA.cpp_float_g(1.0 / 11.0) == "0.0909091"
    assert KA.cpp_float_g(0.00363636363636) == "0.00363636"
    assert KA.cpp_float_g(1e-5) == "1e-05"
    assert KA.cpp_float_g(float("nan")) == "-nan"
    assert KA.cpp_float_f(0.5) == "0.500000" and KA.cpp_float_f(float("nan")) == "-nan"
    p = np.zeros((3, 41))
    p[0, :] = 1.0
    p[1, 0] = 1.0
    ap, det = KA.format_stats(p)
    assert ap == "AP=1\nAP=0.0909091\nAP=0\n"
    assert det.splitlines()[0] == "1.000000 " * 11
    assert det.splitlines()[1] == "1.000000 " + "0.000000 " * 10
    assert det.endswith("\n") and len(det.splitlines()) == 3


def test_recorded_stats_parse_as_evaluate_detections_reads_them(golden_dir):
    """every recorded AP file has three 'AP=' lines that format_stats' rendering can produce"""
    g = np.load(os.path.join(golden_dir, "kitti_ap.npz"))
    names = [k for k in g.files if k.endswith("_ap.txt")]
    assert names
    for k in names:
        lines = str(g[k]).splitlines()
        assert len(lines) == 3 and all(l.startswith("AP=") for l in lines)
        from squeezedet_amd import kitti_ap as KA
        assert all(KA.cpp_float_g(float(l[3:])) == l[3:] for l in lines)


def test_checkpoint_step_parsing(tmp_path):
    from squeezedet_amd.kitti_ap import parse_checkpoint_step
    assert parse_checkpoint_step("/a/b/model.ckpt-20000.npz") == "20000"
    assert parse_checkpoint_step("model-7.npz") == "7"
    assert parse_checkpoint_step("/x/model.ckpt-999") == "999"
    sys.path.insert(0, ROOT)
    import eval as E
    for s in (5, 300, 40):
        (tmp_path / ("model.ckpt-%d.npz" % s)).write_bytes(b"")
    (tmp_path / "notes-x.npz").write_bytes(b"")
    assert E.latest_checkpoint(str(tmp_path)).endswith("model.ckpt-300.npz")
    assert E.latest_checkpoint(str(tmp_path / "missing")) is None


def test_eval_py_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    for flag in ("--dataset", "--data_path", "--image_set", "--eval_dir", "--checkpoint_path", "--eval_interval_secs",
                 "--run_once", "--net", "--gpu", "--batch_size", "--dtype", "--eval_tool", "--synthetic_weights"):
        assert flag in r.stdout, flag
    sys.path.insert(0, ROOT)
    import eval as E
    a = E.parse_args(["--run_once", "--net", "vgg16"])
    assert a.run_once and a.net == "vgg16" and a.dtype == "fp32" and a.batch_size == 0 and a.dataset == "KITTI"
