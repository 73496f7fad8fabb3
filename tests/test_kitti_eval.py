"""KITTI evaluation plumbing (reference src/eval.py:69-101 + src/dataset/kitti.py:100-159): the
detection files squeezedet_amd/kitti_eval.py writes, judged by the REFERENCE'S OWN C++ evaluator built into
oracle/_ref/ (oracle/Makefile).  Host-only."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "oracle", "_ref", "evaluate_object")
CLASSES = ("car", "pedestrian", "cyclist")       # kitti.py:22


def test_detection_file_format(tmp_path):
    from squeezedet_amd import kitti_eval as K
    ab = K.new_all_boxes(3, 1)
    K.add_detections(ab, 0, [[100.0, 50.0, 40.0, 20.0]], [0.87654], [1])
    K.write_detection_files(str(tmp_path), ["000007"], CLASSES, ab)
    line = open(tmp_path / "000007.txt").read()
    assert line == "pedestrian -1 -1 0.0 80.00 40.00 120.00 60.00 0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.877\n"
    ab = K.new_all_boxes(3, 1)
    K.add_detections(ab, 0, [[100.0, 50.0, 40.0, 20.0]], [0.5], [0], scale=(2.0, 0.5))     # eval.py:83-84 rescale
    assert np.allclose(ab[0][0][0], [40.0, 80.0, 60.0, 120.0, 0.5])


def _recorded_evaluator(monkeypatch, golden_dir):
    """Stands in for the reference evaluator where oracle/_ref/ was not built (the reference tree is not on every machine): when
    the detection files it is handed are byte for byte those the real evaluator scored (tests/golden/kitti_eval.npz,
    make_golden.py), it writes the AP files the real one wrote for them; otherwise it writes nothing (every AP reads 0)."""
    from squeezedet_amd import kitti_eval as K
    from tests.golden import cases
    g = np.load(os.path.join(golden_dir, "kitti_eval.npz"))

    def call(cmd, **kw):
        det_dir = cmd[3]
        digest = cases.kitti_detection_digest(os.path.join(det_dir, "data"))
        for name in ("perfect", "half"):
            if digest == str(g[name + "_detections_sha256"]):
                for cls in CLASSES:
                    with open(os.path.join(det_dir, "stats_%s_ap.txt" % cls), "w") as f:
                        f.write(str(g["%s_stats_%s_ap" % (name, cls)]))
        return 0
    monkeypatch.setattr(K, "subprocess", type("recorded", (), {"call": staticmethod(call), "DEVNULL": None}))
    return "evaluate_object (recorded)"


def test_reference_evaluator_reads_our_files(tmp_path, monkeypatch, golden_dir):
    """The reference's own evaluator (oracle/_ref/evaluate_object where built, else its recorded answers) reads the detection
    files we write as intended: every box found -> AP 1 everywhere; half of them replaced by false positives -> below 0.75."""
    from squeezedet_amd import kitti_eval as K
    from tests.golden import cases
    tool = TOOL if os.path.exists(TOOL) else _recorded_evaluator(monkeypatch, golden_dir)
    root = str(tmp_path / "KITTI")
    idxs, tables = cases.make_kitti_case(root)
    aps, names = K.evaluate_detections(tool, root, "val", str(tmp_path / "eval_a"), 100, idxs, CLASSES, tables["perfect"])
    assert names[:3] == ["car_easy", "car_medium", "car_hard"] and len(aps) == 9
    assert all(abs(a - 1.0) < 1e-6 for a in aps), aps
    aps2, _ = K.evaluate_detections(tool, root, "val", str(tmp_path / "eval_b"), 100, idxs, CLASSES, tables["half"])
    assert all(0.0 < a < 0.75 for a in aps2), aps2
