"""CPU-side checks of the COCO-style metric (squeezedet_amd/coco.py): the hand cases of tests/coco_cases.py against the
NumPy restatement (tests/coco_reference.py, the kernels' yardstick) and against summarize_arrays, the ground-truth mappings and
readers on files written here, the results file's round trip, eval.py's flag and the C-ABI section."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from squeezedet_amd import _lib, coco as CO
from tests import coco_cases as CC, coco_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thresholds_are_linspace():
    """What the kernels are handed: np.linspace's values bit for bit -- 0.5 and 0.75 exact -- which are not `0.5 + i * 0.05`: that is why they are passed from the host.  Case (b2)'s AP follows the third one as it is here."""
    assert np.array_equal(CO.IOU_THRS, np.linspace(.5, .95, 10)) and np.array_equal(CO.REC_THRS, np.linspace(0, 1, 101))
    assert np.array_equal(CO.IOU_THRS, CR.IOU_THRS) and np.array_equal(CO.REC_THRS, CR.REC_THRS)
    assert len(CO.IOU_THRS) == 10 and len(CO.REC_THRS) == 101
    assert CO.IOU_THRS[0] == 0.5 and CO.IOU_THRS[5] == 0.75
    assert not np.array_equal(CO.IOU_THRS, 0.5 + np.arange(10) * 0.05)
    assert CC.STATS["b2"][0] == (0.2 if CO.IOU_THRS[2] > 0.6 else 0.3) and CC.STATS["b1"][0] == 0.1
    assert np.array_equal(np.asarray(CO.AREA_RNGS), np.asarray(CR.AREA_RNGS)) and CO.AREA_RNGS[0] == (0, 1e10)
    assert CO.AREA_RNGS[1:] == ((0, 1024), (1024, 9216), (9216, 1e10)) and tuple(CR.MAX_DETS) == CO.MAX_DETS == (1, 10, 100)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_hand_cases(name):
    """Each case's hand-computed numbers hold for the restatement, and summarize_arrays agrees with the restatement's own
    entry-by-entry summary."""
    dets, gts, classes = CC.CASES[name]
    precision, recall, flags = CR.evaluate(dets, gts, classes)
    assert precision.shape == (10, 101, classes, 4, 3) and recall.shape == (10, classes, 4, 3)
    stats = CO.summarize_arrays(precision, recall)
    CC.check(name, precision, recall, flags, stats)
    assert np.allclose(stats, CR.summarize(precision, recall), rtol=0, atol=1e-15)
    lines = CO.summary_lines(stats)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {:0.3f}".format(stats[0])
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = {:0.3f}".format(stats[6])
    assert lines[1].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ]")
    assert lines[11].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ]")


def test_identical_objects_the_later_one_is_taken():
    """Case (d), class 0, where only the matched index can tell: the walk takes `>=`, so of two equal IoUs the later object wins."""
    dets, gts, _ = CC.CASES["d"]
    d = [r[1:] for r in dets[0] if r[0] == 0]
    g = [r[1:] for r in gts[0] if r[0] == 0]
    ious = CR.iou_matrix(d, g)
    assert ious == [[1.0, 1.0]]
    best, m = 0.5, -1
    for k in range(2):
        if ious[0][k] >= best:
            best, m = ious[0][k], k
    assert m == 1
    _, matched, ignored = CR.evaluate_image(d, g, CR.AREA_RNGS[0], CR.IOU_THRS, 100)
    assert matched.all() and not ignored.any()


def test_summarize_arrays_means_and_empty_selections():
    rs = np.random.RandomState(0)
    p, r = rs.uniform(0, 1, (10, 101, 3, 4, 3)), rs.uniform(0, 1, (10, 3, 4, 3))
    p[:, :, 1], r[:, 1] = -1, -1                       # a class without objects
    p[:, :, :, 1], r[:, :, 1] = -1, -1                 # nothing small
    s = CO.summarize_arrays(p, r)
    assert s[3] == -1 and s[9] == -1
    want = {0: p[:, :, [0, 2], 0, 2], 1: p[0, :, [0, 2], 0, 2], 2: p[5, :, [0, 2], 0, 2], 6: r[:, [0, 2], 0, 0], 7: r[:, [0, 2], 0, 1],
            11: r[:, [0, 2], 3, 2]}
    for k, sel in want.items():
        assert abs(s[k] - np.mean(sel)) <= 1e-15          # (the same entries summed in another order)
    assert np.allclose(s, CR.summarize(p, r), rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ mappings and readers --
def test_from_voc(tmp_path):
    from squeezedet_amd import voc as V
    gt = V.GroundTruth([[(3, 48, 240, 195, 371, 0), (-1, 5, 6, 7, 8, 0), (7, 1, 1, 1, 1, 1)], [], [(0, 100, 50, 300, 200, 0)]])
    cg = CO.CocoGroundTruth.from_voc(gt)
    assert cg.num_images == 3 and cg.offsets.tolist() == [0, 2, 2, 3] and cg.offsets.dtype == np.int32
    assert cg.cls.tolist() == [3, 7, 0] and cg.cls.dtype == np.int32
    assert cg.box.tolist() == [[47, 239, 148, 132], [0, 0, 1, 1], [99, 49, 201, 151]] and cg.box.dtype == np.float64
    assert cg.area.tolist() == [148 * 132, 1, 201 * 151] and cg.flags.tolist() == [0, CO.IGNORE, 0]


def test_from_kitti():
    import squeezedet_amd as S
    from squeezedet_amd import kitti_ap as KA
    mc = S.kitti_squeezeDet_config()
    T = KA.TYPE_CODES
    raw = [[(T["car"], 10.5, 20.25, 110.5, 80.25, 0.0, 0), (T["van"], 1, 2, 30, 40, 0.0, 0), (T["dontcare"], 300, 100, 340, 130, -1.0, -1),
            (T["cyclist"], 5, 5, 25, 45, 0.9, 3)], [(KA.TYPE_OTHER, 0, 0, 5, 5, 0.0, 0)]]
    gt = KA.GroundTruth(raw, [[], []])
    cg = CO.CocoGroundTruth.from_kitti(gt, mc)
    names = [n.lower() for n in mc.CLASS_NAMES]
    car, cyc = names.index("car"), names.index("cyclist")
    assert cg.class_names == tuple(mc.CLASS_NAMES) and cg.offsets.tolist() == [0, 5, 5]
    assert cg.cls.tolist() == [car, 0, 1, 2, cyc]
    assert cg.box.tolist() == [[10.5, 20.25, 100, 60], [300, 100, 40, 30], [300, 100, 40, 30], [300, 100, 40, 30], [5, 5, 20, 40]]
    assert cg.area.tolist() == [6000, 1200, 1200, 1200, 800]
    assert cg.flags.tolist() == [0, CO.CROWD, CO.CROWD, CO.CROWD, 0]           # occlusion 3 and truncation 0.9 change nothing
    assert "NOT KITTI's protocol" in CO.CocoGroundTruth.from_kitti.__doc__


def _annotation_file(path):
    d = {"images": [{"id": 42, "file_name": "b.jpg"}, {"id": 7, "file_name": "a.jpg"}, {"id": 19, "file_name": "c.jpg"}],
         "categories": [{"id": 18, "name": "dog"}, {"id": 1, "name": "person"}, {"id": 3, "name": "car"}],
         "annotations": [{"id": 1, "image_id": 42, "category_id": 18, "bbox": [10.5, 20, 30, 40.25], "area": 700.5, "iscrowd": 0},
                         {"id": 2, "image_id": 7, "category_id": 1, "bbox": [0, 0, 100, 50], "iscrowd": 1},
                         {"id": 3, "image_id": 42, "category_id": 3, "bbox": [1, 2, 3, 4], "area": 12, "ignore": 1},
                         {"id": 4, "image_id": 7, "category_id": 3, "bbox": [5, 5, 10, 10], "area": 77.0, "iscrowd": 0, "ignore": 0}]}
    with open(path, "w") as f:
        json.dump(d, f)
    return d


def test_from_json(tmp_path):
    path = str(tmp_path / "ann.json")
    _annotation_file(path)
    g = CO.CocoGroundTruth.from_json(path)
    assert g.image_ids == [7, 19, 42] and g.category_ids == [1, 3, 18] and g.class_names == ("person", "car", "dog")
    assert g.offsets.tolist() == [0, 2, 2, 4]
    assert g.cls.tolist() == [0, 1, 2, 1] and g.box.tolist() == [[0, 0, 100, 50], [5, 5, 10, 10], [10.5, 20, 30, 40.25], [1, 2, 3, 4]]
    assert g.area.tolist() == [5000, 77, 700.5, 12]                              # w * h where the file has none
    assert g.flags.tolist() == [CO.CROWD, 0, 0, CO.IGNORE]
    n = CO.CocoGroundTruth.from_json(path, class_names=("dog", "car"))           # the caller's order; `person` dropped
    assert n.class_names == ("dog", "car") and n.category_ids == [18, 3] and n.cls.tolist() == [1, 0, 1] and n.offsets.tolist() == [0, 1, 1, 3]
    with pytest.raises(_lib.SqdetError, match="no category named 'cat'"):
        CO.CocoGroundTruth.from_json(path, class_names=("cat",))


def test_over_limit_ground_truth_is_refused():
    with pytest.raises(_lib.SqdetUnsupported, match="129 objects"):
        CO.CocoGroundTruth([[(0, 0, 0, 1, 1, 1, 0, 0)] * 129])


def test_results_json_round_trip_is_exact(tmp_path):
    """write_results_json's floats are repr's: json.load gives the table's doubles bit for bit, and read_results_json the
    rows load_rows takes.  (The writer is a method of the device table; it is run here on a stand-in that has tables().)"""
    path = str(tmp_path / "ann.json")
    _annotation_file(path)
    gt = CO.CocoGroundTruth.from_json(path)
    rs = np.random.RandomState(3)
    f32 = lambda: float(np.float32(rs.uniform(0, 500)))
    tables = [[(c, f32() / 3, f32() / 7, f32(), np.nextafter(f32(), 1e9), float(np.float32(rs.uniform()))) for c in sorted(rs.randint(0, 3, 5))]
              for _ in range(3)]
    tables[1] = []

    class Table:
        pass
    ev = Table()
    ev.gt, ev.classes, ev.tables = gt, 3, lambda: tables
    out = str(tmp_path / "coco_results.json")
    CO.CocoEvaluator.write_results_json(ev, out)
    with open(out) as f:
        res = json.load(f)
    flat = [(i, r) for i, rows in enumerate(tables) for r in rows]
    assert len(res) == len(flat) and sorted(res[0]) == ["bbox", "category_id", "image_id", "score"]
    for got, (i, (c, x, y, w, h, s)) in zip(res, flat):
        assert got["image_id"] == gt.image_ids[i] and got["category_id"] == gt.category_ids[c]
        assert np.array_equal(np.array(got["bbox"] + [got["score"]], np.float64).view(np.int64), np.array([x, y, w, h, s], np.float64).view(np.int64))
    assert CO.read_results_json(out, gt) == [[tuple(r) for r in rows] for rows in tables]
    res.append({"image_id": 1234, "category_id": 1, "bbox": [0, 0, 1, 1], "score": 0.5})
    with open(out, "w") as f:
        json.dump(res, f)
    with pytest.raises(_lib.SqdetError, match="image 1234"):
        CO.read_results_json(out, gt)


# ---------------------------------------------------------------------------------------------------------- drivers --
def test_eval_py_coco_metrics_flag():
    sys.path.insert(0, ROOT)
    import eval as E
    a = E.parse_args([])
    assert a.coco_metrics is False                   # off by default; as a class attribute, so vars() is what it was before the flag
    assert vars(a) == {"dataset": "KITTI", "data_path": "", "image_set": "test", "year": "2007", "image_size": None,
                       "eval_dir": "/tmp/squeezeDet/eval", "checkpoint_path": "/tmp/squeezeDet/train", "eval_interval_secs": 60,
                       "run_once": False, "net": "squeezeDet", "gpu": "0", "batch_size": 0, "dtype": "fp32", "eval_tool": "",
                       "synthetic_weights": False, "visualize": 0, "seed": 0, "anchor_shapes": ""}           # today's namespace
    assert E.parse_args(["--coco_metrics"]).coco_metrics is True
    a = E.parse_args(["--dataset", "PASCAL_VOC", "--coco_metrics", "--run_once"])
    assert a.coco_metrics is True and a.dataset == "PASCAL_VOC"


def test_coco_eval_tool_arguments():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tool_coco_eval", os.path.join(ROOT, "tools", "coco_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--annotations", "A.json", "--results", "R.json"])
    assert (a.annotations, a.results, a.gpu) == ("A.json", "R.json", "0")
    with pytest.raises(SystemExit):
        tool.parse_args(["--results", "R.json"])


# ------------------------------------------------------------------------------------------------------------ C-ABI --
def test_library_exports_the_coco_entry_points_and_validates_arguments():
    """The three entry points exist with the header's limits, and the host-side argument checks answer before any device
    work: null pointers and bad dims SQDET_EINVAL, over-limit lists SQDET_EUNSUPPORTED."""
    lib = _lib.lib()
    for name in ("sqdet_coco_ingest", "sqdet_coco_eval_workspace_bytes", "sqdet_coco_evaluate"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "sqdet.h")) as f:
        header = f.read()
    for text in ("SQDET_COCO_MAX_DETECTIONS = 512", "SQDET_COCO_MAX_GROUNDTRUTH = 128", "SQDET_COCO_MAX_CLASSES = 128",
                 "SQDET_COCO_MAX_IOU_THRESHOLDS = 10", "SQDET_COCO_MAX_AREA_RANGES = 4", "SQDET_COCO_MAX_DET_LIMITS = 3",
                 "SQDET_COCO_MAX_KEPT = 128"):
        assert text in header
    assert lib.sqdet_coco_eval_workspace_bytes(0, 64, 3) == 0
    small, big = lib.sqdet_coco_eval_workspace_bytes(10, 64, 3), lib.sqdet_coco_eval_workspace_bytes(20, 64, 3)
    assert 0 < small < big
    assert lib.sqdet_coco_ingest(None, None, None, None, None, 1, 8, 3, None, None, None, None, None, 0, 1, 8, None) != _lib.SQDET_OK
    assert b"null pointer" in lib.sqdet_last_error()
    assert lib.sqdet_coco_evaluate(*([None] * 5), 1, 8, 3, *([None] * 5), 0, None, 10, None, 101, None, 4, None, 3, *([None] * 8)) != _lib.SQDET_OK
    assert b"null pointer" in lib.sqdet_last_error()
    # the list limits are host-side: a fake non-null pointer is never dereferenced before they are checked
    one = (C.c_double * 256)()
    p = C.cast(one, C.c_void_p)
    md = (C.c_int32 * 4)(1, 10, 100, 129)
    pm = C.cast(md, C.c_void_p)
    args = lambda T, R, A, M, K=3: [p] * 5 + [1, 8, K] + [p] * 5 + [0, p, T, p, R, p, A, pm, M] + [p] * 7 + [None]
    for bad, text in ((args(11, 101, 4, 3), b"IoU thresholds"), (args(10, 129, 4, 3), b"recall thresholds"),
                      (args(10, 101, 5, 3), b"area ranges"), (args(10, 101, 4, 4), b"detection limits"),
                      (args(10, 101, 4, 3, K=129), b"129 classes")):
        assert lib.sqdet_coco_evaluate(*bad) == _lib.SQDET_EUNSUPPORTED
        assert text in lib.sqdet_last_error()
