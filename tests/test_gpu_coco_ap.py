"""The GPU COCO-style evaluator (csrc/coco_eval.hip, squeezedet_amd/coco.py) and eval.py --coco_metrics on an MI355X.

Judged by tests/coco_reference.py, the plain-loop float64 NumPy restatement that tests/test_coco_host.py pins by hand: the
per-row flags equal, precision and recall BITWISE equal.  No floating-point sum is involved on either side -- every entry is
one division of integers turned double, a maximum, or a copy -- so there is no tolerance to derive: an entry that differs
means the rule is stated differently on one side.  The statistics come from the same host function on both sides, so they
are bitwise equal as well."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import coco_cases as CC, coco_reference as CR
from tests.golden import voc_ap_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name.replace("/", "_"), os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _evaluator(dets, gts, classes, cap=None, **kw):
    """The case in a device table (rows (cls, x, y, w, h, score) are load_rows' layout already)."""
    from squeezedet_amd import coco as CO
    gt = CO.CocoGroundTruth(gts)
    ev = CO.CocoEvaluator(None, gt, DEV, max_detections=cap or max([1] + [len(r) for r in dets]), classes=classes, **kw)
    ev.load_rows(dets)
    return ev


def _same_flags(got, want):
    assert len(got) == len(want)
    for c, ((gr, gm, gi), (wr, wm, wi)) in enumerate(zip(got, want)):
        assert gr.shape == wr.shape and np.array_equal(gr, wr), ("rank", c)
        assert np.array_equal(gm, wm), ("matched", c, np.argwhere(gm != wm)[:5])
        assert np.array_equal(gi, wi), ("ignored", c, np.argwhere(gi != wi)[:5])


@pytest.fixture(scope="module")
def random_case():
    dets, gts, classes = CC.random_case()
    return dets, gts, classes, CR.evaluate(dets, gts, classes)


# ------------------------------------------------------------------------------------------- kernel against the rule --
def test_random_case_is_the_restatement_bit_for_bit(random_case):
    """7 images, 3 classes, cap 160 (tests/coco_cases.random_case): 130 rows of one class in one image, 70 objects of one
    class in one image, an image without rows, one without objects, a class without objects, crowd / ignore objects, areas
    on 1024 and 9216, duplicated objects, IoUs on 0.5 and 0.75, equal scores within and across images."""
    from squeezedet_amd import coco as CO
    dets, gts, classes, (precision, recall, flags) = random_case
    assert max(sum(1 for r in d if r[0] == 0) for d in dets) == 130 and max(sum(1 for g in gi if g[0] == 1) for gi in gts) >= 70
    ev = _evaluator(dets, gts, classes, cap=160)
    stats = ev.evaluate()
    _same_flags(ev.row_flags(), flags)
    assert ev.num_det.tolist() == [len(f[0]) for f in flags] and ev.num_det[0] >= 100
    assert np.array_equal(_bits(ev.precision), _bits(precision)), np.argwhere(ev.precision != precision)[:8]
    assert np.array_equal(_bits(ev.recall), _bits(recall)), np.argwhere(ev.recall != recall)[:8]
    assert np.array_equal(_bits(stats), _bits(CO.summarize_arrays(precision, recall)))
    assert np.all(ev.precision[:, :, 2] == -1) and ev.per_class_ap[ev.class_names[2]] == -1.0        # the class without objects
    assert 0 < stats[0] < 1 and len(set(ev.precision[ev.precision > -1].tolist())) > 10               # not a trivial table
    # a second call: bitwise the same
    p1, r1, w1 = ev.precision.copy(), ev.recall.copy(), ev.row_word.clone()
    ev.evaluate()
    assert np.array_equal(_bits(ev.precision), _bits(p1)) and np.array_equal(_bits(ev.recall), _bits(r1)) and torch.equal(ev.row_word, w1)


def test_long_case_is_the_restatement_bit_for_bit():
    """300 images, 2 classes (tests/coco_cases.long_case): more images than the scan over images takes at once and more kept
    rows per class than the accumulate kernel walks at once, so both carries run; 120 rows of one class in one image (100
    kept), crowd / ignore objects, images without rows and without objects, equal scores across images."""
    from squeezedet_amd import coco as CO
    dets, gts, classes = CC.long_case()
    precision, recall, flags = CR.evaluate(dets, gts, classes)
    assert len(dets) > 256 and all(len(f[0]) > 256 for f in flags) and len(flags) == 2       # a later edit cannot shrink the case
    assert max(sum(1 for r in d if r[0] == 0) for d in dets) == 120 and not all(dets) and not all(gts)
    assert any(g[6] for gi in gts for g in gi) and any(g[7] for gi in gts for g in gi)
    ev = _evaluator(dets, gts, classes)
    stats = ev.evaluate()
    _same_flags(ev.row_flags(), flags)
    assert ev.num_det.tolist() == [len(f[0]) for f in flags]
    assert np.array_equal(_bits(ev.precision), _bits(precision)), np.argwhere(ev.precision != precision)[:8]
    assert np.array_equal(_bits(ev.recall), _bits(recall)), np.argwhere(ev.recall != recall)[:8]
    assert np.array_equal(_bits(stats), _bits(CO.summarize_arrays(precision, recall)))
    assert 0 < stats[0] < 1 and len(set(ev.precision[ev.precision > -1].tolist())) > 10               # not a trivial table
    # a second call: bitwise the same
    p1, r1, w1 = ev.precision.copy(), ev.recall.copy(), ev.row_word.clone()
    ev.evaluate()
    assert np.array_equal(_bits(ev.precision), _bits(p1)) and np.array_equal(_bits(ev.recall), _bits(r1)) and torch.equal(ev.row_word, w1)


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_hand_cases_through_the_kernel(name):
    from squeezedet_amd import coco as CO
    dets, gts, classes = CC.CASES[name]
    ev = _evaluator(dets, gts, classes)
    stats = ev.evaluate()
    flags = ev.row_flags()
    CC.check(name, ev.precision, ev.recall, flags, stats)
    precision, recall, want = CR.evaluate(dets, gts, classes)
    _same_flags(flags, want)
    assert np.array_equal(_bits(ev.precision), _bits(precision)) and np.array_equal(_bits(ev.recall), _bits(recall))
    assert len(ev.summarize()) == 12 and ev.summarize() == CO.summary_lines(stats)


def test_subset_of_thresholds_and_limits(random_case):
    """Other list lengths than the defaults' (T = 3, R = 11, A = 2, M = 2) index the arrays the same way."""
    dets, gts, classes, _ = random_case
    kw = dict(iou_thrs=np.array([0.5, 0.75, 0.9]), rec_thrs=np.linspace(0, 1, 11), area_rngs=[[0, 1e10], [1024, 9216]], max_dets=[2, 50])
    ev = _evaluator(dets, gts, classes, cap=160, **kw)
    ev.evaluate()
    precision, recall, flags = CR.evaluate(dets, gts, classes, **kw)
    _same_flags(ev.row_flags(), flags)
    assert ev.precision.shape == (3, 11, 3, 2, 2)
    assert np.array_equal(_bits(ev.precision), _bits(precision)) and np.array_equal(_bits(ev.recall), _bits(recall))


# ------------------------------------------------------------------------------------------------------------ ingest --
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scales"])
def test_ingest_is_double_arithmetic_on_the_float32_rows(scaled):
    """add_rows: (cx, cy, w, h) float32 -> double, / the scales, (cx - w/2, cy - h/2, w, h); the score widened, not rounded;
    rows class-major, filter order kept.  Bitwise."""
    from squeezedet_amd import coco as CO
    rs = np.random.RandomState(5)
    n, m, K = 3, 70, 5
    b = np.empty((n, m, 4), np.float32)
    b[..., 0], b[..., 1] = rs.uniform(-20, 500, (n, m)), rs.uniform(-20, 375, (n, m))
    b[..., 2], b[..., 3] = rs.uniform(0, 300, (n, m)), rs.uniform(0, 200, (n, m))
    p = rs.uniform(0, 1, (n, m)).astype(np.float32)
    p[0, :3] = (0.0005, 0.0015, 0.9995)                                 # (nothing is rounded to three decimals here)
    cls = rs.randint(0, K, (n, m)).astype(np.int32)
    cnt = np.array([m, 0, 37], np.int32)
    scales = [(1.0, 1.0), (0.731, 1.377), (256 / 500.0, 128 / 375.0)] if scaled else None
    ev = CO.CocoEvaluator(None, CO.CocoGroundTruth([[] for _ in range(n)]), DEV, max_detections=m, classes=K)
    ev.add_rows(_T(b), _T(p), _T(cls), _T(cnt), 0, scales)
    got = ev.tables()
    for i in range(n):
        sx, sy = (np.float64(scales[i][0]), np.float64(scales[i][1])) if scaled else (np.float64(1), np.float64(1))
        want = []
        for j in sorted(range(cnt[i]), key=lambda j: cls[i, j]):        # (sorted is stable)
            cx, cy, w, h = np.float64(b[i, j, 0]) / sx, np.float64(b[i, j, 1]) / sy, np.float64(b[i, j, 2]) / sx, np.float64(b[i, j, 3]) / sy
            want.append((int(cls[i, j]), float(cx - w / 2), float(cy - h / 2), float(w), float(h), float(np.float64(p[i, j]))))
        assert got[i] == want
    assert got[0][0][5] != round(got[0][0][5], 3)


def test_results_file_scores_like_the_table(random_case, tmp_path):
    """write_results_json -> evaluate_results_file against the same ground truth as an annotation file: the same arrays."""
    from squeezedet_amd import coco as CO
    dets, gts, classes, _ = random_case
    image_ids = [100 + 3 * i for i in range(len(gts))][::-1]            # ids descending: the reader orders images by id
    cat_ids = [5, 9, 2]
    ann = {"images": [{"id": i} for i in image_ids], "categories": [{"id": c, "name": "c%d" % c} for c in cat_ids], "annotations": []}
    order = sorted(range(len(gts)), key=lambda i: image_ids[i])
    names_by_id = sorted(cat_ids)
    for i, rows in enumerate(gts):
        for c, x, y, w, h, area, crowd, ignore in rows:
            ann["annotations"].append({"id": len(ann["annotations"]) + 1, "image_id": image_ids[i], "category_id": names_by_id[c],
                                       "bbox": [x, y, w, h], "area": area, "iscrowd": crowd, "ignore": ignore})
    a_path, r_path = str(tmp_path / "ann.json"), str(tmp_path / "res.json")
    with open(a_path, "w") as f:
        json.dump(ann, f)
    gt = CO.CocoGroundTruth.from_json(a_path)
    assert gt.image_ids == sorted(image_ids) and gt.category_ids == names_by_id
    ev = CO.CocoEvaluator.from_rows(None, gt, [dets[i] for i in order], DEV)
    ev.evaluate()
    ev.write_results_json(r_path)
    ev2 = CO.evaluate_results_file(a_path, r_path, DEV)
    assert ev2.tables() == ev.tables()
    assert np.array_equal(_bits(ev2.precision), _bits(ev.precision)) and np.array_equal(_bits(ev2.recall), _bits(ev.recall))
    assert np.array_equal(_bits(ev2.stats), _bits(ev.stats)) and ev2.per_class_ap == ev.per_class_ap
    # the image order does not change the class order's content here, and tools/coco_eval.py prints the same lines
    tool = _load("tools/coco_eval")
    assert tool.main(["--annotations", a_path, "--results", r_path]).summarize() == ev.summarize()


# ------------------------------------------------------------------------------------------------------------ limits --
def test_limits_and_rejected_ingest():
    from squeezedet_amd import coco as CO
    from squeezedet_amd._lib import SqdetError, SqdetUnsupported
    obj = (0, 0, 0, 10, 10, 100, 0, 0)
    with pytest.raises(SqdetUnsupported, match="129 objects"):
        CO.CocoGroundTruth([[obj] * 129])
    gt = CO.CocoGroundTruth([[obj] * 128, [obj]])                        # 128 is inside the limit
    with pytest.raises(SqdetUnsupported, match="129 classes"):
        CO.CocoEvaluator(None, gt, DEV, max_detections=8, classes=129)
    ev = CO.CocoEvaluator(None, gt, DEV, max_detections=8, classes=128)
    ev.load_rows([[(0, 0, 0, 10, 10, .9)], [(127, 0, 0, 10, 10, .8)]])
    good = ev.evaluate().copy()
    assert ev.npig[0].tolist() == [129, 129, 0, 0] and ev.precision[0, 0, 0, 0, 2] == CC.P1 and np.all(ev.precision[:, :, 127] == -1)
    before = (ev.precision.copy(), ev.recall.copy(), ev.npig.copy(), ev.num_det.copy())
    ev.max_dets = np.array([1, 10, 129], np.int32)
    with pytest.raises(SqdetUnsupported, match="maxDets 129"):
        ev.evaluate()
    ev.max_dets = np.array([1, 10, 100], np.int32)
    # a class outside [0, classes) in the ingest: the call writes nothing, evaluate() raises, the last results stand
    table = [t.clone() for t in (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)]
    boxes, probs = torch.ones((2, 8, 4), device=DEV), torch.full((2, 8), 0.5, device=DEV)
    cls = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    cls[1, 0] = 128
    ev.add_rows(boxes, probs, cls, torch.tensor([1, 1], dtype=torch.int32, device=DEV), 0)
    with pytest.raises(SqdetError) as e:
        ev.evaluate()
    assert not isinstance(e.value, SqdetUnsupported)
    for a, b in zip(table, (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)):
        assert torch.equal(a, b)
    for a, b in zip(before, (ev.precision, ev.recall, ev.npig, ev.num_det)):
        assert np.array_equal(a, b)
    ev.reset()
    ev.load_rows([[(0, 0, 0, 10, 10, .9)], [(127, 0, 0, 10, 10, .8)]])
    assert np.array_equal(_bits(ev.evaluate()), _bits(good))


# ------------------------------------------------------------------------------------------------- eval.py end to end --
SIZES = [(128, 256), (120, 250), (128, 256), (96, 200), (128, 256), (128, 256)]
EVAL_ARGS = ["--dataset", "PASCAL_VOC", "--image_set", "trainval", "--run_once", "--image_size", "128", "256", "--batch_size", "4",
             "--synthetic_weights"]


def _voc_tree(root):
    """The six-image voc20-style tree of tests/test_gpu_voc_ap.py (the smallest configuration the eval tests run)."""
    from PIL import Image
    rs = np.random.RandomState(12)
    voc = os.path.join(root, "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(voc, d))
    idxs = ["%06d" % (i + 1) for i in range(len(SIZES))]
    for k, (idx, (h, w)) in enumerate(zip(idxs, SIZES)):
        im = rs.randint(90, 130, (h, w, 3)).astype(np.uint8)
        objects = []
        for _ in range(0 if k == 3 else rs.randint(1, 4)):
            x1, y1 = rs.randint(1, w - 70), rs.randint(1, h - 50)
            x2, y2 = x1 + rs.randint(20, 68), y1 + rs.randint(15, 48)
            c = rs.randint(20)
            im[y1 - 1:y2, x1 - 1:x2] = (40 + 10 * c, 250 - 10 * c, 30 + (c % 5) * 50)
            objects.append((VC.VOC20[c], x1, y1, x2, y2, int(rs.uniform() < 0.2)))
        Image.fromarray(im).save(os.path.join(voc, "JPEGImages", idx + ".jpg"), quality=92)
        with open(os.path.join(voc, "Annotations", idx + ".xml"), "w") as f:
            f.write(VC.annotation_xml(idx, objects))
    with open(os.path.join(voc, "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("".join(i + "\n" for i in idxs))
    return root


def test_eval_py_coco_metrics(tmp_path, capsys):
    """eval.py --coco_metrics on the VOC tree: the record gains "coco" and keeps the keys it has without the flag, the twelve
    lines are printed after the dataset's own, and coco_results.json scored again gives the record's numbers."""
    from squeezedet_amd import coco as CO, drivers, voc as V
    E = _load("eval")
    root = _voc_tree(str(tmp_path / "VOCdevkit"))
    out = str(tmp_path / "eval")
    rec = E.main(EVAL_ARGS + ["--data_path", root, "--eval_dir", out, "--coco_metrics"])
    text = capsys.readouterr().out
    assert sorted(rec) == sorted(["global_step", "checkpoint", "mAP", "APs", "num_det_per_image", "timing", "coco"])
    assert sorted(rec["APs"]) == sorted(VC.VOC20) and sorted(rec["timing"]) == ["eval", "im_detect", "post_proc"]
    with open(os.path.join(out, "eval_log.jsonl")) as f:
        logged = [json.loads(l) for l in f]
    assert len(logged) == 1 and logged[0]["coco"] == rec["coco"] and sorted(logged[0]) == sorted(rec)
    assert all(logged[0][k] == rec[k] for k in rec)
    coco = rec["coco"]
    assert sorted(coco) == ["per_class_ap", "stats"] and len(coco["stats"]) == 12 and sorted(coco["per_class_ap"]) == sorted(VC.VOC20)
    lines = [l for l in text.splitlines() if l.startswith(" Average ")]
    assert lines == CO.summary_lines(coco["stats"]) and text.index("Mean AP = ") < text.index(lines[0])
    assert sorted(os.listdir(os.path.join(out, "detection_files_0"))) == sorted([c + ".txt" for c in VC.VOC20] + ["coco_results.json"])
    # the results file, scored against the same ground truth from its own rows
    with open(os.path.join(out, "detection_files_0", "coco_results.json")) as f:
        res = json.load(f)
    assert len(res) == int(round(rec["num_det_per_image"] * len(SIZES))) > 0 and sorted(res[0]) == ["bbox", "category_id", "image_id", "score"]
    mc = drivers.make_config("squeezeDet", [128, 256], "PASCAL_VOC")
    gt = CO.CocoGroundTruth.from_voc(V.load_voc(root, "2007", "trainval", mc).gt, mc.CLASS_NAMES)
    rows = [[] for _ in SIZES]
    for r in res:
        rows[r["image_id"]].append((r["category_id"],) + tuple(r["bbox"]) + (r["score"],))
    ev = CO.CocoEvaluator.from_rows(mc, gt, rows, DEV)
    assert [float(v) for v in ev.evaluate()] == coco["stats"] and ev.per_class_ap == coco["per_class_ap"]
