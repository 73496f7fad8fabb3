"""The GPU Pascal VOC evaluator (csrc/voc_eval.hip, squeezedet_amd/voc.py) and the drivers' PASCAL_VOC path on an MI355X.

Judged by the reference's own pascal_voc.evaluate_detections / voc_eval through tests/golden/voc_ap.npz
(make_voc_ap_golden.py): recall, precision and the 11-point AP bitwise, the area AP within 1e-12.  That bound is derived:
the reference sums the area terms with NumPy's pairwise order, the kernel in a fixed order of its own; reordering a sum of
at most n non-negative terms that total at most 1 moves it by at most n * 2^-53, and the cases have n <= 4096
(4096 * 2^-53 = 4.5e-13).  Where both curves hold a NaN (recall of a class without objects, 0 / 0) the payload bits are
not compared: x86 and the GPU produce default NaNs of opposite sign."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests.golden import voc_ap_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
AREA_TOL = 1e-12


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _mc(names):
    import squeezedet_amd as S
    mc = S.base_model_config("PASCAL_VOC")
    mc.CLASS_NAMES = tuple(names)
    mc.CLASSES = len(names)
    return mc


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits_equal(a, b):
    """Bitwise, except that a NaN matches a NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.int64), b[ok].view(np.int64))


# ---------------------------------------------------------------- ingest
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scales"])
def test_ingest_is_the_detection_files_text(scaled):
    """Rows on rounding edges -- x + 1 = 12.25 (an exact tie at one decimal) and 12.35 in float32, scores 0.0005, 0.0015 and
    0.9995 in float32 -- and seeded ones, against float(format(...)) of NumPy's float32 arithmetic.  Bitwise."""
    from squeezedet_amd import voc as V
    rs = np.random.RandomState(5)
    n, m, C = 3, 70, 20
    b = np.empty((n, m, 4), np.float32)
    b[..., 0], b[..., 1] = rs.uniform(-20, 500, (n, m)), rs.uniform(-20, 375, (n, m))
    b[..., 2], b[..., 3] = rs.uniform(0, 300, (n, m)), rs.uniform(0, 200, (n, m))
    p = rs.uniform(0, 1, (n, m)).astype(np.float32)
    b[0, 0] = (11.25, 11.35, 0.0, 0.0)             # x1 = x2 = 11.25, y1 = y2 = float32(11.35)
    b[0, 1] = (12.0, 12.0, 1.5, 1.3)               # x1 + 1 = 12.25, x2 + 1 = 13.75
    b[0, 2] = (np.float32(11.35), 0.05, 0.0, 0.0)
    p[0, :3] = (0.0005, 0.0015, 0.9995)
    cls = rs.randint(0, C, (n, m)).astype(np.int32)
    cnt = np.array([m, 0, 37], np.int32)
    scales = [(1.0, 1.0), (0.731, 1.377), (256 / 500.0, 128 / 375.0)] if scaled else None
    gt = V.GroundTruth([[] for _ in range(n)])
    ev = V.VocEvaluator(_mc(VC.VOC20), gt, DEV, max_detections=m)
    ev.add_rows(_T(b), _T(p), _T(cls), _T(cnt), 0, scales)
    got = ev.tables()
    one, two = np.float32(1), np.float32(2)
    for i in range(n):
        sx, sy = (np.float32(scales[i][0]), np.float32(scales[i][1])) if scaled else (one, one)
        want = []
        for k in np.argsort(cls[i, :cnt[i]], kind="stable"):
            cx, cy, w, h = b[i, k, 0] / sx, b[i, k, 1] / sy, b[i, k, 2] / sx, b[i, k, 3] / sy
            box = [cx - w / two + one, cy - h / two + one, cx + w / two + one, cy + h / two + one]
            assert all(v.dtype == np.float32 for v in box)
            want.append((int(cls[i, k]),) + tuple(float("{:.1f}".format(v)) for v in box) + (float("{:.3f}".format(p[i, k])),))
        assert len(got[i]) == cnt[i]
        for g, w_ in zip(got[i], want):
            assert g[0] == w_[0] and _bits_equal(g[1:], w_[1:]), (i, g, w_)
    # image 0 (scale 1 either way): the exact tie 12.25 goes to even, float32(11.35) + 1 lies above 12.35
    assert (int(cls[0, 0]), 12.2, 12.4, 12.2, 12.4, 0.001) in got[0]
    assert any(r[0] == cls[0, 1] and r[1] == 12.2 and r[3] == 13.8 and r[5] == 0.002 for r in got[0])
    assert any(r[0] == cls[0, 2] and r[1] == 12.4 and r[5] == 0.999 for r in got[0])


# ---------------------------------------------------------------- every case, two routes
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "voc_ap.npz"))


@pytest.mark.parametrize("route", ["add_rows", "load_rows"])
@pytest.mark.parametrize("name", sorted(VC.CASES))
def test_case_matches_the_reference(name, route, golden, tmp_path):
    from squeezedet_amd import voc as V
    case = VC.make_case(name)
    mc = _mc(case["names"])
    VC.write_tree(case, str(tmp_path))
    data = V.load_voc(str(tmp_path), VC.YEAR, VC.IMAGE_SET, mc)
    boxes, probs, cls, count = VC.padded_rows(case)
    ev = V.VocEvaluator(mc, data.gt, DEV, max_detections=boxes.shape[1])
    if route == "add_rows":
        k = len(count) // 2                          # two calls: the second lands at an image offset (k = 0: an empty first call)
        ev.add_rows(_T(boxes[:k]), _T(probs[:k]), _T(cls[:k]), _T(count[:k]), 0)
        ev.add_rows(_T(boxes[k:]), _T(probs[k:]), _T(cls[k:]), _T(count[k:]), k)
    else:
        ev.load_rows(VC.table_rows(case))
    aps07, names = ev.evaluate(True)
    ap07, ap_area, npos, ndet = ev.ap07.copy(), ev.ap_area.copy(), ev.npos.copy(), ev.num_det.copy()
    aps_area, _ = ev.evaluate(False)
    assert tuple(names) == tuple(case["names"]) and aps07 == list(ap07) and _bits_equal(aps_area, ap_area)
    for c, cname in enumerate(case["names"]):
        key = "%s:%s:" % (name, cname)
        want_rec, want_prec = golden[key + "rec"], golden[key + "prec"]
        assert ndet[c] == len(want_rec) == int((cls[np.arange(cls.shape[1])[None, :] < count[:, None]] == c).sum())
        assert npos[c] == sum(1 for objs in case["objects"] for o in objs if o[0] == cname and not o[5])
        print(name, route, cname, "ap07", ap07[c], float(golden[key + "ap07"]), "ap_area", ap_area[c], float(golden[key + "ap_area"]))
        assert _bits_equal(ap07[c], golden[key + "ap07"]), (cname, ap07[c], float(golden[key + "ap07"]))
        want_area = float(golden[key + "ap_area"])
        assert (np.isnan(want_area) and np.isnan(ap_area[c])) or abs(ap_area[c] - want_area) <= AREA_TOL, (cname, ap_area[c], want_area)
        if ndet[c] == 0:
            assert ap07[c] == 0.0 and ap_area[c] == 0.0
            continue
        rec, prec = ev.curve(c)
        assert _bits_equal(rec, want_rec), (cname, rec, want_rec)
        assert _bits_equal(prec, want_prec), (cname, prec, want_prec)
    assert _bits_equal(ev.ap07, ap07) and _bits_equal(ev.ap_area, ap_area)      # curve() evaluated again: the same


def test_tie_rule_image_then_row():
    """Four rows of one score, one class, two images with one object each: image 0 holds (background, hit), image 1
    (hit, background).  Ours: image, then row -> fp, tp, tp, fp.  (Hits first would give AP 1; the reference leaves the
    order of equal scores to an unstable argsort.)"""
    from squeezedet_amd import voc as V
    hit, bg = VC.at(20, 20, 80, 80), VC.at(200, 200, 240, 240)
    gt = V.GroundTruth([[(0, 20, 20, 80, 80, 0)], [(0, 20, 20, 80, 80, 0)]])
    ev = V.VocEvaluator(_mc(("cat",)), gt, DEV, max_detections=2)
    rows = [[(0, 200.0, 200.0, 240.0, 240.0, 0.5), (0, 20.0, 20.0, 80.0, 80.0, 0.5)],
            [(0, 20.0, 20.0, 80.0, 80.0, 0.5), (0, 200.0, 200.0, 240.0, 240.0, 0.5)]]
    ev.load_rows(rows)
    rec, prec = ev.curve(0)
    assert rec.tolist() == [0.0, 0.5, 1.0, 1.0]
    assert prec.tolist() == [0.0, 0.5, 2 / 3.0, 0.5]
    ap = 0.
    for _ in range(11):                                             # every threshold sees max precision 2/3
        ap = ap + (2 / 3.0) / 11.
    assert ev.ap07[0] == ap and abs(ev.ap_area[0] - 2 / 3.0) <= AREA_TOL
    assert ev.npos[0] == 2 and ev.num_det[0] == 4
    # the same rows through the ingest
    b = np.array([[bg, hit], [hit, bg]], np.float32)
    ev.reset()
    ev.add_rows(_T(b), _T(np.full((2, 2), 0.5, np.float32)), _T(np.zeros((2, 2), np.int32)), _T(np.full(2, 2, np.int32)), 0)
    assert ev.tables() == rows
    rec2, prec2 = ev.curve(0)
    assert rec2.tolist() == rec.tolist() and prec2.tolist() == prec.tolist()


# ---------------------------------------------------------------- failure paths (argument and count checks: nothing can fault)
def test_limits_and_rejected_ingest():
    from squeezedet_amd import voc as V
    from squeezedet_amd._lib import SqdetError, SqdetUnsupported
    case = VC.make_case("greedy")
    mc = _mc(case["names"])
    gt = V.GroundTruth([[(case["names"].index(o[0]),) + tuple(o[1:]) for o in objs] for objs in case["objects"]])
    with pytest.raises(SqdetUnsupported):
        V.VocEvaluator(mc, gt, DEV, max_detections=513)
    with pytest.raises(SqdetUnsupported):
        V.VocEvaluator(_mc(["c%d" % i for i in range(65)]), gt, DEV)
    boxes, probs, cls, count = VC.padded_rows(case)
    ev = V.VocEvaluator(mc, gt, DEV, max_detections=8)
    with pytest.raises(SqdetUnsupported):                        # 16 filter rows into a table of 8
        ev.add_rows(_T(np.zeros((4, 16, 4), np.float32)), _T(np.zeros((4, 16), np.float32)), _T(np.zeros((4, 16), np.int32)),
                    _T(np.zeros(4, np.int32)), 0)
    with pytest.raises(SqdetError):                              # images past the table
        ev.add_rows(_T(boxes), _T(probs), _T(cls), _T(count), 1)
    ev.add_rows(_T(boxes), _T(probs), _T(cls), _T(count), 0)
    good, _ = ev.evaluate(True)
    good_area = ev.ap_area.copy()
    assert good[0] > 0
    # an image over the row limit (the count is on the device): SQDET_EUNSUPPORTED, the last results stand
    saved = ev.det_count.clone()
    ev.det_count[1] = 9
    with pytest.raises(SqdetUnsupported, match="more than 128 ground-truth or 8 detection rows"):
        ev.evaluate(True)
    assert list(ev.ap07) == good and np.array_equal(ev.ap_area, good_area)
    ev.det_count.copy_(saved)
    assert ev.evaluate(True)[0] == good
    # a class index out of range at ingest: nothing is written, evaluate fails until reset
    before = [t.clone() for t in (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)]
    bad = cls.copy()
    bad[0, 1] = len(case["names"])
    ev.add_rows(_T(boxes), _T(probs), _T(bad), _T(count), 0)
    for a, b in zip(before, (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)):
        assert torch.equal(a, b)
    with pytest.raises(SqdetError, match="rejected ingest"):
        ev.evaluate(True)
    neg = count.copy()
    neg[2] = -3                                                  # the filter's overflow report
    ev.reset()
    ev.add_rows(_T(boxes), _T(probs), _T(cls), _T(neg), 0)
    with pytest.raises(SqdetError, match="rejected ingest"):
        ev.evaluate(True)
    assert list(ev.ap07) == good
    ev.reset()
    assert ev.evaluate(True)[0] == [0.0, 0.0] and list(ev.num_det) == [0, 0]   # empty: no detections, AP 0
    ev.add_rows(_T(boxes), _T(probs), _T(cls), _T(count), 0)
    assert ev.evaluate(True)[0] == good


# ---------------------------------------------------------------- the drivers end to end
SIZES = [(128, 256), (120, 250), (128, 256), (96, 200), (128, 256), (128, 256)]


@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    """A voc20-style tree: six JPEGs written by PIL (not all of one size) with a filled rectangle planted where each
    object's box is, their XML files, and the image set 'trainval'."""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("VOCdevkit"))
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


EVAL_ARGS = ["--dataset", "PASCAL_VOC", "--image_set", "trainval", "--run_once", "--image_size", "128", "256", "--batch_size", "4"]


def _printed_aps(text):
    per = re.findall(r"^(\w+): AP = (\d\.\d{4})$", text, flags=re.M)
    mean = re.findall(r"^Mean AP = (\S+)$", text, flags=re.M)
    return per, mean


def test_eval_py_pascal_voc_run_once(voc_tree, tmp_path, capsys):
    """eval.py --dataset PASCAL_VOC --synthetic_weights: it runs, prints pascal_voc.py:134-136's lines, and its numbers are
    those of a VocEvaluator fed the same rows and of evaluate_detection_files on the files it wrote.  The net's ConvDet head
    is padded to 23 classes (config.pad_head_classes: 225 channels are not a multiple of 4); no row may carry a padding
    class -- the ingest would reject it and evaluate() raise."""
    from squeezedet_amd import voc as V
    E = _load("eval")
    out = str(tmp_path / "eval")
    rec = E.main(EVAL_ARGS + ["--data_path", voc_tree, "--eval_dir", out, "--synthetic_weights"])
    text = capsys.readouterr().out
    det_dir = os.path.join(out, "detection_files_0")
    assert sorted(os.listdir(det_dir)) == sorted(c + ".txt" for c in VC.VOC20)
    assert rec["num_det_per_image"] > 0 and os.path.exists(os.path.join(out, "eval_log.jsonl"))
    assert not os.path.exists(os.path.join(det_dir, "error_analysis"))
    # the same rows into a second table
    a = E.parse_args(EVAL_ARGS + ["--data_path", voc_tree, "--eval_dir", out, "--synthetic_weights"])
    mc, model = E.make_model(a.net, a.gpu, a.dtype, a.batch_size, None, a.image_size, a.dataset)
    assert tuple(mc.CLASS_NAMES) == VC.VOC20 and (mc.CLASSES, mc.HEAD_PAD_CLASSES) == (23, 3)
    data = V.load_voc(voc_tree, "2007", "trainval", mc)
    ev = V.VocEvaluator(mc, data.gt, model.device)
    E.load_weights(a, model, "")
    E.detect_all(model, data, ev)
    aps, names = ev.evaluate(True)
    assert [rec["APs"][c] for c in names] == aps and rec["mAP"] == float(np.mean(aps)) and len(aps) == 20
    # the padding classes have probability exactly 0: no detection is of one, the real classes' probabilities sum to 1
    x, _ = E.read_image(data.image_paths[0], model)
    probs = model.run([model.pred_class_probs], {model.image_input: x.expand(mc.BATCH_SIZE, -1, -1, -1).contiguous()})[0]
    assert float(probs[..., 20:].abs().max()) == 0.0 and float((probs[..., :20].sum(-1) - 1).abs().max()) < 1e-5
    assert int(ev.det_cls.max()) < 20
    per, mean = _printed_aps(text)
    assert per == [(c, "{:.4f}".format(v)) for c, v in zip(names, aps)]
    assert mean == ["{:.4f}".format(np.mean(aps))]
    # the files it wrote, scored from disk: bitwise the same
    aps_files, names_files = V.evaluate_detection_files(voc_tree, "2007", "trainval", det_dir, mc)
    assert aps_files == aps and tuple(names_files) == tuple(names)
    assert sum(len(V.parse_detection_file(os.path.join(det_dir, c + ".txt"))) for c in names) == int(ev.num_det.sum()) > 0


def test_train_py_pascal_voc_writes_a_checkpoint_eval_py_loads(voc_tree, tmp_path, capsys):
    """train.py --dataset PASCAL_VOC for two steps on the tree, then eval.py on the checkpoint it wrote.  The padded head's
    padding channels receive a zero gradient: after the two steps they are still pinned, bit for bit, and the real ones
    have moved."""
    T, E = _load("train"), _load("eval")
    train_dir = str(tmp_path / "train")
    T.main(["--dataset", "PASCAL_VOC", "--data_path", voc_tree, "--image_set", "trainval", "--train_dir", train_dir,
            "--max_steps", "2", "--image_size", "128", "256", "--batch_size", "2"])
    ckpt = os.path.join(train_dir, "model.ckpt-1.npz")
    assert os.path.exists(ckpt) and os.path.exists(os.path.join(train_dir, "state", "step-1.npz"))
    from squeezedet_amd.config import PAD_CLASS_BIAS
    with np.load(ckpt) as z, np.load(os.path.join(train_dir, "model.ckpt-0.npz")) as z0:
        k, b, b0 = z["conv12/kernels"], z["conv12/biases"], z0["conv12/biases"]
    assert k.shape[-1] == b.shape[0] == 9 * (23 + 1 + 4)                     # 20 classes + 3 of padding
    pad = np.array([a * 23 + c for a in range(9) for c in (20, 21, 22)])
    real = np.setdiff1d(np.arange(b.shape[0]), pad)
    assert np.all(k[..., pad] == 0.0) and np.all(b[pad] == np.float32(PAD_CLASS_BIAS))
    assert np.all(k[..., real].any(axis=(0, 1, 2))) and np.any(b[real] != b0[real])
    capsys.readouterr()
    out = str(tmp_path / "eval")
    rec = E.main(EVAL_ARGS + ["--data_path", voc_tree, "--eval_dir", out, "--checkpoint_path", ckpt])
    text = capsys.readouterr().out
    assert rec["global_step"] == "1" and os.path.isdir(os.path.join(out, "detection_files_1"))
    per, mean = _printed_aps(text)
    assert [c for c, _ in per] == list(VC.VOC20) and len(mean) == 1
