"""The GPU KITTI evaluator (csrc/kitti_eval.hip, squeezedet_amd/kitti_ap.py) and eval.py on an MI355X.

Judged by the reference's own KITTI evaluator: live (oracle/_ref/evaluate_object, oracle/Makefile) where it was built,
otherwise through the stats files it wrote for the same detection files (tests/golden/kitti_ap.npz, make_kitti_ap_golden.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "oracle", "_ref", "evaluate_object")
DEV = "cuda:0"


def _reference_stats(name, root, result_dir, n, golden_dir):
    """{file: text} the reference evaluator writes for the case's detection files."""
    from tests.golden import cases, kitti_ap_cases as KC
    if os.path.exists(TOOL):
        ref_dir = os.path.join(root, "ref_result")
        os.makedirs(ref_dir)
        os.symlink(os.path.join(result_dir, "data"), os.path.join(ref_dir, "data"))
        subprocess.run([TOOL, os.path.join(root, "training"), os.path.join(root, "ImageSets", "val.txt"), ref_dir, str(n)],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True, timeout=120)
        return KC.stats_files(ref_dir)
    g = np.load(os.path.join(golden_dir, "kitti_ap.npz"))
    assert cases.kitti_detection_digest(os.path.join(result_dir, "data")) == str(g[name + "_detections_sha256"])
    return {str(fn): str(g["%s:%s" % (name, fn)]) for fn in g[name + "_files"]}


@pytest.mark.parametrize("name", ["mixed", "all", "few", "large", "wave"])
def test_stats_files_byte_identical_to_reference(name, tmp_path, golden_dir):
    from squeezedet_amd import kitti_ap as KA
    from tests.golden import kitti_ap_cases as KC
    root = str(tmp_path)
    idxs, result_dir = KC.make_case(name, root)
    aps, names = KA.evaluate_detection_files(root, "val", result_dir)
    ours = KC.stats_files(result_dir)
    ref = _reference_stats(name, root, result_dir, len(idxs), golden_dir)
    assert sorted(ours) == sorted(ref)
    for fn in ref:
        assert ours[fn] == ref[fn], (fn, ours[fn], ref[fn])
    # (aps, names) as kitti_eval.evaluate_detections reads them from the AP files
    exp = []
    for c in KC.CLASSES:
        t = ref.get("stats_%s_ap.txt" % c)
        exp += [float(l.split("=")[1]) for l in t.splitlines()] if t else [0.0, 0.0, 0.0]
    assert aps == exp and names[:3] == ["car_easy", "car_medium", "car_hard"]
    if name == "mixed":
        assert "stats_cyclist_ap.txt" not in ours          # a class never detected: no files, AP 0


# ---------------------------------------------------------------- ingest of real filter rows
def _filter_rows(n, seed):
    """filter_prediction_batch rows (device) of n seeded detector-like images at the 1248x384 input."""
    from squeezedet_amd import ops
    from tests.golden import cases
    rs = np.random.RandomState(seed)
    boxes, probs, cls = [], [], []
    for i in range(n):
        b, p, c, _ = cases.make_filter_case(["clustered2", "uniform0", "clustered3"][i % 3])
        boxes.append(b + rs.normal(0, 0.5, b.shape).astype(np.float32))
        probs.append(p)
        cls.append(c)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.stack(a), dtype=dt)).to(DEV)
    return ops.filter_prediction(t(boxes, np.float32), t(probs, np.float32), t(cls, np.int64), 3, 64, 0.4, 0.005)


def _tree_from_rows(root, rows_host, scales, seed=3):
    """A label tree whose objects sit near some of the (rescaled) detections, so the APs are far from 0."""
    rs = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "training", "label_2"))
    os.makedirs(os.path.join(root, "ImageSets"))
    idxs = ["%06d" % i for i in range(len(rows_host))]
    names = ("Car", "Pedestrian", "Cyclist")
    for idx, (b, c, n), (sx, sy) in zip(idxs, rows_host, scales):
        with open(os.path.join(root, "training", "label_2", idx + ".txt"), "w") as f:
            for j in range(0, n, 3):
                cx, cy, w, h = b[j, 0] / sx, b[j, 1] / sy, b[j, 2] / sx, b[j, 3] / sy
                x1, y1 = max(0.0, cx - w / 2 + rs.normal(0, 2)), max(0.0, cy - h / 2 + rs.normal(0, 2))
                f.write("%s 0.00 %d -1.50 %.2f %.2f %.2f %.2f 1.5 1.6 3.9 1.0 1.7 20.0 -1.5\n"
                        % (names[c[j]], rs.randint(0, 2), x1, y1, x1 + w, y1 + h))
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join(idxs) + "\n")
    return idxs


def test_ingest_matches_written_detection_files(tmp_path):
    """add_rows with scales != 1 == add_detections + write_detection_files read back; same stats either way."""
    from squeezedet_amd import config, kitti_ap as KA, kitti_eval as K
    n = 12
    ob, op, oc, oi, cnt = _filter_rows(n, 0)
    scales = [(1248 / 1242.0, 384 / 375.0), (1248 / 1224.0, 384 / 370.0), (0.731, 1.377)] * (n // 3)
    hb, hp, hc, hn = ob.cpu().numpy(), op.cpu().numpy(), oc.cpu().numpy(), cnt.cpu().numpy()
    root = str(tmp_path / "KITTI")
    idxs = _tree_from_rows(root, [(hb[i], hc[i], int(hn[i])) for i in range(n)], scales)
    mc = config.kitti_squeezeDet_config()
    data = KA.load_kitti(root, "val", mc)
    ev = KA.KittiEvaluator(mc, data.gt, DEV)
    ev.add_rows(ob[:5], op[:5], oc[:5], cnt[:5], 0, scales[:5])
    ev.add_rows(ob[5:], op[5:], oc[5:], cnt[5:], 5, scales[5:])
    # the host path: add_detections (float64, the scale) -> write_detection_files -> the evaluator's parser
    ab = K.new_all_boxes(3, n)
    for i in range(n):
        k = int(hn[i])
        K.add_detections(ab, i, hb[i, :k], hp[i, :k], hc[i, :k], scale=scales[i])
    res = str(tmp_path / "host")
    K.write_detection_files(os.path.join(res, "data"), idxs, KA.CLASS_NAMES, ab)
    want = [KA.parse_detection_file(os.path.join(res, "data", i + ".txt")) for i in idxs]
    got = ev.tables()
    assert sum(len(r) for r in got) > 100
    for i in range(n):
        assert got[i] == want[i], i                               # bit-exact doubles, file order
    ours = str(tmp_path / "ours")
    ev.write_detection_files(os.path.join(ours, "data"), idxs)
    for i in idxs:
        assert open(os.path.join(ours, "data", i + ".txt")).read() == open(os.path.join(res, "data", i + ".txt")).read()
    aps, names, prec = ev.evaluate()
    ev.write_stats(ours)
    aps2, _ = KA.evaluate_detection_files(root, "val", res)
    assert aps == aps2 and max(aps) > 0.2, aps
    from tests.golden import kitti_ap_cases as KC
    assert KC.stats_files(ours) == KC.stats_files(res)
    if os.path.exists(TOOL):
        assert KC.stats_files(ours) == _reference_stats("", root, res, n, None)


def test_quantiser_matches_python_formatting():
    """>= 1e5 coordinates (and scores) through ingest against float('%.2f' % v) / float('%.3f' % s), with exact decimal ties
    (k / 8) and products that land on a tie only after rounding (v = (k + 0.5) / 100 * scale, divided by the scale)."""
    from squeezedet_amd import config, kitti_ap as KA
    rs = np.random.RandomState(11)
    n, m = 420, 64
    b = np.empty((n, m, 4), np.float32)
    b[:, :, 0] = rs.uniform(-50, 1300, (n, m))
    b[:, :, 1] = rs.uniform(-50, 400, (n, m))
    b[:, :, 2] = rs.uniform(0, 300, (n, m))
    b[:, :, 3] = rs.uniform(0, 200, (n, m))
    scales = np.stack([rs.uniform(0.5, 2.0, n), rs.uniform(0.5, 2.0, n)], 1)
    scales[:60] = 1.0
    ties = np.float32(rs.randint(0, 8000, (60, m)) / 8.0)          # exact binary .x25 / .x75 ties at two decimals
    b[:60, :, 0], b[:60, :, 2] = ties, 0.0
    k = rs.randint(0, 100000, (60, m))                               # near ties after the division by the scale
    b[60:120, :, 0] = (((k + 0.5) / 100.0) * scales[60:120, :1]).astype(np.float32)
    b[60:120, :, 2] = 0.0
    p = rs.uniform(0, 1, (n, m)).astype(np.float32)
    p[:, :8] = (rs.randint(0, 8000, (n, 8)) / 8000.0).astype(np.float32)
    cls = np.sort(rs.randint(0, 3, (n, m)), axis=1).astype(np.int32)
    cnt = np.full(n, m, np.int32)
    mc = config.kitti_squeezeDet_config()
    gt = KA.GroundTruth([[] for _ in range(n)], [[] for _ in range(n)])
    ev = KA.KittiEvaluator(mc, gt, DEV)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ev.add_rows(T(b), T(p), T(cls), T(cnt), 0, scales)
    box, score = ev.det_box.cpu().numpy(), ev.det_score.cpu().numpy()
    bd = b.astype(np.float64)
    cx, w = bd[:, :, 0] / scales[:, :1], bd[:, :, 2] / scales[:, :1]
    cy, h = bd[:, :, 1] / scales[:, 1:], bd[:, :, 3] / scales[:, 1:]
    exp = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 2)
    q2 = np.vectorize(lambda v: float("%.2f" % v))
    q3 = np.vectorize(lambda v: float("%.3f" % v))
    e2, e3 = q2(exp), q3(p.astype(np.float64))
    assert exp.size >= 100000
    assert np.array_equal(box.view(np.int64), e2.view(np.int64)), np.argwhere(box != e2)[:5]
    assert np.array_equal(score.view(np.int64), e3.view(np.int64))


# ---------------------------------------------------------------- analysis
def _analyze_numpy(rois, dets, image_idx, classes):
    """kitti.analyze_detections restated: dets per image [(cls, x1, y1, x2, y2, score)] in file order."""
    from squeezedet_amd.util import bbox_transform_inv
    c = dict(dets=0, objs=0, correct=0, loc=0, cls=0, bg=0, rep=0, detected=0)
    recs = []
    for i, idx in enumerate(image_idx):
        gt = np.array(rois[i], np.float64).reshape(-1, 5)
        c["objs"] += len(gt)
        det = sorted([bbox_transform_inv(d[1:5]) + [d[0], d[5]] for d in dets[i]], key=lambda x: x[-1], reverse=True)
        if len(gt) < 1:
            continue
        seen = [False] * len(gt)
        for j, d in enumerate(det[:len(gt)]):
            c["dets"] += 1
            g = gt[:, :4]
            lr = np.maximum(np.minimum(g[:, 0] + 0.5 * g[:, 2], d[0] + 0.5 * d[2]) - np.maximum(g[:, 0] - 0.5 * g[:, 2], d[0] - 0.5 * d[2]), 0)
            tb = np.maximum(np.minimum(g[:, 1] + 0.5 * g[:, 3], d[1] + 0.5 * d[3]) - np.maximum(g[:, 1] - 0.5 * g[:, 3], d[1] - 0.5 * d[3]), 0)
            inter = lr * tb
            iou = inter / (g[:, 2] * g[:, 3] + d[2] * d[3] - inter)
            k = int(np.argmax(iou))
            if iou[k] > 0.1:
                if gt[k, 4] == d[4]:
                    if iou[k] >= 0.5:
                        if not seen[k]:
                            c["correct"] += 1
                            seen[k] = True
                        else:
                            c["rep"] += 1
                    else:
                        c["loc"] += 1
                        recs.append((i, "loc") + tuple(d[:4]) + (int(d[4]), d[5]))
                else:
                    c["cls"] += 1
                    recs.append((i, "cls") + tuple(d[:4]) + (int(d[4]), d[5]))
            else:
                c["bg"] += 1
                recs.append((i, "bg") + tuple(d[:4]) + (int(d[4]), d[5]))
        for k in range(len(gt)):
            if not seen[k]:
                recs.append((i, "missed") + tuple(gt[k, :4]) + (int(gt[k, 4]), -1.0))
        c["detected"] += sum(seen)
    return c, recs


@pytest.mark.parametrize("name,exclude_hard", [("all", False), ("mixed", True)])
def test_analysis_matches_numpy_restatement(name, exclude_hard, tmp_path):
    from squeezedet_amd import config, kitti_ap as KA
    from tests.golden import kitti_ap_cases as KC
    root = str(tmp_path)
    idxs, result_dir = KC.make_case(name, root)
    mc = config.kitti_squeezeDet_config()
    mc.EXCLUDE_HARD_EXAMPLES = exclude_hard
    data = KA.load_kitti(root, "val", mc)
    dets = [KA.parse_detection_file(os.path.join(result_dir, "data", i + ".txt")) for i in idxs]
    ev = KA.KittiEvaluator(mc, data.gt, DEV, max_detections=max(len(d) for d in dets))
    ev.load_rows(dets)
    st = ev.analyze()
    c, recs = _analyze_numpy(data.rois, dets, idxs, mc.CLASS_NAMES)
    assert list(ev.counters) == [c[k] for k in ("dets", "objs", "correct", "loc", "cls", "bg", "rep", "detected")]
    assert c["correct"] > 0 and c["loc"] + c["cls"] + c["bg"] > 0
    assert st["% recall"] == c["detected"] / float(c["objs"])
    assert ev.error_records() == recs
    path = str(tmp_path / "err" / "det_error_file.txt")
    ev.write_error_file(path, idxs)
    lines = open(path).read().splitlines()
    assert len(lines) == len(recs) and lines[0].startswith(idxs[recs[0][0]] + " " + recs[0][1] + " ")


# ---------------------------------------------------------------- determinism, limits
def test_deterministic_and_reset(tmp_path):
    from squeezedet_amd import config, kitti_ap as KA
    n = 30
    ob, op, oc, oi, cnt = _filter_rows(n, 5)
    hb, hc, hn = ob.cpu().numpy(), oc.cpu().numpy(), cnt.cpu().numpy()
    scales = [(1.0, 1.0)] * n
    root = str(tmp_path / "KITTI")
    _tree_from_rows(root, [(hb[i], hc[i], int(hn[i])) for i in range(n)], scales, seed=9)
    mc = config.kitti_squeezeDet_config()
    ev = KA.KittiEvaluator(mc, KA.load_kitti(root, "val", mc).gt, DEV)
    ev.add_rows(ob, op, oc, cnt, 0)
    r1 = ev.evaluate()
    a1 = ev.analyze()
    r2 = ev.evaluate()
    assert r1[0] == r2[0] and np.array_equal(r1[2].view(np.int64), r2[2].view(np.int64))
    ev.reset()
    r0 = ev.evaluate()
    assert r0[0] == [0.0] * 9                                     # an empty table: nothing detected
    ev.add_rows(ob, op, oc, cnt, 0)
    r3 = ev.evaluate()
    assert r1[0] == r3[0] and np.array_equal(r1[2].view(np.int64), r3[2].view(np.int64)) and ev.analyze() == a1
    assert max(r1[0]) > 0


def test_limits_and_negative_counts_raise_and_leave_outputs(tmp_path):
    from squeezedet_amd import config, kitti_ap as KA
    from squeezedet_amd._lib import SqdetError, SqdetUnsupported
    mc = config.kitti_squeezeDet_config()
    n = 6
    ob, op, oc, oi, cnt = _filter_rows(n, 7)
    gt = KA.GroundTruth([[(0, 10.0, 10.0, 100.0, 100.0, 0.0, 0)]] * n, [[[55.5, 55.5, 91.0, 91.0, 0]]] * n)
    with pytest.raises(SqdetUnsupported):
        KA.KittiEvaluator(mc, gt, DEV, max_detections=513)
    with pytest.raises(SqdetUnsupported):
        KA.GroundTruth([[(0, 10.0, 10.0, 100.0, 100.0, 0.0, 0)] * 129], [[]])
    small = KA.KittiEvaluator(mc, gt, DEV, max_detections=32)
    with pytest.raises(SqdetUnsupported):                       # 64 filter rows into a table of 32
        small.add_rows(ob, op, oc, cnt, 0)
    ev = KA.KittiEvaluator(mc, gt, DEV)
    with pytest.raises(SqdetError):                             # images past the table
        ev.add_rows(ob, op, oc, cnt, 1)
    ev.add_rows(ob[:3], op[:3], oc[:3], cnt[:3], 0)
    good = ev.evaluate()
    before = [t.clone() for t in (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)]
    bad = cnt[3:].clone()
    bad[1] = -70                                                # the filter's overflow report
    ev.add_rows(ob[3:], op[3:], oc[3:], bad, 3)
    with pytest.raises(SqdetError, match="rejected ingest"):
        ev.evaluate()
    for a, b in zip(before, (ev.det_box, ev.det_score, ev.det_cls, ev.det_count)):
        assert torch.equal(a, b)                                # nothing of the bad call was written
    assert np.array_equal(ev.precision, good[2])                # the last results stand
    with pytest.raises(SqdetError):
        ev.analyze()
    ev.reset()
    ev.add_rows(ob[:3], op[:3], oc[:3], cnt[:3], 0)
    assert ev.evaluate()[0] == good[0]


# ---------------------------------------------------------------- eval.py end to end
def _png_tree(root, n, seed=1):
    from PIL import Image
    rs = np.random.RandomState(seed)
    for d in ("training/image_2", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    idxs = ["%06d" % i for i in range(n)]
    for k, idx in enumerate(idxs):
        h, w = [(120, 400), (96, 320), (125, 410)][k % 3]
        im = (rs.uniform(0, 255, (h, w, 3))).astype(np.uint8)
        Image.fromarray(im).save(os.path.join(root, "training", "image_2", idx + ".png"))
        with open(os.path.join(root, "training", "label_2", idx + ".txt"), "w") as f:
            for _ in range(rs.randint(0, 4)):
                x1, y1 = rs.uniform(0, w - 60), rs.uniform(0, h - 40)
                f.write("%s 0.00 0 -1.5 %.2f %.2f %.2f %.2f 1.5 1.6 3.9 1.0 1.7 20.0 -1.5\n"
                        % (["Car", "Pedestrian", "Cyclist"][rs.randint(3)], x1, y1, x1 + rs.uniform(20, 60), y1 + rs.uniform(25, 40)))
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join(idxs) + "\n")
    return idxs


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_eval_py_run_once(dtype, tmp_path):
    """40 images at batch 12 (a partial last batch of 4), synthetic weights: eval.py's detection files equal a per-image
    loop in the reference's order (rescale on the host in float32 -> filter_prediction -> add_detections) over the same
    forward outputs, and its stats files equal the reference evaluator's on them."""
    sys.path.insert(0, ROOT)
    import eval as E
    from squeezedet_amd import kitti_ap as KA, kitti_eval as K
    from tests.golden import kitti_ap_cases as KC
    root = str(tmp_path / "KITTI")
    idxs = _png_tree(root, 40)
    out = str(tmp_path / "eval")
    rec = E.main(["--data_path", root, "--image_set", "val", "--eval_dir", out, "--run_once", "--synthetic_weights",
                  "--batch_size", "12", "--dtype", dtype])
    res = os.path.join(out, "detection_files_0")
    assert os.path.exists(os.path.join(out, "eval_log.jsonl")) and rec["num_det_per_image"] > 0
    assert os.path.exists(os.path.join(res, "error_analysis", "det_error_file.txt"))
    # the reference order, one image at a time, over the same forward outputs
    mc, model = E.make_model("squeezeDet", "0", dtype, 12)
    from squeezedet_amd import synthetic
    model.load_params(synthetic.synthetic_params(model, seed=0))
    data = KA.load_kitti(root, "val", mc)
    ab = K.new_all_boxes(3, len(idxs))
    for i0 in range(0, len(idxs), 12):
        db, dp, dc, scales = E.detect_batch(model, data.image_paths[i0:i0 + 12])
        db, dp, dc = db.cpu().numpy(), dp.cpu().numpy(), dc.cpu().numpy()
        for j, s in enumerate(scales):
            b = db[j].copy()
            b[:, 0::2] /= np.float32(s[0])
            b[:, 1::2] /= np.float32(s[1])
            fb, fp, fc = model.filter_prediction(b, dp[j], dc[j])
            K.add_detections(ab, i0 + j, fb, fp, fc)
    ref = str(tmp_path / "ref")
    K.write_detection_files(os.path.join(ref, "data"), idxs, KA.CLASS_NAMES, ab)
    for i in idxs:
        assert open(os.path.join(res, "data", i + ".txt")).read() == open(os.path.join(ref, "data", i + ".txt")).read(), i
    if os.path.exists(TOOL):
        exp = _reference_stats("", root, res, len(idxs), None)
    else:
        KA.evaluate_detection_files(root, "val", ref)
        exp = KC.stats_files(ref)
    assert KC.stats_files(res) == exp and exp
