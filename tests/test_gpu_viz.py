"""squeezedet_amd.viz on the GPU: the rasteriser and the item builder against NumPy / Python (tests/draw_reference.py), every
comparison exact, and the three drivers' new options end to end."""
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

from squeezedet_amd import drivers, ops, viz
from tests import draw_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGR_MEANS = (103.939, 116.779, 123.68)
SMALL = ["--image_size", "128", "256", "--batch_size", "2"]


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------ rasteriser --
def _random_items(rs, n, H, W):
    """n items: boxes inside, partly and wholly outside the image, corners in either order, both anchors, labels that run off
    every edge, a few bytes outside ASCII 32..126."""
    items = []
    for _ in range(n):
        kind = rs.randint(6)
        if kind == 0:        # wholly outside
            x0, y0 = (rs.randint(W + 1, W + 60), rs.randint(-50, H + 50)) if rs.randint(2) else (rs.randint(-50, W + 50), rs.randint(-90, -10))
            x1, y1 = x0 + rs.randint(0, 40), y0 + rs.randint(0, 8) - (0 if y0 > 0 else 1)
        elif kind == 1:      # hugging an edge, so that the label runs off it
            x0, y0 = rs.choice([-7, -1, 0, W - 9, W - 1]), rs.choice([-3, 0, 3, H - 4, H - 1])
            x1, y1 = x0 + rs.randint(0, 50), y0 + rs.randint(0, 30)
        else:
            xs, ys = rs.randint(-30, W + 30, size=2), rs.randint(-30, H + 30, size=2)
            x0, x1, y0, y1 = int(xs[0]), int(xs[1]), int(ys[0]), int(ys[1])
        ln = int(rs.choice([0, 1, 5, 13, 31]))
        lab = bytes(rs.randint(32, 127, size=ln).astype(np.uint8))
        if ln and rs.randint(4) == 0:
            lab = bytes([rs.choice([0, 7, 31, 127, 200, 255])]) + lab[1:]
        items.append((int(x0), int(y0), int(x1), int(y1), tuple(int(v) for v in rs.randint(0, 256, size=3)), lab,
                      ("bottom_left", "top_left")[rs.randint(2)]))
    return items


def _images(rs, kind, B, H, W):
    """(device tensor, the uint8 BGR pictures the kernel must restore)."""
    if kind == "u8":
        u8 = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
        return torch.from_numpy(u8).to(DEV), u8
    dt = np.float16 if kind == "fp16" else np.float32
    # a real network input (uint8 - means) with a share of values off the grid and outside [0, 255]: ties and the clamp
    x = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.float32) - np.asarray(BGR_MEANS, np.float32)
    off = rs.rand(B, H, W, 3) < 0.25
    x = np.where(off, x + rs.choice([-0.5, 0.5, -0.25, 0.75, -300.0, 300.0], size=x.shape).astype(np.float32), x).astype(dt)
    return torch.from_numpy(x).to(DEV), R.restore(x, BGR_MEANS)


CASES = [  # kind, order, H, W, B, item counts per image (cycled), tables
    ("fp32", "rgb", 384, 1248, 20, (12, 0, 3, 40), 1),
    ("fp16", "bgr", 384, 1248, 3, (30, 1, 0), 2),
    ("u8", "rgb", 384, 1248, 1, (256,), 1),
    ("u8", "bgr", 375, 1242, 3, (9, 0, 17), 1),
    ("fp32", "bgr", 375, 1242, 1, (256,), 1),
    ("fp16", "rgb", 375, 1242, 20, (5, 2), 2),
    ("fp16", "rgb", 37, 53, 20, (6, 0, 1, 20), 1),
    ("fp32", "rgb", 37, 53, 3, (1,), 1),
    ("u8", "bgr", 37, 53, 1, (0,), 1),
    ("u8", "rgb", 37, 53, 20, (256, 3), 1),
    ("fp32", "bgr", 37, 53, 1, (100,), 4),
]


@pytest.mark.parametrize("kind,order,H,W,B,counts,tables", CASES)
def test_draw_equals_the_restatement(kind, order, H, W, B, counts, tables):
    rs = np.random.RandomState(zlib.crc32(repr((kind, order, H, W, B, counts, tables)).encode()))
    x, u8 = _images(rs, kind, B, H, W)
    per_table = []
    for t in range(tables):
        share = [counts[i % len(counts)] // tables + (counts[i % len(counts)] % tables if t == 0 else 0) for i in range(B)]
        per_table.append([_random_items(rs, n, H, W) for n in share])
    dev_tables = [viz.pack_items(t, DEV) for t in per_table]
    got = viz.draw(x, dev_tables, bgr_means=None if kind == "u8" else BGR_MEANS, order=order)
    torch.cuda.synchronize()
    want = R.draw(u8, per_table, viz.font(), order)
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, "%d pixels differ, first (image, y, x) = %s: got %s want %s" % (
        len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    # the tables came back as they went in
    assert dev_tables[0].decode() == [[it[:5] + (it[5][:31], it[6]) for it in img] for img in per_table[0]]


def test_draw_uint8_in_place_and_item_limit():
    rs = np.random.RandomState(5)
    x, u8 = _images(rs, "u8", 2, 37, 53)
    items = [_random_items(rs, 7, 37, 53) for _ in range(2)]
    out = viz.draw(x, viz.pack_items(items, DEV), order="bgr", out=x)
    torch.cuda.synchronize()
    assert out.data_ptr() == x.data_ptr() and np.array_equal(x.cpu().numpy(), R.draw(u8, [items], viz.font(), "bgr"))
    from squeezedet_amd._lib import SqdetUnsupported
    with pytest.raises(SqdetUnsupported):
        viz.draw(x, viz.pack_items([[]] * 2, DEV, cap=257), order="bgr")
    with pytest.raises(SqdetUnsupported):
        viz.draw(x, [viz.pack_items([[]] * 2, DEV, cap=200), viz.pack_items([[]] * 2, DEV, cap=57)], order="bgr")


# ---------------------------------------------------------------------------------------------------------- item builder --
NAMES = ["car", "pedestrian", "cyclist"]


def test_item_builder_detections_against_python():
    """float32 filtered rows: int(bbox_transform(.)) in float32, the prob > plot_thresh cut, per-image counts and the label
    '%s: (%.2f)' for 10 240 seeded probabilities + the ties."""
    rs = np.random.RandomState(11)
    B, M, thresh = 40, 256, 0.4
    boxes = (rs.uniform(-200, 1400, size=(B, M, 4)) * rs.choice([1.0, 0.37, 1e-3], size=(B, M, 1))).astype(np.float32)
    boxes[0, :4] = [[10.5, 20.5, 21, 41], [-3.25, -7.75, 2.5, 3.5], [0.49, 0.51, 0.98, 1.02], [np.nan, 5, 1e20, -1e20]]
    probs = rs.uniform(0, 1, size=(B, M)).astype(np.float32)
    probs[1, :8] = [0.125, 0.375, 0.005, 0.995, 1.0, 0.4, np.float32(0.4) + np.float32(3e-8), 0.0]
    probs[2, :6] = [0.625, 0.875, 0.405, 0.415, 0.985, 0.999]
    cls = rs.randint(0, 3, size=(B, M)).astype(np.int32)
    cls[3, :3] = [-1, 3, 99]
    probs[3, :3] = 0.9
    counts = rs.randint(0, M + 1, size=B).astype(np.int32)
    counts[:4] = [M, M, M, 64]
    counts[5], counts[6] = 0, -3
    colours = [(255, 191, 0), (255, 0, 191), (0, 191, 255)]
    dev = lambda a: torch.from_numpy(a).to(DEV)
    for label, fmt, anchor in (("name: (p)", "%s: (%.2f)", "bottom_left"), ("name (p)", "%s (%.2f)", "top_left")):
        t = viz.make_items(dev(boxes), dev(cls), dev(counts), NAMES, probs=dev(probs), plot_thresh=thresh, class_colors=colours,
                           color=(1, 2, 3), label=label, anchor=anchor)
        got = t.decode()
        checked = 0
        for i in range(B):
            want = []
            for j in range(max(0, min(int(counts[i]), M))):
                if not float(probs[i, j]) > thresh:          # the reference's comparison: float32 against a Python float, in double
                    continue
                c = int(cls[i, j])
                known = 0 <= c < 3
                text = fmt % (NAMES[c] if known else "?", float(np.float32(probs[i, j])))
                want.append(R.box_item(boxes[i, j], colours[c] if known else (1, 2, 3), text, anchor))
            assert got[i] == want, (i, [(g, w) for g, w in zip(got[i], want) if g != w][:3], len(got[i]), len(want))
            checked += len(want)
        # (not vacuous: the inputs themselves say how many rows pass the cut and how many it drops)
        live = np.arange(M)[None, :] < np.clip(counts, 0, M)[:, None]
        passed = int((live & (probs.astype(np.float64) > thresh)).sum())
        assert checked == passed and passed > 1000 and int(live.sum()) - passed > 1000
    assert float(np.float32(0.995)) > 0.995 and "%.2f" % float(np.float32(0.995)) == "1.00"       # (what the tie rows pin)
    # all labels of 10 240 probabilities with nothing cut: threshold below every value
    t = viz.make_items(dev(boxes), dev(cls), dev(np.full(B, M, np.int32)), NAMES, probs=dev(probs), plot_thresh=-1.0, label="name: (p)")
    got = t.decode()
    n = 0
    for i in range(B):
        assert len(got[i]) == M
        for j in range(M):
            c = int(cls[i, j])
            want = ("%s: (%.2f)" % (NAMES[c] if 0 <= c < 3 else "?", float(np.float32(probs[i, j])))).encode()
            assert got[i][j][5] == want and got[i][j][4] == (0, 255, 0), (i, j, got[i][j], want)
            n += 1
    assert n >= 10000


def test_item_builder_ground_truth_and_diagonal():
    rs = np.random.RandomState(12)
    B, M = 6, 9
    gt = rs.uniform(-50, 1300, size=(B, M, 4)) * rs.choice([1.0, 0.01], size=(B, M, 1))
    gt[0, :3] = [[100.5, 50.5, 201.0, 101.0], [-10.75, -20.25, 3.5, 4.5], [0.3, 0.3, 0.6, 0.6]]
    cls = rs.randint(0, 3, size=(B, M)).astype(np.int32)
    counts = np.asarray([9, 0, 3, 9, 1, 12], np.int32)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    got = viz.make_items(dev(gt), dev(cls), dev(counts), NAMES, color=(0, 255, 0), label="name").decode()
    for i in range(B):
        want = [R.box_item(gt[i, j], (0, 255, 0), NAMES[cls[i, j]]) for j in range(min(int(counts[i]), M))]
        assert got[i] == want, i
    diag = np.concatenate([gt[..., :2] - gt[..., 2:] / 2, gt[..., :2] + gt[..., 2:] / 2], axis=-1)
    for arr in (diag, diag.astype(np.float32)):
        got = viz.make_items(dev(arr), dev(cls), dev(counts), NAMES, form="diagonal", label="name", anchor="top_left").decode()
        for i in range(B):
            want = [R.box_item(arr[i, j], (0, 255, 0), NAMES[cls[i, j]], "top_left", form="diagonal") for j in range(min(int(counts[i]), M))]
            assert got[i] == want, i
    # long names are cut at 31 bytes, the suffix with them
    long = ["x" * 40, "a-class-name-of-25-bytes!", "c"]
    probs = np.full((B, M), 0.75, np.float32)
    got = viz.make_items(dev(gt), dev(cls), dev(counts), long, probs=dev(probs), label="name: (p)").decode()
    for i in range(B):
        for j, it in enumerate(got[i]):
            assert it[5] == ("%s: (%.2f)" % (long[cls[i, j]][:31], 0.75)).encode()[:31]


# ------------------------------------------------------------------------------------------------------------- end to end --
def _train_args(T, train_dir, *more):
    return T.parse_args(["--synthetic", "8", "--seed", "3", "--train_dir", str(train_dir), "--max_steps", "3", "--summary_step", "1"]
                        + SMALL + list(more))


def _run_training(T, args, capture=None):
    os.makedirs(args.train_dir)
    run = T.Run(args)
    if capture is not None and run.images is not None:
        record = run.images.record

        def spy(step, batch, preds):
            n = run.images.max_images
            capture.append((step, batch.image_input[:n].clone(), batch.gt_boxes[:n].clone(), batch.gt_classes[:n].clone(),
                            batch.gt_counts[:n].clone(), preds[:n].clone()))
            record(step, batch, preds)
        run.images.record = spy
    for s in range(args.max_steps):
        run.step(s)
    run.close()
    torch.cuda.synchronize()
    return run


def test_train_image_summary_end_to_end(tmp_path):
    """train.py --image_summary 2: 3 x 2 PNGs whose pixels are the restatement applied to each summary step's batch, ground
    truth and filtered rows; the same run without the option ends in bitwise the same variables."""
    from PIL import Image
    T = _load("train")
    seen = []
    run = _run_training(T, _train_args(T, tmp_path / "with", "--image_summary", "2"), seen)
    assert [s[0] for s in seen] == [0, 1, 2] and run.images.written == 6
    mc, font = run.mc, viz.font()
    assert sorted(os.listdir(tmp_path / "with" / "images")) == ["step-0", "step-1", "step-2"]
    drawn = 0
    for step, x, gtb, gtc, gtn, preds in seen:
        ob, op, oc, _, cnt = run.images.filtered(preds)
        ob, op, oc, cnt = ob.cpu().numpy(), op.cpu().numpy(), oc.cpu().numpy(), cnt.cpu().numpy()
        gtb, gtc, gtn = gtb.cpu().numpy(), gtc.cpu().numpy(), gtn.cpu().numpy()
        gt_items = [[R.box_item(gtb[i, j], (0, 255, 0), mc.CLASS_NAMES[gtc[i, j]]) for j in range(int(gtn[i]))] for i in range(2)]
        det_items = [[R.box_item(ob[i, j], (0, 0, 255), "%s: (%.2f)" % (mc.CLASS_NAMES[oc[i, j]], float(op[i, j])))
                      for j in range(int(cnt[i])) if float(op[i, j]) > mc.PLOT_PROB_THRESH] for i in range(2)]
        drawn += sum(len(v) for v in gt_items) + sum(len(v) for v in det_items)
        want = R.draw(R.restore(x.cpu().numpy(), mc.BGR_MEANS), [gt_items, det_items], font, "rgb")
        assert sorted(os.listdir(tmp_path / "with" / "images" / ("step-%d" % step))) == ["0.png", "1.png"]
        for i in range(2):
            got = np.asarray(Image.open(tmp_path / "with" / "images" / ("step-%d" % step) / ("%d.png" % i)))
            assert got.shape == (128, 256, 3) and np.array_equal(got, want[i]), (step, i)
    assert drawn >= 6, "the pictures carry boxes"
    plain = _run_training(T, _train_args(T, tmp_path / "without"))
    assert plain.images is None and not os.path.exists(tmp_path / "without" / "images")
    for name in ("flat_params", "flat_accum"):
        assert torch.equal(getattr(run.tr, name).view(torch.int32), getattr(plain.tr, name).view(torch.int32)), name
    assert run.tr.global_step == plain.tr.global_step == 3


def test_demo_draw_gpu(tmp_path):
    """demo.py --draw gpu on the sample image: the restatement's picture of the restored network input and the filtered rows."""
    from PIL import Image
    D = _load("demo")
    src = os.path.join(ROOT, "tests", "golden", "sample.png")
    D.main(["--input_path", src, "--out_dir", str(tmp_path), "--draw", "gpu", "--dtype", "fp32"])
    got = np.asarray(Image.open(tmp_path / "out_sample.png"))
    a = D.parse_args(["--dtype", "fp32"])
    mc, model, dtype = D.make_model(a, 1)
    x = ops.preprocess_bgr(torch.from_numpy(drivers.read_bgr(src)).to(model.device)[None], mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, dtype)
    boxes, probs, cls = model.filter_prediction(*[t[0].cpu().numpy() for t in model.detect(x)])
    items = [R.box_item(b, D.CLS2CLR[mc.CLASS_NAMES[c]], "%s: (%.2f)" % (mc.CLASS_NAMES[c], float(p)))
             for b, p, c in zip(boxes, probs, cls) if float(p) > mc.PLOT_PROB_THRESH]
    want = R.draw(R.restore(x.cpu().numpy(), mc.BGR_MEANS), [[items]], viz.font(), "rgb")[0]
    assert got.shape == (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, 3) and np.array_equal(got, want)
    print("demo --draw gpu: %d boxes" % len(items))


def _kitti_tree(root, n=5, seed=5):
    from PIL import Image
    rs = np.random.RandomState(seed)
    for d in ("training/image_2", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    names = []
    for i in range(n):
        h, w = [(122, 250), (126, 254), (131, 262)][i % 3]
        Image.fromarray(rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(root, "training", "image_2", "%06d.png" % i))
        rows = []
        for j in range(int(rs.randint(1, 4))):
            bw, bh = rs.uniform(30, 70), rs.uniform(25, 50)
            x0, y0 = rs.uniform(16, w - bw - 2), rs.uniform(8, h - bh - 2)
            rows.append("%s 0.00 0 0.00 %.2f %.2f %.2f %.2f 1.50 1.60 3.90 1.00 1.00 10.00 0.00"
                        % (("Car", "Pedestrian", "Cyclist")[int(rs.randint(3))], x0, y0, x0 + bw, y0 + bh))
        with open(os.path.join(root, "training", "label_2", "%06d.txt" % i), "w") as f:
            f.write("\n".join(rows) + "\n")
        names.append("%06d" % i)
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")


def test_eval_visualize(tmp_path):
    """eval.py --visualize 2 on a synthetic set: 2 files per error type present (fewer where a type has fewer rows), each the
    restatement's picture; the same --seed picks the same rows, another seed is another permutation."""
    from PIL import Image
    E = _load("eval")
    data = str(tmp_path / "KITTI")
    _kitti_tree(data)
    out = str(tmp_path / "eval")
    E.main(["--data_path", data, "--image_set", "train", "--eval_dir", out, "--run_once", "--synthetic_weights", "--batch_size", "5",
            "--visualize", "2", "--seed", "4"])
    ea = os.path.join(out, "detection_files_0", "error_analysis")
    lines = open(os.path.join(ea, "det_error_file.txt")).read().splitlines()
    per_type = {}
    for ln in lines:
        per_type.setdefault(ln.split(" ")[1], []).append(ln)
    assert per_type, "the error analysis found no rows to draw"
    image_dir = os.path.join(data, "training", "image_2")
    first = {t: sorted(os.listdir(os.path.join(ea, t))) for t in per_type}
    for t, rows in per_type.items():
        assert first[t] == ["%d.png" % i for i in range(min(2, len(rows)))], t
    again = E.visualize_detections(image_dir, ".png", os.path.join(ea, "det_error_file.txt"), str(tmp_path / "again"), 2, 4, DEV)
    other = E.visualize_detections(image_dir, ".png", os.path.join(ea, "det_error_file.txt"), str(tmp_path / "other"), 2, 5, DEV)
    assert len(again) == sum(len(v) for v in first.values()) == len(other)
    font = viz.font()
    for t, i, k in again:
        a, b = open(os.path.join(ea, t, "%d.png" % i), "rb").read(), open(tmp_path / "again" / t / ("%d.png" % i), "rb").read()
        assert a == b, "the same seed draws the same rows"
        obj = lines[k].split(" ")
        assert obj[1] == t
        rgb = np.asarray(Image.open(os.path.join(image_dir, obj[0] + ".png")).convert("RGB"))
        item = tuple(int(float(v)) for v in obj[2:6]) + ((0, 200, 200), ("%s (%.2f)" % (obj[6], float(obj[7]))).encode(), "top_left")
        want = R.draw(rgb[None, :, :, ::-1], [[[item]]], font, "rgb")[0]
        assert np.array_equal(np.asarray(Image.open(os.path.join(ea, t, "%d.png" % i))), want), (t, i)
