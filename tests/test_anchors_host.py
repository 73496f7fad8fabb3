"""Host side of the anchor fitting (squeezedet_amd.anchors, config.with_anchor_shapes, the drivers' flags): everything that
needs no GPU.  The kernels are tested in tests/test_gpu_anchors.py."""
import importlib.util
import json
import os

import numpy as np
import pytest

import squeezedet_amd as S
from squeezedet_amd import anchors, config, drivers
from squeezedet_amd._lib import SqdetError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location("_anchors_host_" + name, os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _closed_form(mc, H, W, shapes):
    """config.py's docstring: ANCHOR_BOX[(h*W+w)*B+k] = [(w+1)*IMG_W/(W+1), (h+1)*IMG_H/(H+1), aw_k, ah_k]."""
    B = len(shapes)
    out = np.empty((H * W * B, 4), np.float64)
    for h in range(H):
        for w in range(W):
            for k in range(B):
                out[(h * W + w) * B + k] = [(w + 1) * float(mc.IMAGE_WIDTH) / (W + 1), (h + 1) * float(mc.IMAGE_HEIGHT) / (H + 1),
                                            shapes[k][0], shapes[k][1]]
    return out


def _shapes_for(a):
    """what eval.py's main asks for"""
    return drivers.driver_anchor_shapes(a.anchor_shapes, a.checkpoint_path)


SHAPES9 = np.array([[20.5, 31.], [44., 40.], [61., 120.25], [90., 70.], [130., 95.], [150., 210.], [240., 130.], [300., 260.], [410., 300.]])


@pytest.mark.parametrize("make, grid", [(lambda: S.kitti_squeezeDet_config_for_input(128, 256), (8, 16)),
                                        (lambda: S.kitti_squeezeDetPlus_config(), (22, 76)),
                                        (lambda: S.voc_squeezeDet_config_for_input(130, 250), (9, 16))])
def test_with_anchor_shapes_is_the_closed_form(make, grid):
    mc = make()
    assert config.anchor_grid(mc) == grid
    m2 = config.with_anchor_shapes(mc, SHAPES9)
    want = _closed_form(mc, grid[0], grid[1], SHAPES9)
    assert m2.ANCHOR_BOX.dtype == np.float64 and np.array_equal(m2.ANCHOR_BOX, want)
    assert m2.ANCHORS == len(want) and m2.ANCHOR_PER_GRID == 9
    assert np.array_equal(config.anchor_shapes_of(m2), SHAPES9)
    # a copy: the config it came from keeps its own anchors; its own shapes put back give its own ANCHOR_BOX bit for bit
    assert np.array_equal(config.anchor_shapes_of(mc), config.SQUEEZEDET_ANCHOR_SHAPES)
    assert np.array_equal(config.with_anchor_shapes(mc, config.SQUEEZEDET_ANCHOR_SHAPES).ANCHOR_BOX, mc.ANCHOR_BOX)
    # another count rebuilds all three fields
    m6 = config.with_anchor_shapes(mc, SHAPES9[:6])
    assert m6.ANCHOR_PER_GRID == 6 and m6.ANCHORS == grid[0] * grid[1] * 6 and np.array_equal(m6.ANCHOR_BOX, _closed_form(mc, grid[0], grid[1], SHAPES9[:6]))


def test_with_anchor_shapes_goes_before_pad_head_classes():
    mc = S.voc_squeezeDet_config_for_input(128, 256)
    padded9 = config.pad_head_classes(config.with_anchor_shapes(mc, SHAPES9))
    assert padded9.CLASSES == 23 and padded9.HEAD_PAD_CLASSES == 3                       # 9 * (23 + 5) = 252
    padded6 = config.pad_head_classes(config.with_anchor_shapes(mc, SHAPES9[:6]))
    assert padded6.CLASSES == 21 and (6 * (padded6.CLASSES + 5)) % 4 == 0              # the padding depends on the count
    with pytest.raises(ValueError, match="before pad_head_classes"):
        config.with_anchor_shapes(config.pad_head_classes(mc), SHAPES9)
    for bad in ([[1.0, 0.0]], [[1.0, float("nan")]], [[-3.0, 2.0]], [], [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError):
            config.with_anchor_shapes(mc, bad)


def test_dataset_shapes_scales_as_the_reader():
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    rois = [[[50., 40., 30., 20., 0], [70., 60., 11., 13., 2]], [], [[100., 90., 64.5, 33.25, 1]]]
    sizes = [(100, 200), (77, 99), (375, 1242)]
    wh = anchors.dataset_shapes(rois, sizes, mc)
    want = np.array([[30. * (256 / 200.), 20. * (128 / 100.)], [11. * (256 / 200.), 13. * (128 / 100.)],
                     [64.5 * (256 / 1242.), 33.25 * (128 / 375.)]])
    assert wh.dtype == np.float64 and np.array_equal(wh, want)
    # bit for bit the boxes BatchReader serves without augmentation
    mc.DATA_AUGMENTATION = False
    mc.BATCH_SIZE = 3
    reader = S.BatchReader(mc, [np.zeros((h, w, 3), np.uint8) for h, w in sizes], rois, seed=0)
    plan = reader.next_plan(shuffle=False)
    assert np.array_equal(np.concatenate([b[:, 2:4] for b in plan.bbox_per_batch if len(b)]), wh)
    # and the padded arrays of the whole dataset, in chunks
    chunks = list(anchors.padded_ground_truth(rois, sizes, mc, chunk_images=2))
    assert [c[0].shape for c in chunks] == [(2, 2, 4), (1, 2, 4)]
    assert np.array_equal(np.concatenate([c[2] for c in chunks]), [2, 0, 1])
    gt = np.concatenate([c[0] for c in chunks])
    assert np.array_equal(gt[0, :2], plan.bbox_per_batch[0]) and np.array_equal(gt[2, :1], plan.bbox_per_batch[2]) and not gt[1].any()
    assert np.array_equal(np.concatenate([c[1] for c in chunks]), [[0, 2], [0, 0], [1, 0]])
    with pytest.raises(ValueError):
        anchors.dataset_shapes(rois, sizes[:2], mc)


def test_initial_draw_is_seeded_and_distinct():
    rs = np.random.RandomState(1)
    wh = rs.randint(1, 30, size=(200, 2)).astype(np.float64)
    wh = np.concatenate([wh, wh[:50]])                                   # duplicates
    a, b = anchors.draw_init(wh, 9, 4, seed=5), anchors.draw_init(wh, 9, 4, seed=5)
    assert a.shape == (4, 9, 2) and np.array_equal(a, b)
    assert not np.array_equal(a, anchors.draw_init(wh, 9, 4, seed=6))
    u = np.unique(wh, axis=0)
    for r in range(4):
        assert len(np.unique(a[r], axis=0)) == 9                         # distinct centroids
        assert all((u == c).all(axis=1).any() for c in a[r])             # drawn from the dataset
    # the draw is the documented one
    rs = np.random.RandomState(5)
    assert np.array_equal(a, np.stack([u[rs.choice(len(u), 9, replace=False)] for _ in range(4)]))
    few = np.array([[1., 2.], [1., 2.], [3., 4.], [3., 4.], [5., 6.]])
    with pytest.raises(ValueError, match="3 distinct"):
        anchors.draw_init(few, 4, 1, seed=0)
    with pytest.raises(ValueError, match="3 distinct"):
        anchors.fit_anchor_shapes(few, k=4)


def test_json_round_trip(tmp_path):
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    shapes = np.array([[1 / 3., 2 / 7.], [1e-3, 123456.789], [np.pi, np.e]])
    p = str(tmp_path / "a.json")
    anchors.save_anchor_shapes(p, shapes, mc, dataset="KITTI", image_set="train", k=3, seed=4, mean_iou=0.6125)
    rec = json.load(open(p))
    assert rec["image_size"] == [128, 256] and rec["dataset"] == "KITTI" and rec["image_set"] == "train"
    assert rec["k"] == 3 and rec["seed"] == 4 and rec["mean_iou"] == 0.6125
    back = anchors.load_anchor_shapes(p)
    assert back.dtype == np.float64 and np.array_equal(back, shapes) and anchors.same_shapes(back, shapes)      # bit for bit
    assert not anchors.same_shapes(back, shapes[::-1]) and not anchors.same_shapes(back, shapes[:2])
    json.dump(shapes.tolist(), open(p, "w"))                             # a bare list is taken too
    assert np.array_equal(anchors.load_anchor_shapes(p), shapes)
    for text in ("{}", "[[1, 2], [3]]", "[[1, 0]]", "not json", '{"anchor_shapes": [[1, "x"]]}'):
        open(p, "w").write(text)
        with pytest.raises(ValueError):
            anchors.load_anchor_shapes(p)
    assert anchors.beside_checkpoint(str(tmp_path / "model.ckpt-3.npz")) is None
    anchors.save_anchor_shapes(str(tmp_path / "anchor_shapes.json"), shapes, mc)
    assert anchors.beside_checkpoint(str(tmp_path / "model.ckpt-3.npz")) == str(tmp_path / "anchor_shapes.json")
    assert anchors.beside_checkpoint(str(tmp_path)) == str(tmp_path / "anchor_shapes.json")


def test_host_validation_messages():
    good = np.array([[4., 5.], [6., 7.], [8., 9.]])
    with pytest.raises(ValueError, match=r"shape 1 is \(0\.0, 7\.0\)"):
        anchors.fit_anchor_shapes([[4., 5.], [0., 7.]], k=1)
    with pytest.raises(ValueError, match="finite and strictly positive: shape 2"):
        anchors.fit_anchor_shapes([[4., 5.], [6., 7.], [float("nan"), 1.]], k=1)
    with pytest.raises(ValueError, match="finite and strictly positive"):
        anchors.fit_anchor_shapes([[4., 5.], [float("inf"), 7.]], k=1)
    with pytest.raises(ValueError, match=r"\[n,2\]"):
        anchors.fit_anchor_shapes([1., 2., 3.], k=1)
    with pytest.raises(ValueError, match="no box shapes"):
        anchors.fit_anchor_shapes(np.zeros((0, 2)), k=1)
    with pytest.raises(ValueError, match="must be positive"):
        anchors.fit_anchor_shapes(good, k=0)
    with pytest.raises(ValueError, match="must be positive"):
        anchors.fit_anchor_shapes(good, k=1, max_iter=0)
    with pytest.raises(SqdetError, match="k = 65"):
        anchors.fit_anchor_shapes(np.tile(good, (30, 1)), k=65)
    with pytest.raises(SqdetError, match="restarts = 65"):
        anchors.fit_anchor_shapes(good, k=2, restarts=65)
    with pytest.raises(ValueError, match=r"init must be \[restarts,2,2\]"):
        anchors.fit_anchor_shapes(good, k=2, init=np.ones((3, 3, 2)))
    with pytest.raises(ValueError, match="centroids must be finite and strictly positive"):
        anchors.kmeans(good, np.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match=r"gt_counts must lie in \[0, 2\]"):
        anchors.coverage(S.kitti_squeezeDet_config_for_input(128, 256), np.ones((1, 2, 4)), np.zeros((1, 2)), [3])
    with pytest.raises(ValueError, match="strictly positive width and height"):
        anchors.coverage(S.kitti_squeezeDet_config_for_input(128, 256), np.array([[[5., 5., 0., 2.]]]), np.zeros((1, 1)), [1])


def test_report_arithmetic():
    """CoverageReport from per-object arrays: the DEBUG_MODE numbers and ours, padding ignored."""
    best = np.array([[0.8, 0.5, 0.0], [0.25, 0.0, 0.0]])
    claimed = np.array([[0.8, 0.4, 0.0], [0.0, 0.0, 0.0]])
    rep = anchors.CoverageReport(best, [[3, 3, 0], [7, -1, -1]], claimed, [[3, 2, 9], [5, -1, -1]], [3, 1])
    assert rep.num_objects == 4 and rep.max_iou == 0.8 and rep.min_iou == 0.0 and rep.num_zero_iou == 2
    assert rep.avg_iou == (0.8 + 0.4) / 4 and rep.mean_best_iou == (0.8 + 0.5 + 0.25) / 4
    assert rep.recall_at == {0.3: 0.5, 0.5: 0.5, 0.7: 0.25} and rep.num_displaced == 2
    both = anchors.CoverageReport.merge([rep, rep])
    assert both.num_objects == 8 and both.avg_iou == rep.avg_iou and both.num_displaced == 4
    text = anchors.format_reports([rep, both], ["current", "fitted"])
    assert "number of objects with 0 iou" in text and "current" in text and len(text.splitlines()) == 11
    json.dumps(rep.summary())


def test_driver_arguments(tmp_path):
    T, E, D, F = _load("train.py", "train"), _load("eval.py", "eval"), _load("demo.py", "demo"), _load("tools/fit_anchors.py", "fit")
    a = T.parse_args(["--synthetic", "4", "--anchor_shapes", "x.json", "--anchor_report"])
    assert a.anchor_shapes == "x.json" and a.anchor_report
    a = T.parse_args([])
    assert a.anchor_shapes == "" and not a.anchor_report
    assert E.parse_args(["--anchor_shapes", "y.json"]).anchor_shapes == "y.json" and E.parse_args([]).anchor_shapes == ""
    assert D.parse_args(["--anchor_shapes", "z.json"]).anchor_shapes == "z.json" and D.parse_args([]).anchor_shapes == ""
    f = F.parse_args(["--synthetic", "12", "--k", "9", "--out", "f.json"])
    assert (f.synthetic, f.k, f.seed, f.restarts, f.out, f.dataset, f.net, f.image_size) == (12, 9, 0, 8, "f.json", "KITTI", "squeezeDet", None)
    f = F.parse_args(["--dataset", "PASCAL_VOC", "--data_path", "d", "--year", "2012", "--image_set", "trainval", "--image_size", "128", "256",
                      "--seed", "3", "--restarts", "4"])
    assert (f.dataset, f.data_path, f.year, f.image_set, f.image_size, f.seed, f.restarts) == ("PASCAL_VOC", "d", "2012", "trainval", [128, 256], 3, 4)
    for bad in (["--k", "0"], ["--dataset", "COCO"], ["--dataset", "PASCAL_VOC", "--net", "vgg16"]):
        with pytest.raises(SystemExit):
            F.parse_args(bad)
    # make_config: the shapes go in before the head is padded; without them the configs are today's
    mc = drivers.make_config("squeezeDet", (128, 256), "PASCAL_VOC", SHAPES9)
    assert mc.CLASSES == 23 and np.array_equal(config.anchor_shapes_of(mc), SHAPES9)
    assert np.array_equal(drivers.make_config("squeezeDet", (128, 256), "PASCAL_VOC").ANCHOR_BOX,
                          config.pad_head_classes(S.voc_squeezeDet_config_for_input(128, 256)).ANCHOR_BOX)
    assert np.array_equal(drivers.make_config("squeezeDet+").ANCHOR_BOX, S.kitti_squeezeDetPlus_config().ANCHOR_BOX)
    # the drivers refuse a count the nets are not built for, by name, before building anything
    p = str(tmp_path / "six.json")
    anchors.save_anchor_shapes(p, SHAPES9[:6], S.kitti_squeezeDet_config())
    with pytest.raises(SystemExit, match="6 anchor shapes"):
        anchors.load_for_driver(p)
    with pytest.raises(SystemExit, match="6 anchor shapes"):
        T.resolve_anchor_shapes(T.parse_args(["--anchor_shapes", p]))
    with pytest.raises(SystemExit, match="--anchor_shapes"):
        anchors.load_for_driver(str(tmp_path / "missing.json"))
    p9 = str(tmp_path / "nine.json")
    anchors.save_anchor_shapes(p9, SHAPES9, S.kitti_squeezeDet_config())
    assert np.array_equal(T.resolve_anchor_shapes(T.parse_args(["--anchor_shapes", p9])), SHAPES9)
    assert T.resolve_anchor_shapes(T.parse_args([])) is None
    # eval.py: the flag, else the file beside the checkpoint, else nothing
    assert _shapes_for(E.parse_args(["--checkpoint_path", str(tmp_path / "none" / "model.ckpt-1.npz")])) is None
    os.makedirs(str(tmp_path / "run"))
    anchors.save_anchor_shapes(str(tmp_path / "run" / "anchor_shapes.json"), SHAPES9[::-1], S.kitti_squeezeDet_config())
    assert np.array_equal(_shapes_for(E.parse_args(["--checkpoint_path", str(tmp_path / "run" / "model.ckpt-1.npz")])), SHAPES9[::-1])
    assert np.array_equal(_shapes_for(E.parse_args(["--checkpoint_path", str(tmp_path / "run"), "--anchor_shapes", p9])), SHAPES9)
