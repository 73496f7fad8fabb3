"""The suppression options on the GPU: sqdet_suppress_rows against the sequential NumPy restatement on every case and every
method x overlap x class-agnostic combination; its nongreedy rule behind a threshold-inf filter against the filter's own rule;
its refusals; the serving step under an option (second launch, no riders) and under the default option (nothing new is called,
today's rows); the custom op."""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O
from squeezedet_amd import ops
from squeezedet_amd._lib import SqdetError
from tests import nms_options_cases as NC
from tests import nms_options_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def to_dev(out):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in out)


def to_np(out):
    return tuple(t.cpu().numpy() for t in out)


def opt(method, overlap="iou", agnostic=False, nms_thresh=0.4, sigma=0.5, score_floor=0.001):
    return dict(method=method, overlap=overlap, class_agnostic=agnostic, nms_thresh=nms_thresh, sigma=sigma, score_floor=score_floor)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_rows_equal(got, want, what, prob_ulps=0):
    names = ("boxes", "probs", "cls", "index", "count")
    for t in (0, 2, 3, 4):
        assert np.array_equal(bits(got[t]), bits(want[t])), "%s: %s differ" % (what, names[t])
    if prob_ulps == 0:
        assert np.array_equal(bits(got[1]), bits(want[1])), "%s: probs differ" % what
    else:           # finite non-negative float32: the distance in ulps is the distance of the bit patterns
        d = np.abs(got[1].view(np.int32).astype(np.int64) - want[1].view(np.int32).astype(np.int64))
        print("%s: largest prob distance %d ulp" % (what, int(d.max()) if d.size else 0))
        assert d.max() <= prob_ulps, "%s: probs differ by %d ulp" % (what, int(d.max()))


@pytest.mark.parametrize("combo", NC.COMBOS, ids=lambda c: "%s-%s-%s" % (c[0], c[1], "agnostic" if c[2] else "per_class"))
@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["name"])
def test_kernel_equals_restatement(case, combo):
    """nongreedy, greedy, soft_linear: all five tensors bit for bit.  soft_gaussian: boxes, cls, index, count bit for bit and the
    probs within one float32 ulp -- the device's and NumPy's float64 exp are each within an ulp or so of float64, far below the
    float32 spacing, so the float32 rounding of the final score can differ only at a rounding boundary."""
    method, overlap, agn = combo
    want = R.suppress(case["out"], case["classes"], method, overlap, agn, case["nms_thresh"], case["sigma"], case["score_floor"])
    dev = to_dev(case["out"])
    got = ops.suppress_rows(dev, case["classes"], opt(method, overlap, agn, case["nms_thresh"], case["sigma"], case["score_floor"]))
    assert all(g is d for g, d in zip(got, dev))                 # in place
    torch.cuda.synchronize()
    assert_rows_equal(to_np(got), want, "%s %s" % (case["name"], combo), prob_ulps=1 if method == "soft_gaussian" else 0)


def _random_detections(n, A, classes, seed):
    rs = np.random.RandomState(seed)
    boxes = np.stack([rs.uniform(0, 1242, (n, A)), rs.uniform(0, 375, (n, A)), rs.uniform(20, 300, (n, A)), rs.uniform(20, 200, (n, A))], -1)
    probs = rs.uniform(0, 1, (n, A)) ** 4                        # few high scores, like a detector's
    cls = rs.randint(0, classes, (n, A))
    return (torch.from_numpy(boxes.astype(np.float32)).to(DEV), torch.from_numpy(probs.astype(np.float32)).to(DEV),
            torch.from_numpy(cls.astype(np.int64)).to(DEV))


@pytest.mark.parametrize("t", [0.2, 0.4])
def test_nongreedy_behind_an_open_filter_is_the_filter(t):
    """filter_prediction(nms_thresh = inf) then suppress_rows(nongreedy, t) == filter_prediction(nms_thresh = t), all five
    outputs bit for bit: the second stage recovers the filter's total order from the class-major rows and runs its rule."""
    boxes, probs, cls = _random_detections(3, 16848, 3, seed=int(t * 100))
    want = ops.filter_prediction(boxes, probs, cls, 3, 64, t, 0.005)
    got = ops.suppress_rows(ops.filter_prediction(boxes, probs, cls, 3, 64, INF, 0.005), 3, opt("nongreedy", nms_thresh=t))
    torch.cuda.synchronize()
    assert int(want[4].min()) > 0 and int(want[4].min()) < 64    # something was kept everywhere, something was suppressed
    assert_rows_equal(to_np(got), to_np(want), "filter_prediction t=%g" % t)


@pytest.mark.parametrize("t", [0.2, 0.4])
def test_nongreedy_behind_an_open_detect_filter_is_detect_filter(t):
    import squeezedet_amd as S
    mc = S.kitti_squeezeDet_config()
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX).astype(np.float32)).to(DEV)
    gh, gw = 24, 78
    assert gh * gw * mc.ANCHOR_PER_GRID == mc.ANCHORS == 16848
    g = torch.Generator().manual_seed(7)
    preds = (torch.randn((2, gh, gw, mc.ANCHOR_PER_GRID * (mc.CLASSES + 5)), generator=g) * 1.5).to(DEV, torch.float16)
    args = (preds, anchors, mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH, mc.TOP_N_DETECTION)
    want = ops.detect_filter(*args, t)
    got = ops.suppress_rows(ops.detect_filter(*args, INF), mc.CLASSES, opt("nongreedy", nms_thresh=t))
    torch.cuda.synchronize()
    assert int(want[4].min()) > 0 and int(want[4].min()) < 64     # something was kept everywhere, something was suppressed
    assert_rows_equal(to_np(got), to_np(want), "detect_filter t=%g" % t)


@pytest.mark.parametrize("what", ["rows65", "bad_method", "bad_overlap", "diou_soft", "sigma0", "floor_inf"])
def test_refusals_leave_the_tensors_alone(what):
    rows = 65 if what == "rows65" else 8
    rs = np.random.RandomState(3)
    out = (rs.uniform(1, 50, (2, rows, 4)).astype(np.float32), rs.uniform(0, 1, (2, rows)).astype(np.float32),
           rs.randint(0, 3, (2, rows)).astype(np.int32), rs.randint(0, 999, (2, rows)).astype(np.int32), np.asarray([rows, 3], np.int32))
    o = {"rows65": opt("greedy"), "bad_method": opt(4), "bad_overlap": opt("greedy", overlap=2), "diou_soft": opt("soft_linear", "diou"),
         "sigma0": opt("soft_gaussian", sigma=0.0), "floor_inf": opt("soft_linear", score_floor=INF)}[what]
    dev = to_dev(out)
    with pytest.raises(SqdetError, match="code -1"):
        ops.suppress_rows(dev, 3, o)
    torch.cuda.synchronize()
    assert_rows_equal(to_np(dev), out, what)


# ---------------------------------------------------------------- the serving step
@pytest.fixture(scope="module")
def planted():
    """A float16 SqueezeDet at 375 x 1242, batch 2, with planted objects (squeezedet_amd.synthetic), its input, and the rows of
    the filter at the config's threshold and at inf -- computed once, by the plain entry points."""
    import squeezedet_amd as S
    from squeezedet_amd import nets, synthetic as SY
    size, batch = (375, 1242), 2
    mc, omc = S.kitti_squeezeDet_config_for_input(*size), O.squeezeDet_config_for_input(*size)
    mc.LOAD_PRETRAINED_MODEL, mc.BATCH_SIZE = False, batch
    m = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float16)
    m.load_params(SY.planted_params(O.init_params("squeezeDet", seed=40, storage="fp16"), omc.ANCHOR_PER_GRID, omc.CLASSES))
    x = SY.planted_images(omc, batch, seed=41)[0].to(DEV, torch.float16)
    b, p, c = m.detect(x)
    rows = {t: to_np(ops.filter_prediction(b, p, c, mc.CLASSES, mc.TOP_N_DETECTION, t, mc.PROB_THRESH)) for t in (mc.NMS_THRESH, INF)}
    torch.cuda.synchronize()
    return m, mc, x, rows


def _count_post_jobs(monkeypatch):
    calls = []
    real = ops.NetPlan.set_post_job
    monkeypatch.setattr(ops.NetPlan, "set_post_job", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    return calls


def _serve(m, x, defer, lanes, steps=5):
    """`steps` calls in flight; a call's pinned host rows are read where serving.Serving.step's completion contract says they are
    complete: after the next call of its lane (`lanes` calls later) and a synchronisation, the last ones after flush_pipeline()."""
    back = lanes or 1
    hist, outs = [], []
    for _ in range(steps):
        hist.append(m.detect_filter_pipelined(x, to_host=True, defer=defer, lanes=lanes))
        if len(hist) > back:
            torch.cuda.synchronize()
            outs.append(tuple(t.clone().numpy() for t in hist[-1 - back]))
    m.flush_pipeline()
    torch.cuda.synchronize()
    outs += [tuple(t.clone().numpy() for t in out) for out in hist[-back:]]
    assert len(outs) == steps
    return outs


SERVE = [(False, None), (True, 1), (True, 2)]
SERVE_IDS = ["eager", "deferred-1lane", "deferred-2lanes"]


@pytest.mark.parametrize("defer, lanes", SERVE, ids=SERVE_IDS)
def test_serving_under_an_option(planted, defer, lanes, monkeypatch):
    """NMS_METHOD = greedy: every step returns the restatement applied to the rows of a threshold-inf filter, and no post job is
    handed to a forward (the riders write into pinned host memory, where the second launch cannot follow)."""
    m, mc, x, rows = planted
    monkeypatch.delenv("SQDET_POST_DEFER", raising=False)
    want = R.suppress(rows[INF], mc.CLASSES, "greedy", nms_thresh=mc.NMS_THRESH)
    # (the option does something to these rows, and something else than the default rule)
    assert (want[4] < rows[INF][4]).all() and not np.array_equal(want[4], rows[mc.NMS_THRESH][4])
    calls = _count_post_jobs(monkeypatch)
    monkeypatch.setitem(mc, "NMS_METHOD", "greedy")
    try:
        outs = _serve(m, x, defer, lanes)
    finally:
        m.flush_pipeline()
    for k, got in enumerate(outs):
        assert_rows_equal(got, want, "step %d" % k)
    assert not calls
    for pipe in [m.serving.pipe] + [ln.pipe for ln in (m._lanes or [])]:
        assert not any(s.ride for s in (pipe.slots or []) if s.nms is not None and s.nms.method == "greedy")


@pytest.mark.parametrize("defer, lanes", SERVE, ids=SERVE_IDS)
def test_serving_under_the_default_option_calls_nothing_new(planted, defer, lanes, monkeypatch):
    m, mc, x, rows = planted
    monkeypatch.delenv("SQDET_POST_DEFER", raising=False)

    def boom(*a, **k):
        raise AssertionError("the default suppression policy must not reach suppress_rows")
    monkeypatch.setattr(ops, "suppress_rows", boom)
    calls = _count_post_jobs(monkeypatch)
    outs = _serve(m, x, defer, lanes)
    for k, got in enumerate(outs):
        assert_rows_equal(got, rows[mc.NMS_THRESH], "step %d" % k)
    b, p, c = m.detect(x)
    assert_rows_equal(to_np(m.filter_prediction_batch(b, p, c)), rows[mc.NMS_THRESH], "filter_prediction_batch")
    if defer and m._native_plan(2).rider_capacity() >= 2:
        assert calls                                                # the riders are still what carries the default rule


def test_model_filter_prediction_batch_under_options(planted, monkeypatch):
    """The one policy at the model's own filter: every method, DIoU and class-agnostic through mc."""
    m, mc, x, rows = planted
    b, p, c = m.detect(x)
    for fields, (method, overlap, agn) in (({"NMS_METHOD": "soft_linear"}, ("soft_linear", "iou", False)),
                                           ({"NMS_OVERLAP": "diou"}, ("nongreedy", "diou", False)),
                                           ({"NMS_METHOD": "greedy", "NMS_CLASS_AGNOSTIC": True}, ("greedy", "iou", True))):
        with monkeypatch.context() as mp:
            for k, v in fields.items():
                mp.setitem(mc, k, v)
            got = to_np(m.filter_prediction_batch(b, p, c))
        assert_rows_equal(got, R.suppress(rows[INF], mc.CLASSES, method, overlap, agn, nms_thresh=mc.NMS_THRESH), str(fields))


def test_custom_op_matches_ops():
    import squeezedet_amd.torch_ops  # noqa: F401  (registers torch.ops.sqdet.*)
    case = NC.CASES[0]
    for method, overlap, agn in (("greedy", "diou", True), ("soft_gaussian", "iou", False)):
        src = to_dev(case["out"])
        got = torch.ops.sqdet.suppress_rows(*src, case["classes"], method, overlap, agn, case["nms_thresh"], case["sigma"], case["score_floor"])
        assert_rows_equal(to_np(src), case["out"], "the op's inputs")           # functional: the inputs are left alone
        want = ops.suppress_rows(to_dev(case["out"]), case["classes"], opt(method, overlap, agn, case["nms_thresh"], case["sigma"], case["score_floor"]))
        torch.cuda.synchronize()
        assert_rows_equal(to_np(got), to_np(want), "custom op %s" % method)
    torch.library.opcheck(torch.ops.sqdet.suppress_rows, (*to_dev(case["out"]), 3, "greedy", "iou", False, 0.4, 0.5, 0.001),
                          test_utils=("test_schema", "test_faketensor"))


def test_eval_py_runs_under_the_flags(tmp_path, capsys):
    """eval.py --nms greedy on a small seeded KITTI tree with synthetic weights: the policy reaches the model, is printed with
    the results and recorded; greedy keeps every row the reference's rule keeps (a row it drops is overlapped by a KEPT
    higher-ranked row, which the reference's rule counts too), so no fewer detections; a run without the flags records nothing."""
    import os
    import sys
    from PIL import Image
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root_dir)
    import eval as E
    root, rs = str(tmp_path / "KITTI"), np.random.RandomState(5)
    for d in ("training/image_2", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    idxs = ["%06d" % i for i in range(4)]
    for idx in idxs:
        Image.fromarray(rs.uniform(0, 255, (120, 400, 3)).astype(np.uint8)).save(os.path.join(root, "training", "image_2", idx + ".png"))
        with open(os.path.join(root, "training", "label_2", idx + ".txt"), "w") as f:
            f.write("Car 0.00 0 -1.5 40.00 30.00 100.00 70.00 1.5 1.6 3.9 1.0 1.7 20.0 -1.5\n")
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("\n".join(idxs) + "\n")
    common = ["--data_path", root, "--image_set", "val", "--run_once", "--synthetic_weights", "--batch_size", "4", "--dtype", "fp16"]
    plain = E.main(common + ["--eval_dir", str(tmp_path / "plain")])
    assert "nms" not in plain and "Suppression: reference, iou > 0.4, per class" in capsys.readouterr().out
    greedy = E.main(common + ["--eval_dir", str(tmp_path / "greedy"), "--nms", "greedy", "--nms_class_agnostic"])
    assert greedy["nms"]["method"] == "greedy" and greedy["nms"]["class_agnostic"] is True and greedy["nms"]["default"] is False
    assert "Suppression: greedy, iou > 0.4, class-agnostic" in capsys.readouterr().out
    per_class = E.main(common + ["--eval_dir", str(tmp_path / "greedy_pc"), "--nms", "greedy"])
    assert per_class["num_det_per_image"] >= plain["num_det_per_image"] > 0
