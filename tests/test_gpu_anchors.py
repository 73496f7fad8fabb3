"""sqdet_anchor_kmeans and sqdet_anchor_coverage (csrc/anchors.hip) against float64 NumPy restatements written here, and the
drivers' anchor flags end to end in child processes.

The k-means reference is the loop of include/sqdet.h: assign by np.argmax of the IoU, stop at the first iteration that changes
no assignment, else move every centroid with members to their mean.  On integer-valued shapes every sum is exact in any
order, so the device's whole trajectory must match it bit for bit.  The coverage reference is util.batch_iou's expression
(utils/util.py:42-54) plus np.argmax, and the mc.DEBUG_MODE loop of imdb.read_batch (imdb.py:135-139, 195-246) restated.

Every child is a fresh process under its own timeout; its exit status is checked before the next one starts."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import squeezedet_amd as S
from squeezedet_amd import anchors, config, drivers, ops
from squeezedet_amd._lib import SqdetError, SqdetUnsupported

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- k-means reference --
def ref_iou(wh, cent):
    """inter = min(w, cw) * min(h, ch); iou = inter / (w*h + cw*ch - inter), float64 [n,k]; the same operations in the same
    order, written in place (the largest case is 66 563 x 9 for up to 100 iterations of 8 restarts)."""
    w, h = wh[:, 0:1], wh[:, 1:2]
    cw, ch = cent[None, :, 0], cent[None, :, 1]
    inter = np.minimum(w, cw)
    inter *= np.minimum(h, ch)
    union = (w * h) + (cw * ch)
    union -= inter
    inter /= union
    return inter


def ref_kmeans(wh, init, max_iter, snapshots=()):
    """One restart.  Returns {max_iter: (centroids, assign, counts, mean_iou, iters)} for max_iter and every value of
    `snapshots` below it (the state a run of that many iterations ends in)."""
    cent = np.array(init, np.float64)
    n, k = len(wh), len(cent)
    assign = np.full(n, -1, np.int64)
    out = {}

    def state(iters):
        own = ref_iou(wh, cent)[np.arange(n), assign]
        return cent.copy(), assign.astype(np.int32), np.bincount(assign, minlength=k).astype(np.int32), own.sum() / n, iters

    iters = None
    for it in range(max_iter):
        new = np.argmax(ref_iou(wh, cent), axis=1)
        changed = bool((new != assign).any())
        assign = new
        if not changed:
            iters = it
            break
        cnt = np.bincount(assign, minlength=k)
        sw, sh = np.bincount(assign, weights=wh[:, 0], minlength=k), np.bincount(assign, weights=wh[:, 1], minlength=k)
        for c in np.flatnonzero(cnt):
            cent[c] = (sw[c] / cnt[c], sh[c] / cnt[c])
        if it + 1 in snapshots:
            out[it + 1] = state(it + 1)
    for m in snapshots:                       # converged before a snapshot point: the fixed point, iters as found
        out.setdefault(m, state(iters if iters is not None and iters < m else m))
    out[max_iter] = state(iters if iters is not None else max_iter)
    return out


def int_shapes(n, seed):
    """Integer-valued (w, h) in 1..400: distinct for small n (a draw needs k distinct ones), with duplicates for the large one."""
    rs = np.random.RandomState(seed)
    code = rs.choice(160000, n, replace=False) if n <= 1000 else rs.randint(0, 160000, n)
    return np.stack([code // 400 + 1, code % 400 + 1], axis=1).astype(np.float64)


CASES = [(1, 1), (9, 9), (257, 9), (66563, 9), (1000, 64)]
_ref_cache = {}


def int_case(n, k):
    """(wh, init [8,k,2], per restart the reference states after 1 and after 100 iterations), computed once per (n, k)."""
    if (n, k) not in _ref_cache:
        wh = int_shapes(n, seed=n + k)
        init = anchors.draw_init(wh, k, 8, seed=11)
        _ref_cache[(n, k)] = (wh, init, [ref_kmeans(wh, init[r], 100, snapshots=(1,)) for r in range(8)])
    return _ref_cache[(n, k)]


@pytest.mark.parametrize("max_iter", [1, 100])
@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("n, k", CASES)
def test_kmeans_integer_shapes_bitwise(n, k, R, max_iter):
    wh, init, ref = int_case(n, k)
    got = anchors.kmeans(wh, init[:R], max_iter, device=DEV)
    assert got.centroids.shape == (R, k, 2) and got.assign.shape == (R, n) and got.assign.dtype == np.int32
    for r in range(R):
        cent, assign, counts, mean_iou, iters = ref[r][max_iter]
        print("n %d k %d restart %d max_iter %d: iters %d (ref %d), mean_iou %.17g (ref %.17g)" % (n, k, r, max_iter, got.iters[r], iters,
                                                                                                  got.mean_iou[r], mean_iou))
        assert got.iters[r] == iters
        assert np.array_equal(got.assign[r], assign)
        assert np.array_equal(got.counts[r], counts)
        assert np.array_equal(got.centroids[r].view(np.int64), cent.view(np.int64)), "centroids differ"
        assert abs(got.mean_iou[r] - mean_iou) <= 2 * (n - 1) * 2.0 ** -53


def test_kmeans_ties_and_empties():
    # (4,4) ties between (2,8) and (8,2): IoU 8 / 24 with both; duplicates everywhere; centroid 3 repeats centroid 2.  The members
    # of centroid 2 are all (30,30), so its mean stays (30,30) and the two centroids stay identical through every iteration: the
    # tie is there in the first iteration and in the last one
    wh = np.array([[4., 4.], [4., 4.], [2., 8.], [2., 9.], [8., 2.], [9., 2.], [30., 30.], [30., 30.], [30., 30.]])
    init = np.array([[[2., 8.], [8., 2.], [30., 30.], [30., 30.]]])
    iou = ref_iou(wh, init[0])
    assert iou[0, 0] == iou[0, 1] and iou[6, 2] == iou[6, 3] == 1.0           # the ties are exact ties
    for max_iter in (1, 100):
        ref = ref_kmeans(wh, init[0], max_iter)[max_iter]
        got = anchors.kmeans(wh, init, max_iter, device=DEV)
        assert np.array_equal(got.assign[0], ref[1]) and np.array_equal(got.counts[0], ref[2]) and got.iters[0] == ref[4]
        assert np.array_equal(got.centroids[0].view(np.int64), ref[0].view(np.int64))
        assert got.assign[0][0] == 0 and got.assign[0][1] == 0               # the lower index wins the tie
        assert list(got.assign[0][6:]) == [2, 2, 2] and got.counts[0][3] == 0  # the lower of two identical centroids takes every member
        assert list(ref[1][6:]) == [2, 2, 2] and ref[2][3] == 0               # (and so says the reference)
        assert np.array_equal(got.centroids[0][3], [30., 30.])                # the empty one keeps its value
        assert int(got.counts[0].sum()) == len(wh)
    # the same through fit_anchor_shapes' init: shapes come back sorted, the empty centroid among them
    fit = anchors.fit_anchor_shapes(wh, k=4, init=init, device=DEV)
    assert fit.restart == 0 and sorted(fit.counts.tolist()) == sorted(ref[2].tolist())
    area = fit.shapes[:, 0] * fit.shapes[:, 1]
    assert (np.diff(area) >= 0).all()


def test_kmeans_real_shapes():
    rs = np.random.RandomState(3)
    n, k, R = 5003, 9, 4
    wh = np.stack([rs.uniform(5, 400, n), rs.uniform(5, 300, n)], axis=1)
    init = anchors.draw_init(wh, k, R, seed=2)
    one = anchors.kmeans(wh, init, 1, device=DEV)
    for r in range(R):
        assign = np.argmax(ref_iou(wh, init[r]), axis=1)
        assert np.array_equal(one.assign[r], assign)                           # the same double expression, no contraction
        assert np.array_equal(one.counts[r], np.bincount(assign, minlength=k))
        for c in range(k):
            m = assign == c
            want = np.array([wh[m, 0].sum() / m.sum(), wh[m, 1].sum() / m.sum()])
            rel = np.abs(one.centroids[r, c] - want) / want
            assert (rel <= (n - 1) * 2.0 ** -52).all(), (r, c, rel)
    a, b = anchors.kmeans(wh, init, 100, device=DEV), anchors.kmeans(wh, init, 100, device=DEV)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    assert (a.counts.sum(axis=1) == n).all() and (a.iters >= 1).all()


def clustered_int_shapes(seed, n=400):
    rs = np.random.RandomState(seed)
    centres = np.array([[20, 30], [45, 40], [60, 150], [110, 70], [200, 120], [260, 300], [380, 90]])
    c = centres[rs.randint(len(centres), size=n)]
    return np.clip(np.rint(c * rs.uniform(0.6, 1.5, size=(n, 2))), 1, 400).astype(np.float64)


def test_fit_picks_the_reference_restart_and_sorts():
    wh = clustered_int_shapes(seed=8)
    k, R, seed = 5, 4, 5
    init = anchors.draw_init(wh, k, R, seed)
    ref = [ref_kmeans(wh, init[r], 100)[100] for r in range(R)]
    means = np.array([s[3] for s in ref])
    best = int(np.argmax(means))
    print("reference mean IoU per restart:", means, "winner", best)
    assert (means[best] - np.delete(means, best) > 1e-9).all(), "the reference's restarts must differ for this test to mean anything"
    fit = anchors.fit_anchor_shapes(wh, k=k, seed=seed, restarts=R, max_iter=100, device=DEV)
    assert fit.restart == best and fit.iters == ref[best][4]
    assert abs(fit.mean_iou - means[best]) <= 2 * (len(wh) - 1) * 2.0 ** -53
    assert np.abs(fit.restart_mean_iou - means).max() <= 2 * (len(wh) - 1) * 2.0 ** -53
    cent, counts = ref[best][0], ref[best][2]
    order = np.lexsort((cent[:, 0], cent[:, 0] * cent[:, 1]))
    assert np.array_equal(fit.shapes.view(np.int64), cent[order].view(np.int64)) and np.array_equal(fit.counts, counts[order])
    area = fit.shapes[:, 0] * fit.shapes[:, 1]
    assert (np.diff(area) >= 0).all()
    # given through init, the same runs give the same winner
    again = anchors.fit_anchor_shapes(wh, k=k, init=init, device=DEV)
    assert again.restart == best and np.array_equal(again.shapes, fit.shapes)


SENTINEL = 0x5A5A5A5A


def _sentinel_out(R, n, k):
    return (torch.full((R, n), SENTINEL, dtype=torch.int32, device=DEV), torch.full((R, k), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((R,), -7.25, dtype=torch.float64, device=DEV), torch.full((R,), SENTINEL, dtype=torch.int32, device=DEV))


def _untouched(out):
    torch.cuda.synchronize()
    return all(bool((t == (-7.25 if t.dtype == torch.float64 else SENTINEL)).all()) for t in out)


def test_kmeans_rejections_leave_the_outputs_alone():
    wh = int_shapes(100, seed=1)
    cases = [(wh, np.ones((1, 65, 2)), 10, SqdetUnsupported, "k 65"),
             (wh, np.ones((65, 3, 2)), 10, SqdetUnsupported, "65 restarts"),
             (np.zeros((0, 2)), np.ones((2, 3, 2)), 10, SqdetError, "null pointer|bad dims"),
             (wh, np.ones((2, 3, 2)), 0, SqdetError, "max_iter 0")]
    for shapes, init, max_iter, err, text in cases:
        out = _sentinel_out(init.shape[0], len(shapes), init.shape[1])
        with pytest.raises(err, match=text):
            anchors.kmeans(shapes, init, max_iter, device=DEV, out=out)
        assert _untouched(out), text
    for bad in (0.0, float("nan")):
        shapes = wh.copy()
        shapes[37, 0] = bad
        out = _sentinel_out(2, len(shapes), 3)
        with pytest.raises(ValueError, match="shape 37"):
            anchors.kmeans(shapes, np.ones((2, 3, 2)), 10, device=DEV, out=out)
        assert _untouched(out)
    # the library itself: the limits and the argument checks come before any launch
    from squeezedet_amd._lib import lib
    assert lib().sqdet_anchor_kmeans_workspace_bytes(100, 65, 1) == 0 and lib().sqdet_anchor_kmeans_workspace_bytes(100, 64, 64) > 0
    assert lib().sqdet_anchor_kmeans(None, None, None, None, None, None, None, 10, 3, 1, 5, None) == -1
    # and a good call into the same buffers does write them
    out = _sentinel_out(2, len(wh), 3)
    anchors.kmeans(wh, anchors.draw_init(wh, 3, 2, seed=0), 10, device=DEV, out=out)
    torch.cuda.synchronize()
    assert not bool((out[0] == SENTINEL).any()) and not bool((out[1] == SENTINEL).any()) and not bool((out[3] == SENTINEL).any())


# ------------------------------------------------------------------------------------------------ coverage reference --
def batch_iou(boxes, box):
    """utils/util.py:42-54, restated."""
    lr = np.maximum(np.minimum(boxes[:, 0] + 0.5 * boxes[:, 2], box[0] + 0.5 * box[2]) - np.maximum(boxes[:, 0] - 0.5 * boxes[:, 2], box[0] - 0.5 * box[2]), 0)
    tb = np.maximum(np.minimum(boxes[:, 1] + 0.5 * boxes[:, 3], box[1] + 0.5 * box[3]) - np.maximum(boxes[:, 1] - 0.5 * boxes[:, 3], box[1] - 0.5 * box[3]), 0)
    inter = lr * tb
    union = boxes[:, 2] * boxes[:, 3] + box[2] * box[3] - inter
    return inter / union


def debug_mode_statistics(anchor_box, gt, counts):
    """imdb.read_batch's mc.DEBUG_MODE accumulation (imdb.py:135-139, 195-226, 241-246) and the anchor each object claims."""
    avg_ious, num_objects, max_iou, min_iou, num_zero_iou_obj = 0., 0., 0.0, 1.0, 0
    aidx_per_batch = []
    for b in range(len(gt)):
        aidx_set, aidx_per_image = set(), []
        for i in range(counts[b]):
            overlaps = batch_iou(anchor_box, gt[b, i])
            aidx = len(anchor_box)
            for ov_idx in np.argsort(overlaps, kind="stable")[::-1]:
                if overlaps[ov_idx] <= 0:
                    min_iou = min(overlaps[ov_idx], min_iou)
                    num_objects += 1
                    num_zero_iou_obj += 1
                    break
                if ov_idx not in aidx_set:
                    aidx_set.add(ov_idx)
                    aidx = ov_idx
                    max_iou = max(overlaps[ov_idx], max_iou)
                    min_iou = min(overlaps[ov_idx], min_iou)
                    avg_ious += overlaps[ov_idx]
                    num_objects += 1
                    break
            if aidx == len(anchor_box):
                dist = np.sum(np.square(gt[b, i] - anchor_box), axis=1)
                for dist_idx in np.argsort(dist, kind="stable"):
                    if dist_idx not in aidx_set:
                        aidx_set.add(dist_idx)
                        aidx = dist_idx
                        break
            aidx_per_image.append(int(aidx))
        aidx_per_batch.append(aidx_per_image)
    return dict(max_iou=max_iou, min_iou=min_iou, avg_iou=avg_ious / num_objects, num_objects=int(num_objects),
                num_zero_iou=num_zero_iou_obj), aidx_per_batch


def coverage_case(mc):
    """B = 3, M = 5, counts (5, 0, 2): an object equal to an anchor, one far outside every anchor, two identical objects, and
    ordinary ones; the padding rows hold values that must never be read as boxes."""
    ab = np.asarray(mc.ANCHOR_BOX, np.float64)
    A, K = len(ab), int(mc.ANCHOR_PER_GRID)
    cells = A // K
    self_iou = np.array([batch_iou(ab[j:j + 1], ab[j])[0] for j in range(0, A, max(1, A // 997))])
    exact = int(np.flatnonzero(self_iou == 1.0)[0]) * max(1, A // 997)     # an anchor whose IoU with itself is exactly 1.0
    near = lambda cell, shape, sx, sy, dx, dy: ab[cell * K + shape] * [1, 1, sx, sy] + [dx, dy, 0, 0]
    twin = near(cells // 2, 0, 0.8, 1.1, 1.3, -0.7)                       # (the smallest shape: no neighbouring cell's anchor ties with its best one)
    gt = np.full((3, 5, 4), 1e9)
    gt[0, 0] = ab[exact]
    gt[0, 1] = [-5000.0, -4000.0, 30.0, 20.0]                              # overlaps no anchor
    gt[0, 2] = twin
    gt[0, 3] = twin
    gt[0, 4] = near(cells - 1, 7, 0.9, 0.7, -0.4, 0.2)
    gt[2, 0] = near(1, 0, 1.25, 0.9, 0.3, 0.3)
    gt[2, 1] = near(cells - 2, 3, 0.6, 1.4, -1.1, 0.9)
    gt[1] = np.nan
    counts = np.array([5, 0, 2], np.int32)
    cls = np.array([[0, 1, 2, 2, 1], [0, 0, 0, 0, 0], [2, 0, 0, 0, 0]], np.int32)
    return gt, cls, counts, exact


def _coverage_configs():
    small = config.with_anchor_shapes(S.kitti_squeezeDet_config_for_input(32, 48), config.SQUEEZEDET_ANCHOR_SHAPES / 8.0)
    return {54: small, 16848: S.kitti_squeezeDet_config()}


@pytest.mark.parametrize("A", [54, 16848])
def test_coverage_bitwise(A):
    mc = _coverage_configs()[A]
    ab = np.asarray(mc.ANCHOR_BOX, np.float64)
    assert len(ab) == A
    gt, cls, counts, exact = coverage_case(mc)
    want, aidx = debug_mode_statistics(ab, gt, counts)
    rep = anchors.coverage(mc, gt, cls, counts, device=DEV)
    N = int(counts.sum())
    for b in range(3):
        for i in range(5):
            if i >= counts[b]:
                assert rep.best_iou[b, i] == 0.0 and rep.best_index[b, i] == -1 and rep.claimed_iou[b, i] == 0.0 and rep.anchor_index[b, i] == -1
                continue
            ov = batch_iou(ab, gt[b, i])
            assert rep.best_iou[b, i].view(np.int64) == ov.max().view(np.int64) and rep.best_index[b, i] == int(np.argmax(ov)), (b, i)
            assert rep.anchor_index[b, i] == aidx[b][i]
            assert rep.claimed_iou[b, i].view(np.int64) == ov[aidx[b][i]].view(np.int64), (b, i)
    assert rep.best_iou[0, 0] == 1.0 and rep.best_index[0, 0] == exact and rep.claimed_iou[0, 0] == 1.0
    assert rep.best_iou[0, 1] == 0.0 and rep.best_index[0, 1] == 0 and rep.claimed_iou[0, 1] == 0.0
    assert rep.best_iou[0, 2] == rep.best_iou[0, 3] and rep.claimed_iou[0, 2] == rep.best_iou[0, 2]
    assert rep.claimed_iou[0, 3] < rep.best_iou[0, 3] and rep.num_displaced == 1
    print("A %d: report %s, reference %s" % (A, rep.summary(), want))
    assert rep.num_objects == want["num_objects"] == N and rep.num_zero_iou == want["num_zero_iou"] == 1
    assert rep.max_iou == want["max_iou"] == 1.0 and rep.min_iou == want["min_iou"] == 0.0
    assert abs(rep.avg_iou - want["avg_iou"]) <= 2 * (N - 1) * 2.0 ** -53
    valid = rep.valid
    assert rep.mean_best_iou == rep.best_iou[valid].sum() / N
    assert rep.recall_at == {t: float((rep.best_iou[valid] >= t).sum() / N) for t in (0.3, 0.5, 0.7)}
    # without anchor_index the claimed IoU is 0 everywhere, and the rest does not change
    best, bidx, claimed = ops.anchor_coverage(ab, torch.from_numpy(gt).to(DEV), torch.from_numpy(counts).to(DEV))
    assert np.array_equal(best.cpu().numpy(), rep.best_iou) and np.array_equal(bidx.cpu().numpy(), rep.best_index) and not bool(claimed.any())
    # a dataset in chunks of images is the same report
    rois = [[[g[0], g[1], g[2], g[3], c] for g, c in zip(gt[b, :counts[b]], cls[b])] for b in range(3)]
    sizes = [(mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH)] * 3
    whole = anchors.dataset_coverage(mc, rois, sizes, chunk_images=2, device=DEV)
    assert whole.summary() == rep.summary() and np.array_equal(whole.claimed_iou, rep.claimed_iou)


# ---------------------------------------------------------------------------------------------------------- drivers --
def _load(name):
    spec = importlib.util.spec_from_file_location("_anchors_gpu_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _child(script, args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    return r


def test_drivers_end_to_end(tmp_path):
    from squeezedet_amd import checkpoint
    E = _load("eval")
    f, d = str(tmp_path / "f.json"), str(tmp_path / "run")
    size = ["--image_size", "128", "256"]
    r = _child("tools/fit_anchors.py", ["--synthetic", "12", "--k", "9", "--out", f] + size)
    assert r.returncode == 0, "fit_anchors.py failed"
    assert "current" in r.stdout and "fitted" in r.stdout and "number of objects with 0 iou" in r.stdout
    rec = json.load(open(f))
    assert rec["k"] == 9 and rec["seed"] == 0 and rec["image_size"] == [128, 256] and rec["dataset"] == "synthetic-12" and 0 < rec["mean_iou"] <= 1
    assert rec["coverage_fitted"]["mean_best_iou"] > rec["coverage_current"]["mean_best_iou"]      # KITTI's shapes at 1248 wide do not fit a 256-wide input
    shapes = anchors.load_anchor_shapes(f)
    assert shapes.shape == (9, 2)
    train = ["--synthetic", "12", "--train_dir", d, "--checkpoint_step", "2", "--summary_step", "0", "--batch_size", "2", "--no_graph"] + size
    r = _child("train.py", train + ["--anchor_shapes", f, "--max_steps", "2", "--anchor_report"])
    assert r.returncode == 0, "train.py failed"
    assert anchors.same_shapes(anchors.load_anchor_shapes(os.path.join(d, "anchor_shapes.json")), shapes)
    assert checkpoint.latest(d) == 1
    assert anchors.same_shapes(checkpoint.read_extra(d, 1)["anchor_shapes"], shapes)
    cov = json.load(open(os.path.join(d, "anchor_coverage.json")))
    assert cov["num_objects"] == rec["coverage_fitted"]["num_objects"] and cov["avg_iou"] == rec["coverage_fitted"]["avg_iou"]
    # eval.py on that directory, without the flag: the anchors are with_anchor_shapes' closed form for those shapes
    a = E.parse_args(["--checkpoint_path", d])
    found = drivers.driver_anchor_shapes(a.anchor_shapes, a.checkpoint_path)
    assert anchors.same_shapes(found, shapes)
    mc, model = E.make_model(a.net, a.gpu, a.dtype, 1, found)
    plain = S.kitti_squeezeDet_config()
    assert np.array_equal(mc.ANCHOR_BOX, config.set_anchors(plain, 24, 78, shapes)) and mc.ANCHORS == 16848
    assert np.array_equal(model.mc.ANCHOR_BOX, mc.ANCHOR_BOX)
    assert np.array_equal(model.anchors_f32().cpu().numpy(), mc.ANCHOR_BOX.astype(np.float32))
    del model
    # no flag and no file: the config's own anchors, as before
    b = E.parse_args(["--checkpoint_path", str(tmp_path / "elsewhere" / "model.ckpt-1.npz")])
    assert drivers.driver_anchor_shapes(b.anchor_shapes, b.checkpoint_path) is None
    assert np.array_equal(E.make_model(b.net, b.gpu, b.dtype, 1, None)[0].ANCHOR_BOX, plain.ANCHOR_BOX)
    # --resume with other shapes is refused; without the flag it runs on the recorded ones
    other = str(tmp_path / "other.json")
    anchors.save_anchor_shapes(other, shapes * [1.0, 1.5], plain)
    r = _child("train.py", train + ["--anchor_shapes", other, "--max_steps", "3", "--resume"], timeout=120)
    assert r.returncode != 0 and "--resume: the checkpoint was trained with anchor shapes" in r.stderr
    assert checkpoint.latest(d) == 1
    r = _child("train.py", train + ["--max_steps", "3", "--resume"])
    assert r.returncode == 0 and "Resuming from step 1" in r.stdout
    assert anchors.same_shapes(checkpoint.read_extra(d, 2)["anchor_shapes"], shapes)
