"""sqdet_augment_bgr_mosaic (squeezedet_amd/csrc/augment.hip) on the GPU against the NumPy restatement of tests/mosaic_cases.py:
per destination one launch over every split of XCS x YCS (the 256-pixel chunk edge, the 4-pixel group edge, the image's own edges,
every form with one, two or four panes) with the parts taken in turn from augment_policy_cases.WIN_IMAGES, under no matrix, a
cross-channel matrix and a per-part mix, at both base offsets.  float32 is compared BIT FOR BIT, float16 is bitwise the float32
output converted once and within input_path_cases.check_augment.  A single pane is bitwise ops.augment_bgr_window; panes and
images that the kernel's own guard skips stay at their canary; BatchReader serves mosaic batches in one launch through both of its
source paths; train.py --mosaic resumes to the same bits.  tests/test_mosaic_host.py shows without a GPU that the cases
discriminate the likely mistakes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_policy_cases as AC
from tests import input_path_cases as IC
from tests import mosaic_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _into_view(fn, n, dtype, hd, wd, base_off, what):
    """fn(out=view) into a view `base_off` elements behind an 8-byte aligned cell of a NaN-filled buffer; the cells around the view
    must stay NaN."""
    m = n * hd * wd * 3
    buf = torch.full((GUARD + base_off + m + GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[GUARD + base_off:GUARD + base_off + m].view(n, hd, wd, 3)
    assert (view.data_ptr() - base_off * buf.element_size()) % 8 == 0
    out = fn(view)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    assert bool(torch.isnan(buf[:GUARD + base_off]).all()), "%s: a cell in front of the view was written" % what
    assert bool(torch.isnan(buf[GUARD + base_off + m:]).all()), "%s: a cell behind the view was written" % what
    return view


def _raw(flat, off, geom, split, color, view, dtype):
    """The library call itself, past the host validator: whatever the arrays hold reaches the device."""
    from squeezedet_amd import _lib
    n, hd, wd = int(view.shape[0]), int(view.shape[1]), int(view.shape[2])
    od, gd, sd = _t(np.asarray(off, np.int64)), _t(np.asarray(geom, np.int32)), _t(np.asarray(split, np.int32))
    cd = None if color is None else _t(np.asarray(color, np.float32).reshape(n, 4, 12))
    assert tuple(od.shape) == (n, 4) and tuple(gd.shape) == (n, 4, 7) and tuple(sd.shape) == (n, 2)
    _lib.check(_lib.lib().sqdet_augment_bgr_mosaic(C.c_void_p(flat.data_ptr()), flat.numel(), C.c_void_p(od.data_ptr()), C.c_void_p(gd.data_ptr()),
                                                   C.c_void_p(sd.data_ptr()), None if cd is None else C.c_void_p(cd.data_ptr()),
                                                   C.c_void_p(view.data_ptr()), n, hd, wd, *[float(v) for v in IC.MEANS.reshape(-1)],
                                                   _lib.dtype_code(dtype), _lib.stream_ptr()), "sqdet_augment_bgr_mosaic")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dst", MC.DSTS, ids=["%dx%d" % d for d in MC.DSTS])
def test_mosaic_cases_against_the_restatement(dst, dtype):
    from squeezedet_amd import ops
    hd, wd = dst
    flat = _t(AC.win_source()[1])
    off, geom, split = MC.mosaic_arrays(hd, wd)
    imgs = MC.mosaic_images(hd, wd)
    n, f16 = len(imgs), dtype == torch.float16
    for color in MC.COLORS:
        ref, pad = MC.mosaic_reference(hd, wd, color)
        M = MC.color_with_garbage(color, hd, wd)
        call = lambda out=None: ops.augment_bgr_mosaic(flat, off, geom, split, M, hd, wd, IC.MEANS, dtype, out=out)
        plain = call()
        for base_off in MC.BASE_OFFSETS:
            what = "mosaic %s -> %s %s offset %d" % (color, dst, dtype, base_off)
            view = _into_view(call, n, dtype, hd, wd, base_off, what)
            assert torch.equal(_bits(view), _bits(plain)), "%s: the store branch changed the values" % what
        out = plain.float().cpu().numpy()
        worst = 0.0
        for k, (name, _, parts) in enumerate(imgs):
            w = "%s %s, colour %s -> %s" % (name, [part and part[:2] + part[3:] for part in parts], color, dst)
            IC.check_augment(out[k], ref[k], pad[k], f16, w)
            worst = max(worst, float(np.abs(out[k] - ref[k]).max()))
            if not f16:
                assert np.array_equal(out[k].view(np.uint32), ref[k].view(np.uint32)), "%s: float32 is not bitwise the restatement (max abs %g)" % (
                    w, np.abs(out[k] - ref[k]).max())
        print("MOSAIC %-7s %-6s %s: %d images, max abs error %.3g" % ("float16" if f16 else "float32", color, dst, n, worst))
        if f16:                                                   # the same float32 value, converted once
            out32 = ops.augment_bgr_mosaic(flat, off, geom, split, M, hd, wd, IC.MEANS, torch.float32)
            assert torch.equal(_bits(plain), _bits(out32.half()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("pane", [0, 1, 2, 3])
def test_one_pane_is_bitwise_the_window_entry(pane, dtype):
    """split = (W, H) shows part 0 alone, (0, H) part 1, (W, 0) part 2, (0, 0) part 3: bitwise ops.augment_bgr_window of that part,
    whatever the other three parts hold -- through ops, and with the garbage uploaded as it is."""
    from squeezedet_amd import ops
    _, flat_np, offsets = AC.win_source()
    flat, g7, n = _t(flat_np), AC.win_geom(), len(AC.WIN_IMAGES)
    for hd, wd in [(7, 261), (12, 5), (9, 520)]:
        split = np.tile(np.array([(wd, hd), (0, hd), (wd, 0), (0, 0)][pane], np.int64), (n, 1))
        off = np.full((n, 4), MC.GARBAGE_OFFSET, np.int64)
        geom = np.tile(np.array(MC.GARBAGE_GEOM, np.int64), (n, 4, 1))
        off[:, pane], geom[:, pane] = offsets, g7
        for color in ("null", "mixed"):
            M1 = AC.color_of(color)
            M4 = None
            if M1 is not None:
                M4 = np.full((n, 4, 12), np.nan, np.float32)
                M4[:, pane] = M1.reshape(n, 12)
            want = ops.augment_bgr_window(flat, offsets, g7, M1, hd, wd, IC.MEANS, dtype)
            got = ops.augment_bgr_mosaic(flat, off, geom, split, M4, hd, wd, IC.MEANS, dtype)
            assert torch.equal(_bits(got), _bits(want)), (hd, wd, color)
            raw = torch.full_like(want, float("nan"))
            _raw(flat, off, geom, split, M4, raw, dtype)
            assert torch.equal(_bits(raw), _bits(want)), (hd, wd, color, "garbage on the device")


def test_skipped_panes_and_images_stay_at_their_canary():
    """Straight through ctypes, past the host validator.  This is the kernel's documented skip path: a workgroup whose pane (or
    split) breaks the rules returns before it loads anything, so nothing faults; the panes around it are written."""
    hd, wd = 7, 261
    xc, yc = 100, 3
    _, flat_np, offsets = AC.win_source()
    flat = _t(flat_np)
    g7 = AC.win_geom()
    pick = [0, 25, 44, 13]                                                      # the four parts of every image
    n = 7
    off = np.tile(offsets[pick], (n, 1))
    geom = np.tile(g7[pick], (n, 1, 1))
    split = np.tile(np.array([xc, yc], np.int64), (n, 1))
    geom[1, 1, 6] = 2                                                           # a flip that is neither 0 nor 1
    geom[2, 2, 4] = 0                                                           # cw = 0
    split[3] = (wd + 1, yc)
    split[4] = (xc, -1)
    off[5, 3] = flat_np.size - 10                                               # a source image that would end past the buffer
    geom[6, 0, 0] = 0                                                           # src_h = 0
    skipped = {1: [1], 2: [2], 3: [0, 1, 2, 3], 4: [0, 1, 2, 3], 5: [3], 6: [0]}
    sources = AC.win_source()[0]
    parts = [AC.WIN_IMAGES[q] for q in pick]
    for dtype in (torch.float32, torch.float16):
        for color in (None, np.tile(AC.CROSS.reshape(12), (n, 4, 1))):
            m = n * hd * wd * 3
            buf = torch.full((GUARD + m + GUARD,), 1234.5, dtype=dtype, device=DEV)
            view = buf[GUARD:GUARD + m].view(n, hd, wd, 3)
            _raw(flat, off, geom, split, color, view, dtype)
            assert bool((buf[:GUARD] == 1234.5).all()) and bool((buf[GUARD + m:] == 1234.5).all())
            ref = MC.mosaic_restatement(sources, parts, (xc, yc), None if color is None else np.tile(AC.CROSS, (4, 1, 1)), hd, wd)
            pad = MC.mosaic_pad_mask(parts, (xc, yc), hd, wd)
            out = view.float().cpu().numpy()
            canary = float(buf[0])                                                # (1234.5 as float32, 1234 as float16)
            for i in range(n):
                want = ref.copy()
                for p in skipped.get(i, []):
                    px0, py0, pw, ph = MC.panes(xc, yc, wd, hd)[p]
                    want[py0:py0 + ph, px0:px0 + pw] = np.nan
                    assert (out[i, py0:py0 + ph, px0:px0 + pw] == canary).all(), "image %d: pane %d was written" % (i, p)
                keep = ~np.isnan(want[..., 0])
                assert (out[i][keep] != canary).any(axis=-1).all() or not keep.any(), "image %d: a valid pane was left alone" % i
                got = np.where(keep[..., None], out[i], 0).astype(np.float32)
                IC.check_augment(got, np.where(keep[..., None], ref, 0).astype(np.float32), pad | ~keep, dtype == torch.float16, "image %d" % i)


@pytest.mark.parametrize("prob", [1.0, 0.5])
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "pinned"])
def test_reader_serves_mosaics_in_one_launch(resident, prob, monkeypatch):
    from squeezedet_amd import BatchReader, ops
    images, rois = AC.policy_dataset()
    mc = AC.policy_config(batch=6)
    mc.AUG_MOSAIC_PROB = prob
    calls = []
    real = ops.augment_bgr_mosaic
    monkeypatch.setattr(ops, "augment_bgr_mosaic", lambda *a, **k: calls.append(np.asarray(a[3]).copy()) or real(*a, **k))
    monkeypatch.setattr(ops, "augment_bgr_window", lambda *a, **k: pytest.fail("the window entry was launched with the mosaic on"))
    monkeypatch.setattr(ops, "augment_bgr", lambda *a, **k: pytest.fail("the drift entry was launched with the mosaic on"))
    r = BatchReader(mc, images, rois, seed=6, device=DEV, resident=resident)
    anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(DEV)
    modes = set()
    for step in range(3):
        b = r.read_batch()
        torch.cuda.synchronize()
        assert len(calls) == step + 1 and len(calls[-1]) == 6                     # one launch for the batch
        assert np.array_equal(calls[-1], b.split)
        out = b.image_input.cpu().numpy()
        assert out.shape == (6, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, 3) and b.part_color.shape == (6, 4, 12)
        ref = MC.plan_restatement(images, b, mc)
        assert np.isfinite(ref).all()
        for k in range(6):
            modes.add(b.mode[k] == "mosaic")
            assert np.array_equal(out[k].view(np.uint32), ref[k].view(np.uint32)), (step, k, b.split[k], b.parts[k])
        M = r.max_objects
        gt, cls, cnt = b.gt_boxes.cpu().numpy(), b.gt_classes.cpu().numpy(), b.gt_counts.cpu().numpy()
        assert gt.shape == (6, M, 4) and cls.shape == (6, M) and M == 4 * max(len(x) for x in rois)
        for k in range(6):
            c = len(b.label_per_batch[k])
            assert cnt[k] == c and np.array_equal(gt[k, :c], b.bbox_per_batch[k]) and cls[k, :c].tolist() == list(b.label_per_batch[k])
            assert (gt[k, c:] == 0).all()
        labels = ops.build_labels(anchors, b.gt_boxes, b.gt_classes, b.gt_counts, mc.CLASSES)
        torch.cuda.synchronize()
        assert float(labels[0].sum().item()) == float(cnt.sum()), "every box claims one anchor"
    assert modes == ({True} if prob == 1.0 else {True, False})


def test_image_summary_draws_a_batch_padded_for_mosaics():
    """A mosaic reader pads the ground truth to four times the largest object count; with TOP_N_DETECTION detections that can pass
    the 256 items of one draw launch although the boxes themselves fit.  The picture is that of the same batch without the padding."""
    from squeezedet_amd import Batch, viz
    mc = AC.policy_config()
    H, W, M = mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, 200
    assert M + mc.TOP_N_DETECTION > viz.MAX_ITEMS
    rs = np.random.RandomState(3)
    x = _t(rs.uniform(-100, 100, (2, H, W, 3)).astype(np.float32))
    gt = np.zeros((2, M, 4), np.float64)
    gt[0, :3] = [[40, 30, 30, 20], [100, 60, 50, 40], [20, 80, 12, 10]]
    gt[1, :1] = [[80, 48, 60, 30]]
    cls = np.zeros((2, M), np.int32)
    cls[0, :3] = [0, 1, 2]
    preds = _t(rs.uniform(-1, 1, (2, H // 16, W // 16, mc.ANCHOR_PER_GRID * (mc.CLASSES + 5))).astype(np.float32))
    assert preds.shape[1] * preds.shape[2] * mc.ANCHOR_PER_GRID == len(mc.ANCHOR_BOX)
    labels = [[0, 1, 2], [0]]
    padded = Batch(x, _t(gt), _t(cls), _t(np.array([3, 1], np.int32)), None, None, labels, [0, 1])
    plain = Batch(x, _t(gt[:, :3]), _t(cls[:, :3]), _t(np.array([3, 1], np.int32)), None, None, labels, [0, 1])
    s = viz.ImageSummary(mc, "unused", 2, device=DEV, write=False)
    got, want = s.render(padded, preds), s.render(plain, preds)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, H, W, 3) and torch.equal(got, want)
    assert not torch.equal(got, s.render(plain._replace(gt_counts=_t(np.zeros(2, np.int32))), preds)), "no ground truth was drawn"


def _child(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    print(r.stdout[-2000:])
    print(r.stderr[-2000:])
    return r


def test_driver_runs_and_resumes_to_the_same_bits(tmp_path):
    """train.py --synthetic 8 --mosaic 0.5: two steps, --resume to three, against three steps straight -- the same variables bit for
    bit; the probability is recorded under its own key beside an unchanged `augment` record; --resume under another one is refused."""
    from squeezedet_amd import checkpoint, weights
    d1, d2 = str(tmp_path / "resumed"), str(tmp_path / "straight")
    common = ["--synthetic", "8", "--mosaic", "0.5", "--image_size", "128", "256", "--batch_size", "2", "--summary_step", "2", "--checkpoint_step", "0"]
    r = _child(common + ["--train_dir", d1, "--max_steps", "2"])
    assert r.returncode == 0, "train.py --mosaic failed"
    extra = checkpoint.read_extra(d1, 1)
    assert extra["mosaic"] == 0.5 and extra["augment"] == dict(geometry="reference", zoom_out=1.0, color_jitter=False)
    r = _child(common + ["--train_dir", d1, "--max_steps", "3", "--resume"])
    assert r.returncode == 0 and "Resuming from step 1" in r.stdout
    r = _child(common + ["--train_dir", d2, "--max_steps", "3"])
    assert r.returncode == 0
    a, b = weights.load_params(os.path.join(d1, "model.ckpt-2.npz")), weights.load_params(os.path.join(d2, "model.ckpt-2.npz"))
    assert set(a) == set(b)
    for name in a:
        assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), name
    refused = _child(["--synthetic", "8", "--mosaic", "0", "--image_size", "128", "256", "--batch_size", "2", "--train_dir", d1, "--max_steps", "4",
                      "--resume"])
    assert refused.returncode != 0 and "--resume: the checkpoint was trained with mosaic 0.5" in refused.stderr
