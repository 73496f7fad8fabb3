"""sqdet_augment_bgr_window (squeezedet_amd/csrc/augment.hip) on the GPU against the NumPy restatement of
tests/augment_policy_cases.py: 60 window cases (crops, zoom-outs, windows across every edge, 1 x 1, one column, one row, all
padding; both flips; three source sizes) in ONE launch, under no matrix, the identity, a saturating and a cross-channel matrix
and a per-image mix, into input_path_cases.AUG_DSTS at both base offsets.  float32 is compared BIT FOR BIT, float16 with
input_path_cases.check_augment (the rounding of the float32 value); padding is exactly 0 under every matrix.  The drift form is
bitwise ops.augment_bgr; BatchReader serves "ssd" batches through both of its source paths; train.py --augment ssd resumes to the
same loss bits.  tests/test_augment_policy_host.py shows without a GPU that the cases discriminate the likely mistakes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_policy_cases as AC
from tests import input_path_cases as IC

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


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dst", IC.AUG_DSTS, ids=["%dx%d" % d for d in IC.AUG_DSTS])
def test_window_cases_against_the_restatement(dst, dtype):
    from squeezedet_amd import ops
    hd, wd = dst
    _, flat_np, offsets = AC.win_source()
    flat, geom, n = _t(flat_np), AC.win_geom(), len(AC.WIN_IMAGES)
    f16 = dtype == torch.float16
    by_color = {}
    for color in AC.COLORS:
        ref, pad = AC.win_reference(hd, wd, color)
        M = AC.color_of(color)
        call = lambda out=None: ops.augment_bgr_window(flat, offsets, geom, M, hd, wd, IC.MEANS, dtype, out=out)
        plain = call()
        for base_off in IC.AUG_BASE_OFFSETS:
            what = "window %s -> %s %s offset %d" % (color, dst, dtype, base_off)
            view = _into_view(call, n, dtype, hd, wd, base_off, what)
            assert torch.equal(_bits(view), _bits(plain)), "%s: the store branch changed the values" % what
        out = plain.float().cpu().numpy()
        by_color[color] = plain
        worst = 0.0
        for k, (si, name, win, fl) in enumerate(AC.WIN_IMAGES):
            w = "%s %s %s flip %d, colour %s -> %s" % (AC.SOURCES[si], name, win, fl, color, dst)
            IC.check_augment(out[k], ref[k], pad[k], f16, w)
            worst = max(worst, float(np.abs(out[k] - ref[k]).max()))
            if not f16:
                assert np.array_equal(out[k].view(np.uint32), ref[k].view(np.uint32)), "%s: float32 is not bitwise the restatement (max abs %g)" % (
                    w, np.abs(out[k] - ref[k]).max())
        print("WINDOW %-7s %-8s %s: max abs error %.3g" % ("float16" if f16 else "float32", color, dst, worst))
        if f16:                                                   # the same float32 value, converted once
            out32 = ops.augment_bgr_window(flat, offsets, geom, M, hd, wd, IC.MEANS, torch.float32)
            assert torch.equal(_bits(plain), _bits(out32.half()))
    assert torch.equal(_bits(by_color["identity"]), _bits(by_color["null"])), "the identity matrix changed the values"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_drift_window_is_bitwise_augment_bgr(dtype):
    from squeezedet_amd import ops
    _, flat_np, offsets = IC.aug_source()
    flat = _t(flat_np)
    g5 = IC.aug_geom()
    g7 = AC.drift_as_window(g5)
    ident = np.tile(AC.IDENTITY.reshape(12), (len(g5), 1))
    for hd, wd in IC.AUG_DSTS:
        want = ops.augment_bgr(flat, offsets, g5, hd, wd, IC.MEANS, dtype)
        got = ops.augment_bgr_window(flat, offsets, g7, None, hd, wd, IC.MEANS, dtype)
        assert torch.equal(_bits(got), _bits(want)), (hd, wd)
        got = ops.augment_bgr_window(flat, offsets, g7, ident, hd, wd, IC.MEANS, dtype)
        assert torch.equal(_bits(got), _bits(want)), (hd, wd, "identity")


def test_only_the_output_is_written_and_invalid_device_geometry_is_left_alone():
    """Straight through ctypes, past the host validator: rows the kernel's own guard returns on (nothing is loaded for them) stay at
    the sentinel, their neighbours are written."""
    from squeezedet_amd import _lib
    hd, wd = 7, 261
    _, flat_np, offsets = AC.win_source()
    keep = [0, 1, 24, 25, 44, 45, 46, 47]
    geom = AC.win_geom()[keep].copy()
    offs = offsets[keep].copy()
    bad = {1: (4, 0), 2: (5, 65536), 3: (2, 65536), 4: (3, -65536), 5: (6, 2), 6: (4, -3)}
    for row, (col, val) in bad.items():
        geom[row, col] = val
    offs[7] = flat_np.size - 10                                     # an image that would end past the buffer
    n = len(keep)
    flat, gd, od = _t(flat_np), _t(geom.astype(np.int32)), _t(offs.astype(np.int64))
    cd = _t(np.tile(AC.CROSS.reshape(12), (n, 1)))
    for dtype in (torch.float32, torch.float16):
        for color in (None, cd):
            m = n * hd * wd * 3
            buf = torch.full((GUARD + m + GUARD,), 1234.5, dtype=dtype, device=DEV)
            view = buf[GUARD:GUARD + m].view(n, hd, wd, 3)
            _lib.check(_lib.lib().sqdet_augment_bgr_window(C.c_void_p(flat.data_ptr()), flat.numel(), C.c_void_p(od.data_ptr()),
                                                           C.c_void_p(gd.data_ptr()), None if color is None else C.c_void_p(color.data_ptr()),
                                                           C.c_void_p(view.data_ptr()), n, hd, wd, *[float(v) for v in IC.MEANS.reshape(-1)],
                                                           _lib.dtype_code(dtype), _lib.stream_ptr()), "sqdet_augment_bgr_window")
            torch.cuda.synchronize()
            assert bool((buf[:GUARD] == 1234.5).all()) and bool((buf[GUARD + m:] == 1234.5).all())
            for row in range(n):
                untouched = bool((view[row] == 1234.5).all())
                assert untouched == (row != 0), "row %d (%s): %s" % (row, geom[row].tolist(), "left alone" if untouched else "written")
            si, _, win, fl = AC.WIN_IMAGES[keep[0]]
            ref = AC.window_restatement(AC.win_source()[0][si], win, fl, None if color is None else AC.CROSS, hd, wd)
            pad = AC.window_pad_mask(*AC.SOURCES[si], win, fl, hd, wd)
            IC.check_augment(view[0].float().cpu().numpy(), ref, pad, dtype == torch.float16, "the valid row")


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "pinned"])
def test_reader_serves_mixed_sizes_in_one_launch(resident, monkeypatch):
    from squeezedet_amd import BatchReader, ops
    images, rois = AC.policy_dataset()
    mc = AC.policy_config(batch=6)
    calls = []
    real = ops.augment_bgr_window
    monkeypatch.setattr(ops, "augment_bgr_window", lambda *a, **k: calls.append(np.asarray(a[2]).copy()) or real(*a, **k))
    monkeypatch.setattr(ops, "augment_bgr", lambda *a, **k: pytest.fail("the drift entry was launched under 'ssd'"))
    r = BatchReader(mc, images, rois, seed=6, device=DEV, resident=resident)
    sizes = set()
    for step in range(3):
        b = r.read_batch()
        torch.cuda.synchronize()
        assert len(calls) == step + 1 and len(calls[-1]) == 6                     # one launch for the batch
        out = b.image_input.cpu().numpy()
        assert out.shape == (6, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, 3) and b.color.shape == (6, 12)
        for k, idx in enumerate(b.batch_idx):
            sizes.add(images[idx].shape[:2])
            win, fl = tuple(int(v) for v in b.window[k]), int(b.aug[k, 2])
            assert calls[-1][k].tolist() == list(images[idx].shape[:2]) + list(win) + [fl]
            ref = AC.window_restatement(images[idx], win, fl, b.color[k].reshape(3, 4), mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH)
            assert np.array_equal(out[k].view(np.uint32), ref.view(np.uint32)), (step, k, win, fl)
            assert int(b.gt_counts[k]) == len(b.bbox_per_batch[k])
    assert len(sizes) >= 3


def _child(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    print(r.stdout[-2000:])
    print(r.stderr[-2000:])
    return r


def test_driver_runs_and_resumes_to_the_same_bits(tmp_path):
    """train.py --synthetic 8 --augment ssd --zoom_out 2 --color_jitter --max_steps 3: two steps, --resume to three, against three
    steps straight (step 1 a graph replay, steps 0 and 2 summary steps) -- the same variables bit for bit and the same printed losses; --resume under another policy is refused."""
    from squeezedet_amd import checkpoint, weights
    d1, d2 = str(tmp_path / "resumed"), str(tmp_path / "straight")
    common = ["--synthetic", "8", "--augment", "ssd", "--zoom_out", "2", "--color_jitter", "--image_size", "128", "256", "--batch_size", "2",
              "--summary_step", "2", "--checkpoint_step", "0"]
    r = _child(common + ["--train_dir", d1, "--max_steps", "2"])
    assert r.returncode == 0, "train.py --augment ssd failed"
    assert checkpoint.read_extra(d1, 1)["augment"] == dict(geometry="ssd", zoom_out=2.0, color_jitter=True)
    r = _child(common + ["--train_dir", d1, "--max_steps", "3", "--resume"])
    assert r.returncode == 0 and "Resuming from step 1" in r.stdout
    resumed = [l for l in r.stdout.splitlines() if l.startswith("conf_loss: ")]
    r = _child(common + ["--train_dir", d2, "--max_steps", "3"])
    assert r.returncode == 0
    straight = [l for l in r.stdout.splitlines() if l.startswith("conf_loss: ")]
    assert len(straight) == 2 and len(resumed) == 1 and resumed[0] == straight[1]          # the summary steps 0 and 2
    a, b = weights.load_params(os.path.join(d1, "model.ckpt-2.npz")), weights.load_params(os.path.join(d2, "model.ckpt-2.npz"))
    assert set(a) == set(b)
    for name in a:
        assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), name
    refused = _child(["--synthetic", "8", "--image_size", "128", "256", "--batch_size", "2", "--train_dir", d1, "--max_steps", "4", "--resume"])
    assert refused.returncode != 0 and "--resume: the checkpoint was trained with augment" in refused.stderr
