"""GPU tests of the two kernels that produce what a training step consumes, at their edges: squeezedet_amd/csrc/labels.hip
(labels_zero_kernel, labels_best_kernel, labels_resolve_kernel behind sqdet_build_labels) and squeezedet_amd/csrc/augment.hip
(augment_kernel behind sqdet_augment_bgr).  The cases, the references (oracle.train_oracle.assign_anchors in float64; the NumPy
restatement of imdb.py:141-186) and the comparison functions are tests/input_path_cases.py; tests/test_input_path_host.py shows
without a GPU that every case reaches the branch it is named after and that the comparisons reject wrong results.

Labels, every case: anchor_index equals the oracle's picks exactly (-1 behind the clipped count); input_mask, labels and
box_input equal the dense reference exactly; box_delta_input[..., 0:2] has the bits of the float64 quotient rounded once to
float32 (the float64 division is correctly rounded, the file is built with -ffp-contract=off); [..., 2:4] is within the project's
rtol 1e-6 / atol 1e-7 of the float64 log rounded once (-inf where the box has no width).

  case        A       what it reaches (oracle: clashes / distance-mode picks / picks tied in IoU / tied in distance, per image)
  dup         546     every value ties between a and a + 273 (other lanes and waves)          3/3/20/2, 0/0/7/0
  mirror      273     two- and four-way IoU ties, a two-way distance tie, a tie's runner-up   1/1/2/1
  full        273     M == A: every anchor claimed, the last word of the bit set              160/38/105/5
  far         546     40 boxes in the distance sweep, tied across the copies                  22/40/0/21
  cap         1080    M = 1024 (thread 1023 keeps a box), counts 1030 (clipped) and -3        541/80/89/0, 568/62/95/0, none
  big         480000  the 60000-byte LDS cap; a bit in its last word, then a clash            1/1/0/0
  classes1/20 273     class ids -1 and C: the row is written without a label                  1/0/3/0, 0/0/1/0; 1/0/0/0, 1/0/1/0
  degenerate  273     a box of width 0: the distance sweep, delta[2] = -inf                    0/1/0/0
  three, one  3, 1    A < 64 and A == 1: threads (lanes, waves) without a candidate            1/1/0/0, 0/0/0/0; none

Augment: AUG_IMAGES (seven geometries x both flips, extreme drifts of -65535 on one axis, a drift that leaves one row and one
column, packed with odd byte counts) into (7, 261), (12, 262), (7, 259), (12, 5), float32 and float16, into a view of a NaN-filled
buffer that starts 8-byte aligned and one element behind that.  float32: the project's criterion (<= 2e-4, >= 99.9 % of the
elements equal, per image); float16: |out - ref| <= 2e-4 + 2^-11 (|ref| + 2e-4) + 2^-25 (the float32 allowance and one correctly
rounded conversion) instead of the flat 0.07; both: exactly 0 wherever the reference is zero padding, and the cells around the
view stay NaN.

Measured on an MI355X: every new augment case is bit-equal to the reference in float32 (share of unequal elements 0 in all eight
destination / offset combinations, max abs error 0), float16 is bitwise the float32 output's .half().  No defect was found:
labels.hip and augment.hip are unchanged."""
import numpy as np
import pytest
import torch

from tests import input_path_cases as IC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                 # NaN cells in front of and behind a destination view


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # a copy: the cases' arrays are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _label_inputs(c):
    return _t(c.anchors), _t(c.gt), _t(c.cls), _t(c.cnt)


def _label_outputs(B, A, M, C, fill=float("nan"), ifill=-7):
    f = lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV)
    return f(B, A), f(B, A, 4), f(B, A, 4), f(B, A, C), torch.full((B, M), ifill, dtype=torch.int32, device=DEV)


def _abi_build_labels(anc, gt, cls, cnt, outs, B, A, M, C):
    """The C entry called as ops.build_labels calls it, on outputs the caller allocated (and dirtied)."""
    from squeezedet_amd import _lib
    p = [t.data_ptr() for t in (anc, gt, cls, cnt) + tuple(outs)]
    _lib.check(_lib.lib().sqdet_build_labels(*p, B, A, M, C, _lib.stream_ptr()), "sqdet_build_labels")
    torch.cuda.synchronize()


def _check_labels(name, outs):
    c, ref = IC.label_case(name), IC.label_reference(name)
    mask, delta, box, lab, aidx = [t.cpu().numpy() for t in outs]
    assert aidx.dtype == np.int32 and mask.dtype == delta.dtype == box.dtype == lab.dtype == np.float32
    for b in range(len(c.cnt)):
        n = IC.clipped_count(c, b)
        assert aidx[b, :n].tolist() == ref.aidx[b, :n].tolist(), "%s image %d: anchor picks differ from the oracle's" % (name, b)
        assert (aidx[b, n:] == -1).all(), "%s image %d: a row behind the count is not -1" % (name, b)
    assert np.array_equal(mask, ref.mask), "%s: input_mask" % name
    assert np.array_equal(lab, ref.labels), "%s: labels" % name
    assert np.array_equal(box, ref.box), "%s: box_input" % name
    want = ref.delta64.astype(np.float32)                       # rounded once
    assert np.array_equal(_bits(delta[..., 0:2]), _bits(want[..., 0:2])), "%s: box_delta_input[..., 0:2] bits" % name
    np.testing.assert_allclose(delta[..., 2:4], want[..., 2:4], rtol=1e-6, atol=1e-7, err_msg="%s: box_delta_input[..., 2:4]" % name)
    assert np.array_equal(np.isinf(delta), np.isinf(want)) and not np.isnan(delta).any()


@pytest.mark.parametrize("name", IC.LABEL_CASES)
def test_build_labels_edge_case_against_the_oracle(name):
    from squeezedet_amd import ops
    c = IC.label_case(name)
    outs = ops.build_labels(*_label_inputs(c), c.C)
    torch.cuda.synchronize()
    _check_labels(name, outs)


@pytest.mark.parametrize("name", ["dup", "full", "classes1", "classes20", "cap", "one"])
def test_build_labels_clears_dirty_outputs(name):
    """Every element of the five outputs, prefilled with NaN / -7, equals the reference: labels_zero_kernel is complete."""
    c = IC.label_case(name)
    (B, M), A = c.cls.shape, len(c.anchors)
    outs = _label_outputs(B, A, M, c.C)
    _abi_build_labels(*_label_inputs(c), outs, B, A, M, c.C)
    _check_labels(name, outs)


def test_build_labels_same_bits_on_a_second_call():
    from squeezedet_amd import ops
    c = IC.label_case("dup")
    first = [t.clone() for t in ops.build_labels(*_label_inputs(c), c.C)]
    o = IC.label_case("far")
    ops.build_labels(*_label_inputs(o), o.C)
    again = ops.build_labels(*_label_inputs(c), c.C)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    _check_labels("dup", again)


@pytest.mark.parametrize("bad", ["M>A", "M=1025", "A=480001", "batch=0", "max_objects=0", "classes=0", "anchors=0"])
def test_build_labels_rejections_leave_the_outputs_untouched(bad):
    from squeezedet_amd import _lib
    B, A, M, C = 1, 1080, 4, 3
    err = _lib.SqdetUnsupported
    if bad == "M>A":
        A = 3
    elif bad == "M=1025":
        M = IC.LABELS_MAX_OBJECTS + 1
    elif bad == "A=480001":
        A = IC.BIG_A + 1
    else:
        err = _lib.SqdetError
    anc = torch.ones((A, 4), dtype=torch.float64, device=DEV)
    gt = torch.ones((B, M, 4), dtype=torch.float64, device=DEV)
    cls = torch.zeros((B, M), dtype=torch.int32, device=DEV)
    cnt = torch.full((B,), M, dtype=torch.int32, device=DEV)
    outs = _label_outputs(B, A, M, C)
    dims = {"batch=0": (0, A, M, C), "max_objects=0": (B, A, 0, C), "classes=0": (B, A, M, 0), "anchors=0": (B, 0, M, C)}.get(bad, (B, A, M, C))
    with pytest.raises(err) as e:
        _abi_build_labels(anc, gt, cls, cnt, outs, *dims)
    assert (e.type is _lib.SqdetUnsupported) == (err is _lib.SqdetUnsupported)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs[:4]) and bool((outs[4] == -7).all())


# ================================================================== augment
def _augment_into_view(flat, offsets, dtype, hd, wd, base_off):
    """ops.augment_bgr into a view that starts `base_off` elements behind an 8-byte aligned cell of a NaN-filled buffer; asserts
    the cells around the view are still NaN; the view."""
    from squeezedet_amd import ops
    n = len(IC.AUG_IMAGES)
    m = n * hd * wd * 3
    buf = torch.full((GUARD + base_off + m + GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = buf[GUARD + base_off:GUARD + base_off + m].view(n, hd, wd, 3)
    assert (view.data_ptr() - base_off * buf.element_size()) % 8 == 0
    out = ops.augment_bgr(flat, offsets, IC.aug_geom(), hd, wd, IC.MEANS, dtype, out=view)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    what = "augment -> %s %s offset %d" % ((hd, wd), dtype, base_off)
    assert bool(torch.isnan(buf[:GUARD + base_off]).all()), "%s: a cell in front of the view was written" % what
    assert bool(torch.isnan(buf[GUARD + base_off + m:]).all()), "%s: a cell behind the view was written" % what
    return view


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("dst", IC.AUG_DSTS, ids=["%dx%d" % d for d in IC.AUG_DSTS])
def test_augment_edge_cases_against_the_restatement(dst, dtype):
    from squeezedet_amd import ops
    hd, wd = dst
    _, flat_np, offsets = IC.aug_source()
    flat = _t(flat_np)
    ref, pad = IC.aug_reference(hd, wd)
    f16 = dtype == torch.float16
    plain = ops.augment_bgr(flat, offsets, IC.aug_geom(), hd, wd, IC.MEANS, dtype)
    for base_off in IC.AUG_BASE_OFFSETS:
        view = _augment_into_view(flat, offsets, dtype, hd, wd, base_off)
        assert torch.equal(view.view(torch.int16 if f16 else torch.int32), plain.view(torch.int16 if f16 else torch.int32)), \
            "the store branch changed the values (offset %d)" % base_off
        out = view.float().cpu().numpy()
        unequal, total, worst = 0.0, 0, 0.0
        for k, (s, dx, dy, fl) in enumerate(IC.AUG_IMAGES):
            share = IC.check_augment(out[k], ref[k], pad[k], f16, "%s (%d, %d) flip %d -> %s offset %d" % (s, dx, dy, fl, dst, base_off))
            unequal, total = unequal + share * out[k].size, total + out[k].size
            worst = max(worst, float(np.abs(out[k] - ref[k]).max()))
        print("AUGMENT %-7s %s offset %d: %.6f of %d elements differ from the reference, max abs error %.3g"
              % ("float16" if f16 else "float32", dst, base_off, unequal / total, total, worst))
    if f16:                                                     # the same float32 value, converted once
        out32 = ops.augment_bgr(flat, offsets, IC.aug_geom(), hd, wd, IC.MEANS, torch.float32)
        assert torch.equal(plain.view(torch.int16), out32.half().view(torch.int16))
