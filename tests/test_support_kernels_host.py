"""The references, bounds and comparison functions of tests/test_gpu_support_kernels.py checked on their own: no GPU.

  * the float64 fold references agree with oracle.resnet_oracle.fold_batchnorm to float32 accuracy (forward) and the closed-form
    float64 gradients with torch-CPU float64 autograd (backward);
  * every derived bound holds for a float32 NumPy restatement of the kernel's own evaluation order on every input the GPU tests
    use: the reference alone stays inside what the GPU test allows;
  * every "exact" preprocessing case is exact: a float64 evaluation of the oracle's algorithm has the bits of its float32
    evaluation, before the mean subtraction without any rounding at all;
  * the comparison functions reject deliberately wrong outputs produced in NumPy (the mutation check: never a broken kernel);
  * the cap cases exceed the caps quoted from bn.hip."""
import numpy as np
import pytest
import torch

from oracle import preproc_oracle as PO
from oracle import resnet_oracle as R
from tests import test_gpu_support_kernels as K


# ------------------------------------------------------------------ fold forward
def _fold_cases():
    return [(shape, bias, kind) for shape, bias in K.FOLD_CASES for kind in K.FOLD_KINDS]


def test_fold_reference_agrees_with_the_float32_oracle():
    for shape, bias, kind in _fold_cases():
        d, eps = K.fold_inputs(shape, bias, kind)
        rw, rb, bw, bb = K.fold_reference(d, eps)
        t = lambda a: torch.from_numpy(a) if a is not None else None
        ow, ob = R.fold_batchnorm(t(d["w"]), t(d["cb"]), t(d["gamma"]), t(d["beta"]), t(d["mean"]), t(d["var"]), eps=eps)
        assert ow.dtype == torch.float32
        assert (np.abs(ow.numpy() - rw) <= bw).all() and (np.abs(ob.numpy() - rb) <= bb).all(), (shape, bias, kind)


def test_fold_inputs_hold_the_edge_table():
    for shape, bias in K.FOLD_CASES:
        d, eps = K.fold_inputs(shape, bias, "edges")
        cout = shape[2]
        assert eps == float(np.float32(R.BN_EPS)) > 0
        assert (d["var"] == 0).sum() == 1 and (d["gamma"] < 0).any() and (d["gamma"] == 0).any() and (np.abs(d["mean"]) > 1e4).any()
        assert (d["mean"] == 0).any() or cout == 4              # (cout 4: the large mean shares channel 0 with var = 0; mean = 0 is channel 3)
        assert d["mean"][3] == 0 and (d["cb"] is not None) == bias
        assert K.fold_inputs(shape, bias, "eps0")[1] == 0.0
        o, _ = K.fold_inputs(shape, bias, "ordinary")
        assert o["gamma"].min() >= 0.5 and o["var"].min() >= 0.5 and o["gamma"].max() <= 1.5 and o["var"].max() <= 1.5


def test_fold_restatement_stays_inside_the_bounds():
    for shape, bias, kind in _fold_cases():
        d, eps = K.fold_inputs(shape, bias, kind)
        wf, bf = K.fold_restatement32(d, eps)
        qw, qb = K.check_fold(wf, bf, d, eps, "%s %s" % (shape, kind))
        # the restatement's operations are correctly rounded: it uses at most 3.5 u of the 6 u and 5.5 u of the 8 u
        assert qw <= 3.5 / 6.0 + 1e-6 and qb <= 5.5 / 8.0 + 1e-6, (shape, kind, qw, qb)


def test_fold_check_rejects_wrong_outputs():
    big = K.FOLD_CASES[-1][0]
    assert big == (1, 4100, 1028)
    for shape, bias in K.FOLD_CASES:
        d, eps = K.fold_inputs(shape, bias, "ordinary")
        wf, bf = K.fold_restatement32(d, eps)
        cout = shape[2]
        if cout > 4:                                            # the folded bias taken from channel c + 4
            with pytest.raises(AssertionError, match="bf error"):
                K.check_fold(wf, np.roll(bf, -4), d, eps)
        with pytest.raises(AssertionError, match="wf error"):   # inv of the neighbouring channel
            K.check_fold(np.roll(wf, 1, axis=-1) if cout > 4 else wf * np.float32(1 + 2.0 ** -20), bf, d, eps)
        if shape == big:                                        # the second grid-stride pass left unwritten
            holed = wf.copy().reshape(-1)
            holed[4 * K.FOLD_CAP_VECS:] = np.nan
            with pytest.raises(AssertionError, match="non-finite"):
                K.check_fold(holed.reshape(wf.shape), bf, d, eps)
            holed[4 * K.FOLD_CAP_VECS:] = d["w"].reshape(-1)[4 * K.FOLD_CAP_VECS:]       # ... or left holding the unfolded kernel
            with pytest.raises(AssertionError, match="wf error"):
                K.check_fold(holed.reshape(wf.shape), bf, d, eps)


# ------------------------------------------------------------------ fold backward
def _fold_bwd_cases():
    return [(shape, bias) for shape in K.FOLD_BWD_SHAPES for bias in (False, True)]


def test_fold_bwd_closed_form_is_autograd():
    for shape, bias in _fold_bwd_cases():
        d = K.fold_bwd_inputs(shape, bias)
        aw, ag, ab = K.fold_bwd_reference(d, K.FOLD_BWD_EPS)
        cw, cg, cb, r, S = K.fold_bwd_closed_form(d, K.FOLD_BWD_EPS)
        assert np.allclose(aw, cw, rtol=1e-13, atol=0) and np.array_equal(ab, cb)
        assert (np.abs(ag - cg) <= 1e-13 * r * S).all(), (shape, bias)          # float64 sums in two orders
        assert (S > 0).all()


def test_fold_bwd_restatement_stays_inside_the_bounds():
    for shape, bias in _fold_bwd_cases():
        d = K.fold_bwd_inputs(shape, bias)
        dw, dg, db = K.fold_bwd_restatement32(d, K.FOLD_BWD_EPS)
        qw, qg = K.check_fold_bwd(dw, dg, db, d, K.FOLD_BWD_EPS, "%s bias=%d" % (shape, bias))
        assert qw <= 4.5 / 8.0 + 1e-6                           # correctly rounded operations: 0.5 + 1 + 1 + 1 + 1 of the 8 u
    for i, shape in enumerate(K.PLAN_21):                       # the plan's items are further draws of the same shapes
        if shape != K.FOLD_BWD_SHAPES[-1]:
            d = K.fold_bwd_inputs(shape, K.plan_bias(i), seed=i + 1)
            K.check_fold_bwd(*K.fold_bwd_restatement32(d, K.FOLD_BWD_EPS), d, K.FOLD_BWD_EPS)


def test_fold_bwd_shapes_are_the_edges_they_claim():
    rows = [s[0] * s[0] * s[1] for s in K.FOLD_BWD_SHAPES]
    assert rows == [1, 3, 33, 180, 4608] and rows[2] % K.FB_ROWS == 1 and K.fold_bwd_nblocks(K.FOLD_BWD_SHAPES[-1]) == 144
    assert [s[2] for s in K.FOLD_BWD_SHAPES[:3]] == [4, 68, 64]
    # workgroups of launch (1): ceil(cout / 64) * nblocks -- only the first shape is a single-workgroup item
    wgs = [-(-s[2] // 64) * K.fold_bwd_nblocks(s) for s in K.FOLD_BWD_SHAPES]
    assert wgs[0] == 1 and min(wgs[1:]) >= 2
    p = K.PLAN_21
    assert len(p) == 21 and p[0] == p[-1] == K._S and any(p[i - 1] == K._L and p[i] == K._S and p[i + 1] == K._L for i in range(1, 20))
    biases = [K.plan_bias(i) for i in range(21)]
    for shape in set(p):                                        # every shape appears with and without a conv bias
        assert {b for s, b in zip(p, biases) if s == shape} == {False, True}, shape


def test_fold_bwd_check_rejects_wrong_outputs():
    for shape in K.FOLD_BWD_SHAPES:
        d = K.fold_bwd_inputs(shape, True)
        dw, dg, db = K.fold_bwd_restatement32(d, K.FOLD_BWD_EPS)
        _, g_nobias, _ = K.fold_bwd_restatement32(d, K.FOLD_BWD_EPS, drop_bias_term=True)          # dgamma missing the conv-bias term ...
        with pytest.raises(AssertionError, match="dgamma error"):
            K.check_fold_bwd(dw, g_nobias, db, d, K.FOLD_BWD_EPS)
        d0 = dict(d, cb=None)                                                                       # ... or only its cbias half
        with pytest.raises(AssertionError, match="dgamma error"):
            K.check_fold_bwd(dw, K.fold_bwd_restatement32(d0, K.FOLD_BWD_EPS)[1], db, d, K.FOLD_BWD_EPS)
        _, g_short, _ = K.fold_bwd_restatement32(d, K.FOLD_BWD_EPS, drop_last_block=True)           # dgamma missing its last row block
        with pytest.raises(AssertionError, match="dgamma error"):
            K.check_fold_bwd(dw, g_short, db, d, K.FOLD_BWD_EPS)
        with pytest.raises(AssertionError, match="dbeta"):
            K.check_fold_bwd(dw, dg, db * np.float32(-1), d, K.FOLD_BWD_EPS)
        with pytest.raises(AssertionError, match="dw error"):                                       # dw without gamma
            K.check_fold_bwd(dw / d["gamma"], dg, db, d, K.FOLD_BWD_EPS)


# ------------------------------------------------------------------ subsample
def test_subsample_inputs_and_mutations():
    h = K.sub_input((3, 8, 8, 40), torch.float16).reshape(-1)
    assert h.dtype == np.float16 and np.array_equal(h[:2048].astype(np.int64), np.arange(2048))      # exact, unique within a window
    for s in range(0, h.size - 2048, 997):
        assert np.unique(h[s:s + 2048]).size == 2048
    f = K.sub_input((3, 8, 8, 20), torch.float32).reshape(-1)
    assert np.array_equal(f.astype(np.int64), np.arange(f.size))
    for dtype, ev in ((torch.float32, 4), (torch.float16, 8)):
        for stride in (2, 3):
            for (hh, ww) in K.SUB_HW:
                if ww <= 1:
                    continue
                x = K.sub_input((3, hh, ww, ev), dtype)
                want = K.sub_reference(x, stride)
                assert want.shape == (3, -(-hh // stride), -(-ww // stride), ev)
                wrong = x[:, ::stride, np.minimum(np.arange(0, ww, stride) + 1, ww - 1), :]       # a kernel that reads ox * stride + 1
                with pytest.raises(AssertionError):
                    K._same_bits(wrong, want, "shifted source column")
    assert K.sub_reference(K.sub_input((1, 2, 5, 4), torch.float32), 3).shape == (1, 1, 2, 4)       # Ho == 1


def test_subsample_cap_case_exceeds_the_cap():
    v = K.sub_cap_vectors()
    assert K.SUB_CAP_VECS == 2097152 and K.SUB_CAP_VECS < v < 2 * K.SUB_CAP_VECS and v % 256 != 0
    n, h, w, c, s = K.SUB_CAP
    assert s == 2 and n * h * w * c * 4 <= 135 * 10 ** 6
    # the second grid-stride pass left unwritten (scaled down: the same comparison on a small tensor)
    x = K.sub_input((1, 9, 9, 8), torch.float32, bit_patterns=True)
    want = K.sub_reference(x, 2)
    holed = want.copy().reshape(-1)
    holed[holed.size * 3 // 4:] = np.nan
    with pytest.raises(AssertionError):
        K._same_bits(holed.reshape(want.shape), want)
    assert np.unique(K._bits(x)).size == x.size


def test_fold_cap_case_exceeds_the_cap():
    k, cin, cout = K.FOLD_CASES[-1][0]
    v = k * k * cin * cout // 4
    assert K.FOLD_CAP_VECS == 1048576 and v == 1053700 and K.FOLD_CAP_VECS < v < 2 * K.FOLD_CAP_VECS
    assert all(s[0] * s[0] * s[1] * s[2] // 4 <= K.FOLD_CAP_VECS for s, _ in K.FOLD_CASES[:-1])


# ------------------------------------------------------------------ preprocessing
def test_preprocess_exact_cases_are_exact():
    cases = K.preproc_exact_cases()
    widths = {c[3] for c in cases.values()}
    assert set(K.PRE_WIDTHS) <= widths and any(c[1] == 1 for c in cases.values()) and any(c[0] == 1 for c in cases.values())
    for name, (hs, ws, hd, wd) in cases.items():
        im = K.preproc_image(hs, ws)
        for i in range(K.PRE_N):
            resized64, out64 = K.preproc_float64(im[i], hd, wd)
            resized32 = PO.resize_linear(im[i].astype(np.float32), hd, wd)
            assert np.array_equal(resized32.astype(np.float64), resized64), name           # no rounding at all before the means
            K._same_bits(PO.preprocess_bgr(im[i], hd, wd, K.MEANS), out64.astype(np.float32), name)     # and one rounding after


def test_preprocess_general_cases_are_not_exact_and_scale_as_claimed():
    for name, (hs, ws, hd, wd) in K.PRE_GENERAL.items():
        im = K.preproc_image(hs, ws)
        resized64, _ = K.preproc_float64(im[0], hd, wd)
        assert not np.array_equal(PO.resize_linear(im[0].astype(np.float32), hd, wd).astype(np.float64), resized64), name
    assert 1242 / 177 > 2 and 73 / 10 == 7.3 and all(c[0] <= 12 and c[2] <= 12 for n, c in K.PRE_GENERAL.items() if n != "vertical_7.3x")


def test_preprocess_comparisons_reject_wrong_outputs():
    for name, (hs, ws, hd, wd) in list(K.preproc_exact_cases().items()) + list(K.PRE_GENERAL.items()):
        if wd < 2 or ws < 2:                                     # (one source column: every destination column is the same)
            continue
        im = K.preproc_image(hs, ws)
        ref = K.preproc_oracle(im, hd, wd)
        shifted = np.roll(ref, 1, axis=2)                       # a destination column shifted by one
        with pytest.raises(AssertionError):
            K._same_bits(shifted, ref, name)
        with pytest.raises(AssertionError):
            K.check_preproc_general(shifted, ref)
        with pytest.raises(AssertionError):                     # float16 of a neighbouring pixel: inside 0.07 on a smooth image or not, not the same bits
            K._check_f16(shifted.astype(np.float16), ref, ref, name)
        K._check_f16(ref.astype(np.float16), ref, ref, name)
        assert K.check_preproc_general(ref.copy(), ref) == 1.0
    # the last column's neighbour pulled in with a weight: a wrong value in the last pixel of the last image only
    ref = K.preproc_oracle(K.preproc_image(3, 5), 3, 5)
    wrong = ref.copy()
    wrong[-1, -1, -1, :] += np.float32(0.5)
    with pytest.raises(AssertionError):
        K._same_bits(wrong, ref)
