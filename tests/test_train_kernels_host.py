"""The references of tests/test_gpu_train_kernels.py checked on their own, and the claims its exact assertions rest on: no GPU.

  * the restated dropout generator finds the draw u = 1 - 2^-24 (seed 1234, element 37 624 421) and float32 rounds 1 + u to 2: why
    dropout_mask_kernel clamps its mask to 1; the restated generator's keep rate is within 5 sigma for the seeds the GPU test uses;
  * sum_f32's integer inputs: every partial sum is an integer below 2^24;
  * the max-pool scatter reference equals autograd where the argmax is unique, its tie rule on a worked example, and the sums of
    the chosen dy values are exact in float32 (and, up to four, in float16);
  * the float64 loss restatement agrees with the float32 oracle to float32 accuracy on every input class, and the input classes
    contain what they claim."""
import numpy as np
import torch

from oracle import sqdet_oracle as O
from tests import test_gpu_train_kernels as K


def test_dropout_generator_draws_the_float32_tie_at_keep_prob_one():
    u = K.dropout_u(1, K.TIE_SEED, start=K.TIE_INDEX)[0]
    assert u.dtype == np.float32 and u == np.float32(0xFFFFFF) * np.float32(2.0 ** -24) == np.float32(1.0) - np.float32(2.0 ** -24)
    assert np.float64(1.0) + np.float64(u) == 2.0 - 2.0 ** -24                 # the exact sum lies half way between 2 - 2^-23 and 2 ...
    assert np.float32(1.0) + u == np.float32(2.0)                              # ... a tie, and float32 rounds it to even: 2
    assert np.floor(np.float32(1.0) + u) == 2.0
    lo = K.TIE_INDEX - 1000
    raw = K.dropout_restatement(2000, 1.0, K.TIE_SEED, start=lo, clamp=False)
    assert raw[1000] == 2.0 and (np.delete(raw, 1000) == 1.0).all()            # floor alone: a keep mask that holds a 2
    assert (K.dropout_restatement(2000, 1.0, K.TIE_SEED, start=lo) == 1.0).all()
    for keep in (0.5, 0.25, 0.9):                                              # below 1 the clamp never acts: keep + u < 2
        a = K.dropout_restatement(1 << 16, keep, K.TIE_SEED, start=lo)
        assert np.array_equal(a, K.dropout_restatement(1 << 16, keep, K.TIE_SEED, start=lo, clamp=False)) and set(np.unique(a)) <= {0.0, 1.0}
    # the mask depends on (seed, index) only: a window equals the same elements of a longer run
    assert np.array_equal(K.dropout_restatement(100, 0.5, 7, start=12345), K.dropout_restatement(12445, 0.5, 7)[12345:])


def test_dropout_generator_keep_rate_is_within_five_sigma_for_the_seeds_used():
    n = 1 << 24
    for seed in K.DROPOUT_SEEDS:
        counts = K.dropout_counts(n, K.DROPOUT_KEEPS, seed)
        for keep, c in counts.items():
            assert K.within_5_sigma(c, n, keep), (seed, keep, c)
        assert counts[1.0] == n


def test_sum_inputs_have_exact_partial_sums_and_the_bound_is_the_trees():
    for n in K.SUM_EXACT_LENGTHS:
        x = K.sum_exact_input(n)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
        assert np.abs(x).sum(dtype=np.float64) < 2 ** 24           # any partial sum, in any order, is an integer below 2^24: exact
    assert K.SUM_EXACT_LENGTHS[-2] == 337000 and {7168 * 4, 8192 * 4} <= set(K.SUM_EXACT_LENGTHS)
    x = K.sum_real_input(1000003)
    # thread 0 of the kernel: ceil(250 000 / 1024) vector additions + 1 tail addition, then (s0 + s1) + (s2 + s3) and ten LDS levels
    assert -(-250000 // 1024) + 1 + 2 + 10 == -(-x.size // 4096) + 13
    assert abs(float(x.sum(dtype=np.float32)) - float(x.sum(dtype=np.float64))) <= K.sum_real_bound(x)


def _autograd_pool(x, dy, k, s, pad):
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = O.pooling_layer(xt, k, s, pad)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    return xt.grad.numpy()


def test_maxpool_reference_is_autograd_where_the_argmax_is_unique():
    rs = np.random.RandomState(0)
    for (k, s, pad, H, W) in ((3, 2, "SAME", 7, 9), (3, 2, "VALID", 20, 31), (2, 2, "VALID", 9, 7), (2, 2, "SAME", 9, 7), (3, 1, "SAME", 13, 17),
                              (3, 2, "SAME", 1, 1), (3, 2, "SAME", 2, 2), (3, 2, "SAME", 1, 40), (3, 2, "SAME", 40, 1)):
        x = rs.permutation(2 * H * W * 3).reshape(2, H, W, 3).astype(np.float32)        # distinct values
        Ho, Wo = K.pool_geometry(H, k, s, pad)[0], K.pool_geometry(W, k, s, pad)[0]
        dy = K.pool_dy((2, Ho, Wo, 3), torch.float32, seed=H)
        assert np.array_equal(K.maxpool_bwd_reference(x, dy, k, s, pad), _autograd_pool(x, dy, k, s, pad)), (k, s, pad, H, W)
        assert np.array_equal(K.maxpool_bwd_reference(x - 1e6, dy, k, s, pad, relu=True), np.zeros_like(x, np.float64))


def test_maxpool_reference_tie_rule_worked_example():
    """3x3 / s2 / VALID on a 3x5 map of ones: windows (0,0) and (0,1) both tie everywhere; each hands its dy to its FIRST cell,
    (0,0) and (0,2).  With the maximum duplicated in a later row the earlier one (row-major) still wins."""
    x = np.ones((1, 3, 5, 1), np.float32)
    dy = np.array([0.5, -0.25], np.float32).reshape(1, 1, 2, 1)
    dx = K.maxpool_bwd_reference(x, dy, 3, 2, "VALID")
    want = np.zeros((1, 3, 5, 1))
    want[0, 0, 0, 0], want[0, 0, 2, 0] = 0.5, -0.25
    assert np.array_equal(dx, want)
    x[0, 0, 2, 0] = x[0, 2, 1, 0] = x[0, 2, 3, 0] = 2.0      # cell (0,2) is in both windows and is each one's first maximum
    want[:] = 0
    want[0, 0, 2, 0] = 0.25
    assert np.array_equal(K.maxpool_bwd_reference(x, dy, 3, 2, "VALID"), want)
    # SAME on a 4x4 zero map pads bottom / right only: each window's first valid cell is its top-left one
    z = np.zeros((1, 4, 4, 1), np.float32)
    d = K.maxpool_bwd_reference(z, np.ones((1, 2, 2, 1), np.float32), 3, 2, "SAME")
    assert K.pool_geometry(4, 3, 2, "SAME") == (2, 0) and d[0, 0, 0, 0] == 1 and d[0, 0, 2, 0] == 1 and d[0, 2, 2, 0] == 1 and d.sum() == 4


def test_maxpool_inputs_tie_and_their_gradient_sums_are_exact():
    for dtype in (torch.float32, torch.float16):
        nt = K._np_dtype(dtype)
        for kind in K.POOL_INPUT_KINDS:
            x = K.pool_input(kind, (2, 47, 156, 8), dtype, seed=1)
            assert x.dtype == nt
            if kind != "last_cell":
                assert np.unique(x).size <= 24                                   # ties are the rule
        x = K.pool_input("relu_halves", (2, 47, 156, 8), dtype, seed=1)
        assert 0.3 < (x == 0).mean() < 0.7
        lc = K.pool_input("last_cell", (1, 7, 9, 8), dtype, seed=1).astype(np.float64)
        assert (np.diff(lc[0, :, :, 0].reshape(-1)) > 0).all()                   # strictly increasing row-major: the maximum is the last cell
        for (k, s, pad, H, W) in ((3, 2, "SAME", 47, 156), (3, 1, "SAME", 13, 17), (2, 2, "SAME", 9, 7)):
            x = K.pool_input("relu_halves", (2, H, W, 8), dtype, seed=2)
            Ho, Wo = K.pool_geometry(H, k, s, pad)[0], K.pool_geometry(W, k, s, pad)[0]
            dy = K.pool_dy((2, Ho, Wo, 8), dtype, seed=3)
            assert np.array_equal(dy.astype(np.float64) * 64, np.round(dy.astype(np.float64) * 64)) and np.abs(dy).max() <= 4
            ref = K.maxpool_bwd_reference(x, dy, k, s, pad)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)          # the float32 accumulation is exact
            if s == 2:                                                                      # at most four windows share a cell
                assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref)
            assert abs(ref.sum() - dy.astype(np.float64).sum()) < 1e-9                      # every window's dy lands exactly once


def test_elementwise_inputs_are_exact_in_both_types_and_the_edge_table_holds_its_edges():
    for dtype in (torch.float32, torch.float16):
        n = 300 * K._ev(dtype)
        v = K.ew_values(n, dtype, 5).astype(np.float64)
        assert np.array_equal(v * 8, np.round(v * 8))
        assert np.abs(v[-257 * K._ev(dtype):]).max() > 900                       # the planted tail
        for scale in K.EW_SCALES:
            p = v * scale
            assert np.array_equal(p.astype(np.float32).astype(np.float64), p)      # the float32 product is exact: one rounding remains
    with np.errstate(over="ignore"):
        t = dict((float(v) * s, np.float32(v * np.float32(s)).astype(np.float16)) for v, s in K.convert_edge_table() if np.isfinite(v))
    assert t[1 + 2.0 ** -11] == 1.0 and t[1 + 3 * 2.0 ** -11] == np.float16(1 + 2.0 ** -9)          # ties to even, down and up
    assert t[65504.0] == 65504 and np.isinf(t[65520.0]) and t[float(np.float32(65519.996))] == 65504 and t[-65520.0] == -np.inf
    assert t[2.0 ** -25] == 0 and t[2.0 ** -24] == np.float16(2.0 ** -24) and t[3 * 2.0 ** -25] == np.float16(2.0 ** -23)


def test_loss_restatement_agrees_with_the_float32_oracle_and_the_inputs_hold_their_edges():
    for name in ("small_c1", "small_c2", "small_c20_edges", "small_one_object", "small_saturated"):
        mc, preds, mask, delta, box, labels = K.loss_inputs(name)
        ref = K.loss_reference64(mc, preds, mask, delta, box, labels)
        e = K.loss_errors(K.loss_oracle32(mc, preds, mask, delta, box, labels), ref)
        scale = [np.abs(r).max() for r in ref]
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
        tol = 1e-3 if "saturated" in name else 2e-5
        assert e[0] <= tol * scale[0] and e[1] <= 1e-5 and e[2] <= tol * scale[2] + 1e-7, (name, e, scale)
        if name == "small_one_object":
            assert mask.sum() == 1
        if K.LOSS_CASES[name][2] == "edges":
            K_, C = mc.ANCHOR_PER_GRID, mc.CLASSES
            d = preds.reshape(preds.shape[0], -1, K_ * (C + 5))[..., K_ * (C + 1):]
            thr = np.float32(mc.EXP_THRESH)
            for v in (thr, np.nextafter(thr, np.float32(0)), np.nextafter(thr, np.float32(2)), np.float32(8), np.float32(60), np.float32(-60)):
                assert (d == v).any(), v
            assert ((box[..., 2] == 0) & (mask[..., 0] > 0)).any()
            assert (ref[1] > 0).any()                                    # and some labelled anchor still overlaps its box
