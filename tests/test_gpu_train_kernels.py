"""GPU tests of the training step's NON-convolution kernels (squeezedet_amd/csrc/train.hip, loss.hip, optim.hip) at their edges: sum_f32, the
dropout mask generator, the element-wise kernels past their grid caps and at float16's edges, the max-pool backward tie rule,
the loss at a size that loops, and the optimizer with more variables than opt_norm_kernel has threads.

Every reference is computed here, on the CPU, in float64 (NumPy, or torch-CPU float64 where autograd is wanted), from the same
input bits the kernel gets; none calls the library.  The references and the input generators are plain functions of this
module so that tests/test_train_kernels_host.py can check them -- and the claims the exact assertions rest on -- without a
GPU.

Loss tolerances (section 5) are not constants: for each compared quantity -- the vector of the three losses, ious, dpreds; the
error of a quantity is its largest absolute element error, _close's metric -- e_ref is the error of the float32 CPU oracle
(oracle.train_oracle.loss_graph + autograd) against the float64 restatement on the same inputs, and the kernel's error against
float64 must be at most 4 * e_ref + 1e-7 (a different but equally valid float32 evaluation order, expf / logf one ulp apart).
Measured on an MI355X (kernel error / oracle error; the cases are LOSS_CASES):

  case                losses                 ious                   dpreds (largest |dpreds|)
  full_randn          3.23e-06 / 3.52e-06    4.75e-07 / 4.75e-07    8.51e-08 / 8.51e-08  (0.934)
  full_edges          1.93e-04 / 1.93e-04    2.03e-07 / 2.03e-07    1.90e-06 / 1.90e-06  (19.5; bbox loss 2389)
  full_saturated      1.19e-06 / 2.10e-06    3.21e-07 / 3.21e-07    5.77e-08 / 7.31e-08  (1.07)
  small_c1            2.53e-06 / 1.85e-06    2.93e-08 / 2.93e-08    9.69e-08 / 9.69e-08  (2.79)
  small_c2            1.17e-03 / 6.80e-04    2.62e-10 / 2.62e-10    8.67e-06 / 8.04e-06  (85.5; bbox loss 7777)
  small_c20           1.48e-06 / 9.31e-07    5.14e-08 / 5.14e-08    2.71e-07 / 1.28e-07  (2.5)
  small_c20_edges     1.89e-06 / 1.89e-06    2.47e-08 / 2.47e-08    9.16e-07 / 9.16e-07  (37.5; bbox loss 4565)
  small_one_object    1.84e-06 / 1.03e-06    1.65e-08 / 1.65e-08    1.07e-06 / 1.07e-06  (13.9)
  small_saturated     1.49e-06 / 2.35e-06    1.14e-07 / 1.14e-07    5.29e-07 / 5.29e-07  (2.05)

The kernel is as accurate as the float32 oracle everywhere (mostly to the digit: the decode is the same float32 expression op
for op); the well-conditioned cases also sit inside the 2e-5 / 5e-5 of tests/test_gpu_train.py, asserted here again.  No input
class had to be dropped in any section.

Two defects these tests found, both fixed in train.hip (scaled_to now stands in train_common.h) with them: dropout_mask_kernel stored a 2 where keep_prob = 1 meets the
top draw (section 2), and convert_scale float32 -> float16 (and some of the mixed loss kernel's float16 stores) lost the sign of
a zero product, because hipcc fuses multiply + convert into an FMA with a +0 addend (section 3's edge table, section 5's mixed
form, which compares bit patterns where torch.equal takes -0 == +0).
"""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O
from oracle import train_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24          # float32 unit roundoff


def _ops():
    from squeezedet_amd import ops
    return ops


def _ev(dtype):
    return 8 if dtype in (torch.float16, np.float16) else 4


def _np_dtype(dtype):
    return np.float16 if dtype == torch.float16 else np.float32


def _bits(a):
    """The array's bit patterns (so that -0 != +0 and an inf is an inf); every NaN compares equal to every NaN."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    u = a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    u[np.isnan(a)] = np.iinfo(u.dtype).max
    return u


def _same_bits(got, ref, what=""):
    g, r = _bits(got), _bits(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, "%s: shape / dtype %s %s vs %s %s" % (what, g.shape, g.dtype, r.shape, r.dtype)
    if not np.array_equal(g, r):
        bad = np.flatnonzero(g.reshape(-1) != r.reshape(-1))
        i = int(bad[0])
        gv = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got).reshape(-1)[i]
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r" % (what, bad.size, g.size, i, gv, np.asarray(ref).reshape(-1)[i]))


# ================================================================== 1. sum_f32
SUM_EXACT_LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097, 28672, 28676, 32768, 32775, 337000, 3 * 32768 + 5]
SUM_REAL_LENGTHS = [337000, 1000003]


def sum_exact_input(n):
    """Integer-valued float32 in [-8, 8]: every partial sum, in any order, is an integer below 2^24 -- exact."""
    return np.random.RandomState(1000 + n % 997).randint(-8, 9, size=n).astype(np.float32)


def sum_real_input(n):
    return np.random.RandomState(n % 1009).randn(n).astype(np.float32)


def sum_real_bound(x):
    """The kernel's addition tree on a 16-byte-aligned tensor: 4096 running sums (1024 threads x 4 lanes) of at most ceil(n / 4096)
    additions each (+ 1 for the n % 4 tail), then 2 + 10 tree levels; each addition rounds by at most 2^-24 relative."""
    n = x.size
    return (-(-n // 4096) + 13) * U32 * float(np.abs(x.astype(np.float64)).sum())


@pytest.mark.parametrize("n", SUM_EXACT_LENGTHS)
def test_sum_f32_exact_on_integers_aligned_and_unaligned(n):
    """sum_f32_kernel's vector loop (eight loads in flight up to nv = 7168 / 8192 vectors, then one at a time), its n % 4 tail
    and -- on buf[1:1 + n], a pointer that is only 4-byte aligned -- its scalar path, on values whose sum is exact in every
    order: ==, no tolerance."""
    ops = _ops()
    x = sum_exact_input(n)
    want = float(x.astype(np.float64).sum())
    fresh = torch.from_numpy(x).to(DEV)
    assert fresh.data_ptr() % 16 == 0
    buf = torch.full((n + 9,), 1000.0, dtype=torch.float32, device=DEV)      # (a neighbour read by mistake would show)
    odd = buf[1:1 + n]
    odd.copy_(fresh)
    assert odd.data_ptr() % 16 == 4 and odd.is_contiguous()
    got = float(ops.sum_f32(fresh).item())
    got_odd = float(ops.sum_f32(odd).item())
    assert got == want, "aligned n=%d: %r != %r" % (n, got, want)
    assert got_odd == want, "unaligned n=%d: %r != %r" % (n, got_odd, want)


@pytest.mark.parametrize("n", SUM_REAL_LENGTHS)
def test_sum_f32_real_values_deterministic_and_within_the_trees_bound(n):
    ops = _ops()
    x = sum_real_input(n)
    xd = torch.from_numpy(x).to(DEV)
    a = ops.sum_f32(xd).cpu().numpy()
    b = ops.sum_f32(xd).cpu().numpy()
    _same_bits(a, b, "two calls")
    want = float(x.astype(np.float64).sum())
    err, bound = abs(float(a[0]) - want), sum_real_bound(x)
    print("sum_f32 n=%d: |err| %.3g, bound %.3g" % (n, err, bound))
    assert err <= bound


# ================================================================== 2. dropout mask
DROPOUT_SEEDS = [0, 1234, (7 << 32) + 5]         # (the last: the trainers' (seed << 32) + call layout)
DROPOUT_KEEPS = [0.5, 0.25, 0.9, 1.0]
DROPOUT_SIZES = [1, 255, 2097152 + 3]            # (the last: past the 8192-workgroup cap, the grid-stride loop)
TIE_SEED, TIE_INDEX = 1234, 37624421             # u = 1 - 2^-24: floor(1.0f + u) = 2 in float32


def dropout_u(n, seed, start=0):
    """The generator of dropout_mask_kernel restated on uint64: splitmix64 of seed + golden * (i + 1), top 24 bits -> [0, 1)."""
    with np.errstate(over="ignore"):
        i = np.arange(start + 1, start + n + 1, dtype=np.uint64)
        z = np.uint64(seed & (2 ** 64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * i
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_restatement(n, keep_prob, seed, start=0, clamp=True):
    """floor(float32(keep_prob) + float32(u)) in float32; clamp: at most 1 (the kernel's fminf)."""
    m = np.floor(np.float32(keep_prob) + dropout_u(n, seed, start))
    assert m.dtype == np.float32
    return np.minimum(m, np.float32(1.0)) if clamp else m


def dropout_counts(n, keeps, seed, chunk=1 << 22):
    """{keep_prob: number of ones among the restated mask's first n elements}."""
    out = dict.fromkeys(keeps, 0)
    for s in range(0, n, chunk):
        u = dropout_u(min(chunk, n - s), seed, start=s)
        for keep in keeps:
            out[keep] += int(np.minimum(np.floor(np.float32(keep) + u), np.float32(1.0)).sum(dtype=np.float64))
    return out


def within_5_sigma(count, n, keep_prob):
    return abs(count - n * keep_prob) <= 5.0 * np.sqrt(n * keep_prob * (1.0 - keep_prob))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("n", DROPOUT_SIZES)
def test_dropout_mask_is_the_restated_generator_bit_for_bit(dtype, n):
    """The mask is a function of (seed, index) only -- what a bitwise --resume rests on: == the NumPy restatement for every
    seed and keep_prob, from dropout_mask and from dropout_mask_into on a view of a larger buffer; and at keep_prob 0.5 the
    (clamped) kernel equals the UNCLAMPED restatement: the clamp moved nothing else."""
    ops = _ops()
    for seed in DROPOUT_SEEDS:
        for keep in DROPOUT_KEEPS:
            want = dropout_restatement(n, keep, seed).astype(_np_dtype(dtype))
            got = ops.dropout_mask((n,), keep, seed, dtype, DEV)
            _same_bits(got, want, "dropout_mask seed %d keep %g n %d" % (seed, keep, n))
            buf = torch.full((n + 16,), 7.0, dtype=dtype, device=DEV)
            ops.dropout_mask_into(buf[8:8 + n], keep, seed)
            _same_bits(buf[8:8 + n], want, "dropout_mask_into seed %d keep %g n %d" % (seed, keep, n))
            assert bool((buf[:8] == 7.0).all()) and bool((buf[8 + n:] == 7.0).all())
        _same_bits(ops.dropout_mask((n,), 0.5, seed, dtype, DEV), dropout_restatement(n, 0.5, seed, clamp=False).astype(_np_dtype(dtype)),
                   "keep 0.5 against the unclamped restatement")


def test_dropout_mask_at_keep_prob_one_holds_only_ones():
    """keep_prob = 1.0, seed 1234, 2^26 float16 elements from element 0: element 37 624 421 draws u = 1 - 2^-24, and the float32
    sum 1 + u is a tie that rounds to 2.0 -- floorf alone stored a 2 there (the parent of this test's commit did).  Every value
    must be 0 or 1; at keep_prob 1 that is: every value is 1."""
    ops = _ops()
    n = 1 << 26
    assert TIE_INDEX < n
    m = ops.dropout_mask((n,), 1.0, TIE_SEED, torch.float16, DEV)
    torch.cuda.synchronize()
    lo = TIE_INDEX - (1 << 19)
    _same_bits(m[lo:lo + (1 << 20)], dropout_restatement(1 << 20, 1.0, TIE_SEED, start=lo).astype(np.float16), "the window around the tie")
    assert float(m[TIE_INDEX].item()) == 1.0, "element %d is %r" % (TIE_INDEX, float(m[TIE_INDEX].item()))
    other = int(((m != 0) & (m != 1)).sum().item())
    assert other == 0, "%d elements are neither 0 nor 1 (max %r)" % (other, float(m.max().item()))
    assert bool((m == 1).all())
    del m
    m32 = ops.dropout_mask((1 << 20,), 1.0, TIE_SEED, torch.float32, DEV)      # (float32 storage would hold the 2 just as well)
    assert bool((m32 == 1).all())


@pytest.mark.parametrize("seed", DROPOUT_SEEDS)
def test_dropout_mask_keep_rate(seed):
    """Over 2^24 elements the number of ones is within 5 sigma of binomial(n, keep_prob) (tests/test_train_kernels_host.py shows the
    restated generator meets that for these seeds) -- and is the restatement's own count."""
    ops = _ops()
    n = 1 << 24
    want = dropout_counts(n, DROPOUT_KEEPS, seed)
    for keep in DROPOUT_KEEPS:
        m = ops.dropout_mask((n,), keep, seed, torch.float32, DEV)
        count = int(m.double().sum().item())
        print("dropout seed %d keep %g: %d ones of %d (%.3f sigma)" % (seed, keep, count, n, (count - n * keep) / max(np.sqrt(n * keep * (1 - keep)), 1e-30)))
        assert within_5_sigma(count, n, keep)
        assert count == want[keep]
        assert int(((m != 0) & (m != 1)).sum().item()) == 0


# ================================================================== 3. element-wise kernels
NV_CAP = 2097152                                   # grid_for(.., 8192) workgroups of 256 threads: one 16-byte vector each
EW_NV = [1, 257, NV_CAP + 257]
EW_SCALES = [1.0, 2.0, 0.5, 512.0, 65536.0]        # powers of two: the float32 product chain is exact, one rounding remains


def ew_values(n, dtype, seed, relu_like=False):
    """Multiples of 1/8 of magnitude < 8 (exact in float16 and float32; any product with a 0/1 mask and a power-of-two scale
    is exact in float32), the last 257 vectors planted with distinctive values k + 0.5, |.| <= 1000.5."""
    rs = np.random.RandomState(seed)
    v = rs.randint(-63, 64, size=n).astype(np.float64) / 8.0
    tail = min(n, 257 * _ev(dtype))
    v[n - tail:] = (np.arange(tail) * 7 + seed) % 2001 - 1000 + 0.5
    if relu_like:
        v = np.maximum(v, 0.0)
    out = v.astype(_np_dtype(dtype))
    assert np.array_equal(out.astype(np.float64), v)
    return out


def ew_mask(n, dtype, seed):
    return (np.random.RandomState(seed).randint(0, 2, size=n)).astype(_np_dtype(dtype))


def _cast(a64, dtype):
    with np.errstate(over="ignore"):
        return a64.astype(_np_dtype(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("nv", EW_NV)
def test_relu_bwd_and_add_relu_past_the_grid_cap(dtype, nv):
    ops = _ops()
    n = nv * _ev(dtype)
    y, dy = ew_values(n, dtype, 1, relu_like=True), ew_values(n, dtype, 2)
    got = ops.relu_bwd(torch.from_numpy(y).to(DEV), torch.from_numpy(dy).to(DEV))
    _same_bits(got, np.where(y > 0, dy, _np_dtype(dtype)(0)), "relu_bwd nv=%d" % nv)
    a, b = ew_values(n, dtype, 3), ew_values(n, dtype, 4)
    s = a.astype(np.float64) + b.astype(np.float64)
    got = ops.add_relu(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    _same_bits(got, _cast(np.where(s > 0, s, 0.0), dtype), "add_relu nv=%d" % nv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("nv", EW_NV)
def test_scale_mask_with_and_without_relu_past_the_grid_cap(dtype, nv):
    ops = _ops()
    n = nv * _ev(dtype)
    x, m, r = ew_values(n, dtype, 5), ew_mask(n, dtype, 6), ew_values(n, dtype, 7, relu_like=True)
    xd, md, rd = [torch.from_numpy(v).to(DEV) for v in (x, m, r)]
    for scale in EW_SCALES:
        p = x.astype(np.float64) * m.astype(np.float64) * scale            # (-0 where a negative x is masked: the kernel's too)
        want = _cast(p, dtype)
        _same_bits(ops.scale_mask(xd, md, scale), want, "scale_mask nv=%d scale=%g" % (nv, scale))
        _same_bits(ops.scale_mask(xd, md, scale, relu_of=rd), np.where(r > 0, want, _np_dtype(dtype)(0)), "scale_mask_relu nv=%d scale=%g" % (nv, scale))
    if dtype == torch.float16:
        assert np.isinf(_cast(x.astype(np.float64) * 65536.0, dtype)).any()    # the overflow to inf was exercised


@pytest.mark.parametrize("src,dst", [(torch.float32, torch.float16), (torch.float16, torch.float32), (torch.float32, torch.float32),
                                     (torch.float16, torch.float16)], ids=["f32_f16", "f16_f32", "f32_f32", "f16_f16"])
@pytest.mark.parametrize("nv", EW_NV)
def test_convert_scale_past_the_grid_cap(src, dst, nv):
    """convert_scale_kernel works on groups of FOUR elements whatever the types: nv groups, past its own cap."""
    ops = _ops()
    n = nv * 4
    x = ew_values(n, src, 8)
    xd = torch.from_numpy(x).to(DEV)
    for scale in EW_SCALES:
        got = ops.convert_scale(xd, dst, scale)
        assert got.dtype == dst
        _same_bits(got, _cast(x.astype(np.float64) * scale, dst), "convert_scale nv=%d scale=%g" % (nv, scale))


def convert_edge_table():
    """float32 inputs whose float16 rounding is an edge: (value, scale)."""
    f = np.float32
    t = [(1 + 2.0 ** -11, 1), (1 + 3 * 2.0 ** -11, 1), (-(1 + 2.0 ** -11), 1), (1 + 2.0 ** -11 + 2.0 ** -23, 1),   # ties to even, just above
         (65504.0, 1), (65519.996, 1), (65520.0, 1), (-65520.0, 1), (65504.0, 2), (-65504.0, 2), (1.0, 65536), (-1.0, 65536),
         (2.0 ** -25, 1), (-2.0 ** -25, 1), (2.0 ** -24, 1), (3 * 2.0 ** -25, 1), (2.0 ** -25 * (1 + 2.0 ** -23), 1), (2.0 ** -14, 1),
         (2.0 ** -14 - 2.0 ** -25, 1), (2.0 ** -10, 2.0 ** -15), (0.0, 1), (-0.0, 1), (-0.0, 512), (np.inf, 1), (-np.inf, 0.5), (np.nan, 1)]
    return [(f(v), float(s)) for v, s in t]


def test_convert_scale_float16_rounding_edges():
    """float32 -> float16 against NumPy's round-to-nearest-even cast, bit for bit: exact ties, the largest finite float16 and
    the first value that becomes inf (sign kept), subnormal results down to the tie at 2^-25 that rounds to zero, -0, NaN."""
    ops = _ops()
    table = convert_edge_table()
    for scale in sorted(set(s for _, s in table)):
        vals = [v for v, s in table if s == scale]
        vals = np.array(vals + [0.0] * (-len(vals) % 4), np.float32)             # (the kernel takes groups of four)
        got = ops.convert_scale(torch.from_numpy(vals).to(DEV), torch.float16, scale)
        want = _cast(vals.astype(np.float64) * scale, torch.float16)
        _same_bits(got, want, "convert_scale edges at scale %g: %r" % (scale, vals))
        back = ops.convert_scale(got, torch.float32, 1.0)                       # and float16 -> float32 is exact
        _same_bits(back, want.astype(np.float32), "float16 -> float32 of the edge table")
    h = np.array([65504.0, -65504.0, 2.0 ** -24, -0.0], np.float16)             # float16 -> float16: overflow, subnormal, -0
    _same_bits(ops.convert_scale(torch.from_numpy(h).to(DEV), torch.float16, 2.0), _cast(h.astype(np.float64) * 2.0, torch.float16), "f16 -> f16 x 2")
    _same_bits(ops.convert_scale(torch.from_numpy(h).to(DEV), torch.float16, 0.5), _cast(h.astype(np.float64) * 0.5, torch.float16), "f16 -> f16 x 0.5")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_relu_bwd_and_add_relu_on_special_values(dtype):
    """What the kernels do, pinned: relu_bwd keeps dy where y > 0 and stores +0 elsewhere -- `y > 0` is false for -0 and for
    NaN, true for +inf.  add_relu stores t = a + b where t > 0 and +0 elsewhere: a NaN sum (NaN operand, inf - inf) becomes 0,
    -0 + -0 becomes +0, +inf stays."""
    ops = _ops()
    nt = _np_dtype(dtype)
    y = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 2.0 ** -14], nt)
    dy = np.array([3.0, -3.0, 5.0, -7.0, 9.0, np.inf, 11.0, -0.5], nt)
    want = np.array([0.0, 0.0, 0.0, -7.0, 0.0, np.inf, 0.0, -0.5], nt)
    _same_bits(ops.relu_bwd(torch.from_numpy(y).to(DEV), torch.from_numpy(dy).to(DEV)), want, "relu_bwd specials")
    a = np.array([-0.0, np.nan, np.inf, np.inf, -np.inf, 1.5, -2.0, 0.0], nt)
    b = np.array([-0.0, 1.0, -np.inf, 1.0, 1.0, -0.25, 1.0, 0.0], nt)
    want = np.array([0.0, 0.0, 0.0, np.inf, 0.0, 1.25, 0.0, 0.0], nt)
    _same_bits(ops.add_relu(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), want, "add_relu specials")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_copy_channels_writes_its_slice_and_nothing_else(dtype):
    """48 channels into a 200-channel (at the size past the grid cap: 176-channel, to keep the tensor near 128 MiB) destination
    pre-filled with a sentinel, at offset 0, in the middle and last."""
    ops = _ops()
    ev, nt = _ev(dtype), _np_dtype(dtype)
    cv = 48 // ev
    big = -(-(NV_CAP + 257) // cv)
    assert 43 * cv >= 257 and big * cv >= NV_CAP + 257
    for pixels, stride in ((1, 200), (43, 200), (big, 176)):
        x = ew_values(pixels * 48, dtype, 9).reshape(pixels, 48)
        xd = torch.from_numpy(x).to(DEV)
        for off in (0, (stride - 48) // 2 // ev * ev, stride - 48):
            out = torch.full((pixels, stride), -77.0, dtype=dtype, device=DEV)
            ops.copy_channels(xd, out, off)
            got = out.cpu().numpy()
            _same_bits(got[:, off:off + 48], x, "copy_channels pixels=%d off=%d" % (pixels, off))
            assert (got[:, :off] == nt(-77)).all() and (got[:, off + 48:] == nt(-77)).all(), (pixels, off)


# ================================================================== 4. max-pool backward
def pool_geometry(h, k, s, pad):
    ho = -(-h // s) if pad == "SAME" else (h - k) // s + 1
    pt = max((ho - 1) * s + k - h, 0) // 2 if pad == "SAME" else 0
    return ho, pt


def maxpool_bwd_reference(x, dy, k, s, pad, relu=False):
    """tf.nn.max_pool's gradient from the definition, float64: in every window the FIRST maximum of its valid cells (row-major)
    gets the window's dy; what a cell receives is summed.  x [N,H,W,C], dy [N,Ho,Wo,C] (any float type) -> float64 dx."""
    N, H, W, C = x.shape
    (Ho, pt), (Wo, pl) = pool_geometry(H, k, s, pad), pool_geometry(W, k, s, pad)
    assert dy.shape == (N, Ho, Wo, C)
    dx = np.zeros((N, H, W, C), np.float64)
    oy, ox = np.arange(Ho), np.arange(Wo)
    for n in range(N):
        xs = x[n].astype(np.float64)
        best = np.full((Ho, Wo, C), -np.inf)
        pos = np.full((Ho, Wo, C), -1, np.int64)
        taps = []
        for t in range(k * k):
            yy, xx = oy * s - pt + t // k, ox * s - pl + t % k
            vy, vx = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W)
            taps.append((yy, xx, vy, vx))
            if not vy.any() or not vx.any():
                continue
            v = xs[np.ix_(yy[vy], xx[vx])]
            sub = np.ix_(vy, vx)
            b, p = best[sub], pos[sub]
            win = (v > b) | (p < 0)                  # strictly greater: the first of equal maxima stays
            best[sub], pos[sub] = np.where(win, v, b), np.where(win, t, p)
        g = dy[n].astype(np.float64)
        for t, (yy, xx, vy, vx) in enumerate(taps):
            if not vy.any() or not vx.any():
                continue
            sub = np.ix_(vy, vx)
            # for one tap the window -> cell map is one-to-one (cells s apart): a plain indexed add
            dx[n][np.ix_(yy[vy], xx[vx])] += np.where(pos[sub] == t, g[sub], 0.0)
    if relu:
        dx = np.where(x.astype(np.float64) > 0, dx, 0.0)
    return dx


POOL_INPUT_KINDS = ["relu_halves", "zeros", "constant", "last_cell", "eight_values"]


def pool_input(kind, shape, dtype, seed):
    rs = np.random.RandomState(seed)
    N, H, W, C = shape
    if kind == "relu_halves":
        v = np.maximum(np.round(2 * rs.randn(*shape)) / 2, 0)                 # about half zeros, the rest in steps of 0.5
    elif kind == "zeros":
        v = np.zeros(shape)
    elif kind == "constant":
        v = np.full(shape, 1.25)
    elif kind == "last_cell":                                                 # increasing row-major: a window's maximum is its LAST valid cell
        v = np.broadcast_to((np.arange(H)[:, None] * W + np.arange(W)[None, :])[None, :, :, None] / 4.0, shape).copy()
    else:
        v = np.array([-2.0, -0.5, 0.0, 0.0, 0.25, 0.25, 1.0, 3.0])[rs.randint(0, 8, size=shape)]     # 6 distinct values, two of them twice as likely
    return v.astype(_np_dtype(dtype))


def pool_dy(shape, dtype, seed):
    """Multiples of 2^-6 in [-4, 4]: any sum of up to nine is exact in float32 (and of up to four, in float16)."""
    return (np.random.RandomState(seed).randint(-256, 257, size=shape) / 64.0).astype(_np_dtype(dtype))


# (k, stride, pad, H, W): 3x3/s2 runs maxpool3s2_bwd_kernel, everything else maxpool_bwd_kernel
POOL_SHAPES = [(3, 2, p, h, w) for p in ("SAME", "VALID") for (h, w) in ((47, 156), (94, 311), (7, 9))] + \
              [(3, 2, "SAME", h, w) for (h, w) in ((1, 1), (2, 2), (1, 40), (40, 1))] + \
              [(2, 2, p, h, w) for p in ("VALID", "SAME") for (h, w) in ((21, 30), (20, 31), (8, 8), (9, 7))] + [(3, 1, "SAME", 13, 17)]
POOL_DEGENERATE_VALID = [(1, 1), (2, 2), (1, 40), (40, 1)]      # 3x3 VALID windows do not fit: there is no output cell


def _pool_nc(i, ev):
    return (1, 2, 5, 3)[i % 4], (ev, 3 * ev, 96)[i % 3]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["k%ds%d_%s_%dx%d" % s for s in POOL_SHAPES])
def test_maxpool_backward_tie_rule_against_the_definition(dtype, shape):
    """maxpool3s2_bwd_kernel / maxpool_bwd_kernel -- the root every other max-pool backward form is compared with bitwise -- on
    inputs where ties are the rule, against maxpool_bwd_reference: ==, the one rounding to the storage type included; with the
    fused ReLU backward; and maxpool_bwd_idx from the forward's window index lands on the same reference, so the chain of bitwise
    comparisons inside the library has an end outside it.  ("last_cell" in float16: above 2048 / 4 neighbouring values round
    together, so some windows tie there too -- the reference sees the same stored bits.)"""
    ops = _ops()
    k, s, pad, H, W = shape
    ev = _ev(dtype)
    idx_form = s == 2 and not (k == 2 and pad == "VALID" and (H < 2 or W < 2))
    for i, kind in enumerate(POOL_INPUT_KINDS):
        N, C = _pool_nc(i + H, ev)
        N = min(N, 2) if H * W > 10000 else N
        x = pool_input(kind, (N, H, W, C), dtype, seed=10 * H + i)
        Ho, Wo = pool_geometry(H, k, s, pad)[0], pool_geometry(W, k, s, pad)[0]
        dy = pool_dy((N, Ho, Wo, C), dtype, seed=20 * W + i)
        xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
        ref = maxpool_bwd_reference(x, dy, k, s, pad)
        for relu in (False, True):
            want = _cast(np.where(x > 0, ref, 0.0) if relu else ref, dtype)      # the reference times (x > 0)
            got = ops.maxpool_bwd(xd, dyd, k, s, pad, relu=relu)
            _same_bits(got, want, "%s %s relu=%d" % (shape, kind, relu))
            if idx_form and kind in ("relu_halves", "eight_values"):
                y, idx = ops.maxpool_nhwc_idx(xd, k, s, pad)
                _same_bits(ops.maxpool_bwd_idx(idx, y, dyd, (H, W), k, s, pad, relu=relu), want, "idx form %s %s relu=%d" % (shape, kind, relu))
        if k == 2 and pad == "VALID":                 # an odd last row / column belongs to no window: zero
            g = got.cpu().numpy()
            assert (g[:, 2 * Ho:] == 0).all() and (g[:, :, 2 * Wo:] == 0).all()


@pytest.mark.parametrize("hw", POOL_DEGENERATE_VALID, ids=["%dx%d" % s for s in POOL_DEGENERATE_VALID])
def test_maxpool_backward_valid_window_that_does_not_fit_is_rejected(hw):
    """3x3 / stride 2 / VALID on a map smaller than the window has no output cell: dy is empty, and the library refuses the call
    (a null dy) instead of launching on it."""
    from squeezedet_amd import _lib
    ops = _ops()
    H, W = hw
    Ho, Wo = max(pool_geometry(H, 3, 2, "VALID")[0], 0), max(pool_geometry(W, 3, 2, "VALID")[0], 0)
    assert Ho * Wo == 0
    x = torch.zeros((1, H, W, 8), dtype=torch.float32, device=DEV)
    dy = torch.zeros((1, Ho, Wo, 8), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.SqdetError):
        ops.maxpool_bwd(x, dy, 3, 2, "VALID")


@pytest.mark.parametrize("case", [("3s2", 3, 2, "SAME", (8, 94, 311, 576)), ("generic", 2, 2, "VALID", (8, 94, 311, 192))], ids=["maxpool3s2", "maxpool_generic"])
def test_maxpool_backward_above_the_workgroup_cap(case):
    """More 16-byte work items than 16 384 workgroups of 256 threads (4 194 304): the grid-stride loop of each kernel.  float16;
    maxpool3s2_bwd_kernel's items are 2x2 cell blocks (8 x 47 x 156 x 72 = 4.2 M), maxpool_bwd_kernel's are cells (5.6 M)."""
    ops = _ops()
    name, k, s, pad, (N, H, W, C) = case
    items = N * (-(-H // 2)) * (-(-W // 2)) * (C // 8) if name == "3s2" else N * H * W * (C // 8)
    assert items > 16384 * 256
    rs = np.random.RandomState(4)
    x = np.array([0.0, 0.0, 0.0, 0.5, 0.5, 1.0, 1.5, 2.0], np.float16)[rs.randint(0, 8, size=(N, H, W, C), dtype=np.uint8)]
    Ho, Wo = pool_geometry(H, k, s, pad)[0], pool_geometry(W, k, s, pad)[0]
    dy = (rs.randint(-256, 257, size=(N, Ho, Wo, C), dtype=np.int16) / np.float32(64.0)).astype(np.float16)
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    got = ops.maxpool_bwd(xd, dyd, k, s, pad, relu=True).cpu().numpy()
    del xd, dyd
    for n in range(N):                                # (image by image: the float64 reference of the whole batch is 1 GiB)
        want = _cast(maxpool_bwd_reference(x[n:n + 1], dy[n:n + 1], k, s, pad, relu=True), torch.float16)
        _same_bits(got[n:n + 1], want, "%s image %d" % (name, n))


# ================================================================== 5. loss
def loss_config(classes, full):
    mc = O.kitti_squeezeDet_config() if full else O.squeezeDet_config_for_input(128, 256)
    mc.CLASSES = classes
    return mc


def loss_reference64(mc, preds, mask, delta_in, box_in, labels):
    """_add_interpretation_graph + _add_loss_graph (nn_skeleton.py:142-327) restated in float64 torch-CPU, written from the
    reference's lines -- not from the kernel and not through oracle.train_oracle: losses [3], ious [B,A], dpreds (autograd; the
    ious carry no gradient, nn_skeleton.py:263-268)."""
    f64 = torch.float64
    p = torch.from_numpy(np.asarray(preds)).to(f64).requires_grad_(True)
    B = p.shape[0]
    K, C, A, eps = mc.ANCHOR_PER_GRID, mc.CLASSES, mc.ANCHORS, float(np.float32(mc.EPSILON))
    m = torch.from_numpy(np.asarray(mask)).to(f64).reshape(B, A)
    dl_in = torch.from_numpy(np.asarray(delta_in)).to(f64).reshape(B, A, 4)
    bx = torch.from_numpy(np.asarray(box_in)).to(f64).reshape(B, A, 4)
    lab = torch.from_numpy(np.asarray(labels)).to(f64).reshape(B, A, C)
    anc = torch.from_numpy(np.asarray(mc.ANCHOR_BOX).astype(np.float32)).to(f64)            # the float32 anchors the kernel reads
    nobj = m.sum()
    pc = torch.softmax(p[..., :K * C].reshape(B, A, C), dim=2)                               # :150-160
    conf = torch.sigmoid(p[..., K * C:K * C + K].reshape(B, A))                              # :163-170
    dl = p[..., K * C + K:].reshape(B, A, 4)                                                 # :173-177
    with torch.no_grad():
        thr = float(np.float32(mc.EXP_THRESH))
        sexp = lambda w: torch.where(w > thr, float(np.exp(thr)) * (w - thr + 1.0), torch.exp(torch.minimum(w, torch.tensor(thr, dtype=f64))))   # util.py:219-231
        cx, cy = anc[:, 0] + dl[..., 0] * anc[:, 2], anc[:, 1] + dl[..., 1] * anc[:, 3]      # :192-201
        bw, bh = anc[:, 2] * sexp(dl[..., 2]), anc[:, 3] * sexp(dl[..., 3])
        w1, h1 = float(mc.IMAGE_WIDTH) - 1.0, float(mc.IMAGE_HEIGHT) - 1.0                   # :214-233
        xmin, ymin = torch.clamp(cx - bw / 2, 0.0, w1), torch.clamp(cy - bh / 2, 0.0, h1)
        xmax, ymax = torch.clamp(cx + bw / 2, 0.0, w1), torch.clamp(cy + bh / 2, 0.0, h1)
        w2, h2 = xmax - xmin + 1.0, ymax - ymin + 1.0                                        # bbox_transform_inv (util.py:181-196)
        dcx, dcy = xmin + 0.5 * w2, ymin + 0.5 * h2
        a = [dcx - w2 / 2, dcy - h2 / 2, dcx + w2 / 2, dcy + h2 / 2]                         # :240-262
        b = [bx[..., 0] - bx[..., 2] / 2, bx[..., 1] - bx[..., 3] / 2, bx[..., 0] + bx[..., 2] / 2, bx[..., 1] + bx[..., 3] / 2]
        iw = torch.clamp(torch.minimum(a[2], b[2]) - torch.maximum(a[0], b[0]), min=0.0)
        ih = torch.clamp(torch.minimum(a[3], b[3]) - torch.maximum(a[1], b[1]), min=0.0)
        inter = iw * ih
        union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
        ious = inter / (union + eps) * m
    m3 = m.reshape(B, A, 1)
    class_loss = ((lab * (-torch.log(pc + eps)) + (1 - lab) * (-torch.log(1 - pc + eps))) * m3 * mc.LOSS_COEF_CLASS).sum() / nobj      # :292-299
    conf_loss = (((ious - conf) ** 2) * (m * mc.LOSS_COEF_CONF_POS / nobj + (1 - m) * mc.LOSS_COEF_CONF_NEG / (A - nobj))).sum(dim=1).mean()   # :304-312
    bbox_loss = (mc.LOSS_COEF_BBOX * (m3 * (dl - dl_in)) ** 2).sum() / nobj                                                              # :317-323
    (dp,) = torch.autograd.grad(class_loss + conf_loss + bbox_loss, p)
    return (np.array([class_loss.item(), conf_loss.item(), bbox_loss.item()]), ious.numpy(), dp.numpy())


def loss_oracle32(mc, preds, mask, delta_in, box_in, labels):
    """The float32 CPU oracle on the same inputs (what tests/test_gpu_train.py compares with)."""
    p = torch.from_numpy(np.asarray(preds, np.float32)).requires_grad_(True)
    parts = TO.loss_graph(mc, p, mask, delta_in, box_in, labels)
    (dp,) = torch.autograd.grad(parts["class_loss"] + parts["conf_loss"] + parts["bbox_loss"], p)
    return (np.array([float(parts["class_loss"]), float(parts["conf_loss"]), float(parts["bbox_loss"])], np.float64),
            parts["ious"].numpy().astype(np.float64), dp.numpy().astype(np.float64))


# name: (classes, full grid (B = 8, 24 x 78, 134 784 anchors) or the 8 x 16 grid (B = 3), input class)
LOSS_CASES = {"full_randn": (3, True, "randn"), "full_edges": (3, True, "edges"), "full_saturated": (3, True, "saturated"),
              "small_c1": (1, False, "randn"), "small_c2": (2, False, "edges"), "small_c20": (20, False, "randn"),
              "small_c20_edges": (20, False, "edges"), "small_one_object": (3, False, "one_object"), "small_saturated": (2, False, "saturated")}


def loss_inputs(name):
    """preds [B,gh,gw,K*(C+5)] float32 and dense labels.  Input classes --
    randn: randn * 1.2 (well conditioned: the inputs of tests/test_gpu_train.py);
    edges: the same with, on labelled and unlabelled anchors alike, width / height deltas exactly at EXP_THRESH, one ulp either
      side and at +8; centre deltas that push the decoded box over each of the four borders and wholly outside the image; and
      ground-truth boxes of zero width;
    one_object: exactly one labelled anchor in the whole batch;
    saturated: class logits +-30 and confidence logits +-20 on a third of the anchors."""
    classes, full, kind = LOSS_CASES[name]
    mc = loss_config(classes, full)
    B = 8 if full else 3
    gh, gw = (24, 78) if full else O.squeezedet_grid(128, 256)
    K, C, A = mc.ANCHOR_PER_GRID, classes, mc.ANCHORS
    assert A == gh * gw * K
    rs = np.random.RandomState(sum(map(ord, name)))
    preds = (rs.randn(B, gh, gw, K * (C + 5)) * 1.2).astype(np.float32)
    anchors = np.asarray(mc.ANCHOR_BOX)
    mask, delta = np.zeros((B, A, 1), np.float32), np.zeros((B, A, 4), np.float32)
    box, labels = np.zeros((B, A, 4), np.float32), np.zeros((B, A, C), np.float32)
    for b in range(B):
        nb = (1 if b == 0 else 0) if kind == "one_object" else rs.randint(1, 9)
        for a in rs.choice(A, nb, replace=False):
            mask[b, a, 0] = 1.0
            delta[b, a] = rs.randn(4) * 0.4
            box[b, a] = anchors[a] * np.array([1, 1, 0, 0]) + anchors[a][[2, 3, 2, 3]] * np.array([rs.uniform(-.3, .3), rs.uniform(-.3, .3), rs.uniform(.6, 1.5), rs.uniform(.6, 1.5)])
            labels[b, a, rs.randint(C)] = 1.0
    pv = preds.reshape(B, A // K, K * (C + 5))
    dview = lambda b, a: pv[b, a // K, K * (C + 1) + 4 * (a % K):K * (C + 1) + 4 * (a % K) + 4]      # the four deltas of anchor a
    if kind == "edges":
        thr = np.float32(mc.EXP_THRESH)
        plant = [(2, thr), (3, thr), (2, np.nextafter(thr, np.float32(2))), (3, np.nextafter(thr, np.float32(0))), (2, np.nextafter(thr, np.float32(0))),
                 (3, np.nextafter(thr, np.float32(2))), (2, np.float32(8)), (3, np.float32(8)), (0, np.float32(-60)), (0, np.float32(60)),
                 (1, np.float32(-60)), (1, np.float32(60)), (0, np.float32(-4)), (0, np.float32(4)), (1, np.float32(-4)), (1, np.float32(4))]
        lab_an = np.argwhere(mask[..., 0] > 0)
        for j, (d, v) in enumerate(plant):
            for b, a in (lab_an[j % len(lab_an)], (j % B, int(rs.randint(A)))):     # on a labelled anchor and on any anchor
                dview(b, a)[d] = v
        for b, a in lab_an[::3]:
            box[b, a, 2] = 0.0                                                      # zero-width ground truth
        # border anchors pushed outwards: boxes clipped at the left / right / top / bottom border
        for b in range(B):
            for cell, d, v in ((0, 0, -1.5), (gw - 1, 0, 1.5), (0, 1, -1.5), ((gh - 1) * gw, 1, 1.5)):
                pv[b, cell, K * (C + 1) + d::4][:K] = v
    if kind == "saturated":
        sel = rs.uniform(size=(B, A // K)) < 1 / 3.0
        pv[sel, :K * C] = np.where(rs.uniform(size=(int(sel.sum()), K * C)) < 0.5, -30.0, 30.0)
        pv[sel, K * C:K * C + K] = np.where(rs.uniform(size=(int(sel.sum()), K)) < 0.5, -20.0, 20.0)
        for b, a in np.argwhere(mask[..., 0] > 0)[::2]:                             # and on labelled anchors, whatever sel drew
            pv[b, a // K, (a % K) * C:(a % K) * C + C] = np.where(rs.uniform(size=C) < 0.5, -30.0, 30.0)
            pv[b, a // K, K * C + a % K] = 20.0 if rs.uniform() < 0.5 else -20.0
    return mc, preds, mask, delta, box, labels


def loss_errors(got, ref):
    """Largest absolute element error of (the three losses, ious, dpreds)."""
    return [float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, ref)]


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_loss_against_float64_within_four_times_the_float32_oracles_error(name):
    ops = _ops()
    mc, preds, mask, delta, box, labels = loss_inputs(name)
    B = preds.shape[0]
    ref = loss_reference64(mc, preds, mask, delta, box, labels)
    e_ref = loss_errors(loss_oracle32(mc, preds, mask, delta, box, labels), ref)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    anchors = t(np.asarray(mc.ANCHOR_BOX).astype(np.float32))
    nobj = float(mask.sum())
    dp, ious, losses = ops.loss_fwd_bwd(t(preds), anchors, t(mask.reshape(B, -1)), t(delta), t(box), t(labels), mc, nobj)
    dp_d, ious_d, losses_d = ops.loss_fwd_bwd(t(preds), anchors, t(mask.reshape(B, -1)), t(delta), t(box), t(labels), mc, ops.sum_f32(t(mask)))
    torch.cuda.synchronize()
    assert torch.equal(dp, dp_d) and torch.equal(ious, ious_d) and torch.equal(losses, losses_d)      # num_objects from the device: same bits
    got = (losses.cpu().numpy(), ious.cpu().numpy(), dp.cpu().numpy())
    e_gpu = loss_errors(got, ref)
    print("LOSS %-18s losses %s | kernel err / oracle err: losses %.2e / %.2e  ious %.2e / %.2e  dpreds %.2e / %.2e (max |dpreds| %.3g)"
          % (name, np.array2string(ref[0], precision=5), e_gpu[0], e_ref[0], e_gpu[1], e_ref[1], e_gpu[2], e_ref[2], np.abs(ref[2]).max()))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    for what, eg, er in zip(("losses", "ious", "dpreds"), e_gpu, e_ref):
        assert eg <= 4.0 * er + 1e-7, "%s %s: kernel error %g, float32 oracle error %g" % (name, what, eg, er)
    if LOSS_CASES[name][2] == "randn":               # well conditioned: also the bounds tests/test_gpu_train.py asserts
        np.testing.assert_allclose(got[0], ref[0], rtol=2e-5)
        np.testing.assert_allclose(got[1], ref[1], rtol=1e-5, atol=1e-6)
        assert e_gpu[2] <= 5e-5 * np.abs(ref[2]).max() + 1e-7


@pytest.mark.parametrize("loss_scale", [512.0, 65536.0])
def test_mixed_precision_loss_at_a_size_that_loops(loss_scale):
    """B = 8 at the full grid (134 784 anchors: the grid-stride loop, 512 workgroups, eight laps of loss_finish_kernel):
    loss_fwd_bwd_mixed stays bitwise convert -> loss -> convert, also where float16 gradients overflow to inf (65 536)."""
    ops = _ops()
    mc, preds, mask, delta, box, labels = loss_inputs("full_edges")
    B = preds.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p16 = t(preds).to(torch.float16)
    args = (t(np.asarray(mc.ANCHOR_BOX).astype(np.float32)), t(mask.reshape(B, -1)), t(delta), t(box), t(labels), mc)
    for nobj in (float(mask.sum()), ops.sum_f32(t(mask))):
        dp, ious, losses = ops.loss_fwd_bwd(ops.convert_scale(p16, torch.float32), *args, nobj)
        want = ops.convert_scale(dp, torch.float16, loss_scale)
        g16, dp2, ious2, losses2 = ops.loss_fwd_bwd_mixed(p16, *args, nobj, loss_scale)
        torch.cuda.synchronize()
        _same_bits(g16, want.cpu().numpy(), "g16 at scale %g" % loss_scale)
        assert torch.equal(dp2, dp) and torch.equal(ious2, ious) and torch.equal(losses2, losses)
        assert bool(torch.isfinite(dp).all()) and bool(torch.isinf(g16).any()) == (loss_scale == 65536.0)


# ================================================================== 6. optimizer
OPT_COUNTS = [1, 255, 256, 257, 2047, 2048, 2049, 131072, 131073]      # around 2048 per block and the 64-block limit
OPT_NVARS = 300                                                        # > opt_norm_kernel's 256 threads: its loop takes a second lap
SENTINEL = -123.456


def opt_layout():
    """300 variables, counts cycling through OPT_COUNTS with one of 600 001, gaps of 1 .. 63 elements between segments (and in
    front of the first), every other decay zero."""
    rs = np.random.RandomState(31)
    cnts = [OPT_COUNTS[v % len(OPT_COUNTS)] for v in range(OPT_NVARS)]
    cnts[150] = 600001
    offs, o = [], 0
    for c in cnts:
        o += int(rs.randint(1, 64))
        offs.append(o)
        o += c
    total = o + int(rs.randint(1, 64))
    decs = [1e-4 if v % 2 == 0 else 0.0 for v in range(OPT_NVARS)]
    return offs, cnts, decs, total


def opt_buffers(offs, cnts, total, seed):
    """params, grads, accum (float32) with SENTINEL in the gaps; gradient norms about 3 (clipped at 1) for every other PAIR of
    variables and about 0.3 for the rest."""
    rs = np.random.RandomState(seed)
    P, G, M = [np.full(total, SENTINEL, np.float32) for _ in range(3)]
    inside = np.zeros(total, bool)
    for v, (o, c) in enumerate(zip(offs, cnts)):
        P[o:o + c] = rs.randn(c) * 0.1
        G[o:o + c] = rs.randn(c) * ((3.0 if (v // 2) % 2 == 0 else 0.3) / np.sqrt(c)) if c > 1 else (3.0 if (v // 2) % 2 == 0 else 0.3)
        M[o:o + c] = rs.randn(c) * 0.01
        inside[o:o + c] = True
    return P, G, M, inside


def opt_reference64(P, G, M, offs, cnts, decs, lr, momentum, clip, grad_scale):
    """g = g * grad_scale + decay * w; per variable g *= clip / max(||g||, clip); accum = m * accum + g; w -= lr * accum -- float64.
    Returns new (P, G, M), the clip factors and the element-wise error scales of the three outputs."""
    P2, G2, M2 = P.astype(np.float64), G.astype(np.float64), M.astype(np.float64)
    tolP, tolG, tolM = np.zeros_like(P2), np.zeros_like(P2), np.zeros_like(P2)
    factors = np.zeros(len(offs))
    for v, (o, c, d) in enumerate(zip(offs, cnts, decs)):
        s = slice(o, o + c)
        w, a = P2[s].copy(), M2[s].copy()
        g = G2[s] * grad_scale + d * w
        f = clip / max(np.sqrt((g * g).sum()), clip)
        acc = momentum * a + g * f
        G2[s], M2[s], P2[s], factors[v] = g, acc, w - lr * acc, f
        tolG[s] = np.abs(G[s].astype(np.float64) * grad_scale) + np.abs(d * w)
        tolM[s] = np.abs(momentum * a) + np.abs(g)
        tolP[s] = np.abs(w) + lr * (np.abs(momentum * a) + np.abs(g))
    return P2, G2, M2, factors, (tolP, tolG, tolM)


def _opt_scale_table(opt, cnts):
    """The per-variable clip factors opt_norm_kernel left in the optimizer's workspace (layout of sqdet_optimizer_step: segment
    table of 32-byte entries | block table | float64 partial sums | float32 scale, each rounded up to 256 bytes)."""
    nblocks = sum(min(64, max(1, -(-c // 2048))) for c in cnts)
    up = lambda b: (b + 255) // 256 * 256
    off = up(up(up(len(cnts) * 32) + nblocks * 4) + nblocks * 8)
    return opt.ws[off:off + 4 * len(cnts)].cpu().numpy().view(np.float32).astype(np.float64)


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_optimizer_300_variables_gaps_and_two_steps_against_float64():
    """Each output is at most six float32 operations on O(1) values, so |got - ref64| <= 8 * 2^-24 * (|w| + lr * (|m * accum| + |g|))
    element-wise (accum and the written-back gradient by the same rule on their own terms); the clip factor -- formed from float64
    norms -- within 2^-22 relative.  Gaps between segments are never touched, and a NaN / inf lying in a gap of `grads` is not
    a gradient: found_inf stays 0.  Two steps, so the momentum term is live."""
    ops = _ops()
    offs, cnts, decs, total = opt_layout()
    lr, mom, clip, gs = 0.01, 0.9, 1.0, 0.5
    P, G, M, inside = opt_buffers(offs, cnts, total, seed=1)
    gaps = np.flatnonzero(~inside)
    assert 300 <= gaps.size <= 301 * 63
    opt = ops.MomentumOptimizer(offs, cnts, decs, DEV)
    Pd, Md = torch.from_numpy(P).to(DEV), torch.from_numpy(M).to(DEV)
    flag = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    Pc, Mc = P, M
    for step in range(2):
        G = opt_buffers(offs, cnts, total, seed=2 + step)[1]
        G[gaps[::3]], G[gaps[1::3]] = np.nan, np.inf                     # not gradients
        Gd = torch.from_numpy(G).to(DEV)
        opt.step(Pd, Gd, Md, lr, mom, clip, gs, found_inf=flag)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0, "a non-finite value in a GAP tripped found_inf"
        Pr, Gr, Mr, fr, (tolP, tolG, tolM) = opt_reference64(Pc, G, Mc, offs, cnts, decs, lr, mom, clip, gs)
        Pg, Gg, Mg = Pd.cpu().numpy(), Gd.cpu().numpy(), Md.cpu().numpy()
        for what, got, before in (("params", Pg, P), ("grads", Gg, G), ("accum", Mg, M)):
            assert np.array_equal(_i32(got)[gaps], _i32(before)[gaps]), "step %d: a gap of %s changed" % (step, what)
        clipped = int((fr < 1.0).sum())
        assert 100 <= clipped <= 200, clipped
        fg = _opt_scale_table(opt, cnts)
        assert (np.abs(fg - fr) <= 2.0 ** -22 * fr).all(), "clip factors: worst %g" % np.abs(fg / fr - 1).max()
        for what, got, ref, tol in (("params", Pg, Pr, tolP), ("grads", Gg, Gr, tolG), ("accum", Mg, Mr, tolM)):
            err = np.abs(got.astype(np.float64) - ref)[inside]
            worst = (err / np.maximum(8 * U32 * tol[inside], 1e-300)).max()
            print("optimizer step %d %s: worst error / bound %.3f" % (step, what, worst))
            assert (err <= 8 * U32 * tol[inside]).all(), "step %d %s: %g of the bound" % (step, what, worst)
        Pc, Mc = Pg, Mg                                                  # the next step starts from the device's float32 state


def test_optimizer_overflow_in_the_last_element_of_the_last_variable():
    """An inf in the LAST element of variable 299 (a second-lap variable of opt_norm_kernel, the last block's last thread): found_inf,
    parameters and momentum bit-identical.  The gradients are not: pass 1 has rewritten them (scaled, weight decay added)
    before the norm is known -- pinned."""
    ops = _ops()
    offs, cnts, decs, total = opt_layout()
    P, G, M, inside = opt_buffers(offs, cnts, total, seed=5)
    G[offs[299] + cnts[299] - 1] = np.inf
    opt = ops.MomentumOptimizer(offs, cnts, decs, DEV)
    Pd, Gd, Md = [torch.from_numpy(a).to(DEV) for a in (P, G, M)]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt.step(Pd, Gd, Md, 0.01, 0.9, 1.0, 0.5, found_inf=flag)
    torch.cuda.synchronize()
    assert int(flag.item()) == 1
    assert np.array_equal(_i32(Pd.cpu().numpy()), _i32(P)) and np.array_equal(_i32(Md.cpu().numpy()), _i32(M))
    Gg = Gd.cpu().numpy()
    assert np.array_equal(_i32(Gg)[~inside], _i32(G)[~inside])
    G0 = np.where(np.isinf(G), 0.0, G)
    _, Gr, _, _, (_, tolG, _) = opt_reference64(P, G0, M, offs, cnts, decs, 0.01, 0.9, 1.0, 0.5)
    fin = inside & ~np.isinf(G)
    assert (np.abs(Gg.astype(np.float64) - Gr)[fin] <= 8 * U32 * tolG[fin]).all() and np.isinf(Gg[offs[299] + cnts[299] - 1])
    opt.step(Pd, torch.from_numpy(opt_buffers(offs, cnts, total, seed=6)[1]).to(DEV), Md, 0.01, 0.9, 1.0, 0.5, found_inf=flag)
    assert int(flag.item()) == 0 and not np.array_equal(_i32(Pd.cpu().numpy()), _i32(P))      # and the next, finite, step applies


def test_trainers_variable_counts_against_opt_norm_kernels_256_threads():
    """How many variables the trainers hand the optimizer, counted from the trainers: SqueezeDet 62, ResNet50+ConvDet 59 (its
    batch norms are frozen and folded: they add no variable).  So no trainer of this project reaches the second lap of
    opt_norm_kernel's 256-thread loop today; the 300 variables of the tests above are what keeps that loop honest for a net that
    would."""
    from tests import test_gpu_train as T
    from tests import test_gpu_resnet as TR
    n_sq = len(T._trainer()[0].names)
    n_res = len(TR._trainer()[0].names)
    print("trainable variables: SqueezeDet %d, ResNet50+ConvDet %d" % (n_sq, n_res))
    assert (n_sq, n_res) == (62, 59) and max(n_sq, n_res) <= 256 < OPT_NVARS
