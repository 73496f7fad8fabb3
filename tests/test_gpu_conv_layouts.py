"""GPU tests, conv output layouts: every conv kernel family writing a CHANNEL SLICE of wider rows (the fire concat, out_coffset),
accumulating into it (sqdet_conv2d_add_nhwc_fwd), adding a residual tensor (sqdet_conv2d_res_nhwc_fwd), and the backward-data
conv reading a slice of dY (sqdet_conv2d_nhwc_bwd_data(_relu)).

Reference: the conv in float64 on the CPU (torch.nn.functional.conv2d, TF SAME / VALID padding) on the operands the kernel sees
(float16-rounded x, W, prior y, residual), then the ReLU, then one rounding to the storage type.  Tolerances as in
tests/test_gpu_ops.py: float32 1e-3 relative + 1e-4 absolute (max relative error < 1e-4), float16 2^-9 relative + 1e-3 absolute.

Canary: the output (and the residual) is filled with seeded random values before each launch; every channel outside the written
slice, and the whole residual, must be BITWISE unchanged afterwards.  Rejected calls must leave every tensor unchanged.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sqdet_oracle as O
from tests.test_gpu_ops import CONV_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_CASES = {c[0]: c for c in CONV_CASES}
# Cin 4: whole 16-byte lane chunks in float32, the im2col-gather kernel in float16 (8 halves per chunk)
_CASES["cin4_3x3"] = ("cin4_3x3", 1, 9, 13, 4, 16, 3, 1, "SAME", True)
_TDT = {"fp32": torch.float32, "fp16": torch.float16}


def _ops():
    from squeezedet_amd import ops
    return ops


@pytest.fixture(params=["auto", "generic"])
def conv_algo(request):
    """auto = the specialised kernels where eligible; generic = conv_direct / conv_gather only."""
    ops = _ops()
    ops.set_option("conv_algo", 1 if request.param == "generic" else 0)
    yield request.param
    ops.set_option("conv_algo", 0)


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (2 ** 31)


def _conv64(x, w, b, stride, padding):
    """float64 NHWC conv + bias, no activation: x [N,H,W,Cin], w HWIO [k,k,Cin,Cout], b [Cout]."""
    k = w.shape[0]
    xn = x.permute(0, 3, 1, 2)
    if padding == "SAME":
        pt, pb = O.same_pads(x.shape[1], k, stride)
        pl, pr = O.same_pads(x.shape[2], k, stride)
        xn = F.pad(xn, (pl, pr, pt, pb))
    y = F.conv2d(xn, w.permute(3, 2, 0, 1), None, stride=stride)
    return (y + b.view(1, -1, 1, 1)).permute(0, 2, 3, 1)


def _finish(v64, relu, dtype):
    """relu? then ONE rounding of the float64 value to the storage type."""
    return (torch.relu(v64) if relu else v64).to(_TDT[dtype])


def _rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _close(got, want, dtype, what):
    g = got.double().cpu().numpy()
    w = want.double().cpu().numpy()
    assert g.shape == w.shape, what
    if dtype == "fp32":
        np.testing.assert_allclose(g, w, rtol=1e-3, atol=1e-4, err_msg=what)
        assert _rel_err(g, w) < 1e-4, what
    else:
        np.testing.assert_allclose(g, w, rtol=2 ** -9, atol=1e-3, err_msg=what)


def _canary(shape, dtype, seed):
    """Seeded random finite values in the storage type, on the device."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(_TDT[dtype]).to(DEV)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same_bits(a, b, what):
    diff = int((_bits(a) != _bits(b)).sum())
    assert diff == 0, "%s: %d values changed" % (what, diff)


def _outside_unchanged(y, before, off, cout, what):
    _same_bits(y[..., :off], before[..., :off], what + ": channels left of the slice")
    _same_bits(y[..., off + cout:], before[..., off + cout:], what + ": channels right of the slice")


class _Conv:
    """One CONV_CASES row's operands (float16-rounded for fp16) on the device, and its float64 conv + bias on the CPU."""

    def __init__(self, name, dtype):
        _, N, H, W, cin, cout, k, s, pad, relu = _CASES[name]
        rs = np.random.RandomState(_seed(name))
        x = torch.from_numpy(rs.randn(N, H, W, cin).astype(np.float32)).to(_TDT[dtype])
        w = torch.from_numpy((rs.randn(k, k, cin, cout) * (2.0 / (k * k * cin)) ** 0.5).astype(np.float32)).to(_TDT[dtype]).float()
        b = torch.from_numpy(rs.uniform(-0.5, 0.5, cout).astype(np.float32))
        self.cout, self.stride, self.pad, self.relu = cout, s, pad, relu
        self.conv = _conv64(x.double(), w.double(), b.double(), s, pad)
        self.x = x.to(DEV).contiguous()
        self.packed = _ops().pack_conv_weights(w.to(DEV), _TDT[dtype])
        self.b = b.to(DEV)

    def out_shape(self, ctot):
        return tuple(self.conv.shape[:3]) + (ctot,)

    def run(self, relu, **kw):
        return _ops().conv2d_nhwc(self.x, self.packed, self.b, self.stride, self.pad, relu, **kw)


_CONV_CACHE = {}


def _conv(name, dtype):
    """Built once per shape and dtype and shared by every layout / form / conv_algo."""
    if (name, dtype) not in _CONV_CACHE:
        _CONV_CACHE[(name, dtype)] = _Conv(name, dtype)
    return _CONV_CACHE[(name, dtype)]


# (coffset, row width) of the written slice:
#   a: offset 0 of a wider row, a neighbour on the right;
#   b: the end of the row, at an offset that is a multiple of 4 but not of 8 (float16: 8-byte, not 16-byte, aligned segments);
#   c: the middle, at a multiple-of-8 offset, neighbours on both sides.
def _layout(which, cout):
    return {"a": (0, cout + 8), "b": (12, 12 + cout), "c": (16, 16 + cout + 8)}[which]


# Under conv_algo = auto these reach (besides conv_direct, which serves every shape under generic):
PLAIN_SHAPES = [
    "conv1_375x1242_like",    # conv_gather (Cin 3, stride 2, odd sizes)
    "e3_multitile_32_128",    # conv3x3_tile, single stage
    "e3_cin32_cout72",        # conv3x3_tile, ragged cout
    "e3_k384_n256",           # conv3x3_tile, K staged
    "convdet_full_24x78",     # split-K ConvDet
    "fire2_squeeze",          # conv1x1_stream
    "c1_k32_n80",             # conv1x1_stream, ragged cout
    "fire3_squeeze",          # float32: conv1x1_tile (one cout tile: the pipelined form does not take it)
    "g1_k264_n40",            # conv1x1_pipe
    "g1_k256_n72",            # conv1x1_pipe, five cout tiles per wave
    "g1_stride2_k256_n128",   # conv1x1_pipe, stride 2
    "k1_k264_n40",            # conv1x1_deepk (>= 8192 pixels)
    "k1_k160_n72",            # conv1x1_deepk, ragged cout
]


@pytest.mark.parametrize("layout", ["a", "b", "c"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", PLAIN_SHAPES)
def test_conv_forward_writes_only_its_channel_slice(name, dtype, layout, conv_algo):
    """sqdet_conv2d_nhwc_fwd into channels [off, off+cout) of wider rows: the slice matches the float64 reference, every other
    channel keeps its bits."""
    cv = _conv(name, dtype)
    off, ctot = _layout(layout, cv.cout)
    y = _canary(cv.out_shape(ctot), dtype, _seed(name, dtype, layout, "plain"))
    before = y.clone()
    got = cv.run(cv.relu, out=y, out_coffset=off)
    torch.cuda.synchronize()
    assert got.data_ptr() == y.data_ptr()
    what = "%s %s layout %s (%s)" % (name, dtype, layout, conv_algo)
    _outside_unchanged(y, before, off, cv.cout, what)
    _close(y[..., off:off + cv.cout], _finish(cv.conv, cv.relu, dtype), dtype, what)


# accumulate / residual forms: the 1x1 GEMM tile (conv1x1_pipe; conv1x1_tile for the one-tile fire2 squeeze), the 3x3 tile (single
# stage, ragged cout, staged K, the ConvDet shape -- not split-K: that kernel is plain-only), and under generic conv_direct
EPI_SHAPES = ["fire2_squeeze", "g1_k264_n40", "g1_k256_n72", "g1_stride2_k256_n128",
              "e3_multitile_32_128", "e3_cin32_cout72", "e3_k384_n256", "convdet_full_24x78"]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("layout", ["a", "b", "c"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", EPI_SHAPES)
def test_conv_accumulate_and_residual_on_channel_slices(name, dtype, layout, relu, conv_algo):
    """sqdet_conv2d_add_nhwc_fwd: y[slice] = relu?(conv + b + y[slice]); sqdet_conv2d_res_nhwc_fwd: y[slice] = relu?(conv + b +
    residual[slice]) with the residual left untouched -- both against the float64 reference, the rest of y unchanged, and the
    residual form bitwise the accumulate form."""
    cv = _conv(name, dtype)
    cout = cv.cout
    off, ctot = _layout(layout, cout)
    shape = cv.out_shape(ctot)
    what = "%s %s layout %s relu %d (%s)" % (name, dtype, layout, relu, conv_algo)
    res = _canary(shape, dtype, _seed(name, dtype, layout, "residual"))
    res_before = res.clone()
    want = _finish(cv.conv + res[..., off:off + cout].double().cpu(), relu, dtype)

    ya = _canary(shape, dtype, _seed(name, dtype, layout, "accumulate"))
    ya[..., off:off + cout] = res[..., off:off + cout]
    ya_before = ya.clone()
    cv.run(relu, out=ya, out_coffset=off, accumulate=True)
    yr = _canary(shape, dtype, _seed(name, dtype, layout, "res-out"))
    yr_before = yr.clone()
    got = cv.run(relu, out=yr, out_coffset=off, residual=res)
    torch.cuda.synchronize()
    assert got.data_ptr() == yr.data_ptr()

    _outside_unchanged(ya, ya_before, off, cout, "accumulate " + what)
    _close(ya[..., off:off + cout], want, dtype, "accumulate " + what)
    _same_bits(res, res_before, "residual " + what + ": the residual tensor")
    _outside_unchanged(yr, yr_before, off, cout, "residual " + what)
    _close(yr[..., off:off + cout], want, dtype, "residual " + what)
    _same_bits(yr[..., off:off + cout], ya[..., off:off + cout], "residual " + what + ": against the accumulate form")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["g1_k264_n40", "e3_cin32_cout72"])
def test_conv_residual_aliased_to_out_is_the_accumulate_form(name, dtype, conv_algo):
    """residual is out (the in-place route of sqdet_conv2d_res_nhwc_fwd): bitwise the accumulate form, on a sliced layout."""
    cv = _conv(name, dtype)
    cout = cv.cout
    off, ctot = _layout("c", cout)
    yr = _canary(cv.out_shape(ctot), dtype, _seed(name, dtype, "alias"))
    before = yr.clone()
    ya = yr.clone()
    want = _finish(cv.conv + yr[..., off:off + cout].double().cpu(), True, dtype)
    cv.run(True, out=yr, out_coffset=off, residual=yr)
    cv.run(True, out=ya, out_coffset=off, accumulate=True)
    torch.cuda.synchronize()
    what = "%s %s (%s)" % (name, dtype, conv_algo)
    _outside_unchanged(yr, before, off, cout, "aliased residual " + what)
    _close(yr[..., off:off + cout], want, dtype, "aliased residual " + what)
    _same_bits(yr, ya, "aliased residual " + what + ": against the accumulate form")


# (name, N, H, W, cin, cout, k): the FORWARD conv cin -> cout; the backward-data conv reads cout channels of dY and writes dx [.., cin]
BWD_CASES = [
    ("1x1_cin72_cout256", 1, 13, 29, 72, 256, 1),     # conv1x1_pipe, ragged dx channels
    ("1x1_cin16_cout64", 2, 23, 31, 16, 64, 1),       # conv1x1_tile (one cout tile)
    ("3x3_cin200_cout64", 2, 9, 19, 200, 64, 3),      # conv3x3_tile, ragged dx channels in 13 one-tile groups
    ("3x3_cin72_cout128", 1, 11, 19, 72, 128, 3),     # conv3x3_tile, ragged dx channels
]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_conv_backward_data_on_a_dy_slice(case, dtype, where, conv_algo):
    """dx = the float64 autograd input gradient of the conv on dY[..., off:off+cout]; accumulate: prior dx + that, rounded once;
    relu_of: zeroed where relu_of <= 0, after the sum.  dY and relu_of stay unchanged."""
    ops = _ops()
    name, N, H, W, cin, cout, k = case
    tdt = _TDT[dtype]
    kg = 8 if dtype == "fp16" else 4
    ctot = cout + 24
    off = {"first": 0, "middle": kg, "last": 24}[where]
    rs = np.random.RandomState(_seed(name))
    w = torch.from_numpy((rs.randn(k, k, cin, cout) / (k * k * cout) ** 0.5).astype(np.float32)).to(tdt).float()
    dy = _canary((N, H, W, ctot), dtype, _seed(name, dtype, where, "dy"))
    relu_of = _canary((N, H, W, cin), dtype, _seed(name, dtype, "relu_of"))
    dy_before, relu_before = dy.clone(), relu_of.clone()
    x64 = torch.zeros((N, H, W, cin), dtype=torch.float64, requires_grad=True)
    _conv64(x64, w.double(), torch.zeros(cout, dtype=torch.float64), 1, "SAME").backward(dy[..., off:off + cout].double().cpu())
    grad = x64.grad
    mask = relu_of.double().cpu() > 0
    pb = ops.PackedConvBwd(w.to(DEV), tdt)
    for accumulate in (False, True):
        for masked in (False, True):
            dx = _canary((N, H, W, cin), dtype, _seed(name, dtype, where, accumulate, masked))
            prior = dx.double().cpu()
            got = ops.conv2d_bwd_data(dy, pb, dx=dx, dy_coffset=off, accumulate=accumulate, relu_of=relu_of if masked else None)
            torch.cuda.synchronize()
            assert got.data_ptr() == dx.data_ptr()
            want = grad + prior if accumulate else grad
            if masked:
                want = torch.where(mask, want, torch.zeros_like(want))
            _close(dx, want.to(tdt), dtype, "%s %s dy_coffset %d accumulate %d relu_of %d (%s)"
                   % (name, dtype, off, accumulate, masked, conv_algo))
    _same_bits(dy, dy_before, "dy")
    _same_bits(relu_of, relu_before, "relu_of")


def _rejected(call, tensors, what):
    """call() must raise SqdetError and leave every tensor of `tensors` bitwise unchanged."""
    from squeezedet_amd import _lib
    before = [t.clone() for t in tensors]
    with pytest.raises(_lib.SqdetError):
        call()
    torch.cuda.synchronize()
    for i, (t, b) in enumerate(zip(tensors, before)):
        _same_bits(t, b, "%s: tensor %d after the rejected call" % (what, i))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_conv_forward_rejections_leave_memory_alone(dtype, conv_algo):
    """SQDET_UNSUPPORTED / SQDET_REQUIRE on the three forward entry points: an error, and out / residual untouched."""
    from squeezedet_amd import _lib
    cv = _conv("e3_cin32_cout72", dtype)
    cout = cv.cout
    bad = {"y_coffset % 4": (2, cout + 8), "y_coffset + cout > y_cstride": (8, cout + 4), "y_cstride % 4": (0, cout + 2)}
    for label, (off, ctot) in bad.items():
        shape = cv.out_shape(ctot)
        y = _canary(shape, dtype, _seed(dtype, label, "y"))
        res = _canary(shape, dtype, _seed(dtype, label, "res"))
        _rejected(lambda: cv.run(True, out=y, out_coffset=off), [y], "plain, " + label)
        _rejected(lambda: cv.run(True, out=y, out_coffset=off, accumulate=True), [y], "accumulate, " + label)
        _rejected(lambda: cv.run(True, out=y, out_coffset=off, residual=res), [y, res], "residual, " + label)
    # Cin not a multiple of 8 halves / 4 floats (the im2col-gather kernel): neither the accumulate nor the residual form
    for name in ["conv1_375x1242_like"] + (["cin4_3x3"] if dtype == "fp16" else []):
        g = _conv(name, dtype)
        for off, ctot in ((0, g.cout), _layout("a", g.cout)):
            shape = g.out_shape(ctot)
            y = _canary(shape, dtype, _seed(dtype, name, ctot, "y"))
            res = _canary(shape, dtype, _seed(dtype, name, ctot, "res"))
            _rejected(lambda: g.run(True, out=y, out_coffset=off, accumulate=True), [y], name + " accumulate")
            _rejected(lambda: g.run(True, out=y, out_coffset=off, residual=res), [y, res], name + " residual")
    # a null residual (the wrapper always passes one: straight through the C ABI)
    ops = _ops()
    off, ctot = _layout("c", cout)
    y = _canary(cv.out_shape(ctot), dtype, _seed(dtype, "null residual"))
    n, h, w, cin = [int(v) for v in cv.x.shape]
    _rejected(lambda: _lib.check(ops.lib().sqdet_conv2d_res_nhwc_fwd(
        cv.x.data_ptr(), cv.packed.data.data_ptr(), cv.b.data_ptr(), None, y.data_ptr(), n, h, w, cin, cout, 3, 1, _lib.PAD_SAME, 1,
        _lib.dtype_code(_TDT[dtype]), ctot, off, _lib.stream_ptr()), "sqdet_conv2d_res_nhwc_fwd"), [y], "null residual")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_conv_backward_data_rejections_leave_memory_alone(dtype, conv_algo):
    """dy_coffset not a multiple of the lane chunk (8 halves / 4 floats), and k = 5 (SQDET_REQUIRE): an error, dx untouched."""
    ops = _ops()
    tdt = _TDT[dtype]
    N, H, W, cin, cout = 1, 9, 13, 72, 64
    kg = 8 if dtype == "fp16" else 4
    dy = _canary((N, H, W, cout + 24), dtype, _seed(dtype, "bwd reject dy"))
    dx = _canary((N, H, W, cin), dtype, _seed(dtype, "bwd reject dx"))
    relu_of = _canary((N, H, W, cin), dtype, _seed(dtype, "bwd reject relu_of"))
    rs = np.random.RandomState(3)
    for k in (1, 3):
        pb = ops.PackedConvBwd(torch.from_numpy(rs.randn(k, k, cin, cout).astype(np.float32)).to(DEV), tdt)
        for off in (kg // 2, kg + kg // 2):
            for masked in (False, True):
                _rejected(lambda: ops.conv2d_bwd_data(dy, pb, dx=dx, dy_coffset=off, accumulate=True,
                                                      relu_of=relu_of if masked else None),
                          [dx, dy, relu_of], "k %d dy_coffset %d relu_of %d" % (k, off, masked))
    pb5 = ops.PackedConvBwd(torch.from_numpy(rs.randn(5, 5, cin, cout).astype(np.float32)).to(DEV), tdt)
    for masked in (False, True):
        _rejected(lambda: ops.conv2d_bwd_data(dy, pb5, dx=dx, dy_coffset=0, accumulate=True, relu_of=relu_of if masked else None),
                  [dx, dy, relu_of], "k 5 relu_of %d" % masked)
