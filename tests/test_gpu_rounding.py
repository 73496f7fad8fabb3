"""GPU tests of the rounding contract (tests/rounding_contract.py) on every conv kernel family and fused launch of the hot path:
each conv of a launch is storage(relu?(float32-accumulated conv + float32 bias [+ residual])), rounded ONCE to nearest even.

Every device tensor is checked (a) element by element against the derived interval and (b) by a rate -- float16: the number
of non-zero elements whose bits differ from the correctly rounded float64 value; float32: max |got - exact| / magnitude --
against a cap of 4 x the largest value three CPU emulations of honest float32 accumulation give for the same case.  No
tolerance of this file's own: a defect the wide bands of the other conv tests let through (a truncating conversion, a bias
added after the rounding, a float16 running sum) changes 30 - 90 % of the elements; the caps sit near 1 %.

The float64 reference and the emulations are computed once per case and shared.  Shapes are the project's small ones; only
N grows, until at least 2000 non-zero elements (and 25 % of the tensor) are compared.
"""
import functools
import math
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import fused_launch_cases as FC
from tests import rounding_contract as RC
from tests.fused_launch_cases import Spec
from tests.test_gpu_conv_layouts import BWD_CASES as DGRAD_CASES
from tests.test_gpu_conv_layouts import EPI_SHAPES, PLAIN_SHAPES, _canary, _layout, _outside_unchanged
from tests.test_gpu_fused_edges import Op, _op, _options, _weights
from tests.test_gpu_ops import CONV_CASES
from tests.test_gpu_train import BWD_CASES as WGRAD_CASES
from tests.test_gpu_vgg16 import PAIRS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_TDT = {"fp32": torch.float32, "fp16": torch.float16}
_CASES = {c[0]: c for c in CONV_CASES}
REPORT = OrderedDict()      # family -> [(what, dtype, figures of RC.measure)]


def _ops():
    from squeezedet_amd import ops
    return ops


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (2 ** 31)


def _rnd(t, dtype):
    return t.half().float() if dtype == "fp16" else t


def _check(family, got, ref, emus, dtype, what):
    m = RC.check(got.detach().cpu(), ref, emus, dtype, what)
    REPORT.setdefault(family, []).append((what, dtype, m))
    return m


def _grown(n, per_image, relu):
    """N grown (only N) until about 2000 non-zero outputs can be compared; a ReLU keeps about half of them."""
    return max(n, int(math.ceil(RC.MIN_COMPARED / (per_image * (0.35 if relu else 0.9)))))


# auto = the specialised kernels where eligible; generic = conv_direct / conv_gather only.  The topmost parametrize varies
# fastest: both algorithms of a case run back to back and share its cached reference.
both_algos = pytest.mark.parametrize("conv_algo", ["auto", "generic"])


def _algo(conv_algo):
    return _options(conv_algo=1 if conv_algo == "generic" else 0)


# ------------------------------------------------------------------------------------------------------------- single convs
class _Single:
    """One CONV_CASES row: storage-rounded operands, and the reference / emulations of the plain form.  regime: a regime of
    tests/rounding_contract.py the operands are moved into; quantum q: the unit input first keeps only the bits it would keep
    under x 2^-q.  The reference and the device copies are made when first asked for."""

    def __init__(self, name, dtype, regime=None, quantum=0):
        _, N, H, W, cin, cout, k, s, pad, relu = _CASES[name]
        ho, wo = (-(-H // s), -(-W // s)) if pad == "SAME" else ((H - k) // s + 1, (W - k) // s + 1)
        N = _grown(N, ho * wo * cout, relu)
        rs = np.random.RandomState(_seed("single", name))
        x = _rnd(torch.from_numpy(rs.randn(N, H, W, cin).astype(np.float32)), dtype)
        w = _rnd(torch.from_numpy((rs.randn(k, k, cin, cout) * (2.0 / (k * k * cin)) ** 0.5).astype(np.float32)), dtype)
        b = torch.from_numpy(rs.uniform(-0.5, 0.5, cout).astype(np.float32))
        if quantum:
            x = RC.on_grid(x, quantum, dtype)
        self.x, ((self.w, self.b),) = RC.move(regime, x, [(w, b, 1)], dtype)
        self.dtype, self.cout, self.stride, self.pad, self.relu, self.regime, self.quantum = dtype, cout, s, pad, relu, regime, quantum
        self.out_shape = (N, ho, wo, cout)
        self._plain = self._res = self._rt = self._dev = None

    @property
    def plain(self):
        if self._plain is None:
            self._plain = RC.Case(RC.conv_program(self.x, self.w, self.b, self.stride, self.pad, self.relu), self.dtype)
            assert tuple(self._plain.ref["y"].want.shape) == self.out_shape
        return self._plain

    def residual_tensor(self):
        """The residual in the storage type on the CPU, scaled as the regime scales it (RC.residual_exponent); made once."""
        if self._rt is None:
            g = torch.Generator().manual_seed(_seed("residual", self.out_shape))
            res = torch.randn(self.out_shape, generator=g).to(_TDT[self.dtype]).float()
            if self.quantum:
                res = RC.on_grid(res, self.quantum, self.dtype)
            self._rt = RC.scaled(res, RC.residual_exponent(self.regime), self.dtype).to(_TDT[self.dtype])
        return self._rt

    def residual(self):
        """(residual tensor in the storage type on the CPU, the Case of relu?(conv + b + residual))."""
        if self._res is None:
            res = self.residual_tensor()
            self._res = (res, RC.Case(RC.conv_program(self.x, self.w, self.b, self.stride, self.pad, self.relu, res=res.float()), self.dtype))
        return self._res

    def run(self, **kw):
        if self._dev is None:
            self._dev = (self.x.to(DEV, _TDT[self.dtype]).contiguous(), _ops().pack_conv_weights(self.w.to(DEV), _TDT[self.dtype]),
                         self.b.to(DEV))
        xd, packed, bd = self._dev
        return _ops().conv2d_nhwc(xd, packed, bd, self.stride, self.pad, self.relu, **kw)


@functools.lru_cache(maxsize=6)
def _single(name, dtype, regime=None, quantum=0):
    return _Single(name, dtype, regime, quantum)


@both_algos
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv2d_rounds_once(case, dtype, conv_algo):
    """Every CONV_CASES row (the ConvDet heads 768 -> 72, 512 -> 72 and 512 -> 252 among them) through conv2d_nhwc."""
    cv = _single(case[0], dtype)
    with _algo(conv_algo):
        y = cv.run()
    torch.cuda.synchronize()
    _check("conv2d " + conv_algo, y, cv.plain.ref["y"], [e["y"] for e in cv.plain.emus], dtype, "%s %s (%s)" % (case[0], dtype, conv_algo))


def _check_slice(family, cv, name, conv_algo, tag=""):
    dtype = cv.dtype
    off, ctot = _layout("b", cv.cout)
    y = _canary(cv.out_shape[:3] + (ctot,), dtype, _seed(name, dtype, "slice"))
    before = y.clone()
    with _algo(conv_algo):
        cv.run(out=y, out_coffset=off)
    torch.cuda.synchronize()
    what = "%s %s slice%s (%s)" % (name, dtype, tag, conv_algo)
    _outside_unchanged(y, before, off, cv.cout, what)
    _check(family, y[..., off:off + cv.cout], cv.plain.ref["y"], [e["y"] for e in cv.plain.emus], dtype, what)


@both_algos
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", PLAIN_SHAPES)
def test_conv2d_channel_slice_rounds_once(name, dtype, conv_algo):
    """The conv into channels [12, 12 + cout) of wider rows (8-byte, not 16-byte, aligned segments in float16)."""
    _check_slice("conv2d slice " + conv_algo, _single(name, dtype), name, conv_algo)


def _run_epilogues(cv, name, conv_algo):
    """(accumulate form, residual form) of the conv on a channel slice in the middle of the row: the device's slices."""
    dtype = cv.dtype
    res = cv.residual_tensor()
    off, ctot = _layout("c", cv.cout)
    shape = cv.out_shape[:3] + (ctot,)
    rfull = _canary(shape, dtype, _seed(name, dtype, "res"))
    rfull[..., off:off + cv.cout] = res.to(DEV)
    ya = rfull.clone()
    yr = _canary(shape, dtype, _seed(name, dtype, "res-out"))
    with _algo(conv_algo):
        cv.run(out=ya, out_coffset=off, accumulate=True)
        cv.run(out=yr, out_coffset=off, residual=rfull)
    torch.cuda.synchronize()
    return ya[..., off:off + cv.cout], yr[..., off:off + cv.cout]


def _check_epilogues(family, cv, name, conv_algo, tag=""):
    _, case = cv.residual()
    emus = [e["y"] for e in case.emus]
    for form, y in zip(("accumulate", "residual"), _run_epilogues(cv, name, conv_algo)):
        _check(family % form, y, case.ref["y"], emus, cv.dtype, "%s %s %s%s (%s)" % (name, cv.dtype, form, tag, conv_algo))


@both_algos
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name", EPI_SHAPES)
def test_conv2d_residual_and_accumulate_round_once(name, dtype, conv_algo):
    """y[slice] = storage(relu?(conv + b + residual[slice])): the residual enters the float32 sum, before the one rounding --
    the residual form and the accumulate form, on a channel slice in the middle of the row."""
    _check_epilogues("conv2d %s " + conv_algo, _single(name, dtype), name, conv_algo)


def _convdet_operands(shape, regime=None, quantum=0):
    """(x, w, b) of the 768 -> 72 ConvDet launch on the CPU (float16 values; x is a ReLU output), moved into `regime`."""
    n, h, w = shape
    rs = np.random.RandomState(_seed("convdet", shape))
    x = torch.from_numpy(np.maximum(rs.randn(n, h, w, 768), 0).astype(np.float32)).half().float()
    wk = torch.from_numpy((rs.randn(3, 3, 768, 72) * (2.0 / (9 * 768)) ** 0.5).astype(np.float32)).half().float()
    b = torch.from_numpy(rs.uniform(-0.5, 0.5, 72).astype(np.float32))
    if quantum:
        x = RC.on_grid(x, quantum, "fp16")
    x, ((wk, b),) = RC.move(regime, x, [(wk, b, 1)], "fp16")
    return x, wk, b


def _run_convdet(x, wk, b):
    ops = _ops()
    preds, _ = ops.convdet(x.to(DEV, torch.float16), ops.pack_conv_weights(wk.to(DEV), torch.float16), b.to(DEV), 9, 3)
    torch.cuda.synchronize()
    return preds


def _check_convdet(family, shape, regime=None):
    x, wk, b = _convdet_operands(shape, regime)
    case = RC.Case(RC.conv_program(x, wk, b, 1, "SAME", False), "fp16")
    if regime is not None:
        RC.conditions(regime, case, ["y"], x, [wk])
    _check(family, _run_convdet(x, wk, b), case.ref["y"], [e["y"] for e in case.emus], "fp16",
           "convdet %dx%dx%d" % shape + (" " + regime if regime else ""))


@pytest.mark.parametrize("shape", [(2, 7, 13), (1, 24, 78)], ids=["2x7x13", "1x24x78"])
def test_convdet_launch_rounds_once(shape):
    """sqdet_convdet_fwd (the 768 -> 72 ConvDet launch with the score epilogue; float16): its preds.  The 512 -> 252 head and
    the other ConvDet shapes run through conv2d_nhwc: CONV_CASES rows of test_conv2d_rounds_once."""
    _check_convdet("convdet launch", shape)


def _pool2_operands(pair, dtype, regime=None, quantum=0):
    cin, cout = pair
    rs = np.random.RandomState(_seed("pool2", pair))
    x = _rnd(torch.from_numpy(rs.randn(2, 9, 17, cin).astype(np.float32)), dtype)
    wk = _rnd(torch.from_numpy((rs.randn(3, 3, cin, cout) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)), dtype)
    b = torch.from_numpy(rs.uniform(-0.5, 0.5, cout).astype(np.float32))
    if quantum:
        x = RC.on_grid(x, quantum, dtype)
    x, ((wk, b),) = RC.move(regime, x, [(wk, b, 1)], dtype)
    return x, wk, b


def _run_pool2(x, wk, b, dtype):
    ops = _ops()
    assert ops.conv2d_maxpool2_supported(x.shape[0], x.shape[1], x.shape[2], wk.shape[2], wk.shape[3], _TDT[dtype])
    y = ops.conv2d_maxpool2_nhwc(x.to(DEV, _TDT[dtype]), ops.pack_conv_weights(wk.to(DEV), _TDT[dtype]), b.to(DEV))
    torch.cuda.synchronize()
    return y


def _check_pool2(family, pair, dtype, regime=None):
    x, wk, b = _pool2_operands(pair, dtype, regime)
    case = RC.Case(RC.conv_pool_program(x, wk, b, 1, "SAME", True, (2, 2, "SAME")), dtype)
    if regime is not None:
        RC.conditions(regime, case, ["y"], x, [wk])
    _check(family, _run_pool2(x, wk, b, dtype), case.ref["y"], [e["y"] for e in case.emus], dtype,
           "conv_maxpool2 %d-%d %s" % (pair[0], pair[1], dtype) + (" " + regime if regime else ""))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_conv_maxpool2_rounds_once(pair, dtype):
    """The fused 3x3 conv + 2x2 / s2 SAME max-pool of the VGG16 pairs: the conv is rounded once, the pool is exact."""
    _check_pool2("conv + maxpool2", pair, dtype)


# ------------------------------------------------------------------------------------------------------------ fused launches
FIRE_MAPS = [(3, 3), (1, 18)]          # of tests/fused_launch_cases.py TINY_MAPS
FUSED = [
    (Spec("fire", "fp16", 64, 16, 64), {}), (Spec("fire", "fp32", 64, 16, 64), {}), (Spec("fire", "fp16", 128, 32, 128), {}),
    (Spec("fire", "fp16", 64, 16, 64), {"dbg": 8}), (Spec("fire", "fp16", 256, 48, 192), {}),
    (Spec("fire_keep", "fp16", 64, 16, 64), {}), (Spec("fire_keep", "fp32", 128, 32, 128), {}), (Spec("fire_keep", "fp16", 256, 48, 192), {}),
    (Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), {}), (Spec("fire_maxpool", "fp32", 128, 16, 64, pool=True), {}),
    (Spec("fire_maxpool", "fp16", 256, 32, 128, pool=True), {}),
    (Spec("fire_expand", "fp16", 0, 16, 64), {}), (Spec("fire_expand", "fp16", 0, 32, 128), {}), (Spec("fire_expand", "fp32", 0, 16, 64), {}),
    (Spec("fire_expand", "fp16", 0, 16, 64, pool=True), {}), (Spec("fire_expand", "fp16", 0, 32, 128, pool=True), {}),
    (Spec("fire_expand", "fp16", 0, 192, 128), {}),
    (Spec("fire_sqnext", "fp16", 64, 16, 64, 16), {}), (Spec("fire_sqnext", "fp16", 128, 32, 128, 32), {}),
    (Spec("fire_expsqnext", s=16, e=64, s2=16), {}), (Spec("fire_expsqnext", s=16, e=64, s2=32, pool=True), {}),
    (Spec("fire_expsqnext", s=32, e=128, s2=32), {}), (Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True), {}),
    (Spec("fire_expsqnext", s=16, e=64, s2=16), {"dbg": 70}), (Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True), {"dbg": 70}),
    # the chain's five squeeze-depth forms (one chunk: 16, 32; the ring: 48, 64, 96), with the next squeeze and with y, expand
    # only, and the persistent weights-resident kernel ("dbg" 31)
    (Spec("chain", "fp16", 0, 16, 64, 16), {}), (Spec("chain", "fp16", 0, 16, 64, 16, want_y=True), {}),
    (Spec("chain", "fp16", 0, 32, 128, 32), {}), (Spec("chain", "fp16", 0, 32, 128, 32, want_y=True), {}),
    (Spec("chain", "fp16", 0, 48, 192, 48), {}), (Spec("chain", "fp16", 0, 48, 192, 48, want_y=True), {}),
    (Spec("chain", "fp16", 0, 64, 256, 64), {}), (Spec("chain", "fp16", 0, 64, 256, 64, want_y=True), {}),
    (Spec("chain", "fp16", 0, 96, 384, 96), {}), (Spec("chain", "fp16", 0, 96, 384, 96, want_y=True), {}),
    (Spec("chain", "fp16", 0, 16, 64, 0), {}), (Spec("chain", "fp16", 0, 48, 192, 0), {}), (Spec("chain", "fp16", 0, 96, 384, 0), {}),
    (Spec("chain", "fp16", 0, 16, 64, 16), {"dbg": 31}), (Spec("chain", "fp16", 0, 32, 128, 32), {"dbg": 31}),
    (Spec("chain", "fp16", 0, 16, 64, 48), {"dbg": 31}),
]
# the stems on the small maps of tests/test_gpu_fused_edges.py (the persistent kernel needs W >= 236, the phase kernel W >= 524)
STEMS = [
    (Spec("stem"), (21, 250)), (Spec("stem"), (21, 530)), (Spec("stem", "fp32"), (21, 250)),
    (Spec("stem", cpad="VALID", ppad="SAME"), (21, 250)), (Spec("stem", "fp32", cpad="VALID", ppad="SAME"), (21, 250)),
    (Spec("stem", k=7, cout=96, cpad="VALID", ppad="VALID"), (45, 250)), (Spec("stem", k=7, cout=64, cpad="SAME", ppad="VALID"), (45, 250)),
    (Spec("stem", "fp32", k=7, cout=96, cpad="VALID", ppad="VALID"), (45, 250)),
    (Spec("stem_sq", s2=16), (21, 250)), (Spec("stem_sq", s2=16), (21, 530)),
]


def _fused_id(p):
    return p[0].id + "".join("-%s%d" % kv for kv in sorted(p[1].items()))


def _fused_input(spec, n, h, w):
    """Zero-mean input (a squeeze tensor for the forms that start from one): about half of every conv's outputs pass the ReLU."""
    rs = np.random.RandomState(_seed("rounding-x", spec.id, n, h, w))
    x = rs.uniform(-2, 2, spec.in_shape(n, h, w)) if spec.entry.startswith("stem") else rs.randn(*spec.in_shape(n, h, w))
    return torch.from_numpy(x.astype(np.float32)).to(FC.TDT[spec.dtype])


def _program(spec, x, wt):
    if spec.entry.startswith("stem"):
        return RC.conv_pool_program(x, wt["w"], wt["b"], 2, spec.cpad, True, (3, 2, spec.ppad), wt.get("wn"), wt.get("bn"))
    return RC.fire_program(x, wt, pool=spec.pool)


def _moved_operands(spec, n, h, w, regime=None, quantum=0):
    """(input in the storage type, weight dict) of the launch on the CPU, moved into `regime`; quantum as in _Single."""
    x, wt = _fused_input(spec, n, h, w), _weights(spec)
    if quantum:
        x = RC.on_grid(x.float(), quantum, spec.dtype).to(x.dtype)
    if regime is None:
        return x, wt
    x2, wt = RC.move_weights(regime, x.float(), wt, spec.dtype)
    return x2.to(x.dtype), wt


@functools.lru_cache(maxsize=8)
def _moved_op(spec, regime):
    """The Op of spec with its weights moved into `regime` (the weights do not depend on the input)."""
    return Op(spec, wt=RC.move_weights(regime, torch.zeros(spec.in_shape(1, 1, 1)), _weights(spec), spec.dtype)[1])


def _moved(spec, n, h, w, regime=None, quantum=0):
    """(the Op of spec with its weights moved into `regime`, the input moved likewise, in the storage type on the CPU)."""
    x, _ = _moved_operands(spec, n, h, w, regime, quantum)
    return (_op(spec) if regime is None else _moved_op(spec, regime)), x


def _launch(op, x, opts):
    """The tensors the launch writes, on the CPU, in the order it writes them."""
    with _options(**opts):
        bufs = op.run(x.to(DEV).contiguous())
    torch.cuda.synchronize()
    return OrderedDict((nm, t.cpu()) for nm, t in op.outputs(bufs).items())


def _check_launch(family, spec, opts, n, h, w, regime=None, cases=None):
    """Runs the launch and checks every tensor it writes.  An intermediate the launch writes out is checked on its own, and the
    stages behind it against the reference computed FROM THE DEVICE'S intermediate (no carried term); a hidden intermediate
    carries its interval forward.  regime: the operands are moved into it, and RC.conditions() is asserted of the reference
    before the launch runs; cases: a dict that keeps the launch's Case between calls."""
    op, x = _moved(spec, n, h, w, regime)
    dtype, what = spec.dtype, "%s %dx%dx%d%s" % (_fused_id((spec, opts)), n, h, w, " " + regime if regime else "")
    key = (spec.id, n, h, w, regime)
    if cases is None or key not in cases:
        case = RC.Case(_program(spec, x.float(), op.wt), dtype)
        if cases is not None:
            cases[key] = case
    else:
        case = cases[key]
    if regime is not None:
        written = [nm for nm, (_, role) in spec.buffers(n, h, w).items() if role == "out"]
        RC.conditions(regime, case, written, x.float(), [op.wt[kw] for kw, _, _ in RC.conv_keys(op.wt)])
    outs = _launch(op, x, opts)
    first = next(iter(outs))
    _check(family, outs[first], case.ref[first], [e[first] for e in case.emus], dtype, what + " " + first)
    if len(outs) == 2:
        # fire_keep writes sq then y; the chain with want_y writes y then sq_out: the later tensor from the device's earlier one
        nm = [k for k in outs if k != first][0]
        if first == "sq":
            behind = {k: v for k, v in op.wt.items() if k not in ("ws", "bs")}
            stage = RC.Case(RC.fire_program(outs["sq"].float(), behind, pool=spec.pool), dtype)
        else:
            stage = RC.Case(RC.conv_program(outs["y"].float(), op.wt["wn"], op.wt["bn"]), dtype)
        _check(family, outs[nm], stage.ref["y"], [e["y"] for e in stage.emus], dtype, "%s %s from the device's %s" % (what, nm, first))


@pytest.mark.parametrize("spec,opts", FUSED, ids=[_fused_id(p) for p in FUSED])
def test_fused_fire_launch_rounds_once_per_conv(spec, opts):
    per_pixel = min(shape[3] for shape, role in spec.buffers(1, 4, 4).values() if role == "out")
    for (h, w) in FIRE_MAPS:
        ho, wo = spec.out_hw(h, w)
        _check_launch("%s%s" % (spec.entry, "".join(" %s %d" % kv for kv in sorted(opts.items()))), spec, opts,
                      _grown(1, ho * wo * per_pixel, True), h, w)


@pytest.mark.parametrize("spec,hw", STEMS, ids=["%s-%dx%d" % (s.id, hw[0], hw[1]) for s, hw in STEMS])
def test_fused_stem_launch_rounds_once_per_conv(spec, hw):
    _check_launch(spec.entry + " k%d" % spec.k, spec, {}, 2, hw[0], hw[1])


# ------------------------------------------------------------------------------------------------------------------ backward
class _Dgrad:
    """One DGRAD_CASES row: W, dY (with cout + 24 channels, the conv's at [kg, kg + cout)), the prior dx and relu_of, on the CPU
    in the storage type.  exps = (dY, W, prior) powers of two the operands are scaled by; quantum as in _Single."""

    def __init__(self, case, dtype, exps=(0, 0, 0), quantum=0):
        name, N, H, W, cin, cout, k = case
        self.name, self.dtype, self.cout, self.kg = name, dtype, cout, 8 if dtype == "fp16" else 4
        rs = np.random.RandomState(_seed("dgrad", name))
        wk = _rnd(torch.from_numpy((rs.randn(k, k, cin, cout) / (k * k * cout) ** 0.5).astype(np.float32)), dtype)
        canary = lambda shape, *seed: torch.randn(shape, generator=torch.Generator().manual_seed(_seed(*seed))).to(_TDT[dtype])
        dy = canary((N, H, W, cout + 24), name, dtype, "dy").float()           # the values of _canary, left on the CPU
        self.relu_of = canary((N, H, W, cin), name, dtype, "relu_of")
        prior = canary((N, H, W, cin), name, dtype, "prior").float()
        if quantum:
            dy, prior = RC.on_grid(dy, quantum, dtype), RC.on_grid(prior, quantum, dtype)
        self.dy, self.wk, self.prior = RC.scaled(dy, exps[0], dtype), RC.scaled(wk, exps[1], dtype), RC.scaled(prior, exps[2], dtype)
        self._cases = {}

    def cases(self, orders=RC.ORDERS):
        """(the Case of the plain form on the dY slice, the Case of accumulate + relu_of), with the emulations of `orders`."""
        if orders not in self._cases:
            wb, zero = RC.flip_for_bwd_data(self.wk), torch.zeros(self.wk.shape[2])
            dys = self.dy[..., self.kg:self.kg + self.cout]
            self._cases[orders] = (
                RC.Case(RC.conv_program(dys, wb, zero, 1, "SAME", False), self.dtype, orders),
                RC.Case(RC.conv_program(dys, wb, zero, 1, "SAME", False, res=self.prior, keep=self.relu_of.float() > 0), self.dtype, orders))
        return self._cases[orders]

    def run(self, conv_algo):
        """(dx of the plain form, dx of accumulate + relu_of) on the device."""
        ops, tdt = _ops(), _TDT[self.dtype]
        pb = ops.PackedConvBwd(self.wk.to(DEV), tdt)
        dy, relu_of = self.dy.to(DEV, tdt), self.relu_of.to(DEV)
        with _algo(conv_algo):
            dx = ops.conv2d_bwd_data(dy, pb, dy_coffset=self.kg)
            dx2 = ops.conv2d_bwd_data(dy, pb, dx=self.prior.to(DEV, tdt), dy_coffset=self.kg, accumulate=True, relu_of=relu_of)
        torch.cuda.synchronize()
        return dx, dx2


@functools.lru_cache(maxsize=2)
def _dgrad(case, dtype, exps=(0, 0, 0), quantum=0):
    return _Dgrad(case, dtype, exps, quantum)


def _check_dgrad(family, dg, conv_algo, tag=""):
    plain, full = dg.cases()
    dx, dx2 = dg.run(conv_algo)
    _check(family, dx, plain.ref["y"], [e["y"] for e in plain.emus], dg.dtype, "%s %s dy slice%s (%s)" % (dg.name, dg.dtype, tag, conv_algo))
    _check(family, dx2, full.ref["y"], [e["y"] for e in full.emus], dg.dtype,
           "%s %s accumulate + relu_of%s (%s)" % (dg.name, dg.dtype, tag, conv_algo))


@both_algos
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_conv_backward_data_rounds_once(case, dtype, conv_algo):
    """dx = storage(mask?(conv(dY slice, rot180(W)^T) [+ prior dx])): plain on a dY channel slice, and accumulate + relu_of."""
    _check_dgrad("bwd_data " + conv_algo, _dgrad(case, dtype), conv_algo)


# one row of tests/test_gpu_train.py BWD_CASES per wgrad_plan (wgrad.hip) tile variant and taps-per-workgroup form:
#   16x64: taps 1 / 3 / 9; 48x64; 64x16; 64x32; 64x48; 64x80; 64x64; 32x64: taps 3 / 9, and a ragged float32-only row
WGRAD_ROWS = ["e1_16_64", "e3_16_64", "e3_16_64_9tap", "e3_48_192", "sq_96_16", "sq_128_32", "sq_256_48", "convdet_768_72",
              "e3_64_256", "e3_96_384", "e3_32_128_9tap", "ragged_20_36"]


# (float16 rows are 16-byte vectors: ragged_20_36 exists for the float32 kernels' ragged tails only)
WGRAD_PARAMS = [(n, t) for n in WGRAD_ROWS for t in ("fp32", "fp16") if not (t == "fp16" and n == "ragged_20_36")]


def _wgrad_operands(name, dtype, dy_exp=0, quantum=0):
    """(x, dY, W) of a WGRAD_CASES row on the CPU, storage-rounded; dY x 2^dy_exp, rounded again; quantum as in _Single."""
    _, N, H, W, cin, cout, k = next(c for c in WGRAD_CASES if c[0] == name)
    rs = np.random.RandomState(_seed("wgrad", name))
    x = _rnd(torch.from_numpy(rs.randn(N, H, W, cin).astype(np.float32)), dtype)
    dy = _rnd(torch.from_numpy(rs.randn(N, H, W, cout).astype(np.float32)), dtype)
    wk = torch.from_numpy(rs.randn(k, k, cin, cout).astype(np.float32))
    if quantum:
        dy = RC.on_grid(dy, quantum, dtype)
    return x, RC.scaled(dy, dy_exp, dtype), wk


def _run_wgrad(name, dtype, x, dy, wk, decay, scale):
    """(dW, dbias) of conv2d_bwd_filter, float32 on the device; WgradPlan must give the same bits."""
    ops, tdt = _ops(), _TDT[dtype]
    N, H, W, cin = x.shape
    k, cout = wk.shape[0], wk.shape[3]
    xd, dyd, wd = x.to(DEV, tdt), dy.to(DEV, tdt), wk.to(DEV)
    dw, db = ops.conv2d_bwd_filter(xd, dyd, k, cin, cout, w_for_decay=wd, weight_decay=decay, grad_scale=scale)
    dwp, dbp = torch.full_like(dw, float("nan")), torch.full_like(db, float("nan"))
    plan = ops.WgradPlan([(name, (N, H, W, cin, cout, k), dwp, dbp, wd, decay)])
    plan.partial(name, xd, dyd)
    plan.reduce(scale)
    torch.cuda.synchronize()
    assert torch.equal(dw, dwp) and torch.equal(db, dbp), name + ": WgradPlan against conv2d_bwd_filter"
    return dw, db


def _check_wgrad(family, name, dtype, dy_exp=0):
    x, dy, wk = _wgrad_operands(name, dtype, dy_exp)
    k = wk.shape[0]
    decay, scale = 1e-3, 0.25
    case = RC.WgradCase(x, dy, k, wk, decay, scale)
    dw, db = _run_wgrad(name, dtype, x, dy, wk, decay, scale)
    flat = lambda d: torch.cat([d["dw"].reshape(-1), d["db"].reshape(-1)])
    ref = RC.Val(*[flat({"dw": getattr(case.ref["dw"], f), "db": getattr(case.ref["db"], f)}) for f in RC.Val.FIELDS])
    got = flat({"dw": dw.cpu(), "db": db.cpu()})
    emus = [flat(e) for e in case.emus]
    what = "wgrad %s %s%s" % (name, dtype, " dY x 2^%d" % dy_exp if dy_exp else "")
    m = RC.measure(got, ref, emus, "fp32")
    print("%s: %s" % (what, RC.describe(m, "fp32")))
    REPORT.setdefault(family, []).append((what, "fp32", m))
    assert m["compared"] >= min(RC.MIN_COMPARED, ref.want.numel()) and m["share"] >= RC.MIN_SHARE, what
    assert m["outside"] == 0, "%s: %d elements outside the derived bound" % (what, m["outside"])
    assert m["value"] <= m["cap"], "%s: %s" % (what, RC.describe(m, "fp32"))
    return got


@pytest.mark.parametrize("name,dtype", WGRAD_PARAMS, ids=["%s-%s" % p for p in WGRAD_PARAMS])
def test_conv_backward_filter_accumulates_in_float32(name, dtype):
    """dW = grad_scale * sum x (x) dY + weight_decay * W and dbias, float32, from conv2d_bwd_filter and from WgradPlan (bitwise
    the same).  The statistic is r = max |got - exact| / magnitude over dW and dbias together.  A dW has k * k * cin * cout
    elements whatever N is: where that is fewer than 2000 (e1_16_64: 1024, sq_96_16: 1536), every element is compared."""
    _check_wgrad("bwd_filter", name, dtype)


# -------------------------------------------------------------------------------------------------------------------- report
def test_zz_report_rounding_figures():
    """Per kernel family, the case nearest its cap: device value, largest emulation value, cap (the table of DESIGN.md)."""
    print("\n%-34s %5s %6s  %-22s %-22s %-12s %s" % ("family", "cases", "dtype", "device", "largest emulation", "cap", "worst case"))
    for family, rows in REPORT.items():
        for dtype in ("fp16", "fp32"):
            sel = [r for r in rows if r[1] == dtype]
            if not sel:
                continue
            what, _, m = max(sel, key=lambda r: r[2]["value"] / r[2]["cap"])
            if dtype == "fp16":
                f = lambda v: "%d (%.3f %%)" % (v, 100.0 * v / m["compared"])
            else:
                f = lambda v: "%.3g" % v
            print("%-34s %5d %6s  %-22s %-22s %-12s %s" % (family, len(sel), dtype, f(m["value"]), f(max(m["emulated"])), f(m["cap"]), what))
            assert all(r[2]["outside"] == 0 and r[2]["value"] <= r[2]["cap"] for r in sel)
