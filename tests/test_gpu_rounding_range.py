"""GPU tests of the rounding contract (tests/rounding_contract.py) across the float16 range: the checks, the reference, the
emulations and the caps of tests/test_gpu_rounding.py, with the operands moved to where that file's randn / He-scaled ones never
are.  No tolerance of this file's own.

REGIMES (RC.move; all factors powers of two, input and weights storage-rounded again, biases float32):
  sub   input and biases x 2^-16: subnormal inputs, hidden intermediates and outputs (mixed-precision gradients without a loss
        scale);
  subw  weights x 2^-12 under an input x 2^12: subnormal weights (float16 storage);
  top   the last stage's weights x 2^7 and bias x 2^15 under x 2^8 before it: the last stored tensor overflows to +-inf -- what
        the overflow flag of the optimizer's norm kernel waits for -- and no conv reads a non-finite value;
  big   (backward filter) dY x 2^13, a loss scale of 8192.
RC.conditions() asserts from the reference alone, before any device value is looked at, that a case is where its regime says.
A kernel that flushes float16 subnormals at its input, in its weights or at its store, or that saturates at 65504, fails here
(tests/test_rounding_contract_host.py plants each) and passes every other test of the suite.

One CONV_CASES row per kernel conv2d_nhwc dispatches to (float16; the comments of CONV_CASES and PLAIN_SHAPES name them):
  fire6_expand3x3    conv3x3_tile, one K stage (also conv_algo = generic: conv_direct)
  e3_k384_n256       conv3x3_tile, K walked in 4-chunk LDS stages
  c1_k64_n48         conv1x1_stream
  fire11_squeeze     the reducing deep-K 1x1 (768 -> 96)
  g1_k384_n256       gemm1x1, the workgroup GEMM tile
  k1_k256_n32        conv1x1k, the streaming deep-K 1x1 of large maps
  conv12_convdet     the ConvDet head, no ReLU: -inf appears (also generic)
  stride2_3x3_valid  conv_direct / conv_gather
and one FUSED / STEMS entry per fused kernel and form, the ConvDet launch, one conv + max-pool pair, two DGRAD_CASES rows and
five WGRAD_CASES rows.

EXACT SCALING.  The same launch on unit operands and on input and biases x 2^k must give 2^k times the same bits: the kernel
and its summation order are the same, and a power of two commutes with every rounding that neither underflows nor overflows.
float16: k = -6 and +5, on the elements that are finite and normal or zero in both runs (at most 1 % may be left out), the
unit input taken on the grid that x 2^-6 keeps (RC.on_grid) so that the operands themselves scale exactly; float32: k = -40 and
+40, every element.  Where a launch keeps an intermediate tensor to itself, an element of it that is subnormal in one run is
rounded differently in the two, and everything computed from it need not scale: RC.Fragile marks those from the reference's
interval and they are not compared; every other element is, bit for bit, in every case.  At most 1 % of a hidden tensor may be
marked itself, and the reference must leave at least 25 % of each output to compare -- 15 % under x 2^-6 for the pooled
fire_expsqnext 32/128/48 alone, of which 84.2 % is computed from one of 256 hidden channels' subnormal elements
(MIN_CLEAR_AT_MINUS_6 gives the shares masked elsewhere: up to 74.6 %).  Every run returns the shapes, types and options of its
operands, asserted equal between the runs: the launcher has nothing to choose another kernel by.

One launch leaves the letter of "top": stem_sq takes its last stage one power of two lower (RC.TOP14, see STEM_PARAMS).
"""
import pytest
import torch

from tests import rounding_contract as RC
from tests.fused_launch_cases import Spec
from tests.test_gpu_rounding import (DGRAD_CASES, FUSED, PAIRS, REPORT, STEMS, WGRAD_CASES, _algo, _check, _check_convdet, _check_dgrad,
                                     _check_epilogues, _check_launch, _check_pool2, _check_slice, _check_wgrad, _convdet_operands, _dgrad,
                                     _fused_id, _grown, _launch, _moved, _pool2_operands, _program, _run_convdet, _run_epilogues, _run_pool2,
                                     _run_wgrad, _single, _wgrad_operands)

pytestmark = pytest.mark.gpu

# (CONV_CASES row, whether it also runs under conv_algo = generic)
SINGLES = [("fire6_expand3x3", True), ("e3_k384_n256", False), ("c1_k64_n48", False), ("fire11_squeeze", False), ("g1_k384_n256", False),
           ("k1_k256_n32", False), ("conv12_convdet", True), ("stride2_3x3_valid", False)]
SINGLE_ALGOS = [(n, a) for n, both in SINGLES for a in (("auto", "generic") if both else ("auto",))]
SINGLE_PARAMS = [(n, r, a) for r in RC.REGIMES for n, a in SINGLE_ALGOS]
EPILOGUE_ROWS = ["fire6_expand3x3", "c1_k64_n48"]      # one 3x3 and one 1x1 row
EPILOGUE_REGIMES = ("sub", "top")
MAP = (3, 3)


def _entries(table, wanted):
    """The entries of FUSED / STEMS (tests/test_gpu_rounding.py) that `wanted` names: none is this file's own."""
    ident = (lambda p: _fused_id(p)) if table is FUSED else (lambda p: (p[0].id, p[1]))
    have = {ident(p): p for p in table}
    return [have[ident(p)] for p in wanted]


RANGE_FUSED = _entries(FUSED, [
    (Spec("fire", "fp16", 64, 16, 64), {}), (Spec("fire", "fp16", 256, 48, 192), {}), (Spec("fire_keep", "fp16", 64, 16, 64), {}),
    (Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), {}), (Spec("fire_maxpool", "fp16", 256, 32, 128, pool=True), {}),
    (Spec("fire_expand", "fp16", 0, 16, 64), {}), (Spec("fire_expand", "fp16", 0, 16, 64, pool=True), {}),
    (Spec("fire_expand", "fp16", 0, 192, 128), {}),                                 # the PAIR tile
    (Spec("fire_sqnext", "fp16", 64, 16, 64, 16), {}),
    (Spec("fire_expsqnext", s=16, e=64, s2=16), {}), (Spec("fire_expsqnext", s=16, e=64, s2=16), {"dbg": 70}),
    (Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True), {}),
    (Spec("chain", "fp16", 0, 16, 64, 16), {}), (Spec("chain", "fp16", 0, 16, 64, 16, want_y=True), {}),
    (Spec("chain", "fp16", 0, 48, 192, 48), {}), (Spec("chain", "fp16", 0, 48, 192, 48, want_y=True), {}),
    (Spec("chain", "fp16", 0, 96, 384, 96), {}), (Spec("chain", "fp16", 0, 96, 384, 96, want_y=True), {}),
    (Spec("chain", "fp16", 0, 16, 64, 0), {}), (Spec("chain", "fp16", 0, 16, 64, 16), {"dbg": 31}),
])
RANGE_STEMS = _entries(STEMS, [(Spec("stem"), (21, 250)), (Spec("stem"), (21, 530)),
                               (Spec("stem", k=7, cout=96, cpad="VALID", ppad="VALID"), (45, 250)), (Spec("stem_sq", s2=16), (21, 250))])
# the float32 forms of the same kernels, for the exact-scaling tests
SCALING_FUSED = RANGE_FUSED + _entries(FUSED, [
    (Spec("fire", "fp32", 64, 16, 64), {}), (Spec("fire_keep", "fp32", 128, 32, 128), {}),
    (Spec("fire_maxpool", "fp32", 128, 16, 64, pool=True), {}), (Spec("fire_expand", "fp32", 0, 16, 64), {})])
SCALING_STEMS = RANGE_STEMS + _entries(STEMS, [(Spec("stem", "fp32"), (21, 250)),
                                               (Spec("stem", "fp32", k=7, cout=96, cpad="VALID", ppad="VALID"), (45, 250))])


def _regimes_of(spec):
    """sub and top everywhere; subw where the float16 launch packs its weights itself (the chain's stream, the stems)."""
    return RC.REGIMES if spec.entry in ("chain", "stem", "stem_sq") else ("sub", "top")


FUSED_PARAMS = [(s, o, r) for s, o in RANGE_FUSED for r in _regimes_of(s)]
# stem_sq runs "top" one power of two lower in its last stage (RC.TOP14: squeeze weights x 2^6, bias x 2^14).  56 % of its squeeze
# outputs are zero, so under the factors of "top" 21.7 % of the last tensor are inf and only 22.0 % finite and non-zero, short of
# the 25 % RC.conditions() asks for (at both STEMS sizes, whose weights are the same); under TOP14 11.0 % are inf and 32.6 % finite
# and non-zero, and the conditions hold as they stand
STEM_PARAMS = [(s, hw, RC.TOP14 if (s.entry, r) == ("stem_sq", "top") else r) for s, hw in RANGE_STEMS for r in _regimes_of(s)]
POOL2_PAIR = PAIRS[0]
CONVDET_SHAPE = (2, 7, 13)
DGRAD_ROWS = [next(c for c in DGRAD_CASES if c[0] == n) for n in ("1x1_cin16_cout64", "3x3_cin72_cout128")]
# (dY, W, prior dx) exponents
DGRAD_REGIMES = {"sub": (RC.SUB, 0, RC.SUB), "top": (RC.TOP_IN, RC.TOP_W, RC.TOP_RES)}
WGRAD_RANGE_ROWS = ["e1_16_64", "e3_16_64", "e3_16_64_9tap", "convdet_768_72", "e3_64_256"]
WGRAD_REGIMES = {"sub": RC.SUB, "big": RC.BIG}


def fused_n(spec, h, w):
    """The batch of test_fused_fire_launch_rounds_once_per_conv: N grown until about 2000 outputs can be compared."""
    per_pixel = min(shape[3] for shape, role in spec.buffers(1, 4, 4).values() if role == "out")
    ho, wo = spec.out_hw(h, w)
    return _grown(1, ho * wo * per_pixel, True)


def _family(spec, opts=None):
    return "%s%s" % (spec.entry, "".join(" %s %d" % kv for kv in sorted((opts or {}).items())))


# ------------------------------------------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize("name,regime,conv_algo", SINGLE_PARAMS, ids=["%s-%s-%s" % p for p in SINGLE_PARAMS])
def test_conv2d_rounds_once_across_the_range(name, regime, conv_algo):
    cv = _single(name, "fp16", regime)
    RC.conditions(regime, cv.plain, ["y"], cv.x, [cv.w])
    with _algo(conv_algo):
        y = cv.run()
    torch.cuda.synchronize()
    _check("conv2d %s, %s" % (conv_algo, regime), y, cv.plain.ref["y"], [e["y"] for e in cv.plain.emus], "fp16",
           "%s fp16 %s (%s)" % (name, regime, conv_algo))


@pytest.mark.parametrize("regime", EPILOGUE_REGIMES)
@pytest.mark.parametrize("name", EPILOGUE_ROWS)
def test_conv2d_epilogues_round_once_across_the_range(name, regime):
    """The channel-slice store, and the residual and accumulate epilogues with the residual scaled as the output is."""
    cv = _single(name, "fp16", regime)
    RC.conditions(regime, cv.plain, ["y"], cv.x, [cv.w])
    RC.conditions(regime, cv.residual()[1], ["y"], cv.x, [cv.w])
    _check_slice("conv2d slice, " + regime, cv, name, "auto", " " + regime)
    _check_epilogues("conv2d %s, " + regime, cv, name, "auto", " " + regime)


_CASES = {}        # the reference and emulations of a fused launch, kept per (form, shape, regime)


@pytest.mark.parametrize("spec,opts,regime", FUSED_PARAMS, ids=["%s-%s" % (_fused_id(p[:2]), p[2]) for p in FUSED_PARAMS])
def test_fused_fire_launch_rounds_once_across_the_range(spec, opts, regime):
    _check_launch("%s, %s" % (_family(spec, opts), regime), spec, opts, fused_n(spec, *MAP), MAP[0], MAP[1], regime, _CASES)


@pytest.mark.parametrize("spec,hw,regime", STEM_PARAMS, ids=["%s-%dx%d-%s" % (s.id, hw[0], hw[1], r) for s, hw, r in STEM_PARAMS])
def test_fused_stem_launch_rounds_once_across_the_range(spec, hw, regime):
    _check_launch("%s k%d, %s" % (spec.entry, spec.k, regime), spec, {}, 2, hw[0], hw[1], regime)


@pytest.mark.parametrize("regime", ("sub", "top"))
def test_convdet_launch_rounds_once_across_the_range(regime):
    _check_convdet("convdet launch, " + regime, CONVDET_SHAPE, regime)


@pytest.mark.parametrize("regime", ("sub", "top"))
def test_conv_maxpool2_rounds_once_across_the_range(regime):
    _check_pool2("conv + maxpool2, " + regime, POOL2_PAIR, "fp16", regime)


def dgrad_conditions(dg, regime, orders=RC.ORDERS):
    for case in dg.cases(orders):
        RC.conditions(regime, case, ["y"])
    if regime == "sub":
        share = float(RC.subnormal16(dg.dy).double().mean())
        assert share >= RC.MIN_SUBNORMAL, "only %.1f %% of dY is subnormal" % (100 * share)


@pytest.mark.parametrize("conv_algo", ["auto", "generic"])
@pytest.mark.parametrize("regime", sorted(DGRAD_REGIMES))
@pytest.mark.parametrize("case", DGRAD_ROWS, ids=[c[0] for c in DGRAD_ROWS])
def test_conv_backward_data_rounds_once_across_the_range(case, regime, conv_algo):
    """sub: dY and the prior dx x 2^-16; top: dY x 2^8, W x 2^7, the prior x 2^13 (RC.residual_exponent) -- plain, and accumulate +
    relu_of."""
    dg = _dgrad(case, "fp16", DGRAD_REGIMES[regime])
    dgrad_conditions(dg, regime)
    _check_dgrad("bwd_data %s, %s" % (conv_algo, regime), dg, conv_algo, " " + regime)


@pytest.mark.parametrize("regime", sorted(WGRAD_REGIMES))
@pytest.mark.parametrize("name", WGRAD_RANGE_ROWS)
def test_conv_backward_filter_across_the_range(name, regime):
    """float16 x and dY, float32 dW and dbias, r = max |got - exact| / magnitude as tests/test_gpu_rounding.py takes it: dY x 2^-16
    (what a float16 gradient is without a loss scale: more than half of dY subnormal) and dY x 2^13.  WgradPlan stays bitwise
    conv2d_bwd_filter (asserted by the helper); no inf in dW."""
    _, dy, _ = _wgrad_operands(name, "fp16", WGRAD_REGIMES[regime])
    assert bool(torch.isfinite(dy).all())
    if regime == "sub":
        share = float(RC.subnormal16(dy).double().mean())
        assert share > RC.MIN_SUBNORMAL, "only %.1f %% of dY is subnormal and non-zero" % (100 * share)
    got = _check_wgrad("bwd_filter, " + regime, name, "fp16", WGRAD_REGIMES[regime])
    assert bool(torch.isfinite(got).all()), "a non-finite value in dW / dbias"


# ------------------------------------------------------------------------------------------------------------ exact scaling
KS = {"fp16": (-6, 5), "fp32": (-40, 40)}
QUANTUM = {"fp16": 6, "fp32": 0}
MAX_LEFT_OUT = 0.01


# The share of an output that must stay clear of RC.Fragile's upstream mask, asserted from the reference alone.  Under x 2^5 it
# is RC.MIN_SHARE everywhere (next to nothing is subnormal in either run).  Under x 2^-6 about one hidden element in a thousand
# may be subnormal, and an output computed from C hidden channels is masked with probability near C / 1000: the reference masks
# 84.2 % of the pooled fire_expsqnext 32/128/48 (256 hidden channels under a 3x3 pool), 73.0 / 74.6 % of chain s96 (768
# channels; without / with y), 42.9 - 44.4 % of chain s48, 38.8 % of stem_sq, 33.3 % of fire_maxpool 256/32/128, less elsewhere.
# Only the first leaves less than RC.MIN_SHARE, and it alone gets a minimum of its own; what is left is compared bit for bit.
MIN_CLEAR_AT_MINUS_6 = {Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True).id: 0.15}


def _sig(*tensors, **options):
    """What a launcher can choose a kernel by: the shape and type of every operand, and the options."""
    return tuple((tuple(t.shape), t.dtype) for t in tensors) + tuple(sorted(options.items()))


def _assert_scales(what, dtype, run, program=None, min_clear=RC.MIN_SHARE):
    """run(k, q) -> ({name: device tensor}, _sig of the operands) of the launch on input and biases x 2^k (unit input on the grid of
    2^-q); program: the launch as a program of its UNIT operands where it has more than one stage; min_clear: the share of an
    output RC.Fragile must leave unmasked under x 2^-6."""
    unit, sig = run(0, QUANTUM[dtype])
    for k in KS[dtype]:
        moved, sig_k = run(k, QUANTUM[dtype])
        assert sig_k == sig, "%s: the operands of the x 2^%d run differ in shape, type or options: another kernel may serve them" % (what, k)
        fragile = program(RC.Fragile(k)) if (program is not None and dtype == "fp16") else None
        assert list(moved) == list(unit)
        for nm in unit:
            u, m = unit[nm].detach().cpu(), moved[nm].detach().cpu()
            assert u.shape == m.shape and u.dtype == m.dtype
            upstream = None if fragile is None else fragile[nm][1]
            if upstream is not None:
                clear = 1.0 - float(upstream.double().mean())
                need = min_clear if k < 0 else RC.MIN_SHARE
                assert clear >= need, "%s %s x 2^%d: the reference leaves only %.1f %% to compare" % (what, nm, k, 100 * clear)
            bad, left, compared = RC.scales_exactly(u, m, k, upstream)
            print("%s %s x 2^%d: %d of %d differ; %.3f %% left out, %.1f %% compared" % (what, nm, k, bad, u.numel(), 100 * left, 100 * compared))
            assert left <= MAX_LEFT_OUT, "%s %s x 2^%d: %.2f %% subnormal or not finite" % (what, nm, k, 100 * left)
            assert bad == 0, "%s %s x 2^%d: %d elements are not 2^%d times the unit run's" % (what, nm, k, bad, k)
        if fragile is not None:
            for nm, (_, _, own) in fragile.items():
                if nm in unit:
                    continue      # a tensor the launch writes: `left`, from what the device stored
                share = float(own.double().mean())
                assert share <= MAX_LEFT_OUT, "%s: %.2f %% of %s may round differently under x 2^%d" % (what, 100 * share, nm, k)


SCALING_SINGLES = [(n, t, a) for t in ("fp16", "fp32") for n, a in SINGLE_ALGOS]


@pytest.mark.parametrize("name,dtype,conv_algo", SCALING_SINGLES, ids=["%s-%s-%s" % p for p in SCALING_SINGLES])
def test_conv2d_scales_exactly(name, dtype, conv_algo):
    def run(k, q):
        cv = _single(name, dtype, k, q)
        with _algo(conv_algo):
            y = cv.run()
        torch.cuda.synchronize()
        return {"y": y}, _sig(cv.x, cv.w, cv.b, stride=cv.stride, pad=cv.pad, relu=cv.relu, conv_algo=conv_algo)
    _assert_scales("%s %s (%s)" % (name, dtype, conv_algo), dtype, run)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name", EPILOGUE_ROWS)
def test_conv2d_epilogues_scale_exactly(name, dtype):
    def run(k, q):
        cv = _single(name, dtype, k, q)
        ya, yr = _run_epilogues(cv, name, "auto")
        return {"accumulate": ya, "residual": yr}, _sig(cv.x, cv.w, cv.b, cv.residual_tensor(), stride=cv.stride, pad=cv.pad, relu=cv.relu)
    _assert_scales("%s %s epilogues" % (name, dtype), dtype, run)


def _fused_scales(spec, opts, n, h, w):
    def run(k, q):
        op, x = _moved(spec, n, h, w, k, q)
        return _launch(op, x, opts), _sig(x, *[op.wt[key] for key in sorted(op.wt)], entry=spec.id, **opts)
    op, x = _moved(spec, n, h, w, None, QUANTUM[spec.dtype])
    stages = max(st for _, _, st in RC.conv_keys(op.wt))
    _assert_scales("%s %dx%dx%d" % (_fused_id((spec, opts)), n, h, w), spec.dtype, run, _program(spec, x.float(), op.wt) if stages > 1 else None,
                   MIN_CLEAR_AT_MINUS_6.get(spec.id, RC.MIN_SHARE))


@pytest.mark.parametrize("spec,opts", SCALING_FUSED, ids=[_fused_id(p) for p in SCALING_FUSED])
def test_fused_fire_launch_scales_exactly(spec, opts):
    _fused_scales(spec, opts, fused_n(spec, *MAP), MAP[0], MAP[1])


@pytest.mark.parametrize("spec,hw", SCALING_STEMS, ids=["%s-%dx%d" % (s.id, hw[0], hw[1]) for s, hw in SCALING_STEMS])
def test_fused_stem_launch_scales_exactly(spec, hw):
    _fused_scales(spec, {}, 2, hw[0], hw[1])


def test_convdet_launch_scales_exactly():
    def run(k, q):
        operands = _convdet_operands(CONVDET_SHAPE, k, q)
        return {"preds": _run_convdet(*operands)}, _sig(*operands)
    _assert_scales("convdet %dx%dx%d" % CONVDET_SHAPE, "fp16", run)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_conv_maxpool2_scales_exactly(dtype):
    def run(k, q):
        operands = _pool2_operands(POOL2_PAIR, dtype, k, q)
        return {"y": _run_pool2(*operands, dtype)}, _sig(*operands)
    _assert_scales("conv_maxpool2 %d-%d %s" % (POOL2_PAIR + (dtype,)), dtype, run)


@pytest.mark.parametrize("conv_algo", ["auto", "generic"])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("case", DGRAD_ROWS, ids=[c[0] for c in DGRAD_ROWS])
def test_conv_backward_data_scales_exactly(case, dtype, conv_algo):
    """dY and the prior dx x 2^k."""
    def run(k, q):
        dg = _dgrad(case, dtype, (k, 0, k), q)
        dx, dx2 = dg.run(conv_algo)
        return {"dx": dx, "accumulate + relu_of": dx2}, _sig(dg.dy, dg.wk, dg.prior, dg.relu_of, kg=dg.kg, conv_algo=conv_algo)
    _assert_scales("%s %s (%s)" % (case[0], dtype, conv_algo), dtype, run)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name", WGRAD_RANGE_ROWS)
def test_conv_backward_filter_scales_exactly(name, dtype):
    """dY x 2^k: dW and dbias (float32 whatever the storage type, so every element is compared) x 2^k; no weight decay, which
    does not scale with dY."""
    def run(k, q):
        x, dy, wk = _wgrad_operands(name, dtype, k, q)
        dw, db = _run_wgrad(name, dtype, x, dy, wk, 0.0, 0.25)
        return {"dw": dw, "db": db}, _sig(x, dy, wk)
    _assert_scales("wgrad %s %s" % (name, dtype), "fp32" if dtype == "fp32" else "fp16", run)


# -------------------------------------------------------------------------------------------------------------------- report
def test_zz_report_range_figures():
    """Per kernel family and regime, the case nearest its cap: device value, largest emulation value, cap (the table of DESIGN.md)."""
    print("\n%-44s %5s  %-22s %-22s %-12s %s" % ("family, regime", "cases", "device", "largest emulation", "cap", "worst case"))
    for family, rows in REPORT.items():
        if ", " not in family:
            continue          # a family of tests/test_gpu_rounding.py, when both files run in one session
        what, dtype, m = max(rows, key=lambda r: r[2]["value"] / r[2]["cap"])
        f = (lambda v: "%d (%.3f %%)" % (v, 100.0 * v / m["compared"])) if dtype == "fp16" else (lambda v: "%.3g" % v)
        print("%-44s %5d  %-22s %-22s %-12s %s" % (family, len(rows), f(m["value"]), f(max(m["emulated"])), f(m["cap"]), what))
        assert all(r[2]["outside"] == 0 and r[2]["value"] <= r[2]["cap"] for r in rows)
