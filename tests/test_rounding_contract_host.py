"""tests/rounding_contract.py checked without a GPU: the honest float32 emulations pass its two checks against each other, every
planted defect sits 10 x or more above the cap of check (b), and the carried bound of check (a) holds through a fire module.

Shapes and weight scaling are the project's own (tests/test_gpu_ops.py CONV_CASES, tests/fused_launch_cases.py make_weights):
a 1x1 16 -> 64, a shallow 3x3 64 -> 256, the deep 3x3 768 -> 72 without ReLU, and fire2 (64 -> 16 -> 64 + 64, squeeze hidden).

The regimes of tests/test_gpu_rounding_range.py likewise: the honest orders pass in each, the four defects of range sit 10 x
above the cap of their regime and under the cap on the unit operands, every (case, regime) that file parametrizes meets
RC.conditions() by its reference alone, and an honest emulation scales exactly under input and biases x 2^k.
"""
import functools

import numpy as np
import pytest
import torch

from tests import fused_launch_cases as FC
from tests import rounding_contract as RC

# (N, H, W, Cin, Cout, k, relu)
CONVS = {"c1_16_64": (2, 9, 11, 16, 64, 1, True), "e3_64_256": (1, 9, 11, 64, 256, 3, True), "convdet_768_72": (2, 7, 13, 768, 72, 3, False)}
FIRE = FC.Spec("fire", "fp16", 64, 16, 64)
NAMES = list(CONVS) + ["fire2"]
DEFECT_FACTOR = 10


def _rnd(t, dtype):
    return t.half().float() if dtype == "fp16" else t


@functools.lru_cache(maxsize=None)
def _operands(name, dtype):
    rs = np.random.RandomState(len(name) * 131 + 7)
    if name == "fire2":
        wt = FC.make_weights(FC.Spec("fire", dtype, 64, 16, 64), 11)
        return _rnd(torch.from_numpy(rs.randn(2, 9, 11, 64).astype(np.float32)), dtype), wt
    n, h, w, cin, cout, k, relu = CONVS[name]
    x = _rnd(torch.from_numpy(rs.randn(n, h, w, cin).astype(np.float32)), dtype)
    wk = _rnd(torch.from_numpy((rs.randn(k, k, cin, cout) * (2.0 / (k * k * cin)) ** 0.5).astype(np.float32)), dtype)
    return x, (wk, torch.from_numpy(rs.uniform(-0.5, 0.5, cout).astype(np.float32)), relu)


def _program(name, dtype):
    x, rest = _operands(name, dtype)
    if name == "fire2":
        return RC.fire_program(x, rest)
    wk, b, relu = rest
    return RC.conv_program(x, wk, b, 1, "SAME", relu)


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    return RC.Case(_program(name, dtype), dtype)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("name", NAMES)
def test_honest_orders_pass_both_checks(name, dtype):
    """Each of the three summation orders, taken as the device result, passes (a) and (b); the reference alone meets the
    conditions on the compared elements.  (fire2: only y is observed -- its bound is the one carried through the squeeze.)"""
    case = _case(name, dtype)
    ref = case.ref["y"]
    for order, emu in zip(RC.ORDERS, case.emus):
        RC.check(emu["y"], ref, [e["y"] for e in case.emus], dtype, "%s %s order %s" % (name, dtype, order))


# defect -> the (case, dtype) rows it is planted in (half_carry needs more than one chunk of 32; half_x is the float32 path's)
PLANTED = [(d, n, "fp16", None) for d in ("rz", "bias_after") for n in NAMES] + \
          [("half_carry", n, "fp16", None) for n in ("e3_64_256", "convdet_768_72", "fire2")] + \
          [("bf16_w", n, t, None) for n in NAMES for t in ("fp16", "fp32")] + \
          [("half_x", n, "fp32", None) for n in NAMES] + \
          [("rz", "fire2", "fp16", (1,))]          # toward-zero rounding of the hidden squeeze only


@pytest.mark.parametrize("defect,name,dtype,at", PLANTED, ids=["%s-%s-%s%s" % (p[0], p[1], p[2], "-hidden" if p[3] else "") for p in PLANTED])
def test_planted_defect_is_ten_times_over_the_cap(defect, name, dtype, at):
    """Replace the defect by the honest emulation (defect=None) and this fails: the honest value is at most the cap."""
    case = _case(name, dtype)
    ref, emus = case.ref["y"], [e["y"] for e in case.emus]
    for order in RC.ORDERS:
        bad = _program(name, dtype)(RC.Emulation(dtype, order, defect=defect, at=at))["y"]
        m = RC.measure(bad, ref, emus, dtype)
        print("%s in %s %s, order %s: %s" % (defect, name, dtype, order, RC.describe(m, dtype)))
        assert m["honest"]
        assert m["value"] >= DEFECT_FACTOR * m["cap"], RC.describe(m, dtype)


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_carried_bound_through_the_fire_module(dtype):
    """The interval of y carries the hidden squeeze's: every honest chain lies inside it; the squeeze's own interval holds every
    honest squeeze; and the interval without the carried term (the expand convs bounded as if the reference's squeeze tensor
    had been their input) is left by honest chains -- the carried term is needed, not slack."""
    case = _case("fire2", dtype)
    for emu in case.emus:
        assert RC.out_of_bounds(emu["sq"], case.ref["sq"]) == 0
        assert RC.out_of_bounds(emu["y"], case.ref["y"]) == 0
    assert float(case.ref["y"].d.max()) > 0
    x, wt = _operands("fire2", dtype)
    direct = RC.fire_program(RC.Val(case.ref["sq"].want), {k: v for k, v in wt.items() if k not in ("ws", "bs")})(RC.Reference(dtype))["y"]
    assert bool((direct.want == case.ref["y"].want).all())
    assert bool(((case.ref["y"].lo <= direct.lo) & (direct.hi <= case.ref["y"].hi)).all())
    # a squeeze tensor at either end of its interval (or a mix) is one the contract allows a device: the module's y from it
    # stays inside the carried interval and leaves the direct one
    sq = case.ref["sq"]
    pick = torch.from_numpy(np.random.RandomState(5).rand(*sq.want.shape) < 0.5)
    left = 0
    for hidden in (sq.lo, sq.hi, torch.where(pick, sq.lo, sq.hi)):
        for order in RC.ORDERS:
            y = RC.fire_program(hidden.float(), {k: v for k, v in wt.items() if k not in ("ws", "bs")})(RC.Emulation(dtype, order))["y"]
            assert RC.out_of_bounds(y, case.ref["y"]) == 0
            left += RC.out_of_bounds(y, direct)
    assert left > 0


def test_storage_rounds_once_to_nearest_even():
    v = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -40, -(1.0 + 2.0 ** -11), 65519.9, 2.0 ** -25],
                     dtype=torch.float64)
    assert RC.storage(v, "fp16").tolist() == [1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, -1.0, 65504.0, 0.0]
    # a float32 step in between would round 1 + 2^-11 + 2^-40 down to the tie and then to even
    assert float(RC.storage(v[2:3], "fp32")) == 1.0 + 2.0 ** -11
    rz = RC.round_half_toward_zero(torch.tensor([1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 1.0, -0.75], dtype=torch.float32))
    assert rz.tolist() == [1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0, -0.75]


def test_cap_and_conditions():
    assert RC.cap([0, 1, 0], "fp16") == 8 and RC.cap([3, 9, 4], "fp16") == 36 and RC.cap([1e-7, 3e-7], "fp32") == pytest.approx(1.2e-6)
    assert RC.gamma(27) > 28 * RC.U and RC.gamma(6913) < 1.001 * 6914 * RC.U
    few = RC.Val(torch.cat([torch.ones(1999), torch.zeros(10)]))
    thin = RC.Val(torch.cat([torch.ones(2000), torch.zeros(6001)]))
    assert not RC.honest(few)[2] and not RC.honest(thin)[2] and RC.honest(RC.Val(torch.ones(2000)))[2]


def test_backward_filter_case_on_a_small_conv():
    """WgradCase: the honest orders pass both checks; a float16 running sum between chunks of pixels does not."""
    rs = np.random.RandomState(3)
    x = torch.from_numpy(rs.randn(2, 9, 11, 16).astype(np.float32)).half().float()
    dy = torch.from_numpy(rs.randn(2, 9, 11, 32).astype(np.float32)).half().float()
    w = torch.from_numpy(rs.randn(3, 3, 16, 32).astype(np.float32))
    case = RC.WgradCase(x, dy, 3, w, 1e-3, 0.25)
    for nm in ("dw",):
        for emu in case.emus:
            RC.check(emu[nm], case.ref[nm], [e[nm] for e in case.emus], "fp32", "wgrad " + nm)
    for emu in case.emus:
        assert RC.out_of_bounds(emu["db"], case.ref["db"]) == 0
    cols, _ = RC.im2col(x, 3, 1, "SAME")
    bad = RC.matmul_ordered(cols.t().contiguous(), dy.reshape(-1, 32), 32, carry=lambda a: a.half().float()) * np.float32(0.25) + \
        np.float32(1e-3) * w.reshape(-1, 32)
    m = RC.measure(bad.view(3, 3, 16, 32), case.ref["dw"], [e["dw"] for e in case.emus], "fp32")
    assert m["value"] >= DEFECT_FACTOR * m["cap"]


# ------------------------------------------------------------------------------------------------------------------ regimes
def _moved_operands(name, regime):
    """The float16 operands of _operands() moved into a regime (RC.move): (x, weights as _program takes them)."""
    x, rest = _operands(name, "fp16")
    if name == "fire2":
        return RC.move_weights(regime, x, rest, "fp16")
    wk, b, relu = rest
    x, ((wk, b),) = RC.move(regime, x, [(wk, b, 1)], "fp16")
    return x, (wk, b, relu)


def _moved_program(name, regime):
    x, rest = _moved_operands(name, regime)
    return RC.fire_program(x, rest) if name == "fire2" else RC.conv_program(x, rest[0], rest[1], 1, "SAME", rest[2])


@functools.lru_cache(maxsize=None)
def _moved_case(name, regime):
    return RC.Case(_moved_program(name, regime), "fp16")


def _stored_weights(name, regime):
    rest = _moved_operands(name, regime)[1]
    return [rest[kw] for kw, _, _ in RC.conv_keys(rest)] if name == "fire2" else [rest[0]]


@pytest.mark.parametrize("regime", RC.REGIMES)
@pytest.mark.parametrize("name", NAMES)
def test_honest_orders_pass_both_checks_in_every_regime(name, regime):
    """The reference of the moved case is where the regime says (RC.conditions), and each honest order, taken as the device
    result, lies in the derived interval and under the cap there too."""
    case = _moved_case(name, regime)
    print(RC.conditions(regime, case, ["y"], _moved_operands(name, regime)[0], _stored_weights(name, regime)))
    for order, emu in zip(RC.ORDERS, case.emus):
        RC.check(emu["y"], case.ref["y"], [e["y"] for e in case.emus], "fp16", "%s %s order %s" % (name, regime, order))


# defect -> the regime that shows it; planted in every conv of every case, and in one conv of fire2: the hidden squeeze (its
# input, its weights, its store) and, for the saturating store, the 3x3 expand
# the deep-K rows have a few subnormal weights per thousand as they are (He scaling: sigma 0.017 at K = 6912)
SEEN_AT_UNIT = {("ftz_w", "e3_64_256"), ("ftz_w", "convdet_768_72")}
RANGE_OF = {"ftz_in": "sub", "ftz_out": "sub", "ftz_w": "subw", "sat": "top"}
# sat in convdet_768_72 is over the cap by less: 14.8 % of its outputs are inf, and at K = 6912 the honest orders already differ
# from the correctly rounded value in 0.7 %, a cap of 2.6 %
RANGE_FACTOR = {("sat", "convdet_768_72"): 5}
RANGE_PLANTED = [(d, n, None) for d in RC.RANGE_DEFECTS for n in NAMES] + \
                [(d, "fire2", (3,) if d == "sat" else (1,)) for d in RC.RANGE_DEFECTS]


@pytest.mark.parametrize("defect,name,at", RANGE_PLANTED, ids=["%s-%s%s" % (p[0], p[1], "-one-conv" if p[2] else "") for p in RANGE_PLANTED])
def test_range_defect_is_ten_times_over_the_cap_and_invisible_at_unit_magnitude(defect, name, at):
    """In its regime a defect of range sits 10 x over the cap (RANGE_FACTOR: 5 x for the one deep-K case of sat); on the unit operands it stays under the cap, which is why no test
    on randn / He-scaled operands sees it (but flushed weights in the two deep-K rows, SEEN_AT_UNIT)."""
    regime = RANGE_OF[defect]
    case = _moved_case(name, regime)
    ref, emus = case.ref["y"], [e["y"] for e in case.emus]
    unit_case = _case(name, "fp16")
    for order, honest in zip(RC.ORDERS, unit_case.emus):
        bad = _moved_program(name, regime)(RC.Emulation("fp16", order, defect=defect, at=at))["y"]
        m = RC.measure(bad, ref, emus, "fp16")
        print("%s in %s %s, order %s: %s" % (defect, name, regime, order, RC.describe(m, "fp16")))
        assert m["honest"]
        assert m["value"] >= RANGE_FACTOR.get((defect, name), DEFECT_FACTOR) * m["cap"], RC.describe(m, "fp16")
        unit = _program(name, "fp16")(RC.Emulation("fp16", order, defect=defect, at=at))["y"]
        mu = RC.measure(unit, unit_case.ref["y"], [e["y"] for e in unit_case.emus], "fp16")
        print("    on the unit operands: %s" % RC.describe(mu, "fp16"))
        if (defect, name) not in SEEN_AT_UNIT:
            assert mu["value"] <= mu["cap"]


def _range_cases():
    """Every (case, regime) tests/test_gpu_rounding_range.py parametrizes, as (id, regime, program, written tensors, input, stored
    weights): built from that file's own lists and operand builders, on the CPU."""
    from tests import test_gpu_rounding as G
    from tests import test_gpu_rounding_range as R
    out = []
    for name, regime in sorted(set((n, r) for n, r, _ in R.SINGLE_PARAMS)):
        def single(name=name, regime=regime):
            cv = G._Single(name, "fp16", regime)
            yield RC.conv_program(cv.x, cv.w, cv.b, cv.stride, cv.pad, cv.relu), ["y"], cv.x, [cv.w]
            if name in R.EPILOGUE_ROWS and regime in R.EPILOGUE_REGIMES:
                yield RC.conv_program(cv.x, cv.w, cv.b, cv.stride, cv.pad, cv.relu, res=cv.residual_tensor().float()), ["y"], cv.x, [cv.w]
        out.append(("conv2d-%s-%s" % (name, regime), regime, single))
    launches = [(s, R.fused_n(s, *R.MAP), R.MAP, r) for s, _, r in R.FUSED_PARAMS] + [(s, 2, hw, r) for s, hw, r in R.STEM_PARAMS]
    for spec, n, hw, regime in launches:
        def launch(spec=spec, n=n, hw=hw, regime=regime):
            x, wt = G._moved_operands(spec, n, hw[0], hw[1], regime)
            written = [nm for nm, (_, role) in spec.buffers(n, hw[0], hw[1]).items() if role == "out"]
            yield G._program(spec, x.float(), wt), written, x.float(), [wt[kw] for kw, _, _ in RC.conv_keys(wt)]
        out.append(("%s-%dx%d-%s" % (spec.id, hw[0], hw[1], regime), regime, launch))
    for regime in ("sub", "top"):
        def convdet(regime=regime):
            x, wk, b = G._convdet_operands(R.CONVDET_SHAPE, regime)
            yield RC.conv_program(x, wk, b, 1, "SAME", False), ["y"], x, [wk]

        def pool2(regime=regime):
            x, wk, b = G._pool2_operands(R.POOL2_PAIR, "fp16", regime)
            yield RC.conv_pool_program(x, wk, b, 1, "SAME", True, (2, 2, "SAME")), ["y"], x, [wk]
        out += [("convdet-" + regime, regime, convdet), ("conv_maxpool2-" + regime, regime, pool2)]
    return {ident: (regime, build) for ident, regime, build in out}


RANGE_CASES = _range_cases()


@pytest.mark.parametrize("ident", sorted(RANGE_CASES))
def test_gpu_range_case_meets_the_conditions_of_its_regime(ident):
    """From the reference alone (no emulation): the conditions tests/test_gpu_rounding_range.py asserts again before it looks at
    a device value.  A case that cannot meet them is replaced in that file's lists, not skipped on the GPU."""
    regime, build = RANGE_CASES[ident]
    for program, written, x, weights in build():
        print(ident, RC.conditions(regime, RC.Case(program, "fp16", orders=()), written, x, weights))


def test_gpu_range_backward_cases_meet_the_conditions_of_their_regimes():
    from tests import test_gpu_rounding as G
    from tests import test_gpu_rounding_range as R
    for case in R.DGRAD_ROWS:
        for regime, exps in R.DGRAD_REGIMES.items():
            R.dgrad_conditions(G._Dgrad(case, "fp16", exps), regime, orders=())
    for name in R.WGRAD_RANGE_ROWS:
        _, dy, _ = G._wgrad_operands(name, "fp16", R.WGRAD_REGIMES["sub"])
        assert float(RC.subnormal16(dy).double().mean()) > RC.MIN_SUBNORMAL
        assert bool(torch.isfinite(G._wgrad_operands(name, "fp16", R.WGRAD_REGIMES["big"])[1]).all())


@pytest.mark.parametrize("k", [-6, 5])
@pytest.mark.parametrize("name", NAMES)
def test_emulation_scales_exactly(name, k):
    """Input and biases x 2^k change an honest emulation's float16 result by exactly 2^k on every element that is finite and
    normal or zero in both runs -- in fire2, on those not computed from a squeeze element that may be subnormal in one of the
    runs (RC.Fragile) -- with the unit input on the grid that x 2^-6 keeps.  The exact-scaling tests on the device rely on this."""
    x, rest = _operands(name, "fp16")
    x = RC.on_grid(x, 6, "fp16")

    def program(regime):
        if name == "fire2":
            return RC.fire_program(*RC.move_weights(regime, x, rest, "fp16"))
        xs, ((wk, b),) = RC.move(regime, x, [(rest[0], rest[1], 1)], "fp16")
        return RC.conv_program(xs, wk, b, 1, "SAME", rest[2])
    upstream = program(None)(RC.Fragile(k))["y"][1] if name == "fire2" else None
    for order in RC.ORDERS:
        unit, moved = [program(r)(RC.Emulation("fp16", order))["y"].half() for r in (None, k)]
        bad, left, compared = RC.scales_exactly(unit, moved, k, upstream)
        print("%s x 2^%d, order %s: %d differ, %.3f %% left out, %.1f %% compared" % (name, k, order, bad, 100 * left, 100 * compared))
        assert bad == 0 and left <= 0.01 and compared >= RC.MIN_SHARE
    if name == "fire2" and k < 0:      # the mask is needed: without it elements behind a subnormal squeeze value differ
        assert RC.scales_exactly(unit, moved, k)[0] > 0 or not bool(upstream.any())
