"""tests/rounding_contract.py checked without a GPU: the honest float32 emulations pass its two checks against each other, every
planted defect sits 10 x or more above the cap of check (b), and the carried bound of check (a) holds through a fire module.

Shapes and weight scaling are the project's own (tests/test_gpu_ops.py CONV_CASES, tests/fused_launch_cases.py make_weights):
a 1x1 16 -> 64, a shallow 3x3 64 -> 256, the deep 3x3 768 -> 72 without ReLU, and fire2 (64 -> 16 -> 64 + 64, squeeze hidden).
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
