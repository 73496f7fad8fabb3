"""tests/size_limit_cases.py on any machine: the byte arithmetic of every case, the memory cap, the restated guards and the two
planted mutations, the *_supported probes that take sizes on both sides of their limit, and the planner: a plan created on
either side of a fused launch's limit holds no layer its launcher will decline."""
import ctypes as C

import pytest

from tests import net_plan_cases as NP
from tests import size_limit_cases as SL
from tests.fused_launch_cases import cdiv
from tests.golden import make_net_plans_golden as G

F32, F16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    return G.load_lib()


@pytest.mark.parametrize("case", SL.CASES, ids=[c.name for c in SL.CASES])
def test_below_and_at_straddle_the_limit_by_one_image(case):
    ib = case.image_bytes()
    h, w = case.hw
    assert ib == case.tensor_bytes(case.crossing, 1)
    assert case.below * ib < case.limit <= case.at * ib and case.at == case.below + 1
    assert (case.below + 1) * ib >= case.limit > (case.at - 1) * ib           # off by one image either way fails one side
    assert case.limit in (SL.G2, SL.G4) and (case.crossing in case.shapes(1) or case.crossing in case.virtual)
    # ragged maps: no tile size of the kernels (16 x 8, 16 x 4, 7 x 4 pooled) divides them -- but for the one exact case and
    # ConvDet's own 24 x 78 map (whole tile rows, ragged columns)
    if case.name != "c1stream-x-exact" and case.hw != SL.MAP_DET:
        assert h % 4 and w % 16
        if getattr(case.op, "pool", False):
            assert cdiv(w, 2) % 7            # (47 x 61 pools to 24 x 31: ragged pooled columns, whole pooled rows)
    picks = case.picks(case.at)
    assert picks[0] == 0 and picks[-1] == case.at - 1 and (SL.G2 - 1) // ib in picks
    assert all(0 <= p < case.at for p in picks) and len(picks) <= 5 <= case.sub


@pytest.mark.parametrize("case", SL.CASES, ids=[c.name for c in SL.CASES])
def test_declared_device_memory_is_under_the_cap(case):
    for n in (case.below, case.at):
        assert case.device_bytes(n) <= SL.DEVICE_BYTES_CAP, "%s: %.2f GiB" % (case.name, case.device_bytes(n) / 2.0 ** 30)
        assert n * case.hw[0] * case.hw[1] <= 1 << 30                          # conv2d's own bound on the pixel count (conv.hip)
    assert case.sub * case.hw[0] * case.hw[1] >= 8192                           # conv1x1_deepk's pixel class
    if case.launch.startswith("conv1x1"):
        assert case.sub_batch_pixels() >= 65536                                 # conv1x1_stream's four-block tiles (c.P >= 16 * 4 * 1024)
    if case.launch == "chain":
        assert case.sub_batch_pixels() > 100000                                 # the persistent chain


@pytest.mark.parametrize("case", SL.CASES, ids=[c.name for c in SL.CASES])
def test_restated_guard_agrees_with_the_declared_outcome(case):
    """Below the limit the launcher's size condition holds; at it the condition fails exactly where the case says the launch
    hands over or refuses, and still holds where the case says the kernel runs on."""
    assert case.guard_ok(case.below)
    assert case.guard_ok(case.at) == (case.at_outcome == "runs")
    assert case.at_outcome in ("handover", "refuse", "runs") and (case.handover_to is not None) == (case.at_outcome == "handover")


def test_the_two_planted_mutations_flip_a_named_case():
    """Both mutations are shown on guard_ok(), this module's RESTATEMENT of the guards -- Python, not tied to the C sources.
    Mutation 1, conv1x1_stream's `xb >= 2^31` written `>`: case c1stream-x-exact (16 x 16 x 64 float16 = 32768 bytes per
    image, exactly 2^31 bytes at batch 65536) passes the mutated restatement at `at`; the ragged cases cannot (their `at`
    tensors are over, not at, 2^31).  ONLY this restatement sees the mutation: conv1x1.hip has no host probe, and
    test_at_the_limit[c1stream-x-exact] would pass with the mutated C guard -- at exactly 2^31 bytes every real offset is
    still below 2^31, the streaming kernel and its hand-over agree bitwise on this data (differs = False), and the test does
    not learn which kernel ran.  The same `>=` of the fire launches IS tied to the C guard: fire3+pool3's input is exactly
    2^31 bytes at 64 x 64, batch 32768, and test_the_planner_unfuses_only_what_its_launcher_would_decline asks the library.
    Mutation 2, the y term of fire_stream's condition dropped (fire2.hip stream_sizes_ok, formerly fire_stream_launch_full's
    `|| yb >= 2^31`): case fire-stream-y passes the mutated restatement at `at` with a y of 2^31 + 4864 bytes, x at half of
    it; test_at_the_limit[fire-stream-y] makes that call and judges its last image by the rounding contract, so it fails
    only if the streaming kernel is wrong on such a y.  Neither mutated kernel was run."""
    exact = SL.BY_NAME["c1stream-x-exact"]
    assert exact.tensor_bytes("x", exact.at) == SL.G2
    assert not exact.guard_ok(exact.at) and exact.guard_ok(exact.at, strict=True)
    assert all(c.guard_ok(c.at, strict=True) == c.guard_ok(c.at) for c in SL.CASES if c is not exact)
    fy = SL.BY_NAME["fire-stream-y"]
    assert fy.tensor_bytes("y", fy.at) == SL.G2 + 4864 and 2 * fy.tensor_bytes("x", fy.at) == fy.tensor_bytes("y", fy.at)
    assert not fy.guard_ok(fy.at) and fy.guard_ok(fy.at, drop=("y",)) and fy.guard_ok(fy.below, drop=("y",))


def test_chain_shapes_of_the_cases_are_chain_shapes(lib):
    for c in SL.CASES:
        if c.launch == "chain":
            assert lib.sqdet_fire_chain_stream_bytes(c.op.s, c.op.e, c.op.e3, c.op.s2, F16) > 0, c.name


# (probe, arguments before n, arguments after n, pixels per image, what is bounded, its limit): n does the rest
def _probe_rows():
    hp, wp = 5, 59           # 19 x 236 through the 3x3/s2 SAME conv and the 3x3/s2 SAME pool
    return [
        # conv.hip / conv3x3.hip conv2d_maxpool2_eligible: n * h * w <= 2^30 pixels
        ("sqdet_conv2d_maxpool2_supported", lambda n: (n, 47, 61, 64, 64, F16), 47 * 61, (1 << 30) + 1),
        # conv3x3.hip conv3x3_pair_eligible: the concat tensor n * h * w * (e1 + e3) * 2 under 2^31 bytes
        ("sqdet_fire_expand_pair_supported", lambda n: (n, 13, 29, 192, 256, 256, F16), 13 * 29 * 512 * 2, SL.G2),
        # (its squeeze tensor is the smaller one wherever the form reaches the limit: s <= 192 there, e1 + e3 >= 256)
        # stem.hip stem_pers_shape: the pooled stem output n * Hp * Wp * 64 * 2 under 2^31 bytes (the squeeze form is gated on it)
        ("sqdet_stem_conv_pool_squeeze_supported", lambda n: (19, 236, 64, 3, 0, 0, 16, F16, n), hp * wp * 64 * 2, SL.G2),
    ]


@pytest.mark.parametrize("row", range(3))
def test_supported_probes_on_both_sides_of_their_limit(lib, row):
    name, args, per_image, limit = _probe_rows()[row]
    below = (limit - 1) // per_image
    fn = getattr(lib, name)
    assert fn(*args(2)) == 1, "the shape itself must be covered"
    assert fn(*args(below)) == 1 and below * per_image < limit
    assert fn(*args(below + 1)) == 0 and (below + 1) * per_image >= limit


# --------------------------------------------------------------------------------------------------------------------- plans
def _plan(lib, arch, dtype, batch, size, opt):
    """(layer names, launchable flags) of a plan created under `opt`."""
    h = C.c_void_p()
    if opt is not None:
        assert lib.sqdet_set_option(opt[0].encode(), opt[1]) == 0
    try:
        rc = lib.sqdet_net_create(C.byref(h), NP.ARCH_ID[arch], NP.DTYPE_ID[dtype], batch, size[0], size[1], G.CLASSES, G.APG)
        assert rc == 0, lib.sqdet_last_error()
        name = C.create_string_buffer(256)
        names, flags = [], []
        for i in range(lib.sqdet_net_num_layers(h)):
            assert lib.sqdet_net_layer_info(h, i, name, 256, None, None) == 0
            names.append(name.value.decode())
            flags.append(lib.sqdet_net_layer_launchable(h, i))
        assert lib.sqdet_net_layer_launchable(h, -1) == 0 and lib.sqdet_net_layer_launchable(h, len(names)) == 0
        return names, flags
    finally:
        if h:
            lib.sqdet_net_destroy(h)
        if opt is not None:
            assert lib.sqdet_set_option(opt[0].encode(), opt[2]) == 0


_PAIR_IDS = ["%s-%s-%dx%d-%s" % (a, d, s[0], s[1], "default" if o is None else "%s%d" % o[:2]) for a, d, _, s, o in SL.NET_PAIRS]


@pytest.mark.parametrize("pair", SL.NET_PAIRS, ids=_PAIR_IDS)
def test_plans_on_both_sides_hold_no_layer_their_launcher_declines(lib, pair):
    arch, dtype, batches, size, opt = pair
    for b in batches:
        names, flags = _plan(lib, arch, dtype, b, size, opt)
        assert flags == [1] * len(names), [n for n, f in zip(names, flags) if not f]
        assert names == list(NP.structure(lib, arch, dtype, b, size, opt))


def test_the_planner_unfuses_only_what_its_launcher_would_decline(lib):
    """64 x 64 float16: at batch 32768 fire2's / fire3's concat tensors are exactly 2^31 bytes.  The default plan keeps them
    inside launches that write squeeze tensors only -- the same structure on both sides.  With one launch per module
    ("fire_fuse" 5) fire3+pool3 reads fire2's 2^31-byte output: below the limit it is one launch, at it the module is three
    convs and a pool, and nothing else changes.  The input is EXACTLY 2^31 bytes: a `>` for the `>=` of fire2.hip's
    stream_sizes_ok would keep fire3+pool3 fused here.  With the pools kept apart ("fire_fuse" 4) the run fire2 -> fire3 ends
    in a chain launch that would write the 2^31-byte concat tensor: at the limit fire3 alone becomes three convs, fire2 stays
    one launch and the chains behind it stay chains."""
    size = (64, 64)
    d_lo, _ = _plan(lib, "squeezedet", "f16", 32767, size, None)
    d_hi, _ = _plan(lib, "squeezedet", "f16", 32768, size, None)
    assert d_lo == d_hi and "fire2+fire3/squeeze1x1" in d_hi
    ff5 = ("fire_fuse", 5, 0)
    lo, _ = _plan(lib, "squeezedet", "f16", 32767, size, ff5)
    hi, _ = _plan(lib, "squeezedet", "f16", 32768, size, ff5)
    assert "fire3+pool3" in lo and "fire3+pool3" not in hi
    assert [n for n in hi if n.startswith("fire3") or n == "pool3"] == ["fire3/squeeze1x1", "fire3/expand1x1", "fire3/expand3x3", "pool3"]
    assert [n for n in lo if not n.startswith(("fire2", "fire3", "pool3"))] == [n for n in hi if not n.startswith(("fire2", "fire3", "pool3"))]
    ff4 = ("fire_fuse", 4, 0)
    lo, _ = _plan(lib, "squeezedet", "f16", 32767, size, ff4)
    hi, _ = _plan(lib, "squeezedet", "f16", 32768, size, ff4)
    assert lo[1:4] == ["fire2+fire3/squeeze1x1", "fire3/expand", "pool3"]
    assert hi[1:6] == ["fire2", "fire3/squeeze1x1", "fire3/expand1x1", "fire3/expand3x3", "pool3"]
    assert lo[3:] == hi[5:] and "fire4+fire5/squeeze1x1" in hi and any(n.endswith("/expand+fire7/squeeze1x1") for n in hi)


def test_backward_filter_rows_straddle_both_limits():
    (below2, n0, _), (at2, n1, _), (below4, n2, _), (at4, n3, out3) = SL.WGRAD
    assert SL.wgrad_x_bytes(n0) < SL.G2 <= SL.wgrad_x_bytes(n1) and n1 == n0 + 1
    assert SL.wgrad_x_bytes(n2) < SL.WGRAD_LIMIT <= SL.wgrad_x_bytes(n3) and n3 == n2 + 1 and out3 == "refuse"
    assert SL.wgrad_x_bytes(n3) + n3 * 13 * 29 * SL.WGRAD_COUT * 2 + (64 << 20) <= SL.DEVICE_BYTES_CAP
    assert (SL.G4 - 1) // (13 * 29 * 64 * 2) in SL.wgrad_picks(n3) or SL.wgrad_x_bytes(n3) < SL.G4
    assert SL.WGRAD_COUT % 8 == 0 and SL.WGRAD_CIN % 8 == 0                     # 16-byte rows in float16 (wgrad.hip)
    n = SL.POOL_4G["n"]
    ib = SL.POOL_4G["hw"][0] * SL.POOL_4G["hw"][1] * SL.POOL_4G["c"] * 2
    assert (n - 1) * ib < SL.G4 <= n * ib


def test_left_out_launches_carry_a_reason():
    assert all(len(reason) > 10 for reason in SL.LEFT_OUT.values())
