"""GPU tests of the fused persistent launches at their edges (cases and geometry: tests/fused_launch_cases.py).

  * looped launches: batches at which every workgroup of fire_stream / fire_dma / fire_chain_stream / stem_pers /
    stem_phase_dma / stem_k7 takes three or four tiles (asserted from the device's CU count), BITWISE against the same launch
    on chunks of images small enough that nobody takes a second tile, and against the unfused path under the rule
    tests/test_gpu_ops.py states for that launch;
  * guards and poison: every input inside NaN guards, every output and scratch inside canary guards and pre-filled with
    the canary;
  * maps smaller than one tile (H, W of 1..3, 4x1, 1x18), also against the float64 restatement of the module;
  * refusals (non-positive sizes, null pointers) and agreement of the *_supported predicates with the *_fwd calls.

The C entry points are called directly (ops.lib()) so that every buffer is the test's own.  No tolerance of this file's
own: comparisons are bitwise, or use _same_as_unfused / the stated stem rules of tests/test_gpu_ops.py, or -- against the
float64 restatement -- that module's float32 rtol 1e-3 / atol 1e-4 and float16 rtol 2^-8 / atol 2e-3.
"""
import contextlib
import ctypes as C
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import fused_launch_cases as FC
from tests.fused_launch_cases import Spec
from tests.test_gpu_conv_layouts import _canary, _same_bits
from tests.test_gpu_ops import _same_as_unfused

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64 * 1024          # bytes either side of a guarded tensor: a multiple of 256, so the tensor stays 256-byte aligned
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


def _ops():
    from squeezedet_amd import ops
    return ops


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (2 ** 31)


@contextlib.contextmanager
def _options(**opts):
    ops = _ops()
    try:
        for k, v in opts.items():
            ops.set_option(k, v)
        yield
    finally:
        for k in opts:
            ops.set_option(k, 0)


def _cus():
    return FC.cu_count(torch.cuda.get_device_properties(0).multi_processor_count)


def _numel(shape):
    return int(np.prod(shape))


def _embed(t, nan_dtype):
    """A copy of t (same shape and dtype) inside a flat buffer with GUARD bytes of NaN (of nan_dtype) on each side."""
    body = t.contiguous().view(torch.uint8).reshape(-1)
    nb = body.numel()
    g = torch.full((GUARD * 8 // torch.finfo(nan_dtype).bits,), float("nan"), dtype=nan_dtype, device=DEV).view(torch.uint8)
    flat = torch.cat([g, body, g])
    assert flat.data_ptr() % 256 == 0
    return flat[GUARD:GUARD + nb].view(t.dtype).reshape(t.shape)


class _Guarded:
    """An output / scratch tensor inside GUARD bytes of canary on each side, itself pre-filled with the canary."""

    def __init__(self, shape, dtype, seed):
        self.g = GUARD // FC.ESZ[dtype]
        self.n = _numel(shape)
        self.flat = _canary((2 * self.g + self.n,), dtype, seed)
        self.before = self.flat.clone()
        assert self.flat.data_ptr() % 256 == 0
        self.t = self.flat[self.g:self.g + self.n].view(shape)

    def guards_unchanged(self, what):
        _same_bits(self.flat[:self.g], self.before[:self.g], what + ": guard in front")
        _same_bits(self.flat[self.g + self.n:], self.before[self.g + self.n:], what + ": guard behind")

    def unchanged(self, what):
        _same_bits(self.flat, self.before, what)


# entry -> (C function, its pointer arguments in order, its int arguments between the pointers and dtype)
_SIG = {
    "fire": ("sqdet_fire_fwd", "x ws bs w1 b1 w3 b3 sq y", lambda s, n, h, w: (n, h, w, s.cin, s.s, s.e, s.e3)),
    "fire_keep": ("sqdet_fire_fwd_keep", "x ws bs w1 b1 w3 b3 sq y", lambda s, n, h, w: (n, h, w, s.cin, s.s, s.e, s.e3)),
    "fire_maxpool": ("sqdet_fire_maxpool_fwd", "x ws bs w1 b1 w3 b3 sq full y", lambda s, n, h, w: (n, h, w, s.cin, s.s, s.e, s.e3)),
    "fire_expand": ("sqdet_fire_expand_fwd", "x w1 b1 w3 b3 y", lambda s, n, h, w: (n, h, w, s.s, s.e, s.e3, int(s.pool))),
    "fire_sqnext": ("sqdet_fire_squeeze_next_fwd", "x ws bs w1 b1 w3 b3 wn bn sq_out",
                    lambda s, n, h, w: (n, h, w, s.cin, s.s, s.e, s.e3, s.s2)),
    "fire_expsqnext": ("sqdet_fire_expand_squeeze_next_fwd", "x w1 b1 w3 b3 wn bn sq_out",
                       lambda s, n, h, w: (n, h, w, s.s, s.e, s.e3, s.s2, int(s.pool))),
    "chain": ("sqdet_fire_chain_fwd", "x stream b1 b3 bn y sq_out", lambda s, n, h, w: (n, h, w, s.s, s.e, s.e3, s.s2)),
    "stem": ("sqdet_stem_conv_pool_fwd", "x w b y", lambda s, n, h, w: (n, h, w, s.cout, s.k, _pad(s.cpad), _pad(s.ppad))),
    "stem_sq": ("sqdet_stem_conv_pool_squeeze_fwd", "x w b wn bn sq_out",
                lambda s, n, h, w: (n, h, w, s.cout, s.k, _pad(s.cpad), _pad(s.ppad), s.s2)),
}


def _pad(p):
    return 0 if p == "SAME" else 1


def _weights(sp):
    """The seeded float32 CPU kernels (storage-rounded) and biases of a Spec."""
    if sp.entry.startswith("stem"):
        rs = np.random.RandomState(_seed("stem", sp.id))
        rnd = (lambda t: t.half().float()) if sp.dtype == "fp16" else (lambda t: t)
        wt = {"w": rnd(torch.from_numpy((rs.randn(sp.k, sp.k, 3, sp.cout) * (2.0 / (sp.k * sp.k * 3)) ** 0.5).astype(np.float32))),
              "b": torch.from_numpy(rs.uniform(-0.5, 0.5, sp.cout).astype(np.float32))}
        if sp.s2:
            wt["wn"] = rnd(torch.from_numpy((rs.randn(1, 1, sp.cout, sp.s2) * (2.0 / sp.cout) ** 0.5).astype(np.float32)))
            wt["bn"] = torch.from_numpy(rs.uniform(-0.3, 0.3, sp.s2).astype(np.float32))
        return wt
    return FC.make_weights(sp, _seed("fire", sp.id))


class Op:
    """A Spec with seeded weights on the device: calls the entry point on caller-owned buffers, and computes what the
    unfused path gives."""

    def __init__(self, spec, wt=None):
        """wt: the float32 CPU kernels (storage-rounded) and biases to use in place of the seeded ones of _weights()."""
        ops = _ops()
        self.spec, self.tdt = spec, FC.TDT[spec.dtype]
        sp = spec
        if wt is None:
            wt = _weights(sp)
        self.wt = wt
        self.packed = {k: ops.pack_conv_weights(v.to(DEV), self.tdt) for k, v in wt.items() if k.startswith("w")}
        self.operands = OrderedDict((k, (self.packed[k].data if k.startswith("w") else v.to(DEV))) for k, v in wt.items())
        self.nan_dtype = {k: (self.tdt if k.startswith("w") else torch.float32) for k in wt}
        if sp.entry == "chain":
            if ops.fire_chain_supported(sp.s, sp.e, sp.e3, sp.s2, self.tdt):
                self.chain = ops.FireChainStream(wt["w1"].to(DEV), wt["w3"].to(DEV), wt["wn"].to(DEV) if sp.s2 else None, self.tdt)
                stream = self.chain.data
            else:      # never read: the call refuses before any launch
                stream = torch.zeros(4096, dtype=torch.uint8, device=DEV)
            self.operands = OrderedDict([("stream", stream), ("b1", self.operands["b1"]), ("b3", self.operands["b3"])] +
                                        ([("bn", self.operands["bn"])] if sp.s2 else []))
            self.nan_dtype["stream"] = self.tdt

    def make_input(self, n, h, w, seed=0):
        sp = self.spec
        rs = np.random.RandomState(_seed("x", sp.id, n, h, w, seed))
        shape = sp.in_shape(n, h, w)
        if sp.entry.startswith("stem"):
            x = rs.uniform(-2, 2, shape)
        else:
            x = rs.randn(*shape) - 0.3                    # many negative pre-activations
        return torch.from_numpy(x.astype(np.float32)).to(self.tdt).to(DEV).contiguous()

    def call(self, x, bufs, n, h, w, operands=None, null=None):
        """The raw C call: x and bufs (name -> tensor) as they are; `null` names one pointer argument passed as NULL."""
        from squeezedet_amd import _lib
        fn_name, ptr_names, ints = _SIG[self.spec.entry]
        have = dict(operands or self.operands)
        have.update(bufs)
        have["x"] = x
        ptrs = [None if (nm == null or have.get(nm) is None) else C.c_void_p(have[nm].data_ptr()) for nm in ptr_names.split()]
        return getattr(_ops().lib(), fn_name)(*ptrs, *[int(v) for v in ints(self.spec, n, h, w)], _lib.dtype_code(self.tdt),
                                              _lib.stream_ptr())

    def alloc(self, n, h, w):
        """Plain (unguarded) buffers, pre-filled with a canary: a pixel the launch does not write keeps a random value."""
        return OrderedDict((nm, _canary(shape, self.spec.dtype, _seed("dirty", nm)))
                           for nm, (shape, _) in self.spec.buffers(n, h, w).items())

    def run(self, x, bufs=None):
        n, h, w = [int(v) for v in x.shape[:3]]
        bufs = self.alloc(n, h, w) if bufs is None else bufs
        rc = self.call(x, bufs, n, h, w)
        assert rc == OK, "%s: code %d: %s" % (self.spec.id, rc, _ops().lib().sqdet_last_error())
        return bufs

    def outputs(self, bufs):
        roles = self.spec.buffers(1, 4, 4)
        return OrderedDict((nm, t) for nm, t in bufs.items() if roles[nm][1] == "out")

    def run_chunks(self, x, c):
        """The same launch on consecutive chunks of c images, into slices of one set of buffers."""
        n, h, w = [int(v) for v in x.shape[:3]]
        bufs = self.alloc(n, h, w)
        for i0 in range(0, n, c):
            i1 = min(n, i0 + c)
            rc = self.call(x[i0:i1], {nm: t[i0:i1] for nm, t in bufs.items()}, i1 - i0, h, w)
            assert rc == OK, "%s: chunk at %d: code %d" % (self.spec.id, i0, rc)
        return bufs

    def unfused(self, x):
        """What the separate launches give for every output, as tests/test_gpu_ops.py compares each launch:
        name -> (tensor, rule); rule "bitwise", "s16" (_same_as_unfused) or "stem3" / "stem7" (the one-ulp stem rules)."""
        ops, sp, pk, o = _ops(), self.spec, self.packed, self.operands
        if sp.entry.startswith("stem"):
            pool1 = ops.maxpool_nhwc(ops.conv2d_nhwc(x, pk["w"], o["b"], 2, sp.cpad, True), 3, 2, sp.ppad)
            # test_fused_stem_conv_pool_parity: the float16 persistent 3x3 stems (even W, W * 6 >= 1408) and the float16 7x7
            # stems (even W, VALID pool) differ from conv -> pool by float32 summation order; everything else is bitwise
            rule = "bitwise"
            if sp.dtype == "fp16" and x.shape[2] % 2 == 0:
                if sp.k == 3 and x.shape[2] * 6 >= 1408:
                    rule = "stem3"
                elif sp.k == 7 and sp.ppad == "VALID":
                    rule = "stem7"
            if sp.entry == "stem":
                return {"y": (pool1, rule)}
            # test_stem_conv_pool_squeeze: bitwise the fused stem followed by the squeeze conv (the stem itself under its rule)
            fused_pool1 = ops.stem_conv_pool(x, pk["w"], o["b"], sp.cpad, sp.ppad)
            _stem_rule(fused_pool1, pool1, rule, sp.id + ": stem behind the squeeze form")
            return {"sq_out": (ops.conv2d_nhwc(fused_pool1, pk["wn"], o["bn"], 1, "SAME", True), "bitwise")}
        n, h, w = [int(v) for v in x.shape[:3]]
        sq = x if sp.from_squeeze else ops.conv2d_nhwc(x, pk["ws"], o["bs"], 1, "SAME", True)
        y = torch.empty((n, h, w, sp.e + sp.e3), dtype=self.tdt, device=DEV)
        b1, b3 = (o["b1"], o["b3"])
        ops.conv2d_nhwc(sq, pk["w1"], b1, 1, "SAME", True, out=y, out_coffset=0)
        ops.conv2d_nhwc(sq, pk["w3"], b3, 1, "SAME", True, out=y, out_coffset=sp.e)
        if sp.pool:
            y = ops.maxpool_nhwc(y, 3, 2, "SAME")
        if sp.entry == "chain":       # test_fire_chain_parity: bitwise the separate convs
            want = {}
            if sp.want_y or not sp.s2:
                want["y"] = (y, "bitwise")
            if sp.s2:
                want["sq_out"] = (ops.conv2d_nhwc(y, pk["wn"], o["bn"], 1, "SAME", True), "bitwise")
            return want
        want = {}
        if sp.entry in ("fire", "fire_keep", "fire_maxpool", "fire_expand"):
            want["y"] = (y, "s16")
            if sp.entry == "fire_keep":          # test_fire_keep_squeeze: the squeeze tensor bitwise the squeeze conv's
                want["sq"] = (sq, "bitwise")
            return want
        # test_fire_squeeze_next_one_launch / test_fire_expand_squeeze_next: bitwise the fused module (itself under
        # _same_as_unfused against the separate convs) followed by the squeeze conv
        if sp.entry == "fire_sqnext":
            fused = ops.fire(x, pk["ws"], o["bs"], pk["w1"], b1, pk["w3"], b3)
        else:
            fused = ops.fire_expand(x, pk["w1"], b1, pk["w3"], b3, pool=sp.pool)
        _same_as_unfused(fused, y, sp.s, sp.dtype, sp.id + ": fused module behind the squeeze-next form")
        return {"sq_out": (ops.conv2d_nhwc(fused, pk["wn"], o["bn"], 1, "SAME", True), "bitwise")}

    def compare(self, bufs, want, what):
        outs = self.outputs(bufs)
        assert set(outs) == set(want), (set(outs), set(want))
        for nm, (w_, rule) in want.items():
            got, msg = outs[nm], "%s %s: %s" % (self.spec.id, what, nm)
            assert got.shape == w_.shape, msg
            if rule == "bitwise":
                _same_bits(got, w_, msg)
            elif rule == "s16":
                _same_as_unfused(got, w_, self.spec.s, self.spec.dtype, msg)
            else:
                _stem_rule(got, w_, rule, msg)


def _stem_rule(y, y2, rule, what):
    """The fused stems against conv -> pool, as test_fused_stem_conv_pool_parity (tests/test_gpu_ops.py) states them: the
    float16 persistent 3x3 stems and the float16 7x7 stems are float16-identical but for rare one-ulp flips (and absolute
    float32 noise next to 0); the project's own bounds, observed there, not re-measured here."""
    if rule == "bitwise":
        _same_bits(y, y2, what)
        return
    gap_max, frac_max = {"stem3": (2e-5, 1e-3), "stem7": (5e-5, 2e-3)}[rule]
    ulps = (y.view(torch.int16).int() - y2.view(torch.int16).int()).abs()
    gap = (y.float() - y2.float()).abs()
    assert bool(((ulps <= 1) | (gap <= gap_max)).all()) and float((ulps != 0).float().mean()) < frac_max, \
        "%s: %d ulps, %g, %g flipped" % (what, int(ulps.max()), float(gap.max()), float((ulps != 0).float().mean()))


_OPS = {}


def _op(spec):
    """Weights are built and packed once per form."""
    if spec.id not in _OPS:
        _OPS[spec.id] = Op(spec)
    return _OPS[spec.id]


# --------------------------------------------------------------------------------------------------------- looped launches
@pytest.mark.parametrize("case", FC.LOOP_CASES, ids=lambda c: c.name)
def test_looped_launch_equals_chunked_and_unfused(case):
    """Every workgroup takes three or four tiles; the result is bitwise the one-tile-per-workgroup launches' (an output
    depends only on its own tile, in the same accumulation order) and matches the unfused path under the launch's rule."""
    cu = _cus()
    h, w = case.hw
    n = FC.batch_for(case, cu)
    ok, lo, hi, tiles = case.looping(n, cu)
    assert ok and lo >= 3 and hi >= 4 and tiles % 8 != 0, (case.name, cu, n, lo, hi, tiles)
    c = FC.chunk_for(case, cu)
    assert case.chunk_ok(c, cu) and not case.chunk_ok(n, cu)
    print("%s: %d CUs, N = %d, %d tiles, %d..%d steps per %s, chunks of %d images"
          % (case.name, cu, n, tiles, lo, hi, "wave" if case.geo.walk == "flat" else "workgroup", c))
    op = _op(case.spec)
    x = op.make_input(n, h, w)
    with _options(**case.opts):
        whole = op.run(x)
        parts = op.run_chunks(x, c)
    torch.cuda.synchronize()
    for nm, t in op.outputs(whole).items():
        _same_bits(t, parts[nm], "%s: %s of the whole batch against the chunked launches" % (case.name, nm))
    op.compare(whole, op.unfused(x), "looped")


# -------------------------------------------------------------------------------------------------------- guards and poison
# (id, spec, its looped case or None, options): each entry point on its looped case and on a small multi-image map
GUARD_CASES = [
    ("fire", "fire2-fp16", {}), ("fire_keep", "keep-fire2-fp16", {}), ("fire_maxpool", "pool-fire3-fp16", {}),
    ("fire_expand", "expand-fire2", {}), ("fire_expand-pool", "pool-expand-fire3", {}), ("fire_sqnext", "sqnext-fire2-3", {}),
    ("fire_expsqnext", "dma-f2", {}), ("fire_expsqnext-pool", "dma-f3", {}), ("chain-persistent", "chain-s2-16", {"dbg": 31}),
    ("chain-ring", Spec("chain", "fp16", 0, 48, 192, 48), {}), ("chain-ring-y", Spec("chain", "fp16", 0, 48, 192, 48, want_y=True), {}),
    ("chain-ring-expand-only", Spec("chain", "fp16", 0, 96, 384, 0), {}),
    ("stem", "stem-phase", {}), ("stem_sq", "stem-pers-squeeze", {}), ("stem-k7", "stem-k7-c96", {}),
]
SMALL_HW = {"fire": (11, 19), "stem": (21, 250), "stem7": (45, 250)}


def _guard_shapes(which):
    """(spec, [(n, h, w)]): the looped case of an entry point (when it has one) and a small multi-image case."""
    if isinstance(which, Spec):
        return which, [(3, 11, 19), (5, 9, 33)]
    case = FC.LOOP_BY_NAME[which]
    sp = case.spec
    small = SMALL_HW["fire"] if not sp.entry.startswith("stem") else SMALL_HW["stem7" if sp.k == 7 else "stem"]
    if case.geo is FC.STEM_PHASE:
        small = (21, 530)       # (wide enough for the phase kernel)
    return sp, [(FC.batch_for(case, _cus()),) + case.hw, (3,) + small]


@pytest.mark.parametrize("name,which,opts", GUARD_CASES, ids=[g[0] for g in GUARD_CASES])
def test_guarded_outputs_and_poisoned_inputs(name, which, opts):
    spec, shapes = _guard_shapes(which)
    op = _op(spec)
    for (n, h, w) in shapes:
        what = "%s %dx%dx%d" % (name, n, h, w)
        x = op.make_input(n, h, w, seed=1)
        gx = _embed(x, op.tdt)
        goper = OrderedDict((k, _embed(v, op.nan_dtype[k])) for k, v in op.operands.items())
        guarded = OrderedDict((nm, _Guarded(shape, spec.dtype, _seed("guard", nm))) for nm, (shape, _) in spec.buffers(n, h, w).items())
        with _options(**opts):
            plain = op.run(x)
            rc = op.call(gx, {nm: g.t for nm, g in guarded.items()}, n, h, w, operands=goper)
        torch.cuda.synchronize()
        assert rc == OK, what
        roles = spec.buffers(n, h, w)
        for nm, g in guarded.items():
            g.guards_unchanged("%s: %s" % (what, nm))
            if roles[nm][1] == "out":
                assert not bool(torch.isnan(g.t).any()), "%s: NaN in %s" % (what, nm)
                _same_bits(g.t, plain[nm], "%s: %s between NaN guards against the plain run" % (what, nm))
            elif spec.entry == "fire_maxpool":
                # include/sqdet.h: the scratches are only used by the unfused fallback; these shapes run as one launch
                g.unchanged("%s: scratch %s of the one-launch form" % (what, nm))
        if n <= 8:      # (the looped shape is compared with the unfused path by test_looped_launch_equals_chunked_and_unfused)
            op.compare(plain, op.unfused(x), what)


# ------------------------------------------------------------------------------------------------ maps smaller than a tile
TINY_SPECS = [
    (Spec("fire", "fp16", 64, 16, 64), {}), (Spec("fire", "fp32", 64, 16, 64), {}), (Spec("fire", "fp16", 128, 32, 128), {}),
    (Spec("fire", "fp16", 64, 16, 64), {"dbg": 8}), (Spec("fire", "fp16", 256, 48, 192), {}),
    (Spec("fire_keep", "fp16", 64, 16, 64), {}), (Spec("fire_keep", "fp32", 128, 32, 128), {}),
    (Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), {}), (Spec("fire_maxpool", "fp32", 128, 16, 64, pool=True), {}),
    (Spec("fire_maxpool", "fp16", 256, 32, 128, pool=True), {}), (Spec("fire_maxpool", "fp16", 256, 32, 128, pool=True), {"dbg": 8}),
    (Spec("fire_expand", "fp16", 0, 16, 64), {}), (Spec("fire_expand", "fp16", 0, 32, 128), {}),
    (Spec("fire_expand", "fp16", 0, 16, 64, pool=True), {}), (Spec("fire_expand", "fp16", 0, 32, 128, pool=True), {}),
    (Spec("fire_expand", "fp16", 0, 192, 128), {}),
    (Spec("fire_sqnext", "fp16", 64, 16, 64, 16), {}), (Spec("fire_sqnext", "fp16", 128, 32, 128, 32), {}),
    (Spec("fire_expsqnext", s=16, e=64, s2=16), {}), (Spec("fire_expsqnext", s=16, e=64, s2=32, pool=True), {}),
    (Spec("fire_expsqnext", s=32, e=128, s2=32), {}), (Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True), {}),
    (Spec("fire_expsqnext", s=16, e=64, s2=16), {"dbg": 70}), (Spec("fire_expsqnext", s=16, e=64, s2=32, pool=True), {"dbg": 70}),
    (Spec("fire_expsqnext", s=32, e=128, s2=32), {"dbg": 70}), (Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True), {"dbg": 70}),
    (Spec("chain", "fp16", 0, 48, 192, 48), {}), (Spec("chain", "fp16", 0, 48, 192, 48, want_y=True), {}),
    (Spec("chain", "fp16", 0, 96, 384, 0), {}), (Spec("chain", "fp16", 0, 16, 64, 16), {}),
    (Spec("chain", "fp16", 0, 16, 64, 16), {"dbg": 31}), (Spec("chain", "fp16", 0, 32, 128, 32), {"dbg": 31}),
    (Spec("chain", "fp16", 0, 16, 64, 48), {"dbg": 31}),
]


def _tiny_id(p):
    return p[0].id + "".join("-%s%d" % kv for kv in sorted(p[1].items()))


@pytest.mark.parametrize("spec,opts", TINY_SPECS, ids=[_tiny_id(p) for p in TINY_SPECS])
def test_maps_smaller_than_a_tile(spec, opts):
    """H and W of 1, 2, 3 (and 4x1, 1x18), batches of 1 and 3: every tile row and column is an edge at once; the pooled forms
    reach pooled sizes 1 and 2 with both SAME pad splits.  Bitwise against the unfused path (under the launch's rule) and
    against the float64 restatement at the module tolerance of tests/test_gpu_ops.py."""
    op = _op(spec)
    tol = dict(rtol=1e-3, atol=1e-4) if spec.dtype == "fp32" else dict(rtol=2 ** -8, atol=2e-3)
    for (h, w) in FC.TINY_MAPS:
        for n in FC.TINY_BATCHES:
            what = "%dx%dx%d" % (n, h, w)
            x = op.make_input(n, h, w)
            with _options(**opts):
                bufs = op.run(x)
            op.compare(bufs, op.unfused(x), what)
            ref = FC.fire_ref64(x.cpu(), op.wt, spec.dtype, pool=spec.pool)
            for nm, got in op.outputs(bufs).items():
                g, r = got.float().cpu().numpy(), ref[nm].float().numpy()
                assert g.shape == r.shape, (what, nm)
                np.testing.assert_allclose(g, r, err_msg="%s %s %s against float64" % (spec.id, what, nm), **tol)


# ------------------------------------------------------------------------------------------------------------------ refusals
REFUSAL_SPECS = [
    Spec("fire", "fp16", 64, 16, 64), Spec("fire_keep", "fp32", 64, 16, 64), Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True),
    Spec("fire_expand", "fp16", 0, 16, 64), Spec("fire_expand", "fp16", 0, 32, 128, pool=True), Spec("fire_sqnext", "fp16", 64, 16, 64, 16),
    Spec("fire_expsqnext", s=16, e=64, s2=16), Spec("fire_expsqnext", s=32, e=128, s2=48, pool=True),
    Spec("chain", "fp16", 0, 48, 192, 48, want_y=True), Spec("chain", "fp16", 0, 96, 384, 0), Spec("stem"), Spec("stem_sq", s2=16),
    Spec("stem", k=7, cout=96, cpad="VALID", ppad="VALID"),
]


@pytest.mark.parametrize("spec", REFUSAL_SPECS, ids=lambda s: s.id)
def test_degenerate_sizes_and_null_pointers_are_refused(spec):
    """n, h or w of 0 or -1 and a NULL for any operand: SQDET_EINVAL with a message, from the entry point's own checks ahead of
    any launch (csrc/net.cpp, stem.hip, chain.hip fire_chain_launch_ride), every output and scratch bitwise unchanged."""
    op = _op(spec)
    lib = _ops().lib()
    n, h, w = (2, 19, 236) if spec.entry.startswith("stem") and spec.k == 3 else (2, 41, 40) if spec.entry.startswith("stem") else (2, 5, 7)
    x = op.make_input(n, h, w)
    guarded = OrderedDict((nm, _Guarded(shape, spec.dtype, _seed("refuse", nm))) for nm, (shape, _) in spec.buffers(n, h, w).items())
    bufs = {nm: g.t for nm, g in guarded.items()}

    def refused(rc, what):
        torch.cuda.synchronize()
        assert rc == EINVAL, "%s %s: code %d" % (spec.id, what, rc)
        assert lib.sqdet_last_error(), what
        for nm, g in guarded.items():
            g.unchanged("%s %s: %s" % (spec.id, what, nm))

    for bad in (0, -1):
        for i in range(3):
            dims = [n, h, w]
            dims[i] = bad
            refused(op.call(x, bufs, *dims), "dims %r" % (dims,))
    names = _SIG[spec.entry][1].split()
    for nm in names:
        if spec.entry == "chain" and nm == "y" and spec.s2:
            continue          # (a chain call without y is the valid squeeze-only form)
        if spec.entry == "chain" and (nm == "bn" or nm == "sq_out") and not spec.s2:
            continue          # (NULL already: the expand-only form)
        refused(op.call(x, bufs, n, h, w, null=nm), "NULL %s" % nm)
    assert op.call(x, bufs, n, h, w) == OK       # and the same buffers are accepted as they are
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- predicates against the calls
def _agree(spec, supported, n, h, w, opts=None):
    """supported: the call succeeds and matches the unfused path; else SQDET_EUNSUPPORTED and untouched outputs."""
    op = _op(spec)
    x = op.make_input(n, h, w)
    what = "%s %dx%dx%d" % (spec.id, n, h, w)
    if supported:
        with _options(**(opts or {})):
            bufs = op.run(x)
        op.compare(bufs, op.unfused(x), what)
        return
    guarded = OrderedDict((nm, _Guarded(shape, spec.dtype, _seed("agree", nm))) for nm, (shape, _) in spec.buffers(n, h, w).items())
    rc = op.call(x, {nm: g.t for nm, g in guarded.items()}, n, h, w)
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED, "%s: the predicate says 0, the call returns %d" % (what, rc)
    assert _ops().lib().sqdet_last_error()
    for nm, g in guarded.items():
        g.unchanged("%s: %s after the refusal" % (what, nm))


def _code(dtype):
    return 1 if dtype == "fp16" else 0


def test_fire_squeeze_next_supported_agrees_with_the_call():
    lib = _ops().lib()
    seen = set()
    for dtype in ("fp16", "fp32"):
        for (cin, s, e, e3) in ((64, 16, 64, 64), (128, 32, 128, 128), (64, 24, 64, 64), (64, 16, 96, 96), (64, 16, 64, 128),
                                (128, 16, 64, 64), (256, 48, 192, 192)):
            for s2 in (16, 32, 48):
                sup = lib.sqdet_fire_squeeze_next_supported(cin, s, e, e3, s2, _code(dtype))
                seen.add(sup)
                _agree(Spec("fire_sqnext", dtype, cin, s, e, s2, e3=e3), sup, 2, 9, 17)
    assert seen == {0, 1}
    assert lib.sqdet_fire_squeeze_next_supported(64, 16, 64, 64, 16, 1) == 1 and lib.sqdet_fire_squeeze_next_supported(128, 32, 128, 128, 32, 1) == 1


def test_fire_expand_squeeze_next_supported_agrees_with_the_call():
    lib = _ops().lib()
    n_sup = 0
    for dtype in ("fp16", "fp32"):
        for (s, e, e3) in ((16, 64, 64), (32, 128, 128), (24, 64, 64), (16, 96, 96), (32, 128, 64), (16, 128, 128), (32, 64, 64)):
            for s2 in (16, 32, 48, 24):
                for pool in (0, 1):
                    sup = lib.sqdet_fire_expand_squeeze_next_supported(s, e, e3, s2, pool, _code(dtype))
                    n_sup += sup
                    _agree(Spec("fire_expsqnext", dtype, 0, s, e, s2, pool=pool, e3=e3), sup, 2, 9, 17)
    assert n_sup == 4           # SqueezeDet's four pairs, float16 only


def test_stem_squeeze_supported_agrees_with_the_call():
    lib = _ops().lib()
    seen = set()
    for (h, w) in ((19, 234), (19, 236), (19, 237), (19, 522), (19, 524), (9, 480)):
        for spec in (Spec("stem_sq", s2=16), Spec("stem_sq", s2=32), Spec("stem_sq", "fp32", s2=16),
                     Spec("stem_sq", s2=16, cpad="VALID", ppad="VALID"), Spec("stem_sq", s2=16, k=7, cout=64, cpad="SAME", ppad="VALID")):
            sup = lib.sqdet_stem_conv_pool_squeeze_supported(h, w, spec.cout, spec.k, _pad(spec.cpad), _pad(spec.ppad), spec.s2,
                                                             _code(spec.dtype), 2)
            seen.add((w, spec.id, spec.cpad, sup))
            _agree(spec, sup, 2, h, w)
    base = Spec("stem_sq", s2=16).id
    assert (234, base, "SAME", 0) in seen and (236, base, "SAME", 1) in seen and (237, base, "SAME", 0) in seen
    assert (522, base, "SAME", 1) in seen and (524, base, "SAME", 1) in seen
    with _options(stem_algo=2):     # the strip kernel only: no stem + squeeze launch
        assert lib.sqdet_stem_conv_pool_squeeze_supported(19, 524, 64, 3, 0, 0, 16, 1, 2) == 0
        _agree(Spec("stem_sq", s2=16), 0, 2, 19, 524)


def test_fire_chain_supported_agrees_with_the_call():
    """ops.fire_chain_supported (sqdet_fire_chain_stream_bytes > 0) around its edges: squeeze depths 96 / 100 / 104, next-squeeze
    widths outside the set instantiated behind each squeeze depth class (16 / 32 / 48 behind one chunk, 48 / 64 / 96 behind
    more), expand widths that are no multiple of 64, float32."""
    ops = _ops()
    seen = set()
    for dtype in ("fp16", "fp32"):
        for (s, e) in ((16, 64), (32, 128), (48, 192), (96, 384), (100, 192), (104, 192), (48, 96)):
            for s2 in (0, 16, 24, 48, 64, 96, 128):
                sup = int(ops.fire_chain_supported(s, e, e, s2, FC.TDT[dtype]))
                seen.add(sup)
                _agree(Spec("chain", dtype, 0, s, e, s2), sup, 2, 9, 17)
    assert seen == {0, 1}
    assert not ops.fire_chain_supported(16, 64, 64, 96, torch.float16) and not ops.fire_chain_supported(48, 192, 192, 16, torch.float16)


def test_fire_expand_pair_supported_and_the_fallbacks():
    """sqdet_fire_expand_fwd (unpooled), sqdet_fire_fwd and sqdet_fire_maxpool_fwd fall back instead of refusing: shapes no
    fused kernel covers must equal the separate launches BITWISE; the pooled sqdet_fire_expand_fwd refuses them."""
    lib = _ops().lib()
    seen = set()
    for (s, e, e3) in ((192, 128, 128), (384, 256, 256), (192, 64, 64), (192, 128, 192), (48, 192, 192), (40, 64, 64), (16, 64, 128)):
        for dtype in ("fp16", "fp32"):
            sup = lib.sqdet_fire_expand_pair_supported(2, 9, 17, s, e, e3, _code(dtype))
            seen.add(sup)
            spec = Spec("fire_expand", dtype, 0, s, e, e3=e3)
            op = _op(spec)
            x = op.make_input(2, 9, 17)
            bufs = op.run(x)
            # the tile kernel's PAIR form or two convs: bitwise either way
            op.compare(bufs, {"y": (op.unfused(x)["y"][0], "bitwise")}, "pair %d" % sup)
    assert seen == {0, 1}
    for dtype in ("fp16", "fp32"):
        for (cin, s, e, e3) in ((40, 24, 64, 96), (256, 48, 192, 192), (72, 16, 64, 96)):
            for entry in ("fire", "fire_maxpool"):
                spec = Spec(entry, dtype, cin, s, e, e3=e3, pool=entry == "fire_maxpool")
                op = _op(spec)
                x = op.make_input(3, 9, 15)
                bufs = op.run(x)
                want = op.unfused(x)
                op.compare(bufs, {"y": (want["y"][0], "bitwise")}, "fallback")
    _agree(Spec("fire_expand", "fp16", 0, 48, 192, pool=True), 0, 2, 9, 17)
    _agree(Spec("fire_expand", "fp32", 0, 16, 64, pool=True), 0, 2, 9, 17)
