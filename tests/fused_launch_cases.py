"""Cases for tests/test_gpu_fused_edges.py, importable without a GPU (tests/test_fused_launch_cases_host.py checks them).

Three things per persistent launch of the inference hot path:

  1. the launch geometry RESTATED from the launch code (tile size, tiles per image, workgroup cap as a function of the CU
     count, how a workgroup walks on to further tiles) -- every piece names the source line it restates.  These are a
     reading of the code, not a measurement: if a launcher changes, the restatement here has to follow, and the GPU
     tests' looping assertions are only as good as this reading;
  2. batch_for(): the smallest batch at which EVERY workgroup of the launch takes at least three tiles and at least one
     takes four, with a tile count that is no multiple of 8 (the eighth XCD band is short) -- and, for the persistent
     chain, no multiple of 4 (the last quad is partial) with a quad count that is no multiple of 8 either;
  3. fire_ref64(): the fused operation in float64 on the storage-rounded operands, one rounding to the storage type per
     conv (the reference of tests/test_gpu_conv_layouts.py, _conv64 / _finish, carried through a whole fire module).
"""
import functools
from collections import OrderedDict

import torch

from oracle import sqdet_oracle as O
from tests.test_gpu_conv_layouts import _conv64, _finish

# Device bytes one case may hand to the launch under test (input + outputs + scratch; weights are a few hundred KiB).  The
# largest case is the float32 pooled fire3 with both of its fallback scratches at 304 CUs: 463 images of 9x15, 77.5 MB.
BYTES_CAP = 96 << 20
ESZ = {"fp16": 2, "fp32": 4}
TDT = {"fp16": torch.float16, "fp32": torch.float32}


def cdiv(a, b):
    return -(-a // b)


def cu_count(multiprocessors):
    """csrc/common.cpp cu_count(): the device's compute units rounded down to a multiple of 8; 256 when fewer than 8."""
    return 256 if multiprocessors < 8 else multiprocessors // 8 * 8


def _same(n, k, s):
    return cdiv(n, s)


def _valid(n, k, s):
    return (n - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------- geometry
class Geometry:
    """One persistent kernel's tiling and walk.

    walk "band" (fire2.hip:199-203 and 648-656, fire3.hip:94-99, chain.hip:611-613 and 654, stem3.hip:126-158,
    stem4.hip:128-155): units = tiles (chain: quads of 4 tiles); grid = min(cap, units rounded up to 8); XCD x = block % 8
    owns the contiguous band [x * per, min(units, (x + 1) * per)), per = ceil(units / 8); workgroup lid = block / 8 of
    that XCD takes the band's units lid, lid + grid / 8, ...
    walk "flat" (stem5.hip:104 and 151): units = items, one per WAVE: wave wid = block * 4 + wave takes items wid,
    wid + 4 * grid, ...; grid = min(ceil(items / 4), cap) (stem5.hip:240-242)."""

    def __init__(self, name, tiles, cap, walk="band", group=1):
        self.name, self.tiles, self.cap, self.walk, self.group = name, tiles, cap, walk, group

    def units(self, n, h, w):
        return cdiv(n * self.tiles(h, w), self.group)

    def grid(self, units, cu):
        if self.walk == "flat":
            return min(cdiv(units, 4), self.cap(cu))
        return min(self.cap(cu), cdiv(units, 8) * 8)

    def steps(self, n, h, w, cu):
        """Units taken by every workgroup (walk "flat": every wave) of the launch, idle ones included as 0."""
        units = self.units(n, h, w)
        grid = self.grid(units, cu)
        if self.walk == "flat":
            nw = 4 * grid
            return [cdiv(units - wid, nw) if wid < units else 0 for wid in range(nw)]
        nl, per = grid // 8, cdiv(units, 8)
        out = []
        for xcd in range(8):
            band = max(min(units, (xcd + 1) * per) - xcd * per, 0)
            out += [cdiv(band - lid, nl) if lid < band else 0 for lid in range(nl)]
        return out


def _t16x8(h, w):        # fire2.hip:38 SCOLS = 16, :769 tiles_y = (h + 7) / 8; chain.hip:37 CROWS = 8, CCOLS = 16, :938
    return cdiv(w, 16) * cdiv(h, 8)


def _t16x4(h, w):        # fire3.hip:40 XCOLS = 16, :441 rows_t = 4 for f4, :443
    return cdiv(w, 16) * cdiv(h, 4)


def _tpool(h, w):        # fire2.hip:768 / fire3.hip:442: 7 x 4 POOLED pixels of the 3x3/s2 SAME pool
    return cdiv(cdiv(w, 2), 7) * cdiv(cdiv(h, 2), 4)


def _stem_hw(h, w, k, cpad, ppad):   # stem.hip:21-22
    f = _same if cpad == "SAME" else _valid
    g = _same if ppad == "SAME" else _valid
    return g(f(h, k, 2), 3, 2), g(f(w, k, 2), 3, 2)


def _tphase(h, w):       # stem4.hip:34-35 PPR = 4, PPC = 64, :349-350 (the SAME / SAME 3x3 stem)
    hp, wp = _stem_hw(h, w, 3, "SAME", "SAME")
    return cdiv(wp, 64) * cdiv(hp, 4)


def _tpers(h, w):        # stem.h:38-39 QPR = 4, QSP = 7, stem3.hip:318-319: 4 strips of 7 pooled columns
    hp, wp = _stem_hw(h, w, 3, "SAME", "SAME")
    return cdiv(wp, 28) * cdiv(hp, 4)


def _tk7(h, w):          # stem5.hip:35-36 S5_PROWS = 7, :261-263 (the VALID / VALID 7x7 stem)
    hp, wp = _stem_hw(h, w, 7, "VALID", "VALID")
    return cdiv(wp, 7) * cdiv(hp, 7)


# fire3.hip:409 NWAVES = (4 * NG / NTW) * RS, :415 WGPC = WPS * 4 / NWAVES, :416 grid = cu_count() * WGPC, with the template
# arguments of fire3.hip:451-464: f2 <NG 1, NTW 2, RS 4, WPS 4> 8 waves, 2 per CU; f3 <1, 2, 2, WPS 4> 4 waves, 4 per CU;
# f4 <2, 2, 2, WPS 4> 8 waves, 2 per CU; f5 <2, 1, 1, WPS 4> 8 waves, 2 per CU
DMA_F2 = Geometry("fire_dma f2", _t16x8, lambda cu: 2 * cu)
DMA_F3 = Geometry("fire_dma f3", _tpool, lambda cu: 4 * cu)
DMA_F4 = Geometry("fire_dma f4", _t16x4, lambda cu: 2 * cu)
DMA_F5 = Geometry("fire_dma f5", _tpool, lambda cu: 2 * cu)
# fire2.hip:688 / :806 grid = cu_count() * (8 / NWAVES), NWAVES = 4 per 64 expand couts (:675 4 * g1.ngroups, :909)
STREAM_E64 = Geometry("fire_stream E=64", _t16x8, lambda cu: 2 * cu)
STREAM_E128 = Geometry("fire_stream E=128", _t16x8, lambda cu: cu)
STREAM_POOL_E64 = Geometry("fire_stream pooled E=64", _tpool, lambda cu: 2 * cu)
STREAM_POOL_E128 = Geometry("fire_stream pooled E=128", _tpool, lambda cu: cu)
# chain.hip:564 CS_TILES = 4 tiles per step, :955 nquads, :790-791 one workgroup per CU
CHAIN = Geometry("fire_chain_stream", _t16x8, lambda cu: cu, group=4)
# stem4.hip:353 grid = cu_count() * WPC, :369-370 WPC = 2
STEM_PHASE = Geometry("stem_phase_dma", _tphase, lambda cu: 2 * cu)
# stem3.hip:322 grid = 1024 whatever the device
STEM_PERS = Geometry("stem_pers", _tpers, lambda cu: 1024)
# stem5.hip:37 S5_WAVES = 4, :241 cap = cu_count() * 2 workgroups
STEM_K7 = Geometry("stem_k7", _tk7, lambda cu: 2 * cu, walk="flat")


# ------------------------------------------------------------------------------------------------------------ entry points
class Spec:
    """One C entry point in one form: the tensors it is handed (shapes from the batch and the map) and its channel shape.
    entry: fire | fire_keep | fire_maxpool | fire_expand | fire_sqnext | fire_expsqnext | chain | stem | stem_sq."""

    def __init__(self, entry, dtype="fp16", cin=0, s=0, e=0, s2=0, pool=False, want_y=False, k=3, cout=64, cpad="SAME", ppad="SAME", e3=None):
        self.e3 = e if e3 is None else e3
        self.entry, self.dtype, self.cin, self.s, self.e, self.s2, self.pool, self.want_y = entry, dtype, cin, s, e, s2, bool(pool), want_y
        self.k, self.cout, self.cpad, self.ppad = k, cout, cpad, ppad

    @property
    def id(self):
        if self.entry.startswith("stem"):
            return "%s-%s-k%d-c%d-%s-%s-n%d" % (self.entry, self.dtype, self.k, self.cout, self.cpad, self.ppad, self.s2)
        return "%s-%s-c%d-s%d-e%d-n%d%s%s" % (self.entry, self.dtype, self.cin, self.s, self.e, self.s2, "-pool" if self.pool else "",
                                            "-y" if self.want_y else "") + \
            ("" if self.e3 == self.e else "-e3x%d" % self.e3)

    @property
    def from_squeeze(self):
        return self.entry in ("fire_expand", "fire_expsqnext", "chain")

    def in_shape(self, n, h, w):
        if self.entry.startswith("stem"):
            return (n, h, w, 3)
        return (n, h, w, self.s if self.from_squeeze else self.cin)

    def out_hw(self, h, w):
        if self.entry.startswith("stem"):
            return _stem_hw(h, w, self.k, self.cpad, self.ppad)
        return (cdiv(h, 2), cdiv(w, 2)) if self.pool else (h, w)

    def buffers(self, n, h, w):
        """name -> (shape, role) of every tensor the entry point writes or may write, in the order of its arguments;
        role "out": every element is written; "scratch": only the unfused fallback writes it."""
        ho, wo = self.out_hw(h, w)
        b = OrderedDict()
        if self.entry == "fire":
            b["sq"] = ((n, h, w, self.s), "scratch")
            b["y"] = ((n, h, w, self.e + self.e3), "out")
        elif self.entry == "fire_keep":
            b["sq"] = ((n, h, w, self.s), "out")
            b["y"] = ((n, h, w, self.e + self.e3), "out")
        elif self.entry == "fire_maxpool":
            b["sq"] = ((n, h, w, self.s), "scratch")
            b["full"] = ((n, h, w, self.e + self.e3), "scratch")
            b["y"] = ((n, ho, wo, self.e + self.e3), "out")
        elif self.entry == "fire_expand":
            b["y"] = ((n, ho, wo, self.e + self.e3), "out")
        elif self.entry in ("fire_sqnext", "fire_expsqnext"):
            b["sq_out"] = ((n, ho, wo, self.s2), "out")
        elif self.entry == "chain":
            if self.want_y or not self.s2:
                b["y"] = ((n, h, w, self.e + self.e3), "out")
            if self.s2:
                b["sq_out"] = ((n, h, w, self.s2), "out")
        elif self.entry == "stem":
            b["y"] = ((n, ho, wo, self.cout), "out")
        elif self.entry == "stem_sq":
            b["sq_out"] = ((n, ho, wo, self.s2), "out")
        else:
            raise ValueError(self.entry)
        return b

    def device_bytes(self, n, h, w):
        def numel(shape):
            r = 1
            for v in shape:
                r *= v
            return r
        return ESZ[self.dtype] * (numel(self.in_shape(n, h, w)) + sum(numel(s) for s, _ in self.buffers(n, h, w).values()))


class LoopCase:
    """A launch that must loop: entry-point form, the kernel that takes it (under the options `opts`), a map just over one tile
    each way so every image is a handful of ragged tiles."""

    def __init__(self, name, spec, geo, hw, **opts):
        self.name, self.spec, self.geo, self.hw, self.opts = name, spec, geo, hw, opts

    def looping(self, n, cu):
        """The issue's looping conditions at batch n; (ok, smallest steps, largest steps, tiles)."""
        h, w = self.hw
        tiles = n * self.geo.tiles(h, w)
        st = self.geo.steps(n, h, w, cu)
        ok = min(st) >= 3 and max(st) >= 4 and tiles % 8 != 0
        if self.geo.group == 4:    # the persistent chain: a partial last quad, and a short last band of quads
            ok = ok and tiles % 4 != 0 and self.geo.units(n, h, w) % 8 != 0
        return ok, min(st), max(st), tiles

    def chunk_ok(self, n, cu):
        return max(self.geo.steps(n, self.hw[0], self.hw[1], cu)) <= 1


@functools.lru_cache(maxsize=None)
def _batch_for(case, cu):
    n = 1
    while not case.looping(n, cu)[0]:
        n += 1
        assert n < 100000, case.name
    return n


def batch_for(case, cu):
    """Smallest batch meeting case.looping() on a device of `cu` (already rounded) compute units."""
    return _batch_for(case, cu)


@functools.lru_cache(maxsize=None)
def chunk_for(case, cu):
    """Largest number of images in one launch at which no workgroup (wave) takes a second unit; even when more than one,
    so that every chunk of a batch starts at the 16-byte phase image 0 starts at."""
    c = 1
    while case.chunk_ok(c + 1, cu):
        c += 1
    return c if c < 2 else c // 2 * 2


_F2 = dict(s=16, e=64, s2=16)
_F3 = dict(s=16, e=64, s2=32, pool=True)
_F4 = dict(s=32, e=128, s2=32)
_F5 = dict(s=32, e=128, s2=48, pool=True)

LOOP_CASES = [
    # fire_dma (fire3.hip: sqdet_fire_expand_squeeze_next_fwd's four shapes)
    LoopCase("dma-f2", Spec("fire_expsqnext", **_F2), DMA_F2, (9, 17)),
    LoopCase("dma-f3", Spec("fire_expsqnext", **_F3), DMA_F3, (9, 15)),
    LoopCase("dma-f4", Spec("fire_expsqnext", **_F4), DMA_F4, (5, 17)),
    LoopCase("dma-f5", Spec("fire_expsqnext", **_F5), DMA_F5, (9, 15)),
    # the same four on the fire_stream SQIN / NTS2 forms they fall back to ("dbg" 70: fire2.hip:847-850)
    LoopCase("dbg70-f2", Spec("fire_expsqnext", **_F2), STREAM_E64, (9, 17), dbg=70),
    LoopCase("dbg70-f3", Spec("fire_expsqnext", **_F3), STREAM_POOL_E64, (9, 15), dbg=70),
    LoopCase("dbg70-f4", Spec("fire_expsqnext", **_F4), STREAM_E128, (9, 17), dbg=70),
    LoopCase("dbg70-f5", Spec("fire_expsqnext", **_F5), STREAM_POOL_E128, (9, 15), dbg=70),
    # fire_stream, unpooled: whole modules (two tiles in flight, and "dbg" 8: one), the squeeze kept, from the squeeze
    # tensor, and ending in the next module's squeeze
    LoopCase("fire2-fp16", Spec("fire", "fp16", 64, 16, 64), STREAM_E64, (9, 17)),
    LoopCase("fire2-fp16-one-in-flight", Spec("fire", "fp16", 64, 16, 64), STREAM_E64, (9, 17), dbg=8),
    LoopCase("fire2-fp32", Spec("fire", "fp32", 64, 16, 64), STREAM_E64, (9, 17)),
    LoopCase("fire2-fp32-one-in-flight", Spec("fire", "fp32", 64, 16, 64), STREAM_E64, (9, 17), dbg=8),
    LoopCase("fire4-fp16", Spec("fire", "fp16", 128, 32, 128), STREAM_E128, (9, 17)),
    LoopCase("fire4-fp16-one-in-flight", Spec("fire", "fp16", 128, 32, 128), STREAM_E128, (9, 17), dbg=8),
    LoopCase("keep-fire2-fp16", Spec("fire_keep", "fp16", 64, 16, 64), STREAM_E64, (9, 17)),
    LoopCase("keep-fire4-fp16-one-in-flight", Spec("fire_keep", "fp16", 128, 32, 128), STREAM_E128, (9, 17), dbg=8),
    LoopCase("expand-fire2", Spec("fire_expand", "fp16", 0, 16, 64), STREAM_E64, (9, 17)),
    LoopCase("expand-fire4-one-in-flight", Spec("fire_expand", "fp16", 0, 32, 128), STREAM_E128, (9, 17), dbg=8),
    LoopCase("sqnext-fire2-3", Spec("fire_sqnext", "fp16", 64, 16, 64, 16), STREAM_E64, (9, 17)),
    LoopCase("sqnext-fire4-5", Spec("fire_sqnext", "fp16", 128, 32, 128, 32), STREAM_E128, (9, 17)),
    # fire_stream, pooled
    LoopCase("pool-fire3-fp16", Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), STREAM_POOL_E64, (9, 15)),
    LoopCase("pool-fire3-fp16-one-in-flight", Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), STREAM_POOL_E64, (9, 15), dbg=8),
    LoopCase("pool-fire3-fp32", Spec("fire_maxpool", "fp32", 128, 16, 64, pool=True), STREAM_POOL_E64, (9, 15)),
    LoopCase("pool-fire5-fp16", Spec("fire_maxpool", "fp16", 256, 32, 128, pool=True), STREAM_POOL_E128, (9, 15)),
    LoopCase("pool-expand-fire3", Spec("fire_expand", "fp16", 0, 16, 64, pool=True), STREAM_POOL_E64, (9, 15)),
    LoopCase("pool-expand-fire5-one-in-flight", Spec("fire_expand", "fp16", 0, 32, 128, pool=True), STREAM_POOL_E128, (9, 15), dbg=8),
    # the persistent chain at any size ("dbg" 31: chain.hip:948)
    LoopCase("chain-s2-16", Spec("chain", "fp16", 0, 16, 64, 16), CHAIN, (9, 33), dbg=31),
    LoopCase("chain-s2-32", Spec("chain", "fp16", 0, 32, 128, 32), CHAIN, (9, 33), dbg=31),
    LoopCase("chain-s2-48", Spec("chain", "fp16", 0, 16, 64, 48), CHAIN, (9, 33), dbg=31),
    # the stems, with and without the fused squeeze
    LoopCase("stem-phase", Spec("stem"), STEM_PHASE, (19, 524)),
    LoopCase("stem-phase-squeeze", Spec("stem_sq", s2=16), STEM_PHASE, (19, 524)),
    LoopCase("stem-pers", Spec("stem"), STEM_PERS, (19, 236)),
    LoopCase("stem-pers-squeeze", Spec("stem_sq", s2=16), STEM_PERS, (19, 236)),
    LoopCase("stem-k7-c64", Spec("stem", k=7, cout=64, cpad="VALID", ppad="VALID"), STEM_K7, (41, 40)),
    LoopCase("stem-k7-c96", Spec("stem", k=7, cout=96, cpad="VALID", ppad="VALID"), STEM_K7, (41, 40)),
]
LOOP_BY_NAME = {c.name: c for c in LOOP_CASES}

# Maps smaller than one tile: every tile row and column is an edge at once; H / W of 1, 2, 3 and 4 give pooled sizes 1 and 2
# with both SAME pad splits ((1,1) for odd, (0,1) for even sizes).
TINY_MAPS = [(h, w) for h in (1, 2, 3) for w in (1, 2, 3)] + [(4, 1), (1, 18)]
TINY_BATCHES = (1, 3)


# ------------------------------------------------------------------------------------------------------- float64 restatement
def fire_ref64(x, wt, dtype, pool=False):
    """The fused fire operation in float64.  x: CPU tensor in the storage type -- the module input [N,H,W,Cin] when wt has
    "ws", else its squeeze tensor [N,H,W,S]; wt: float32 CPU kernels (HWIO, storage-rounded) and biases ws/bs (optional),
    w1/b1, w3/b3, wn/bn (optional: the next module's squeeze).  Each conv: float64 sum, + bias, ReLU, ONE rounding to the
    storage type.  Returns the tensors a fused launch can emit: "sq", "y" (pooled when pool), "sq_out"."""
    d = lambda t: t.double()
    r = {}
    sq = x
    if "ws" in wt:
        sq = r["sq"] = _finish(_conv64(d(x), d(wt["ws"]), d(wt["bs"]), 1, "SAME"), True, dtype)
    e1 = _finish(_conv64(d(sq), d(wt["w1"]), d(wt["b1"]), 1, "SAME"), True, dtype)
    e3 = _finish(_conv64(d(sq), d(wt["w3"]), d(wt["b3"]), 1, "SAME"), True, dtype)
    y = torch.cat([e1, e3], dim=3)
    if pool:    # a max of stored values: exact in any type
        y = O.pooling_layer(y.float(), 3, 2, "SAME").to(TDT[dtype])
    r["y"] = y
    if "wn" in wt:
        r["sq_out"] = _finish(_conv64(d(y), d(wt["wn"]), d(wt["bn"]), 1, "SAME"), True, dtype)
    return r


def make_weights(spec, seed):
    """Seeded float32 CPU kernels (storage-rounded) and biases for a fire-family Spec: dict with ws/bs (forms that start
    from x), w1/b1, w3/b3, wn/bn (forms that end in the next squeeze)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    rnd = (lambda t: t.half().float()) if spec.dtype == "fp16" else (lambda t: t)
    mk = lambda k, ci, co: rnd(torch.from_numpy((rs.randn(k, k, ci, co) * (2.0 / (k * k * ci)) ** 0.5).astype(np.float32)))
    mb = lambda c: torch.from_numpy(rs.uniform(-0.3, 0.3, c).astype(np.float32))
    wt = {}
    if not spec.from_squeeze:
        wt["ws"], wt["bs"] = mk(1, spec.cin, spec.s), mb(spec.s)
    wt["w1"], wt["b1"], wt["w3"], wt["b3"] = mk(1, spec.s, spec.e), mb(spec.e), mk(3, spec.s, spec.e3), mb(spec.e3)
    if spec.s2:
        wt["wn"], wt["bn"] = mk(1, spec.e + spec.e3, spec.s2), mb(spec.s2)
    return wt
