"""Cases for tests/test_gpu_size_limits.py, importable without a GPU (tests/test_size_limits_host.py checks them): launches that
address a tensor through a buffer resource with 32-bit offsets, run with that tensor just under and at its limit (DESIGN.md,
"tensor size limits", has the audit these cases follow).

A case names the launch, the tensor that crosses (`crossing`: x, y, dy), the limit in bytes (2^31, or 2^32 for the
backward-filter conv and the generic fallbacks) and what the launcher does at the limit (`at_outcome`):

    "handover"  another kernel (or another staging path of the same kernel) takes the launch: still right, judged by the rounding
                contract of tests/rounding_contract.py on the picked images;
    "refuse"    the entry point returns SQDET_EUNSUPPORTED and writes nothing;
    "runs"      the tensor is not one the kernel addresses with 32-bit offsets (64-bit pointer stores): the same kernel runs on
                both sides, bitwise the sub-batch result on both.

Maps are small and ragged (tile tails everywhere), channels the smallest that select the kernel form, and the batch does the
rest: `below` is the largest N whose crossing tensor is under the limit, `at` = below + 1.  image_bytes() RESTATES the
launcher's byte arithmetic (source lines named per kind); guard_ok() restates its comparison, so the two mutations the
host test plants -- `>=` turned `>`, a dropped y term -- are seen to flip a named case.
"""
from collections import OrderedDict

from tests.fused_launch_cases import ESZ, Spec, cdiv

G2, G4 = 1 << 31, 1 << 32
WGRAD_LIMIT = 0xfffffff0                 # wgrad.hip: the offset kept for "out of range"
DEVICE_BYTES_CAP = 10 << 30              # no case holds more device memory than this at once
# Images of a sub-batch (the picked images first, then filler images).  Large enough that the pixel-count classes of the
# dispatch are those of the full batch: 256 images of 7x13 are 23296 pixels (>= 8192: conv1x1_deepk; >= 65536 at 13x29: the
# streaming 1x1's four-block tiles); the chain cases take 1280 (116480 pixels > 100000: fire_chain's persistent form).
SUB = 256

MAP_S, MAP_T, MAP_DET, MAP_POOL = (13, 29), (7, 13), (24, 78), (47, 61)


class Conv:
    """conv2d_nhwc of `cin` -> `cout` channels: the row of tests/test_gpu_conv_layouts.py that selects the kernel, at another map."""

    def __init__(self, cin, cout, k=1, relu=True, dtype="fp16", conv_algo=0, pool2=None, residual=False):
        """pool2: None, "y" (conv2d_maxpool2_nhwc: the 2x2/s2 SAME pool in the epilogue) or "idx" (its _idx form: + the window index).
        residual: conv2d_nhwc(residual=): a tensor of y's shape, random everywhere, added in the epilogue."""
        self.cin, self.cout, self.k, self.relu, self.dtype, self.conv_algo, self.pool2 = cin, cout, k, relu, dtype, conv_algo, pool2
        self.residual = residual


class Bwd(Conv):
    """conv2d_bwd_data of a stride-1 SAME conv cin -> cout: reads channels [coffset, coffset + cout) of dY [N, H, W, ctot] (the
    launch's x: a channel slice of a wider tensor) and writes dx [N, H, W, cin] (its y).  relu_of: the accumulate + relu_of form
    -- dx holds the prior gradient, relu_of is a tensor of dx's shape, both random everywhere."""

    def __init__(self, cin, cout, k, ctot, coffset, relu_of=False, dtype="fp16"):
        Conv.__init__(self, cin, cout, k, False, dtype)
        self.ctot, self.coffset, self.relu_of = ctot, coffset, relu_of


class SizeCase:
    def __init__(self, name, launch, crossing, limit, hw, op, at_outcome, handover_to=None, differs=True, note="", sub=SUB, virtual=None):
        """differs: whether, on the test's data, the fast kernel's sub-batch result differs from conv_algo = generic in at least
        one element (measured once on an MI355X and then asserted); False: the two agree bitwise, the `below` case proves addressing
        only; None: the entry point has no generic form.  sub: images of the sub-batch.  virtual: name -> bytes per image of an
        extent the guard bounds that is no tensor of the call (the chain's concat extent where only sq_out is written, the pooled
        64-channel stem output behind the stem + squeeze launch)."""
        self.virtual = virtual or {}
        self.name, self.launch, self.crossing, self.limit, self.hw, self.op = name, launch, crossing, limit, hw, op
        self.at_outcome, self.handover_to, self.differs, self.note, self.sub = at_outcome, handover_to, differs, note, sub

    # ---- shapes
    def shapes(self, n):
        """name -> (shape, element bytes) of every device tensor of the launch on n images (weights: a few hundred KiB, left out)."""
        h, w = self.hw
        if isinstance(self.op, Bwd):
            e = ESZ[self.op.dtype]
            r = OrderedDict([("x", ((n, h, w, self.op.ctot), e)), ("y", ((n, h, w, self.op.cin), e))])
            if self.op.relu_of:
                r["relu_of"] = r["y"]
            return r
        if isinstance(self.op, Conv):
            e = ESZ[self.op.dtype]
            ho, wo = (cdiv(h, 2), cdiv(w, 2)) if self.op.pool2 else (h, w)
            r = OrderedDict([("x", ((n, h, w, self.op.cin), e)), ("y", ((n, ho, wo, self.op.cout), e))])
            if self.op.pool2 == "idx":
                r["idx"] = ((n, ho, wo, self.op.cout), 1)
            if self.op.residual:
                r["residual"] = r["y"]
            return r
        sp = self.op
        e = ESZ[sp.dtype]
        r = OrderedDict([("x", (sp.in_shape(n, h, w), e))])
        for nm, (shape, _) in sp.buffers(n, h, w).items():
            r[nm] = (shape, e)
        return r

    def tensor_bytes(self, name, n):
        if name in self.virtual:
            return n * self.virtual[name]
        if name == "xs":      # conv3x3.hip tile_launch_impl: xs_bytes = N * H * W * x_cstride * es - x_coffset * es
            return self.tensor_bytes("x", n) - self.op.coffset * ESZ[self.op.dtype]
        shape, e = self.shapes(n)[name]
        r = e
        for v in shape:
            r *= v
        return r

    def image_bytes(self):
        """Bytes of one image of the crossing tensor."""
        return self.tensor_bytes(self.crossing, 1)

    @property
    def below(self):
        return (self.limit - 1) // self.image_bytes()

    @property
    def at(self):
        return self.below + 1

    def device_bytes(self, n):
        """Everything the test holds at once: the launch's tensors at n images, the guards, and the sub-batch copies."""
        full = sum(self.tensor_bytes(nm, n) for nm in self.shapes(n))
        return full + 2 * sum(self.tensor_bytes(nm, self.sub) for nm in self.shapes(self.sub)) + (8 << 20)

    # ---- the launcher's guard, restated
    def guarded(self, n):
        """(name, bytes) of the tensors the launcher's size guard looks at, in the order of its condition."""
        return [(nm, self.tensor_bytes(nm, n)) for nm in GUARDED[self.launch]]

    def guard_ok(self, n, strict=False, drop=()):
        """The launcher's condition on n images: every guarded tensor under the limit.  strict / drop plant the two mutations:
        `>=` written `>` (a tensor of exactly `limit` bytes passes), a term of the condition left out."""
        lim = self.limit - 1 if self.launch in LIMIT_0X7FFFFFFF else self.limit
        return all((b <= lim if strict else b < lim) for nm, b in self.guarded(n) if nm not in drop)

    def picks(self, n):
        """The images a test copies back: 0, n - 1, the one holding byte 2^31 - 1 of the crossing tensor, the one holding byte
        2^31 when the tensor reaches it, and for a 4 GiB case the one holding byte 2^32 - 1."""
        ib = self.image_bytes()
        p = [0, n - 1, min(n - 1, (G2 - 1) // ib)]
        if n * ib > G2:
            p.append(G2 // ib)
        if self.limit > G2:
            p.append(min(n - 1, (G4 - 1) // ib))
        return sorted(set(p))

    def sub_batch_pixels(self):
        return self.sub * self.hw[0] * self.hw[1]


# launch kind -> the tensors its size guard compares with the limit.
#   conv1x1_stream   conv1x1.hip conv1x1_stream_launch: xb = P * Cin * es, yb = P * y_cstride * es, either >= 2^31 declines
#   conv1x1_deepk    conv1x1k.hip conv1x1_deepk_launch: the same two
#   conv1x1_pipe     gemm1x1.hip conv1x1_tile_launch: xb (x_cstride), yb; at the limit the conv1x1_tile form of the same file
#   conv3x3_tile     conv3x3.hip tile_launch_impl: xs_bytes < 0x7fffffff selects LDS-DMA staging, else register staging
#   conv_direct      conv.hip: 64-bit indices, only the pixel counts are bounded (2^30)
#   fire_fused       fire.hip fused_sizes_ok: x only (y and sq_out through 64-bit pointers)
#   fire_stream      fire2.hip stream_sizes_ok through fire_stream_eligible_at: x and y
#   fire_maxpool     the same with the pooled y
#   fire_expand      fire2.hip fire_expand_stream_eligible_at: x (the squeeze tensor) and y
#   fire_sqnext      fire2.hip fire_squeeze_next_eligible_at: x
#   fire_expsqnext   fire2.hip fire_expand_squeeze_next_eligible_at: x (fire3.hip fire_dma_launch also bounds sq_out, and hands
#                    over to the fire_stream form, which stores it through pointers)
#   chain            chain.hip chain_sizes_ok: the concat extent n*h*w*(e1+e3)*2, whether y is written or not
LIMIT_0X7FFFFFFF = ("conv3x3_tile", "conv3x3_tile_slice", "convdet_splitk", "conv_pool2")     # these compare with 0x7fffffff, not 2^31
GUARDED = {
    "conv1x1_stream": ("x", "y"), "conv1x1_deepk": ("x", "y"), "conv1x1_pipe": ("x", "y"), "conv3x3_tile": ("x",),
    "conv_direct": (), "fire_fused": ("x",), "fire_stream": ("x", "y"), "fire_maxpool": ("x", "y"), "fire_expand": ("x", "y"),
    "fire_sqnext": ("x",), "fire_expsqnext": ("x",), "chain": ("concat",),
    # conv3x3.hip tile_launch_impl: split-K needs x_bytes < 0x7fffffff; the POOL2 forms stage by DMA under the same bound
    "convdet_splitk": ("x",), "conv_pool2": ("x",),
    # stem.hip stem_pers_shape (stem3.hip / stem4.hip) and stem5.hip stem_k7_launch: N * Hp * Wp * y_cstride * 2 under 2^31
    "stem": ("y",), "stem_sq": ("stem_y",),
    # conv3x3.hip tile_launch_impl on a channel-slice input: the extent of the WIDER tensor from the slice's first channel on
    "conv3x3_tile_slice": ("xs",),
    # conv3x3.hip conv3x3_pair_eligible: the squeeze tensor (staged by DMA) and the concat extent
    "expand_pair": ("x", "y"),
}


_FIRE2 = dict(cin=64, s=16, e=64)
_FIRE6 = dict(cin=256, s=48, e=192)        # no streaming form (three-chunk squeeze): fire.hip's own kernel

CASES = [
    # ---- single convs (conv2d_nhwc)
    SizeCase("c1stream-x", "conv1x1_stream", "x", G2, MAP_S, Conv(64, 16), "handover", "conv1x1_tile", differs=False),
    SizeCase("c1stream-x-exact", "conv1x1_stream", "x", G2, (16, 16), Conv(64, 16), "handover", "conv1x1_tile", differs=False,
             note="the one map that is not ragged: 32768 bytes per image, EXACTLY 2^31 bytes at batch 65536 (a `>` for `>=` shows here only)"),
    SizeCase("c1stream-y", "conv1x1_stream", "y", G2, MAP_S, Conv(32, 80, relu=False), "handover", "conv1x1_tile", differs=False),
    SizeCase("c1deepk-x", "conv1x1_deepk", "x", G2, MAP_S, Conv(264, 40), "handover", "conv1x1_tile", differs=False),
    SizeCase("c1pipe-x", "conv1x1_pipe", "x", G2, MAP_S, Conv(264, 256), "handover", "conv1x1_tile", differs=False),
    # conv1x1_pipe's epilogue tensors share y_bytes: the residual (conv2d_nhwc residual=), and relu_of with the prior dx
    # (conv2d_bwd_data, whose x is a channel slice [8, 144) of a 144-channel dY: xb comes from x_cstride)
    SizeCase("c1pipe-res-y", "conv1x1_pipe", "y", G2, MAP_S, Conv(136, 256, residual=True), "handover",
             "conv1x1_tile adding into a copy of the residual", differs=False),
    SizeCase("c1pipe-relu-of-y", "conv1x1_pipe", "y", G2, MAP_S, Bwd(256, 136, 1, 144, 8, relu_of=True), "handover", "conv1x1_tile",
             differs=False),
    # the 3x3 tile kernel on the expand3x3 half [64, 128) of a 128-channel dY: the wider tensor's extent crosses
    SizeCase("c3tile-slice-x", "conv3x3_tile_slice", "x", G2, MAP_S, Bwd(32, 64, 3, 128, 64), "handover",
             "conv3x3_tile, register staging", differs=True),
    # (the tile kernel compares with 0x7fffffff, not 2^31: the same for these even byte counts)
    SizeCase("c3tile-fp16-x", "conv3x3_tile", "x", G2, MAP_S, Conv(64, 32, k=3), "handover", "conv3x3_tile, register staging", differs=True),
    SizeCase("c3tile-fp32-x", "conv3x3_tile", "x", G2, MAP_S, Conv(32, 16, k=3, dtype="fp32"), "handover", "conv3x3_tile, register staging", differs=True),
    # ---- the fused fire launches (C entry points, tests/test_gpu_fused_edges.py Op)
    SizeCase("fire-fused-y", "fire_fused", "y", G2, MAP_T, Spec("fire", "fp16", **_FIRE6), "runs", differs=True,
             note="x stays below 2^31 (1.4 GiB); y is stored through 64-bit pointers, so fire.hip needs no y term"),
    SizeCase("fire-stream-y", "fire_stream", "y", G2, MAP_S, Spec("fire", "fp16", **_FIRE2), "handover", "fire_fused (fire.hip)", differs=False),
    SizeCase("fire-maxpool-x", "fire_maxpool", "x", G2, MAP_POOL, Spec("fire_maxpool", "fp16", 128, 16, 64, pool=True), "handover",
             "three convs + maxpool_nhwc", differs=False),
    SizeCase("fire-expand-y", "fire_expand", "y", G2, MAP_S, Spec("fire_expand", "fp16", 0, 16, 64), "handover", "two convs", differs=False),
    SizeCase("expand-pair-y", "expand_pair", "y", G2, MAP_S, Spec("fire_expand", "fp16", 0, 192, 256), "handover", "two convs",
             note="conv3x3_pair_launch: a three-chunk squeeze has no streaming form"),
    SizeCase("fire-expand-pool-y", "fire_expand", "y", G2, MAP_POOL, Spec("fire_expand", "fp16", 0, 32, 128, pool=True), "refuse", differs=None,
             note="the pooled concat tensor is twice the squeeze tensor's bytes: y always crosses first"),
    SizeCase("fire-sqnext-x", "fire_sqnext", "x", G2, MAP_S, Spec("fire_sqnext", "fp16", 64, 16, 64, 16), "refuse", differs=None),
    SizeCase("fire-dma-x", "fire_expsqnext", "x", G2, MAP_S, Spec("fire_expsqnext", "fp16", 0, 16, 64, 16), "refuse", differs=None,
             note="fire_dma (fire3.hip) below the limit; at it fire_dma and the fire_stream form behind it both decline"),
    SizeCase("chain-y", "chain", "y", G2, MAP_T, Spec("chain", "fp16", 0, 48, 192, 0), "refuse", differs=None, sub=1280,
             virtual={"concat": 7 * 13 * 384 * 2}),
    SizeCase("chain-sqout", "chain", "concat", G2, MAP_T, Spec("chain", "fp16", 0, 48, 192, 48), "refuse",
             note="only sq_out (48 channels, 0.25 GiB) is written; the guard is still the concat extent", differs=None, sub=1280,
             virtual={"concat": 7 * 13 * 384 * 2}),
    # ---- ConvDet's split-K form, conv + 2x2 pool, the stems (output crossing: the per-image input limit needs a 2 GiB image)
    SizeCase("convdet-x", "convdet_splitk", "x", G2, MAP_DET, Conv(768, 72, k=3, relu=False), "handover", "conv3x3_tile, register staging",
             differs=True, sub=8),
    SizeCase("pool2-x", "conv_pool2", "x", G2, MAP_POOL, Conv(64, 64, k=3, pool2="y"), "handover", "conv3x3_tile POOL2, register staging",
             differs=None, sub=32),
    SizeCase("pool2-idx-x", "conv_pool2", "x", G2, MAP_POOL, Conv(64, 64, k=3, pool2="idx"), "handover", "conv3x3_tile POOL2, register staging",
             differs=None, sub=32),
    SizeCase("stem-y", "stem", "y", G2, (19, 236), Spec("stem"), "handover", "stem_strip", differs=None),
    SizeCase("stem-k7-y", "stem", "y", G2, (41, 40), Spec("stem", k=7, cout=96, cpad="VALID", ppad="VALID"), "handover", "stem_strip",
             differs=None),
    SizeCase("stem-sq-y", "stem_sq", "stem_y", G2, (19, 236), Spec("stem_sq", s2=16), "refuse", differs=None,
             note="bounded by the pooled 64-channel stem output, which this launch never writes", virtual={"stem_y": 5 * 59 * 64 * 2}),
    # ---- the generic fallback beyond 4 GiB (conv_algo = generic): picked images only, no limit on either side
    SizeCase("direct-1x1-4g", "conv_direct", "x", G4, MAP_S, Conv(64, 16, conv_algo=1), "runs"),
    SizeCase("direct-3x3-4g", "conv_direct", "x", G4, MAP_S, Conv(64, 16, k=3, conv_algo=1), "runs"),
]
BY_NAME = {c.name: c for c in CASES}

# Launches of the audit with no GPU case here, and why (DESIGN.md repeats this list).
LEFT_OUT = OrderedDict([
    ("fire_chain launches inside a NetPlan at their limit", "a plan whose chain layer reaches 2^31 bytes needs more than 10 GiB of workspace"),
])

# ---- plans (host: created and every layer launchable; GPU: NET_GPU run)
# (arch, dtype, batch, (h, w), option) as tests/net_plan_cases.py; each pair straddles a fused launch's limit:
#   64x64 float16: fire2 / fire3 outputs are 16x16x128x2 bytes per image = 2^31 at batch 32768 (fire_fuse 5: fire3+pool3 reads it);
#   375x1242 float16: fire2's output 94x311x128x2 reaches 2^31 at batch 287; float32 at 144.
NET_PAIRS = [
    ("squeezedet", "f16", (32767, 32768), (64, 64), None),
    ("squeezedet", "f16", (32767, 32768), (64, 64), ("fire_fuse", 5, 0)),
    ("squeezedet", "f16", (286, 287), (375, 1242), ("fire_fuse", 5, 0)),
    ("squeezedet", "f32", (143, 144), (375, 1242), None),
    ("squeezedet_plus", "f16", (100, 200), (375, 1242), None),
]
NET_GPU = [("squeezedet", "f16", 32767, (64, 64), None), ("squeezedet", "f16", 32768, (64, 64), None),
           ("squeezedet", "f16", 32768, (64, 64), ("fire_fuse", 5, 0))]

# ---- ConvDet with the score epilogue (ops.convdet): split-K only; at the limit the call is UNSUPPORTED
CONVDET_SCORED = BY_NAME["convdet-x"]

# ---- conv2d_bwd_filter and WgradPlan: x crosses, dy is narrow (8 channels) and nonzero on the picked images only.
# (name, images, what the call does): the kernel runs on both sides of 2^31 (unsigned offsets) and refuses from 0xfffffff0 bytes.
WGRAD_HW, WGRAD_CIN, WGRAD_COUT, WGRAD_K = MAP_S, 64, 8, 3
_WG_IMG = MAP_S[0] * MAP_S[1] * WGRAD_CIN * 2
WGRAD = [("wgrad-below-2g", (G2 - 1) // _WG_IMG, "runs"), ("wgrad-at-2g", (G2 - 1) // _WG_IMG + 1, "runs"),
         ("wgrad-below-4g", (WGRAD_LIMIT - 1) // _WG_IMG, "runs"), ("wgrad-at-4g", (WGRAD_LIMIT - 1) // _WG_IMG + 1, "refuse")]


def wgrad_x_bytes(n):
    return n * _WG_IMG


def wgrad_picks(n):
    return sorted(set([0, n - 1, min(n - 1, (G2 - 1) // _WG_IMG)] + ([G2 // _WG_IMG] if n * _WG_IMG > G2 else []) +
                      ([min(n - 1, (G4 - 1) // _WG_IMG)] if n * _WG_IMG > G2 + G2 // 2 else [])))


# ---- maxpool_nhwc 3x3/s2 on an input just over 2^32 bytes (pool.hip: 64-bit indices)
POOL_4G = dict(hw=MAP_POOL, c=64, n=G4 // (MAP_POOL[0] * MAP_POOL[1] * 64 * 2) + 1)
