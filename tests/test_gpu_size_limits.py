"""GPU tests of the launches that address a tensor with 32-bit buffer offsets, with that tensor just under and at its limit
(cases, byte arithmetic and the restated guards: tests/size_limit_cases.py; the audit: DESIGN.md, "tensor size limits").

A wrong guard does not fault -- out-of-range buffer reads return zeros, out-of-range stores are dropped -- it leaves wrong
images at the end of a large batch.  So every case runs the launch on the REAL tensor (random everywhere, generated on the
device in the storage type: a wrapped offset reads plausible wrong data, not zeros) and looks at picked images: the first,
the last, the one holding byte 2^31 - 1 of the crossing tensor, the one holding byte 2^31 (and 2^32 - 1).  Only those are
copied to the host.

  below the limit   the fast kernel runs.  The picked images must equal BITWISE the same call on a sub-batch (the picked
                    images, then filler images up to the pixel count that keeps every other dispatch condition: SizeCase.sub),
                    that sub-batch result must differ somewhere from conv_algo = generic (SizeCase.differs says where it does
                    not: the equality then proves addressing only), and the picked images pass the rounding contract.
  at the limit      "handover": the picked images pass the rounding contract (tests/rounding_contract.py, as
                    tests/test_gpu_rounding.py applies it to that launch: the same statistics, caps, MIN_COMPARED, MIN_SHARE);
                    "refuse": SQDET_EUNSUPPORTED, outputs and guards untouched -- called with real tensors of the stated size;
                    "runs": as below the limit.

Outputs live inside canary guards; every test frees its tensors and empties the cache.  No tolerance of this file's own.
The `below` tests stand first.
"""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

from tests import rounding_contract as RC
from tests import size_limit_cases as SL
from tests.fused_launch_cases import TDT
from tests.size_limit_cases import Bwd, Conv
from tests.test_gpu_conv_layouts import _same_bits
from tests.test_gpu_fused_edges import EUNSUPPORTED, OK, Op, _options, _seed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64 * 1024          # bytes of canary either side of an output


def _ops():
    from squeezedet_amd import ops
    return ops


def _gen(shape, dtype, seed):
    """Seeded standard-normal values in the storage type, generated on the device (no host copy, no float32 staging)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=TDT[dtype], device=DEV)


class _Guarded:
    """An output inside GUARD bytes of canary on each side, itself pre-filled with the canary (regenerated from the seed when
    a refusal has to show the whole buffer untouched)."""

    def __init__(self, shape, dtype, seed):
        self.shape, self.dtype, self.seed = tuple(shape), dtype, seed
        self.g = GUARD // SL.ESZ[dtype]
        self.n = int(np.prod(shape))
        self.flat = _gen((2 * self.g + self.n,), dtype, seed)
        assert self.flat.data_ptr() % 256 == 0
        self.front, self.back = self.flat[:self.g].clone(), self.flat[self.g + self.n:].clone()
        self.t = self.flat[self.g:self.g + self.n].view(self.shape)

    def guards_unchanged(self, what):
        _same_bits(self.flat[:self.g], self.front, what + ": guard in front")
        _same_bits(self.flat[self.g + self.n:], self.back, what + ": guard behind")

    def untouched(self, what):
        again = _gen((2 * self.g + self.n,), self.dtype, self.seed)
        same = torch.equal(self.flat.view(torch.int16), again.view(torch.int16))
        del again
        assert same, what + ": the refused call wrote to its output"


class _Measured:
    """Prints wall time and peak device memory of a test body and holds the peak to the cap; frees the cache on the way out."""

    def __init__(self, what, cap=SL.DEVICE_BYTES_CAP):
        self.what, self.cap = what, cap

    def __enter__(self):
        gc.collect()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.time()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        peak, dt = torch.cuda.max_memory_allocated(), time.time() - self.t0
        gc.collect()
        torch.cuda.empty_cache()
        print("%s: %.2f s, peak %.2f GiB" % (self.what, dt, peak / 2.0 ** 30))
        if exc[0] is None:
            assert peak <= self.cap, "%s held %.2f GiB of device memory" % (self.what, peak / 2.0 ** 30)
        return False


def _sub_index(case, picks, n):
    """The sub-batch: the picked images, then the first images that are not picked, case.sub in all."""
    fill = [i for i in range(case.sub + len(picks)) if i not in picks][:case.sub - len(picks)]
    assert len(fill) + len(picks) == case.sub <= n
    return torch.tensor(picks + fill, device=DEV)


def _contract(got_cpu, case_rc, name, dtype, what):
    RC.check(got_cpu, case_rc.ref[name], [e[name] for e in case_rc.emus], dtype, what)


# ------------------------------------------------------------------------------------------------------------- single convs
class _ConvOp:
    def __init__(self, case):
        c, self.case = case.op, case
        rs = np.random.RandomState(_seed("size-limit", case.name))
        rnd = (lambda t: t.half().float()) if c.dtype == "fp16" else (lambda t: t)
        self.w = rnd(torch.from_numpy((rs.randn(c.k, c.k, c.cin, c.cout) * (2.0 / (c.k * c.k * c.cin)) ** 0.5).astype(np.float32)))
        self.b = torch.from_numpy(rs.uniform(-0.5, 0.5, c.cout).astype(np.float32))
        self.packed = _ops().pack_conv_weights(self.w.to(DEV), TDT[c.dtype])
        self.bd = self.b.to(DEV)

    accumulates = False

    def extras(self, shape):
        """The further input tensors of the launch, random everywhere: name -> tensor shaped like y."""
        return {"residual": _gen(shape, self.case.op.dtype, _seed("residual", self.case.name))} if self.case.op.residual else {}

    def run(self, x, out=None, conv_algo=None, idx=None, extras=None):
        """y (and, for the _idx form, the window index in `idx`, allocated when None and kept in self.idx)."""
        c = self.case.op
        with _options(conv_algo=c.conv_algo if conv_algo is None else conv_algo):
            if not c.pool2:
                return _ops().conv2d_nhwc(x, self.packed, self.bd, 1, "SAME", c.relu, out=out, residual=(extras or {}).get("residual"))
            from squeezedet_amd import _lib
            n, h, w, _ = [int(v) for v in x.shape]
            shape = (n, -(-h // 2), -(-w // 2), c.cout)
            y = torch.empty(shape, dtype=x.dtype, device=DEV) if out is None else out
            P = lambda t: C.c_void_p(t.data_ptr())
            tail = (n, h, w, c.cin, c.cout, int(c.relu), _lib.dtype_code(x.dtype), _lib.stream_ptr())
            if c.pool2 == "idx":
                self.idx = torch.empty(shape, dtype=torch.uint8, device=DEV) if idx is None else idx
                rc = _ops().lib().sqdet_conv2d_maxpool2_nhwc_fwd_idx(P(x), P(self.packed.data), P(self.bd), P(y), P(self.idx), *tail)
            else:
                rc = _ops().lib().sqdet_conv2d_maxpool2_nhwc_fwd(P(x), P(self.packed.data), P(self.bd), P(y), *tail)
            assert rc == OK, "%s: code %d: %s" % (self.case.name, rc, _ops().lib().sqdet_last_error())
            return y

    def reference(self, x_cpu, extras=None, prior=None):
        c = self.case.op
        if c.pool2:
            return RC.Case(RC.conv_pool_program(x_cpu.float(), self.w, self.b, 1, "SAME", c.relu, (2, 2, "SAME")), c.dtype)
        res = extras["residual"].float() if c.residual else None
        return RC.Case(RC.conv_program(x_cpu.float(), self.w, self.b, 1, "SAME", c.relu, res=res), c.dtype)


class _BwdOp:
    """conv2d_bwd_data as tests/test_gpu_rounding.py _Dgrad runs and judges it: plain on a dY channel slice, or accumulate +
    relu_of (dx holds the prior gradient when the call starts)."""

    def __init__(self, case):
        c, self.case = case.op, case
        rs = np.random.RandomState(_seed("size-limit", case.name))
        self.w = torch.from_numpy((rs.randn(c.k, c.k, c.cin, c.cout) / (c.k * c.k * c.cout) ** 0.5).astype(np.float32)).half().float()
        self.packed = _ops().PackedConvBwd(self.w.to(DEV), TDT[c.dtype])
        self.accumulates = c.relu_of

    def extras(self, shape):
        return {"relu_of": _gen(shape, self.case.op.dtype, _seed("relu_of", self.case.name))} if self.case.op.relu_of else {}

    def run(self, x, out=None, conv_algo=None, idx=None, extras=None):
        c = self.case.op
        with _options(conv_algo=0 if conv_algo is None else conv_algo):
            return _ops().conv2d_bwd_data(x, self.packed, dx=out, dy_coffset=c.coffset, accumulate=self.accumulates,
                                          relu_of=(extras or {}).get("relu_of"))

    def reference(self, x_cpu, extras=None, prior=None):
        c = self.case.op
        wb, zero = RC.flip_for_bwd_data(self.w), torch.zeros(c.cin)
        dys = x_cpu.float()[..., c.coffset:c.coffset + c.cout]
        if not c.relu_of:
            return RC.Case(RC.conv_program(dys, wb, zero, 1, "SAME", False), c.dtype)
        return RC.Case(RC.conv_program(dys, wb, zero, 1, "SAME", False, res=prior.float(), keep=extras["relu_of"].float() > 0), c.dtype)


def _conv_side(case, n, fast):
    """One side of a conv case.  fast: the kernel named by the case runs (bitwise against the sub-batch); else the hand-over."""
    c, what = case.op, "%s n=%d" % (case.name, n)
    h, w = case.hw
    op = _BwdOp(case) if isinstance(c, Bwd) else _ConvOp(case)
    x = _gen(case.shapes(n)["x"][0], c.dtype, _seed("x", case.name))
    y = _Guarded(case.shapes(n)["y"][0], c.dtype, _seed("y", case.name))
    extras = op.extras(y.shape)
    picks = case.picks(n)
    sub = _sub_index(case, picks, n)
    prior = y.t.index_select(0, sub) if op.accumulates else None      # (the accumulate form: what dx held before the call)
    idx = None
    if c.pool2 == "idx":      # (uint8: a guarded buffer of its own kind)
        g = torch.Generator(device=DEV).manual_seed(_seed("idx", case.name))
        flat = torch.randint(0, 256, (2 * GUARD + y.n,), generator=g, dtype=torch.uint8, device=DEV)
        edges = (flat[:GUARD].clone(), flat[GUARD + y.n:].clone())
        idx = flat[GUARD:GUARD + y.n].view(y.shape)
    op.run(x, out=y.t, idx=idx, extras=extras)
    torch.cuda.synchronize()
    y.guards_unchanged(what)
    if idx is not None:
        assert torch.equal(flat[:GUARD], edges[0]) and torch.equal(flat[GUARD + y.n:], edges[1]), what + ": guards of the window index"
    got = y.t[picks]
    differs = case.differs
    # the tile kernel's two staging paths (LDS-DMA below the limit, registers at it) feed the same MFMAs in the same order: at
    # the limit the picked images are still bitwise those of the sub-batch call, which stages by DMA
    same_kernel = case.launch in ("conv3x3_tile", "conv3x3_tile_slice", "conv_pool2")
    if fast or same_kernel:
        xs = x.index_select(0, sub)
        es = {nm: t.index_select(0, sub) for nm, t in extras.items()}
        ys = op.run(xs, out=prior.clone() if op.accumulates else None, extras=es)
        _same_bits(got, ys[:len(picks)], what + ": picked images against the sub-batch call")
        if idx is not None:
            assert torch.equal(idx[picks], op.idx[:len(picks)]), what + ": window index of the picked images against the sub-batch call"
        if fast and c.conv_algo == 0 and case.differs is not None:
            differs = bool((op.run(xs, out=prior.clone() if op.accumulates else None, conv_algo=1, extras=es) != ys).any())
            print("%s: sub-batch differs from conv_algo = generic: %s" % (what, differs))
    ref = op.reference(x[picks].cpu(), {nm: t[picks].cpu() for nm, t in extras.items()}, None if prior is None else prior[:len(picks)].cpu())
    _contract(got.cpu(), ref, "y", c.dtype, what)
    # (differs False: both kernels sum in the same order on this data -- the equality above then proves addressing only, and the
    # contract on the picked images carries the rest)
    assert differs == case.differs, what


# -------------------------------------------------------------------------------------------------------- fused fire launches
def _fire_side(case, n, mode):
    """mode "fast" (bitwise against the sub-batch, then the contract), "handover" (the contract) or "refuse"."""
    sp, what = case.op, "%s n=%d" % (case.name, n)
    h, w = case.hw
    op = Op(sp)
    x = _gen(sp.in_shape(n, h, w), sp.dtype, _seed("x", case.name))
    bufs = {nm: _Guarded(shape, sp.dtype, _seed("buf", case.name, nm)) for nm, (shape, _) in sp.buffers(n, h, w).items()}
    rc = op.call(x, {nm: b.t for nm, b in bufs.items()}, n, h, w)
    torch.cuda.synchronize()
    if mode == "refuse":
        assert rc == EUNSUPPORTED, "%s: code %d" % (what, rc)
        for nm, b in bufs.items():
            b.untouched("%s %s" % (what, nm))
        return
    assert rc == OK, "%s: code %d: %s" % (what, rc, _ops().lib().sqdet_last_error())
    for nm, b in bufs.items():
        b.guards_unchanged("%s %s" % (what, nm))
    outs = [nm for nm, (_, role) in sp.buffers(n, h, w).items() if role == "out"]
    picks = case.picks(n)
    differs = case.differs
    if mode == "fast":
        xs = x.index_select(0, _sub_index(case, picks, n))
        sub = op.run(xs)
        for nm in outs:
            _same_bits(bufs[nm].t[picks], sub[nm][:len(picks)], "%s %s: picked images against the sub-batch call" % (what, nm))
        if case.differs is not None:      # (None: the entry point has no generic form -- it refuses under conv_algo = generic)
            with _options(conv_algo=1):
                gen = op.run(xs)
            differs = any(bool((gen[nm] != sub[nm]).any()) for nm in outs)
            print("%s: sub-batch differs from conv_algo = generic: %s" % (what, differs))
    first = outs[0]
    from tests.test_gpu_rounding import _program
    ref = RC.Case(_program(sp, x[picks].cpu().float(), op.wt), sp.dtype)
    _contract(bufs[first].t[picks].cpu(), ref, first, sp.dtype, "%s %s" % (what, first))
    assert differs == case.differs, what


def _side(case, n, fast):
    with _Measured("%s n=%d" % (case.name, n)):
        assert case.device_bytes(n) <= SL.DEVICE_BYTES_CAP
        if isinstance(case.op, Conv):
            _conv_side(case, n, fast)
        else:
            _fire_side(case, n, "fast" if fast else case.at_outcome)


@pytest.mark.parametrize("case", SL.CASES, ids=[c.name for c in SL.CASES])
def test_below_the_limit(case):
    """The largest batch whose crossing tensor is under the limit: the fast kernel, its last image included."""
    _side(case, case.below, True)


@pytest.mark.parametrize("case", SL.CASES, ids=[c.name for c in SL.CASES])
def test_at_the_limit(case):
    """One image more: the hand-over is right, the refusal writes nothing, or the kernel does not depend on that tensor's size."""
    _side(case, case.at, case.at_outcome == "runs")


# ------------------------------------------------------------------------------------------- ConvDet with the score epilogue
def test_convdet_scores_below_and_refused_at_the_limit():
    """ops.convdet (preds + det_probs in the split-K kernel's epilogue): below the limit preds are bitwise conv2d_nhwc's (the
    same kernel without the epilogue) and the picked images' preds and scores those of the sub-batch call; at the limit the
    split-K form drops out and the call is UNSUPPORTED -- preds and scores untouched (the plain conv is still right there:
    convdet-x)."""
    from squeezedet_amd import _lib
    case = SL.CONVDET_SCORED
    h, w = case.hw
    op = _ConvOp(case)
    for n in (case.below, case.at):
        with _Measured("convdet-scored n=%d" % n):
            x = _gen((n, h, w, case.op.cin), "fp16", _seed("x", case.name))
            preds = _Guarded((n, h, w, 72), "fp16", _seed("preds"))
            scores = torch.full((2 * GUARD + n * h * w * 9,), -1.0, dtype=torch.float32, device=DEV)
            sview = scores[GUARD:GUARD + n * h * w * 9].view(n, h * w * 9)
            if n == case.at:
                with pytest.raises(_lib.SqdetUnsupported):
                    _ops().convdet(x, op.packed, op.bd, 9, 3, preds=preds.t, scores=sview)
                torch.cuda.synchronize()
                preds.untouched("convdet-scored preds")
                assert float(scores.max()) == -1.0 and float(scores.min()) == -1.0
            else:
                _ops().convdet(x, op.packed, op.bd, 9, 3, preds=preds.t, scores=sview)
                torch.cuda.synchronize()
                preds.guards_unchanged("convdet-scored preds")
                assert float(scores[:GUARD].max()) == -1.0 == float(scores[GUARD + sview.numel():].max())
                picks = case.picks(n)
                xs = x.index_select(0, _sub_index(case, picks, n))
                ps, ss = _ops().convdet(xs, op.packed, op.bd, 9, 3)
                _same_bits(preds.t[picks], ps[:len(picks)], "convdet-scored preds against the sub-batch call")
                assert torch.equal(sview[picks], ss[:len(picks)]) and float(sview[picks].min()) >= 0.0
                _same_bits(preds.t[picks], op.run(xs)[:len(picks)], "convdet-scored preds against conv2d_nhwc")
            del x, preds, scores, sview


# ------------------------------------------------------------------------------------------------------ backward-filter conv
@pytest.mark.parametrize("row", SL.WGRAD, ids=[r[0] for r in SL.WGRAD])
def test_conv_backward_filter_between_2_and_4_gib(row):
    """conv2d_bwd_filter and WgradPlan (bitwise the same) with x on both sides of 2^31 bytes, just under 2^32, and refused from
    0xfffffff0 bytes.  x is random everywhere, dY nonzero on the picked images only: dW and dbias are then those images'
    contribution (a product with a zero dY is an exact zero), judged as tests/test_gpu_rounding.py judges the backward-filter
    conv (RC.WgradCase on the picked images; dW and dbias together)."""
    from squeezedet_amd import _lib
    name, n, outcome = row
    (h, w), cin, cout, k = SL.WGRAD_HW, SL.WGRAD_CIN, SL.WGRAD_COUT, SL.WGRAD_K
    ops = _ops()
    with _Measured("%s n=%d" % (name, n)):
        x = _gen((n, h, w, cin), "fp16", _seed("wgrad-x"))
        picks = SL.wgrad_picks(n)
        dy = torch.zeros((n, h, w, cout), dtype=torch.float16, device=DEV)
        dy[picks] = _gen((len(picks), h, w, cout), "fp16", _seed("wgrad-dy", name))
        dw = torch.full((k, k, cin, cout), 7.0, dtype=torch.float32, device=DEV)
        db = torch.full((cout,), 7.0, dtype=torch.float32, device=DEV)
        if outcome == "refuse":
            assert SL.wgrad_x_bytes(n) >= SL.WGRAD_LIMIT > SL.wgrad_x_bytes(n - 1)
            with pytest.raises(_lib.SqdetUnsupported):
                ops.conv2d_bwd_filter(x, dy, k, cin, cout, dw=dw, db=db)
            torch.cuda.synchronize()
            assert float(dw.min()) == 7.0 == float(dw.max()) and float(db.min()) == 7.0 == float(db.max())
            return
        ops.conv2d_bwd_filter(x, dy, k, cin, cout, dw=dw, db=db)
        dwp, dbp = torch.full_like(dw, float("nan")), torch.full_like(db, float("nan"))
        plan = ops.WgradPlan([(name, (n, h, w, cin, cout, k), dwp, dbp, None, 0.0)])
        plan.partial(name, x, dy)
        plan.reduce(1.0)
        torch.cuda.synchronize()
        assert torch.equal(dw, dwp) and torch.equal(db, dbp), name + ": WgradPlan against conv2d_bwd_filter"
        case = RC.WgradCase(x[picks].cpu().float(), dy[picks].cpu().float(), k)
        flat = lambda d: torch.cat([d["dw"].reshape(-1), d["db"].reshape(-1)])
        ref = RC.Val(*[flat({"dw": getattr(case.ref["dw"], f), "db": getattr(case.ref["db"], f)}) for f in RC.Val.FIELDS])
        m = RC.measure(flat({"dw": dw.cpu(), "db": db.cpu()}), ref, [flat(e) for e in case.emus], "fp32")
        print("%s: %s" % (name, RC.describe(m, "fp32")))
        assert m["compared"] >= min(RC.MIN_COMPARED, ref.want.numel()) and m["share"] >= RC.MIN_SHARE, name
        assert m["outside"] == 0, "%s: %d elements outside the derived bound" % (name, m["outside"])
        assert m["value"] <= m["cap"], "%s: %s" % (name, RC.describe(m, "fp32"))
        del plan, x, dy


# ----------------------------------------------------------------------------------------------------- max-pool beyond 4 GiB
def test_maxpool_on_an_input_over_4_gib():
    """maxpool_nhwc 3x3/s2 SAME on an input just over 2^32 bytes (pool.hip: 64-bit indices): the first image, the last and the
    ones holding bytes 2^31 - 1 and 2^32 - 1 equal the oracle's pool of the same images (a max of stored values: exact)."""
    from oracle import sqdet_oracle as O
    (h, w), c, n = SL.POOL_4G["hw"], SL.POOL_4G["c"], SL.POOL_4G["n"]
    ib = h * w * c * 2
    assert (n - 1) * ib < SL.G4 <= n * ib
    with _Measured("maxpool-4g n=%d" % n):
        x = _gen((n, h, w, c), "fp16", _seed("pool-x"))
        y = _ops().maxpool_nhwc(x, 3, 2, "SAME")
        torch.cuda.synchronize()
        picks = sorted(set([0, (SL.G2 - 1) // ib, SL.G2 // ib, (SL.G4 - 1) // ib, n - 1]))
        want = O.pooling_layer(x[picks].cpu().float(), 3, 2, "SAME").to(torch.float16)
        _same_bits(y[picks].cpu(), want, "maxpool-4g picked images")
        del x, y


# ------------------------------------------------------------------------------------------------------------------ NetPlan
@pytest.mark.parametrize("net", SL.NET_GPU, ids=["%s-%s-b%d-%dx%d-%s" % (a, d, b, s[0], s[1], "default" if o is None else "%s%d" % o[:2])
                                                 for a, d, b, s, o in SL.NET_GPU])
def test_net_plan_at_the_fused_fire_limit(net):
    """SqueezeDet float16 at 64x64: fire2's and fire3's concat tensors are exactly 2^31 bytes at batch 32768.  The plan is
    created, every layer launchable, and runs; image 0 and the last image against oracle/sqdet_oracle.py under the criterion of
    tests/test_gpu_model.py test_native_plan_other_sizes_and_batches_fp16_vs_oracle (_check_layers).  (Before plan creation
    asked the launchers' size-aware predicates, the fire_fuse = 5 plan at 32768 held fire3+pool3 as one launch, whose launcher
    declines a 2^31-byte input: every forward failed with "fused fire no longer eligible".)"""
    from oracle import sqdet_oracle as O
    from tests.test_gpu_model import _check_layers, _model
    arch, dt, batch, (h, w), opt = net
    ops = _ops()
    with _Measured("net %s b%d %s" % (arch, batch, opt)):
        m, mc, params, storage = _model("squeezeDet", torch.float16, 1, (h, w))
        opts = {} if opt is None else {opt[0]: opt[1]}
        with _options(**opts):
            plan = ops.NetPlan(m.NATIVE_ARCH, torch.float16, batch, h, w, mc.CLASSES, mc.ANCHOR_PER_GRID, DEV)
            assert all(plan.layers_launchable())
            plan.set_bn_epsilon(mc.BATCH_NORM_EPSILON)
            for name, t in m.params.items():
                plan.set_param(name, t)
            x = _gen((batch, h, w, 3), "fp16", _seed("net-x", batch))
            preds = _Guarded((batch, plan.gh, plan.gw, plan.out_ch), "fp16", _seed("net-preds"))
            plan.forward(x, preds=preds.t)
            torch.cuda.synchronize()
        preds.guards_unchanged("preds")
        picks = [0, batch - 1]
        ref = O.forward("squeezeDet", params, x[picks].cpu().float(), storage)
        _check_layers(preds.t[picks], ref, torch.float16, "preds of images 0 and %d" % (batch - 1))
        del plan, x, preds
