"""The rounding contract of a conv launch, its float64 reference, CPU emulations of honest float32 accumulation, and the two
checks tests/test_gpu_rounding.py makes of a device result.  No GPU is needed (tests/test_rounding_contract_host.py).

CONTRACT.  Every conv of a launch is  storage(relu?(float32-accumulated conv + float32 bias [+ residual])):  ONE rounding to
the storage type per conv, round-to-nearest-even -- what _conv64 / _finish of tests/test_gpu_conv_layouts.py and fire_ref64 of
tests/fused_launch_cases.py state.  The reference and every emulation see the operands the kernel sees: storage-rounded x, w,
dY, the bias in float32.

CHECKS of a device tensor `got` against a reference Val (exact float64 value `v`, magnitude `mag` = the same conv on |x|, |w|,
|b|, K = additions per output element):

  (a) in_bounds: got lies in [storage(relu?(ex - e)), storage(relu?(ex + e))], e = gamma(K) * mag, gamma(K) = n / (1 - n) with
      n = (K + 1) * 2^-23 (one product rounding and K additions, each within 2^-23 relative whether rounded or truncated; the
      quotient makes the first-order sum rigorous).  Rounding, ReLU and max-pooling are monotone, so no summation order leaves
      the interval.  Where an intermediate tensor is not written out, its interval is carried forward: with d = the larger
      distance from the reference's stored value to an end of its interval, the next conv's e grows by conv(d, |w|) and its mag
      is taken on |x| + d.
  (b) a rate: float16 storage -- the number of elements with non-zero want = storage(relu?(ex)) whose value differs from want;
      float32 storage and the float32 gradients of the backward-filter conv -- r = max |got - relu?(ex)| / mag over the same
      elements.  The same statistic is taken for three emulations of float32 accumulation (ORDERS: torch's float32 conv,
      sequential K chunks of 4, sequential K chunks of 32), each rounding once per conv through the same chain.  The cap is
      4 x the largest emulation value, for the count never below 8 elements.  The three orders differ by up to 7 x among
      themselves; every defect planted in tests/test_rounding_contract_host.py sits 10 x or more above the cap.
      The compared elements (want != 0) must be at least 2000 and at least 25 % of the tensor; the others are covered by (a).

REGIMES.  The same contract away from unit magnitude (tests/test_gpu_rounding_range.py): move() scales the operands of a program
by powers of two -- "sub" (float16 subnormal inputs, intermediates and outputs), "subw" (subnormal weights), "top" (the last
stored tensor overflows to +-inf; everything a conv reads stays finite), "big" (the backward-filter conv on dY x 2^13), or an
integer k (input and biases x 2^k: the exact-scaling property, Fragile).  storage() rounds into the subnormal range and to
+-inf from 65520 on, so the reference and both checks stay as they are; conditions() states what the reference of a moved
case must show before a device value is looked at.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import sqdet_oracle as O
from tests.test_gpu_conv_layouts import _conv64

U = 2.0 ** -23
ORDERS = ("torch", 4, 32)
CAP_FACTOR = 4
CAP_MIN_ELEMENTS = 8
MIN_COMPARED, MIN_SHARE = 2000, 0.25
_NPT = {"fp16": np.float16, "fp32": np.float32}


def gamma(K):
    n = (K + 1) * U
    return n / (1.0 - n)


def storage(v64, dtype):
    """ONE round-to-nearest-even of float64 values to the storage type (NumPy converts float64 straight to float16, without
    a float32 step in between), returned as float64."""
    with np.errstate(over="ignore"):          # from 65520 on a float16 is +-inf: that is the contract, not an accident
        return torch.from_numpy(v64.contiguous().numpy().astype(_NPT[dtype]).astype(np.float64))


def _pads(n, k, s, padding):
    return O.same_pads(n, k, s) if padding == "SAME" else (0, 0)


def maxpool(t, size, stride, padding):
    """TF max-pool of an NHWC tensor of any float type (padding never wins)."""
    pt, pb = _pads(t.shape[1], size, stride, padding)
    pl, pr = _pads(t.shape[2], size, stride, padding)
    tn = F.pad(t.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=float("-inf"))
    return F.max_pool2d(tn, size, stride).permute(0, 2, 3, 1).contiguous()


def im2col(x, k, stride, padding):
    """x [N,H,W,C] -> ([N*Ho*Wo, k*k*C] in (kh, kw, c) order: HWIO kernels reshape to [k*k*C, Cout] as they are, (N, Ho, Wo))."""
    n, h, w, c = x.shape
    pt, pb = _pads(h, k, stride, padding)
    pl, pr = _pads(w, k, stride, padding)
    xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    ho, wo = (xn.shape[2] - k) // stride + 1, (xn.shape[3] - k) // stride + 1
    cols = F.unfold(xn, k, stride=stride).view(n, c, k * k, ho * wo).permute(0, 3, 2, 1)
    return cols.reshape(n * ho * wo, k * k * c).contiguous(), (n, ho, wo)


def flip_for_bwd_data(w):
    """HWIO kernel of the backward-data conv: rot180(W)^T."""
    return torch.flip(w, (0, 1)).permute(0, 1, 3, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- reference
class Val:
    """A tensor of a launch as the reference knows it, all float64: want = the stored value the contract gives, [lo, hi] = the
    interval a device value must lie in, v = the unrounded value relu?(ex), mag = the magnitude sum."""

    FIELDS = ("want", "lo", "hi", "v", "mag")

    def __init__(self, want, lo=None, hi=None, v=None, mag=None):
        self.want = want
        self.lo = want if lo is None else lo
        self.hi = want if hi is None else hi
        self.v = want if v is None else v
        self.mag = want.abs() if mag is None else mag

    @property
    def d(self):
        return torch.maximum(self.hi - self.want, self.want - self.lo)

    def map(self, fn):
        return Val(*[fn(getattr(self, f)) for f in self.FIELDS])

    @property
    def compared(self):
        return self.want != 0


class Reference:
    """The arithmetic of the contract in float64, with the interval of check (a)."""

    def __init__(self, dtype):
        self.dtype = dtype
        self.reads_finite = True        # every tensor a conv has read so far is finite over its whole interval

    def input(self, t):
        return t if isinstance(t, Val) else Val(t.double())

    def conv(self, x, w, b, stride=1, padding="SAME", relu=True, res=None):
        for t in (x,) if res is None else (x, res):
            self.reads_finite = self.reads_finite and all(bool(torch.isfinite(getattr(t, f)).all()) for f in ("want", "lo", "hi"))
        w64, b64 = w.double(), b.double()
        K = w.shape[0] * w.shape[1] * w.shape[2] + 1 + (res is not None)
        ex = _conv64(x.want, w64, b64, stride, padding)
        d = x.d
        mag = _conv64(x.want.abs() + d, w64.abs(), b64.abs(), stride, padding)
        carried = _conv64(d, w64.abs(), torch.zeros_like(b64), stride, padding) if bool((d != 0).any()) else torch.zeros_like(ex)
        if res is not None:
            ex, mag, carried = ex + res.want, mag + res.want.abs() + res.d, carried + res.d
        e = gamma(K) * mag + carried
        f = torch.relu if relu else (lambda t: t)
        return Val(storage(f(ex), self.dtype), storage(f(ex - e), self.dtype), storage(f(ex + e), self.dtype), f(ex), mag)

    def cat(self, vals):
        return Val(*[torch.cat([getattr(v, f) for v in vals], dim=3) for f in Val.FIELDS])

    def pool(self, x, size, stride, padding):
        return x.map(lambda t: maxpool(t, size, stride, padding))

    def mask(self, x, keep):
        return x.map(lambda t: torch.where(keep, t, torch.zeros_like(t)))


# --------------------------------------------------------------------------------------------------------------- emulations
def round_half_toward_zero(v32):
    """float32 -> float16 toward zero (a planted defect), as float32."""
    a = v32.numpy()
    h = a.astype(np.float16)
    bits = h.view(np.uint16).copy()
    over = np.abs(h.astype(np.float32)) > np.abs(a)
    bits[over] -= 1
    return torch.from_numpy(bits.view(np.float16).astype(np.float32))


def matmul_ordered(A, B, order, carry=None):
    """A [M,K] @ B [K,N] in float32; order "torch": one matmul; an int: K in sequential chunks of that many, the running sum
    passed through carry() after each chunk (a planted defect) when given."""
    if order == "torch":
        return A @ B
    K = A.shape[1]
    pad = -K % order
    if pad:
        A, B = F.pad(A, (0, pad)), F.pad(B, (0, 0, 0, pad))
    Ab = A.view(A.shape[0], -1, order).permute(1, 0, 2).contiguous()
    Bb = B.contiguous().view(-1, order, B.shape[1])
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for i in range(Ab.shape[0]):
        acc = acc + Ab[i] @ Bb[i]
        if carry is not None:
            acc = carry(acc)
    return acc


DEFECTS = ("rz", "bias_after", "half_carry", "bf16_w", "half_x")
# defects of range, invisible at unit magnitude: float16 subnormals flushed to zero at the conv's input, in its weights, at
# its store; a store that saturates at +-65504 instead of overflowing to +-inf
RANGE_DEFECTS = ("ftz_in", "ftz_w", "ftz_out", "sat")
H_MIN_NORMAL, H_MAX = 2.0 ** -14, 65504.0


def subnormal16(t):
    """Non-zero and below the smallest normal float16."""
    return (t != 0) & (t.abs() < H_MIN_NORMAL)


def flush16(t):
    return torch.where(subnormal16(t), torch.zeros_like(t), t)


class Emulation:
    """float32 accumulation in one of ORDERS, one rounding per conv.  defect (one of DEFECTS) plants a subtle error, in every
    conv or in the convs whose ordinal (1, 2, ...) is in `at`."""

    def __init__(self, dtype, order, defect=None, at=None):
        self.dtype, self.order, self.defect, self.at, self.n = dtype, order, defect, at, 0

    def input(self, t):
        return t.float()

    def _accumulate(self, x, w, stride, padding, defect):
        if self.order == "torch" and defect != "half_carry":
            pt, pb = _pads(x.shape[1], w.shape[0], stride, padding)
            pl, pr = _pads(x.shape[2], w.shape[1], stride, padding)
            xn = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
            return F.conv2d(xn, w.permute(3, 2, 0, 1).contiguous(), None, stride=stride).permute(0, 2, 3, 1).contiguous()
        cols, (n, ho, wo) = im2col(x, w.shape[0], stride, padding)
        carry = (lambda a: a.half().float()) if defect == "half_carry" else None
        order = 32 if self.order == "torch" else self.order
        return matmul_ordered(cols, w.reshape(-1, w.shape[3]), order, carry).view(n, ho, wo, w.shape[3])

    def conv(self, x, w, b, stride=1, padding="SAME", relu=True, res=None):
        self.n += 1
        defect = self.defect if (self.at is None or self.n in self.at) else None
        w = w.float()
        if defect == "bf16_w":
            w = w.bfloat16().float()
        if defect == "half_x":
            x = x.half().float()
        if defect == "ftz_w":
            w = flush16(w)
        if defect == "ftz_in":
            x = flush16(x)
        acc = self._accumulate(x, w, stride, padding, defect)
        if defect == "bias_after":
            v = (acc.half().float() + b.half().float()).half().float()
        else:
            v = acc + b.float()
        if res is not None:
            v = v + res
        if relu:
            v = torch.relu(v)
        if self.dtype == "fp32":
            return v
        if defect == "rz":
            return round_half_toward_zero(v)
        v = v.half().float()
        if defect == "ftz_out":
            v = flush16(v)
        if defect == "sat":
            v = v.clamp(-H_MAX, H_MAX)
        return v

    def cat(self, vals):
        return torch.cat(vals, dim=3)

    def pool(self, x, size, stride, padding):
        return maxpool(x, size, stride, padding)

    def mask(self, x, keep):
        return torch.where(keep, x, torch.zeros_like(x))


# ------------------------------------------------------------------------------------------------------------------ programs
# A program is a function of an arithmetic (Reference or Emulation) returning {name: tensor of the launch}.
def conv_program(x, w, b, stride=1, padding="SAME", relu=True, res=None, keep=None):
    def run(A):
        y = A.conv(A.input(x), w, b, stride, padding, relu, res=None if res is None else A.input(res))
        return {"y": y if keep is None else A.mask(y, keep)}
    return run


def conv_pool_program(x, w, b, stride, padding, relu, pool, wn=None, bn=None):
    """conv -> max-pool `pool` = (size, stride, padding) [-> the next squeeze]: the stems and the VGG16 conv + pool pairs."""
    def run(A):
        r = {"y": A.pool(A.conv(A.input(x), w, b, stride, padding, relu), *pool)}
        if wn is not None:
            r["sq_out"] = A.conv(r["y"], wn, bn)
        return r
    return run


def fire_program(x, wt, pool=False):
    """tests/fused_launch_cases.py fire_ref64 as a program: x is the module input when wt has "ws", else its squeeze tensor."""
    def run(A):
        r = {}
        sq = A.input(x)
        if "ws" in wt:
            sq = r["sq"] = A.conv(sq, wt["ws"], wt["bs"])
        y = A.cat([A.conv(sq, wt["w1"], wt["b1"]), A.conv(sq, wt["w3"], wt["b3"])])
        r["y"] = A.pool(y, 3, 2, "SAME") if pool else y
        if "wn" in wt:
            r["sq_out"] = A.conv(r["y"], wt["wn"], wt["bn"])
        return r
    return run


class Case:
    """A program evaluated once: the reference and the honest emulations, shared by every test of the case."""

    def __init__(self, program, dtype, orders=ORDERS):
        self.dtype = dtype
        reference = Reference(dtype)
        self.ref = program(reference)
        self.reads_finite = reference.reads_finite
        self.emus = [program(Emulation(dtype, o)) for o in orders]


# ------------------------------------------------------------------------------------------------------------------- regimes
# A regime is a name of REGIMES, or an integer k: input and every bias x 2^k ("sub" is k = -16).  All factors are powers of two.
REGIMES = ("sub", "subw", "top")
SUB, SUBW, TOP_IN, TOP_W, TOP_OUT, TOP_RES, BIG = -16, 12, 8, 7, 15, 13, 13
MIN_SUBNORMAL, TOP_MIN_INF, TOP_MIN_FINITE = 0.5, 0.01, 0.25
# "top" with the last stage one power of two lower (weights x 2^6, bias x 2^14), under the same conditions: for a launch more
# than half of whose last tensor is zero, where the factors of "top" push more elements to inf than they leave finite
TOP14 = "top14"


def scaled(t, k, dtype):
    """t x 2^k, storage-rounded again (the operands are what the kernel sees), as float32."""
    return storage(t.double() * 2.0 ** k, dtype).float()


def on_grid(t, q, dtype):
    """t with the bits dropped that t x 2^-q would lose: every t x 2^k, k >= -q, is then exact in the storage type."""
    return scaled(scaled(t, -q, dtype), q, dtype)


def input_exponent(regime):
    return regime if isinstance(regime, int) else {"sub": SUB, "subw": SUBW, "top": TOP_IN, TOP14: TOP_IN}[regime]


def conv_exponents(regime, stage, last):
    """(weights, bias, output) exponents of a conv in stage `stage` (1, 2, ...) of a launch whose last stage is `last`.
    sub / k: only the biases follow the input.  subw: every conv's weights x 2^-12 under an input x 2^12, so stage i stores
    x 2^(-12 (i - 1)) and its bias carries that factor.  top: x 2^8 up to the last stage, whose weights x 2^7 and bias x 2^15
    make it the only one that stores x 2^15."""
    if isinstance(regime, int) or regime == "sub":
        k = input_exponent(regime)
        return 0, k, k
    if regime == "subw":
        return -SUBW, -SUBW * (stage - 1), -SUBW * (stage - 1)
    assert regime in ("top", TOP14), regime
    lower = regime == TOP14
    return (TOP_W - lower, TOP_OUT - lower, TOP_OUT - lower) if stage == last else (0, TOP_IN, TOP_IN)


def move(regime, x, convs, dtype):
    """x and convs = [(w, b, stage)] in program order, moved into `regime`: (x', [(w', b')]).  None is the unit regime."""
    if regime is None:
        return x, [(w, b) for w, b, _ in convs]
    last = max(st for _, _, st in convs)
    out = []
    for w, b, st in convs:
        kw, kb, _ = conv_exponents(regime, st, last)
        out.append((scaled(w, kw, dtype) if kw else w, b * np.float32(2.0 ** kb)))
    return scaled(x, input_exponent(regime), dtype), out


def conv_keys(wt):
    """[(weight key, bias key, stage)] of the convs of a weight dict, in program order: a stem ("w", then the squeeze "wn") or a
    fire module ("ws" when it starts from the module input, both expands in one stage, then the next squeeze "wn")."""
    if "w" in wt:
        return [("w", "b", 1)] + ([("wn", "bn", 2)] if "wn" in wt else [])
    s = 1 if "ws" in wt else 0
    return ([("ws", "bs", 1)] if s else []) + [("w1", "b1", s + 1), ("w3", "b3", s + 1)] + ([("wn", "bn", s + 2)] if "wn" in wt else [])


def move_weights(regime, x, wt, dtype):
    """move() on a weight dict of tests/fused_launch_cases.py make_weights (or a stem's): (x', wt')."""
    keys = conv_keys(wt)
    x2, moved = move(regime, x, [(wt[kw], wt[kb], st) for kw, kb, st in keys], dtype)
    out = {}
    for (kw, kb, _), (w, b) in zip(keys, moved):
        out[kw], out[kb] = w, b
    return x2, out


def residual_exponent(regime):
    """The exponent of the residual (the prior dx) of a single conv: that of the conv's output -- but 2^13 in "top", the largest
    power of two at which a randn residual (|r| < 7.9) stays finite: at the output's 2^15 one element in 22 of the residual
    would itself be +-inf, and no conv may read a non-finite value."""
    return 0 if regime is None else TOP_RES if regime == "top" else conv_exponents(regime, 1, 1)[2]


def conditions(regime, case, written, x=None, weights=()):
    """What the REFERENCE of a moved case must show, asserted before any device value is looked at.  written: the names of the
    tensors the launch writes, the last one last; x, weights: the moved input and stored weights (subw).  Returns the figures."""
    out = {}
    for nm in written:
        ref = case.ref[nm]
        n, share, ok = honest(ref)
        assert ok, "%s: only %d compared elements (%.1f %% of the tensor)" % (nm, n, 100 * share)
        if regime == "sub":
            out[nm] = float(subnormal16(ref.want[ref.compared]).double().mean())
            assert out[nm] >= MIN_SUBNORMAL, "%s: only %.1f %% of the compared elements are subnormal" % (nm, 100 * out[nm])
    if regime == "subw":
        assert x is not None and bool(torch.isfinite(x).all()), "the scaled input overflows"
        out["w"] = min(float(subnormal16(w).double().mean()) for w in weights)
        assert out["w"] >= MIN_SUBNORMAL, "only %.1f %% of a conv's weights are subnormal and non-zero" % (100 * out["w"])
    if regime in ("top", TOP14):
        assert case.reads_finite, "a conv reads a non-finite value"
        for nm in written[:-1]:
            ref = case.ref[nm]
            assert all(bool(torch.isfinite(getattr(ref, f)).all()) for f in ("want", "lo", "hi")), nm + " is written before the last stage"
        want = case.ref[written[-1]].want
        out["inf"] = float(torch.isinf(want).double().mean())
        out["finite"] = float((torch.isfinite(want) & (want != 0)).double().mean())
        assert out["inf"] >= TOP_MIN_INF and out["finite"] >= TOP_MIN_FINITE, \
            "%s: %.2f %% infinite, %.1f %% finite and non-zero" % (written[-1], 100 * out["inf"], 100 * out["finite"])
    return out


class Fragile:
    """An arithmetic that tells where scaling a float16 launch's input and biases by 2^k need not scale its result by exactly 2^k.
    A power of two commutes with every rounding that neither underflows nor overflows, so a stored element is safe unless it can
    be float16 subnormal or overflow in one of the two runs -- read off the reference's interval for it -- or a conv computed it
    from an element that is not safe.  A tensor is (Val, upstream, own): `upstream` marks elements computed from an unsafe one;
    `own` the elements that may themselves round differently.  A test takes `upstream` for the tensor it compares (what the
    device stored tells the rest) and `own` for the share of a hidden tensor that is unsafe."""

    def __init__(self, k):
        self.ref, self.k = Reference("fp16"), k

    def _own(self, v):
        small, big = H_MIN_NORMAL * 2.0 ** max(-self.k, 0), 65520.0 * 2.0 ** min(-self.k, 0)
        return (((v.lo != 0) | (v.hi != 0)) & (v.lo < small) & (v.hi > -small)) | (torch.maximum(v.lo.abs(), v.hi.abs()) >= big)

    def input(self, t):
        """An operand is safe: the test hands over values whose scaling is exact (on_grid)."""
        v = self.ref.input(t)
        none = torch.zeros_like(v.want, dtype=torch.bool)
        return v, none, none

    def conv(self, x, w, b, stride=1, padding="SAME", relu=True, res=None):
        v = self.ref.conv(x[0], w, b, stride, padding, relu, None if res is None else res[0])
        unsafe = (x[1] | x[2]).any(dim=3, keepdim=True).double()
        k = w.shape[0]
        up = _conv64(unsafe, torch.ones(k, k, 1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), stride, padding) > 0
        up = up.expand_as(v.want)
        if res is not None:
            up = up | res[1] | res[2]
        return v, up, self._own(v)

    def cat(self, vals):
        return (self.ref.cat([v[0] for v in vals]),) + tuple(torch.cat([v[i] for v in vals], dim=3) for i in (1, 2))

    def pool(self, x, size, stride, padding):
        return (self.ref.pool(x[0], size, stride, padding),) + tuple(maxpool(x[i].double(), size, stride, padding) > 0 for i in (1, 2))

    def mask(self, x, keep):
        return (self.ref.mask(x[0], keep),) + tuple(x[i] & keep for i in (1, 2))


def scales_exactly(unit, moved, k, upstream=None):
    """moved against 2^k * unit, bit for bit: (elements that differ among the compared, share of the tensor left out by the
    device's own values, share of the tensor compared).  float16 tensors: an element is left out when it is not finite or is
    subnormal in one of the runs, and not compared either when it is in `upstream`; other types: every element is compared."""
    u, m = unit.double(), moved.double()
    ok = torch.ones_like(u, dtype=torch.bool)
    if unit.dtype == torch.float16:
        ok = torch.isfinite(u) & torch.isfinite(m) & ~subnormal16(u) & ~subnormal16(m)
    left = 1.0 - float(ok.double().mean())
    if upstream is not None:
        ok = ok & ~upstream
    return int(((m != u * 2.0 ** k) & ok).sum()), left, float(ok.double().mean())


# ----------------------------------------------------------------------------------------------------- backward-filter conv
class WgradCase:
    """dW [k,k,cin,cout] = scale * sum_pixels x (x) dY + decay * W and dbias = scale * sum_pixels dY of a stride-1 SAME conv,
    float32 results whatever the storage type of x / dY: K = pixels + 2 additions per element."""

    def __init__(self, x, dy, k, w=None, decay=0.0, scale=1.0, orders=ORDERS):
        self.dtype = "fp32"
        cols, _ = im2col(x.float(), k, 1, "SAME")
        dyf = dy.float().reshape(-1, dy.shape[3])
        cin, cout = x.shape[3], dy.shape[3]
        K = cols.shape[0] + 2
        A64, B64 = cols.double().t().contiguous(), dyf.double()

        def val(ex, mag):
            e = gamma(K) * mag
            return Val(storage(ex, "fp32"), storage(ex - e, "fp32"), storage(ex + e, "fp32"), ex, mag)

        wdec = decay * w.double().reshape(-1, cout) if w is not None else torch.zeros(1, dtype=torch.float64)
        self.ref = {"dw": val(scale * (A64 @ B64) + wdec, scale * (A64.abs() @ B64.abs()) + wdec.abs()),
                    "db": val(scale * B64.sum(0, keepdim=True), scale * B64.abs().sum(0, keepdim=True))}
        self.ref = {nm: v.map(lambda t: t.reshape((k, k, cin, cout) if nm == "dw" else (cout,))) for nm, v in self.ref.items()}
        self.emus = []
        At, ones = cols.t().contiguous(), torch.ones(1, cols.shape[0])
        for o in orders:
            dw = matmul_ordered(At, dyf, o) * np.float32(scale)
            if w is not None:
                dw = dw + np.float32(decay) * w.float().reshape(-1, cout)
            db = matmul_ordered(ones, dyf, o) * np.float32(scale)
            self.emus.append({"dw": dw.view(k, k, cin, cout), "db": db.view(cout)})


# -------------------------------------------------------------------------------------------------------------------- checks
def out_of_bounds(got, ref):
    """(a): the number of elements outside [lo, hi] (a NaN is outside)."""
    g = got.double()
    return int((~((g >= ref.lo) & (g <= ref.hi))).sum())


def statistic(got, ref, dtype):
    """(b): float16 -- the number of compared elements that differ from want; float32 -- max |got - v| / mag over them."""
    g, m = got.double(), ref.compared
    if dtype == "fp16":
        return int(((g != ref.want) & m).sum())
    if not bool(m.any()):
        return 0.0
    r = ((g - ref.v).abs() / ref.mag)[m]
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def cap(emulated, dtype):
    top = CAP_FACTOR * max(emulated)
    return max(top, CAP_MIN_ELEMENTS) if dtype == "fp16" else top


def honest(ref):
    """The conditions that keep (b) honest: (compared elements, their share of the tensor, whether both are enough)."""
    n, tot = int(ref.compared.sum()), ref.want.numel()
    return n, n / tot, n >= MIN_COMPARED and n >= MIN_SHARE * tot


def measure(got, ref, emus, dtype):
    """Every figure of the two checks for one tensor: dict(outside, value, emulated, cap, compared, share, honest)."""
    n, share, ok = honest(ref)
    em = [statistic(e, ref, dtype) for e in emus]
    return dict(outside=out_of_bounds(got, ref), value=statistic(got, ref, dtype), emulated=em, cap=cap(em, dtype), compared=n,
                share=share, honest=ok)


def describe(m, dtype):
    if dtype == "fp16":
        return "%d of %d changed (%.3f %%), emulations %s, cap %d; %d outside the bound" % (
            m["value"], m["compared"], 100.0 * m["value"] / max(m["compared"], 1), m["emulated"], m["cap"], m["outside"])
    return "r %.3g, emulations %s, cap %.3g over %d elements; %d outside the bound" % (
        m["value"], ["%.3g" % v for v in m["emulated"]], m["cap"], m["compared"], m["outside"])


def check(got, ref, emus, dtype, what):
    """Asserts (a), (b) and the honesty conditions for one device tensor (on the CPU); returns measure()'s figures."""
    assert tuple(got.shape) == tuple(ref.want.shape), "%s: shape %r, reference %r" % (what, tuple(got.shape), tuple(ref.want.shape))
    m = measure(got, ref, emus, dtype)
    print("%s: %s" % (what, describe(m, dtype)))
    assert m["honest"], "%s: only %d compared elements (%.1f %% of the tensor)" % (what, m["compared"], 100 * m["share"])
    assert m["outside"] == 0, "%s: %d elements outside the derived bound" % (what, m["outside"])
    assert m["value"] <= m["cap"], "%s: %s" % (what, describe(m, dtype))
    return m
