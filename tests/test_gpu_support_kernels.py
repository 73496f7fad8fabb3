"""GPU tests of the small kernels that feed the ResNet50 path and the image input, at their edges: squeezedet_amd/csrc/bn.hip
(fold_bn_kernel, fold_bn_bwd_kernel + fold_bn_bwd_finish_kernel, the two *_many kernels, subsample_kernel) and
squeezedet_amd/csrc/preproc.hip (preprocess_kernel).

Every reference is computed here, on the CPU, in float64 (NumPy, or torch-CPU float64 autograd for the fold backward), from the
same input bits the kernel gets; none calls the library.  Preprocessing is the one exception: its specification is cv2's float32
algorithm, so its reference is oracle/preproc_oracle.py.  The references, the input generators, the bounds and the comparison
functions are plain functions of this module so that tests/test_support_kernels_host.py can check them -- and turn them on
deliberately wrong outputs -- without a GPU.  Outputs are slices of larger NaN-filled buffers (float16 preprocessing: a sentinel
bit pattern), handed to the library entry directly (ops.lib()), and every cell outside the slice must keep its sentinel.

Bounds (u = 2^-24, the float32 unit roundoff; a device sqrtf / divide may be one ulp = 2 u off correct rounding):

  fold forward   inv = gamma / sqrtf(var + eps): add (u, halved by the root), sqrtf (2 u), divide (2 u) = 4.5 u; wf = w * inv one
                 more: 5.5 u, asserted at 6 u |wf|.  bf = (cb - mean) * inv + beta: subtract, inv, multiply = 6.5 u on the
                 product, one add on the sum: asserted at 8 u (|(cb - mean) * inv| + |beta|).
  fold backward  dw = dwf * (gamma * (1 / sqrtf(var + eps))): 0.5 + 2 + 2 + 1 + 1 = 6.5 u, asserted at 8 u |dw|.
                 dgamma = r * (sum_rows(dwf * w) + (cb - mean) * dbf), the addition tree as sum_real_bound of
                 tests/test_gpu_train_kernels.py counts its own: 1 product, at most 8 additions per thread and row block, 3 LDS
                 additions, nblocks sequential additions, 2 operations of the conv-bias term and its addition, r (4.5 -> 5), the
                 last multiply: n = nblocks + 21 roundings, each applied to the sum of magnitudes S = sum |dwf * w| +
                 |(cb - mean) * dbf|: |error| <= n u / (1 - n u) * r * S.

Measured on an MI355X, worst error / bound over the elements of a case (the three parameter draws of a forward case: ordinary,
edge table, eps = 0; backward: without / with a conv bias):

  fold forward (k, cin, cout)   wf / 6 u |wf|   bf / 8 u (...)        fold backward     dw / 8 u |dw|    dgamma / its bound (n)
  (1, 1, 4)       bias          0.313           0.209                 (1, 1, 4)         0.097 / 0.232    0.011 / 0.040  (22)
  (1, 3, 68)      -             0.367           0.209                 (1, 3, 68)        0.273 / 0.301    0.094 / 0.116  (22)
  (3, 24, 40)     bias          0.365           0.236                 (1, 33, 64)       0.281 / 0.380    0.055 / 0.069  (23)
  (3, 24, 40)     -             0.380           0.200                 (3, 20, 72)       0.335 / 0.347    0.017 / 0.021  (27)
  (3, 5, 64)      bias          0.382           0.373                 (3, 512, 512)     0.369 / 0.406    0.003 / 0.002  (165)
  (1, 4100, 1028) bias          0.459           0.367

(wf 0.459 x 6 u = 2.8 u and dw 0.406 x 8 u = 3.2 u: what correctly rounded float32 operations give -- the float32 NumPy restatement
uses at most 3.5 u and 4.5 u.)  General preprocessing cases, share of elements equal to the oracle's: 1242 -> 177, 53 -> 259,
640 -> 1242 and the 7.3x vertical reduction all 1.00000 (max abs error 0); float16 is bitwise the float32 output's .half() in
every case.

Cases -> paths:
  second grid-stride pass         fold forward (1, 4100, 1028) (1 053 700 float4 > 4096 x 256); subsample "cap" (stride 2,
                                  2 105 350 vectors > 8192 x 256), float32 and float16
  conv-bias term of dgamma        every FOLD_BWD_SHAPES case with bias = True; the plan tests mix None / tensor
  rows < 4, rows 1, rows % 32 = 1 fold backward (1, 3, 68), (1, 1, 4), (1, 33, 64); cout 4 / 64 / 68 the same three
  in-place fold forward           every test_fold_batchnorm_* case (w_folded == w_hwio through ops.lib())
  in-place fold backward          every test_fold_batchnorm_bwd_* case (dw == dw_folded)
  one-item / 21-item plans        test_fold_bwd_plan_one_item, test_fold_bwd_plan_21_items (single-workgroup items first, last
                                  and between the 3 x 3 x 512 x 512 ones)
  8-byte vector stores            preprocessing Wd = 256 (both types, even offsets), float32 every even Wd at an even offset
  float16 dword stores            Wd = 258 at an element offset of 2 (every second row; the others are 8-byte aligned)
  scalar stores                   odd Wd (every second float16 row is 2-byte aligned only), Wd < 4, odd element offsets
  masked tail load                image 2's last pixels in every preprocessing case (N = 3); test_preprocess_trailing_bytes
  rejections                      fold forward cout = 6; subsample float16 c = 4

No defect was found: every case passed on the kernels as they were, bn.hip and preproc.hip are unchanged.  No input class
had to be dropped in any section.
"""
import numpy as np
import pytest
import torch

from oracle import preproc_oracle as PO
from oracle import resnet_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24          # float32 unit roundoff
GUARD = 64                # sentinel cells in front of and behind every output slice (256 bytes of float32: slices stay 16-byte aligned)
FOLD_CAP_VECS = 4096 * 256      # bn.hip:41  `if (blocks > 4096) blocks = 4096;`  x 256 threads, one float4 each
SUB_CAP_VECS = 8192 * 256       # bn.hip:197 `if (blocks > 8192) blocks = 8192;`  x 256 threads, one 16-byte vector each
FB_ROWS = 32                    # bn.hip:57  rows of a fold_bn_bwd_kernel workgroup
MEANS = [103.939, 116.779, 123.68]


def _ops():
    from squeezedet_amd import ops
    return ops


def _bits(a):
    """The array's bit patterns (so that -0 != +0); every NaN compares equal to every NaN."""
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    u = a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    if a.dtype.kind == "f":
        u[np.isnan(a)] = np.iinfo(u.dtype).max
    return u


def _same_bits(got, ref, what=""):
    g, r = _bits(got), _bits(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, "%s: shape / dtype %s %s vs %s %s" % (what, g.shape, g.dtype, r.shape, r.dtype)
    if not np.array_equal(g, r):
        bad = np.flatnonzero(g.reshape(-1) != r.reshape(-1))
        i = int(bad[0])
        gv = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got).reshape(-1)[i]
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r" % (what, bad.size, g.size, i, gv, np.asarray(ref).reshape(-1)[i]))


def _worst(err, bound):
    """Largest error / bound; where the bound is 0 (a zero gamma) the error must be 0."""
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(ratio)) if ratio.size else 0.0


def _guarded(n, dtype=torch.float32):
    """(buffer, its slice [GUARD, GUARD + n)): NaN everywhere."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, what):
    assert bool(torch.isnan(buf[:GUARD]).all()), "%s: a cell in front of the slice was written" % what
    assert bool(torch.isnan(buf[GUARD + n:]).all()), "%s: a cell behind the slice was written" % what


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================== 1. sqdet_fold_batchnorm
# (shape (k, cin, cout), conv bias)
FOLD_CASES = [((1, 1, 4), True), ((1, 3, 68), False), ((3, 24, 40), True), ((3, 24, 40), False), ((3, 5, 64), True), ((1, 4100, 1028), True)]
FOLD_KINDS = ["ordinary", "edges", "eps0"]
# the edge table, entry i on channel i % cout: var = 0 (eps > 0), gamma < 0, gamma = 0, mean = 0, large |mean|
FOLD_EDGES = [{"var": 0.0}, {"gamma": -0.75}, {"gamma": 0.0}, {"mean": 0.0}, {"mean": -12345.678}]
FOLD_W_ULPS, FOLD_B_ULPS = 6.0, 8.0


def fold_inputs(shape, with_bias, kind):
    """float32 w [k,k,cin,cout], gamma / var in [0.5, 1.5], beta / mean / conv bias normal; kind "edges": FOLD_EDGES planted in the
    first channels; "eps0": the ordinary draw with eps = 0.  Returns (dict of arrays, eps as the float32 the library receives)."""
    k, cin, cout = shape
    rs = np.random.RandomState(k * 1000003 + cin * 1009 + cout + (7 if with_bias else 0))
    d = {"w": rs.randn(k, k, cin, cout).astype(np.float32), "gamma": rs.uniform(0.5, 1.5, cout).astype(np.float32),
         "var": rs.uniform(0.5, 1.5, cout).astype(np.float32), "beta": rs.randn(cout).astype(np.float32),
         "mean": rs.randn(cout).astype(np.float32), "cb": rs.randn(cout).astype(np.float32) if with_bias else None}
    if kind == "edges":
        for i, e in enumerate(FOLD_EDGES):
            for name, v in e.items():
                d[name][i % cout] = v
    return d, float(np.float32(0.0 if kind == "eps0" else R.BN_EPS))


def fold_reference(d, eps):
    """float64: (wf, bf, bound on |wf error|, bound on |bf error|)."""
    f = lambda a: a.astype(np.float64)
    inv = f(d["gamma"]) / np.sqrt(f(d["var"]) + eps)
    cb = f(d["cb"]) if d["cb"] is not None else 0.0
    wf, p = f(d["w"]) * inv, (cb - f(d["mean"])) * inv
    bf = p + f(d["beta"])
    return wf, bf, FOLD_W_ULPS * U32 * np.abs(wf), FOLD_B_ULPS * U32 * (np.abs(p) + np.abs(f(d["beta"])))


def fold_restatement32(d, eps):
    """fold_bn_kernel's expressions in float32 NumPy (correctly rounded sqrt and divide)."""
    f1 = np.float32
    inv = d["gamma"] / np.sqrt(d["var"] + f1(eps))
    cb = d["cb"] if d["cb"] is not None else np.zeros_like(d["mean"])
    wf, bf = d["w"] * inv, (cb - d["mean"]) * inv + d["beta"]
    assert wf.dtype == np.float32 and bf.dtype == np.float32
    return wf, bf


def check_fold(wf, bf, d, eps, what=""):
    """wf / bf (float32 arrays) against the float64 reference within the derived bounds; returns the worst error / bound of each."""
    rw, rb, bw, bb = fold_reference(d, eps)
    assert wf.shape == rw.shape and bf.shape == rb.shape and wf.dtype == np.float32 and bf.dtype == np.float32
    assert np.isfinite(wf).all() and np.isfinite(bf).all(), "%s: a non-finite output (an unwritten cell?)" % what
    ew, eb = np.abs(wf.astype(np.float64) - rw), np.abs(bf.astype(np.float64) - rb)
    qw, qb = _worst(ew, bw), _worst(eb, bb)
    assert qw <= 1.0, "%s: wf error is %g of its bound" % (what, qw)
    assert qb <= 1.0, "%s: bf error is %g of its bound" % (what, qb)
    return qw, qb


def _fold_call(w_t, d_t, eps, wf_t, bf_t, shape):
    from squeezedet_amd import _lib
    k, cin, cout = shape
    _lib.check(_lib.lib().sqdet_fold_batchnorm(_ptr(w_t), _ptr(d_t["cb"]), _ptr(d_t["gamma"]), _ptr(d_t["beta"]), _ptr(d_t["mean"]),
                                               _ptr(d_t["var"]), eps, _ptr(wf_t), _ptr(bf_t), k, cin, cout, _lib.stream_ptr()),
               "sqdet_fold_batchnorm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", FOLD_CASES, ids=["%dx%dx%d_%s" % (s + ("bias" if b else "nobias",)) for s, b in FOLD_CASES])
def test_fold_batchnorm_against_float64_guards_and_in_place(case):
    shape, with_bias = case
    k, cin, cout = shape
    n = k * k * cin * cout
    for kind in FOLD_KINDS:
        d, eps = fold_inputs(shape, with_bias, kind)
        d_t = {name: (_t(v) if v is not None else None) for name, v in d.items()}
        wbuf, wf = _guarded(n)
        bbuf, bf = _guarded(cout)
        assert wf.data_ptr() % 16 == 0
        _fold_call(d_t["w"], d_t, eps, wf, bf, shape)
        _guards_intact(wbuf, n, "w_folded %s %s" % (shape, kind))
        _guards_intact(bbuf, cout, "b_folded %s %s" % (shape, kind))
        got_w, got_b = wf.cpu().numpy().reshape(d["w"].shape), bf.cpu().numpy()
        qw, qb = check_fold(got_w, got_b, d, eps, "%s %s" % (shape, kind))
        print("FOLD %-16s %-5s %-8s wf %.3f of 6u  bf %.3f of 8u" % (shape, "bias" if with_bias else "-", kind, qw, qb))
        # in place: w_folded == w_hwio
        ibuf, iw = _guarded(n)
        iw.copy_(d_t["w"].reshape(-1))
        b2buf, b2 = _guarded(cout)
        _fold_call(iw, d_t, eps, iw, b2, shape)
        _guards_intact(ibuf, n, "in-place w %s %s" % (shape, kind))
        _guards_intact(b2buf, cout, "in-place b %s %s" % (shape, kind))
        _same_bits(iw, wf, "in-place wf %s %s" % (shape, kind))
        _same_bits(b2, bf, "in-place bf %s %s" % (shape, kind))
        # and the tensor-level entry gives the same bits
        ow, ob = _ops().fold_batchnorm(d_t["w"], d_t["cb"], d_t["gamma"], d_t["beta"], d_t["mean"], d_t["var"], eps)
        _same_bits(ow.reshape(-1), wf, "ops.fold_batchnorm wf")
        _same_bits(ob, bf, "ops.fold_batchnorm bf")


def test_fold_batchnorm_rejects_cout_not_a_multiple_of_four():
    from squeezedet_amd import _lib
    shape = (3, 5, 6)
    d = {name: torch.rand(6, device=DEV) + 0.5 for name in ("gamma", "beta", "mean", "var", "cb")}
    w = torch.randn(3, 3, 5, 6, device=DEV)
    wbuf, wf = _guarded(w.numel())
    bbuf, bf = _guarded(6)
    with pytest.raises(_lib.SqdetUnsupported):
        _fold_call(w, d, float(np.float32(R.BN_EPS)), wf, bf, shape)
    torch.cuda.synchronize()
    assert bool(torch.isnan(wbuf).all()) and bool(torch.isnan(bbuf).all())


# ================================================================== 2. sqdet_fold_batchnorm_bwd, sqdet_fold_batchnorm_bwd_many
FOLD_BWD_SHAPES = [(1, 1, 4), (1, 3, 68), (1, 33, 64), (3, 20, 72), (3, 512, 512)]
FOLD_BWD_DW_ULPS = 8.0
FOLD_BWD_EPS = float(np.float32(R.BN_EPS))


def fold_bwd_inputs(shape, with_bias, seed=0):
    k, cin, cout = shape
    rs = np.random.RandomState(k * 1000003 + cin * 1009 + cout + (7 if with_bias else 0) + 31 * seed)
    return {"w": rs.randn(k, k, cin, cout).astype(np.float32), "dwf": rs.randn(k, k, cin, cout).astype(np.float32),
            "dbf": rs.randn(cout).astype(np.float32), "gamma": rs.uniform(0.5, 1.5, cout).astype(np.float32),
            "var": rs.uniform(0.5, 1.5, cout).astype(np.float32), "mean": rs.randn(cout).astype(np.float32),
            "cb": rs.randn(cout).astype(np.float32) if with_bias else None}


def fold_bwd_nblocks(shape):
    return -(-(shape[0] * shape[0] * shape[1]) // FB_ROWS)


def fold_bwd_reference(d, eps):
    """torch-CPU float64 autograd on wf = w * gamma * r, bf = (cb - mean) * gamma * r + beta: (dw, dgamma, dbeta) float64."""
    f = lambda a: torch.from_numpy(a).double()
    w, gamma = f(d["w"]).requires_grad_(True), f(d["gamma"]).requires_grad_(True)
    beta = torch.zeros_like(gamma).requires_grad_(True)
    r = 1.0 / torch.sqrt(f(d["var"]) + eps)
    cb = f(d["cb"]) if d["cb"] is not None else torch.zeros_like(r)
    wf, bf = w * gamma * r, (cb - f(d["mean"])) * gamma * r + beta
    ((wf * f(d["dwf"])).sum() + (bf * f(d["dbf"])).sum()).backward()
    return w.grad.numpy(), gamma.grad.numpy(), beta.grad.numpy()


def fold_bwd_closed_form(d, eps):
    """The same gradients from their formulas in float64 NumPy, and the sum of magnitudes S the dgamma bound is applied to:
    (dw, dgamma, dbeta, r, S)."""
    f = lambda a: a.astype(np.float64)
    cout = d["w"].shape[-1]
    r = 1.0 / np.sqrt(f(d["var"]) + eps)
    cb = f(d["cb"]) if d["cb"] is not None else 0.0
    prod = (f(d["dwf"]) * f(d["w"])).reshape(-1, cout)
    term = (cb - f(d["mean"])) * f(d["dbf"])
    return f(d["dwf"]) * (f(d["gamma"]) * r), r * (prod.sum(axis=0) + term), f(d["dbf"]), r, np.abs(prod).sum(axis=0) + np.abs(term)


def fold_bwd_bounds(d, eps):
    """(bound on |dw error| per element, bound on |dgamma error| per channel): see the module docstring."""
    dw, _, _, r, S = fold_bwd_closed_form(d, eps)
    k, _, cin, cout = d["w"].shape
    n = fold_bwd_nblocks((k, cin, cout)) + 21
    return FOLD_BWD_DW_ULPS * U32 * np.abs(dw), n * U32 / (1.0 - n * U32) * r * S


def fold_bwd_restatement32(d, eps, drop_bias_term=False, drop_last_block=False):
    """fold_bn_bwd_kernel + fold_bn_bwd_finish_kernel in float32 NumPy, in the kernels' order: per row block of 32 the four row
    partitions rp, rp + 4, ... summed ((p0 + p1) + p2) + p3, the blocks added in order.  The two flags produce the wrong
    results the host test feeds to check_fold_bwd."""
    f1 = np.float32
    cout = d["w"].shape[-1]
    w, g = d["w"].reshape(-1, cout), d["dwf"].reshape(-1, cout)
    rows = w.shape[0]
    rinv = f1(1) / np.sqrt(d["var"] + f1(eps))
    dw = g * (d["gamma"] * rinv)
    nblocks = -(-rows // FB_ROWS)
    tot = np.zeros(cout, f1)
    for b in range(nblocks - (1 if drop_last_block else 0)):
        r0, r1 = b * FB_ROWS, min(rows, (b + 1) * FB_ROWS)
        part = []
        for rp in range(4):
            s = np.zeros(cout, f1)
            for row in range(r0 + rp, r1, 4):
                s = s + g[row] * w[row]
            part.append(s)
        tot = tot + (((part[0] + part[1]) + part[2]) + part[3])
    cb = d["cb"] if d["cb"] is not None else np.zeros(cout, f1)
    term = np.zeros(cout, f1) if drop_bias_term else (cb - d["mean"]) * d["dbf"]
    dgamma = rinv * (tot + term)
    assert dw.dtype == f1 and dgamma.dtype == f1
    return dw.reshape(d["w"].shape), dgamma, d["dbf"].copy()


def check_fold_bwd(dw, dgamma, dbeta, d, eps, what=""):
    """float32 outputs against the float64 autograd reference within the derived bounds, dbeta bitwise dbf; returns the worst
    error / bound of dw and dgamma."""
    rw, rg, rb = fold_bwd_reference(d, eps)
    bw, bg = fold_bwd_bounds(d, eps)
    assert dw.dtype == np.float32 and dgamma.dtype == np.float32 and dw.shape == rw.shape and dgamma.shape == rg.shape
    assert np.isfinite(dw).all() and np.isfinite(dgamma).all(), "%s: a non-finite output (an unwritten cell?)" % what
    _same_bits(dbeta, d["dbf"], "%s dbeta" % what)
    assert np.array_equal(rb, d["dbf"].astype(np.float64))
    qw = _worst(np.abs(dw.astype(np.float64) - rw), bw)
    qg = _worst(np.abs(dgamma.astype(np.float64) - rg), bg)
    assert qw <= 1.0, "%s: dw error is %g of its bound" % (what, qw)
    assert qg <= 1.0, "%s: dgamma error is %g of its bound" % (what, qg)
    return qw, qg


def _fold_bwd_call(d_t, dwf_t, dw_t, dg_t, db_t, ws_t, shape):
    from squeezedet_amd import _lib
    k, cin, cout = shape
    _lib.check(_lib.lib().sqdet_fold_batchnorm_bwd(_ptr(d_t["w"]), _ptr(dwf_t), _ptr(d_t["dbf"]), _ptr(d_t["cb"]), _ptr(d_t["gamma"]),
                                                   _ptr(d_t["mean"]), _ptr(d_t["var"]), FOLD_BWD_EPS, _ptr(dw_t), _ptr(dg_t), _ptr(db_t),
                                                   _ptr(ws_t), k, cin, cout, _lib.stream_ptr()), "sqdet_fold_batchnorm_bwd")
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", FOLD_BWD_SHAPES, ids=["%dx%dx%d" % s for s in FOLD_BWD_SHAPES])
def test_fold_batchnorm_bwd_against_float64_autograd_guards_and_in_place(shape, with_bias):
    from squeezedet_amd import _lib
    k, cin, cout = shape
    n, nblocks = k * k * cin * cout, fold_bwd_nblocks(shape)
    d = fold_bwd_inputs(shape, with_bias)
    d_t = {name: (_t(v) if v is not None else None) for name, v in d.items()}
    used = nblocks * cout
    assert int(_lib.lib().sqdet_fold_batchnorm_bwd_workspace_bytes(k, cin, cout)) == 4 * used     # what the library asks for
    bufs = {name: _guarded(m) for name, m in (("dw", n), ("dgamma", cout), ("dbeta", cout), ("ws", used))}
    _fold_bwd_call(d_t, d_t["dwf"], bufs["dw"][1], bufs["dgamma"][1], bufs["dbeta"][1], bufs["ws"][1], shape)
    for name, m in (("dw", n), ("dgamma", cout), ("dbeta", cout), ("ws", used)):
        _guards_intact(bufs[name][0], m, "%s %s" % (name, shape))
    assert not bool(torch.isnan(bufs["ws"][1]).any()), "a partial of the workspace was not written"
    dw, dg, db = [bufs[name][1].cpu().numpy() for name in ("dw", "dgamma", "dbeta")]
    qw, qg = check_fold_bwd(dw.reshape(d["w"].shape), dg, db, d, FOLD_BWD_EPS, "%s bias=%d" % (shape, with_bias))
    print("FOLDBWD %-14s %-5s dw %.3f of 8u  dgamma %.3f of its bound (n = %d)" % (shape, "bias" if with_bias else "-", qw, qg, nblocks + 21))
    # in place: dw == dw_folded
    ibuf, idw = _guarded(n)
    idw.copy_(d_t["dwf"].reshape(-1))
    g2, b2, w2 = _guarded(cout), _guarded(cout), _guarded(used)
    _fold_bwd_call(d_t, idw, idw, g2[1], b2[1], w2[1], shape)
    _guards_intact(ibuf, n, "in-place dw %s" % (shape,))
    _same_bits(idw, bufs["dw"][1], "in-place dw")
    _same_bits(g2[1], bufs["dgamma"][1], "in-place dgamma")
    _same_bits(b2[1], bufs["dbeta"][1], "in-place dbeta")
    # and the tensor-level entry gives the same bits
    ow, og, ob = _ops().fold_batchnorm_bwd(d_t["w"], d_t["dwf"], d_t["dbf"], d_t["cb"], d_t["gamma"], d_t["mean"], d_t["var"], FOLD_BWD_EPS)
    _same_bits(ow.reshape(-1), bufs["dw"][1], "ops.fold_batchnorm_bwd dw")
    _same_bits(og, bufs["dgamma"][1], "ops.fold_batchnorm_bwd dgamma")
    _same_bits(ob, bufs["dbeta"][1], "ops.fold_batchnorm_bwd dbeta")


_S, _M1, _M2, _M3, _L = FOLD_BWD_SHAPES       # _S is the one shape of a single workgroup (and a single finish workgroup)
# single-workgroup items first, last, next to each other and between the large ones
PLAN_21 = [_S, _L, _S, _L, _M1, _M2, _M3, _S, _S, _M3, _M2, _L, _M1, _S, _M2, _M3, _M1, _M2, _M3, _M1, _S]


PLAN_21_NO_BIAS = {1, 4, 6, 10, 13, 17}      # every shape once without a conv bias (its other items have one)


def plan_bias(i):
    return i not in PLAN_21_NO_BIAS


def _run_plan_against_per_conv(shapes, bias=plan_bias):
    ops = _ops()
    items, want, outs = [], [], []
    for i, shape in enumerate(shapes):
        d = fold_bwd_inputs(shape, bias(i), seed=i + 1)
        d_t = {name: (_t(v) if v is not None else None) for name, v in d.items()}
        out = [torch.empty_like(d_t["w"]), torch.empty(shape[2], device=DEV), torch.empty(shape[2], device=DEV)]
        items.append((d_t["w"], d_t["dwf"], d_t["dbf"], d_t["cb"], d_t["gamma"], d_t["mean"], d_t["var"]) + tuple(out))
        want.append(ops.fold_batchnorm_bwd(d_t["w"], d_t["dwf"], d_t["dbf"], d_t["cb"], d_t["gamma"], d_t["mean"], d_t["var"], FOLD_BWD_EPS))
        outs.append(out)
    plan = ops.FoldBwdPlan(items, FOLD_BWD_EPS)
    for rnd in range(2):
        for out in outs:
            for t in out:
                t.fill_(float("nan"))
        plan.run()
        torch.cuda.synchronize()
        for i, (out, ref) in enumerate(zip(outs, want)):
            for name, got, r in zip(("dw", "dgamma", "dbeta"), out, ref):
                _same_bits(got, r, "run %d item %d %s %s" % (rnd, i, shapes[i], name))


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", [_S, _M3], ids=["single_workgroup", "3x20x72"])
def test_fold_bwd_plan_one_item(shape, with_bias):
    _run_plan_against_per_conv([shape], lambda i: with_bias)


def test_fold_bwd_plan_21_items():
    assert len(PLAN_21) == 21 and PLAN_21[0] == PLAN_21[-1] == _S
    _run_plan_against_per_conv(PLAN_21)


# ================================================================== 3. sqdet_subsample_nhwc
SUB_HW = [(7, 9), (1, 1), (2, 5), (8, 8)]
SUB_CAP = (1, 2049, 2053, 8, 2)           # N, H, W, float32 channels (float16: twice as many), stride: 134.6 MB in, 33.7 MB out


def sub_cap_vectors():
    n, h, w, c, s = SUB_CAP
    return n * (-(-h // s)) * (-(-w // s)) * (c * 4 // 16)


def sub_input(shape, dtype, bit_patterns=False):
    """float32: consecutive integers (above 2^24 elements they are carried in the bit patterns instead: the kernel moves bits);
    float16: i % 2048, unique within any 2048-element window."""
    n = int(np.prod(shape))
    if dtype in (torch.float16, np.float16):
        return (np.arange(n, dtype=np.int32) % 2048).astype(np.float16).reshape(shape)
    if bit_patterns:
        return np.arange(n, dtype=np.int32).view(np.float32).reshape(shape)
    assert n <= 2 ** 24
    return np.arange(n, dtype=np.float32).reshape(shape)


def sub_reference(x, stride):
    return np.ascontiguousarray(x[:, ::stride, ::stride, :])


def _sub_call(x_t, y_t, shape, stride, dtype):
    from squeezedet_amd import _lib
    n, h, w, c = shape
    _lib.check(_lib.lib().sqdet_subsample_nhwc(_ptr(x_t), _ptr(y_t), n, h, w, c, stride, _lib.dtype_code(dtype), _lib.stream_ptr()),
               "sqdet_subsample_nhwc")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_subsample_small_shapes_bitwise_with_guards(dtype, stride):
    ev = 8 if dtype == torch.float16 else 4
    for (h, w) in SUB_HW:
        for c in (ev, 5 * ev):
            for n in (1, 3):
                x = sub_input((n, h, w, c), dtype)
                want = sub_reference(x, stride)
                ybuf, y = _guarded(want.size, dtype)
                _sub_call(_t(x), y, (n, h, w, c), stride, dtype)
                what = "subsample %s stride %d" % ((n, h, w, c), stride)
                _guards_intact(ybuf, want.size, what)
                _same_bits(y.cpu().numpy().reshape(want.shape), want, what)
                _same_bits(_ops().subsample_nhwc(_t(x), stride), want, what + " (ops)")
    if stride == 3:
        assert sub_reference(sub_input((1, 2, 5, ev), dtype), 3).shape == (1, 1, 2, ev)       # Ho == 1: H smaller than the stride


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_subsample_past_the_grid_cap(dtype):
    n, h, w, c, stride = SUB_CAP
    c = c * 2 if dtype == torch.float16 else c
    x = sub_input((n, h, w, c), dtype, bit_patterns=True)
    want = sub_reference(x, stride)
    assert SUB_CAP_VECS < want.nbytes // 16 == sub_cap_vectors() < 2 * SUB_CAP_VECS and sub_cap_vectors() % 256 != 0
    ybuf, y = _guarded(want.size, dtype)
    _sub_call(_t(x), y, (n, h, w, c), stride, dtype)
    _guards_intact(ybuf, want.size, "subsample cap")
    _same_bits(y.cpu().numpy().view(want.dtype).reshape(want.shape), want, "subsample past the cap")


def test_subsample_rejects_channel_bytes_not_a_multiple_of_16():
    from squeezedet_amd import _lib
    x = _t(sub_input((1, 4, 4, 4), torch.float16))
    ybuf, y = _guarded(2 * 2 * 4, torch.float16)
    with pytest.raises(_lib.SqdetUnsupported):
        _sub_call(x, y, (1, 4, 4, 4), 2, torch.float16)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all())


# ================================================================== 4. sqdet_preprocess_bgr
PRE_N = 3
PRE_WIDTHS = [1, 2, 3, 5, 6, 10, 255, 256, 257, 258, 259]
SENT16 = 0x7D5A           # the float16 sentinel's bit pattern (a NaN no conversion produces)


def preproc_exact_cases():
    """{name: (Hs, Ws, Hd, Wd)} with dyadic interpolation weights on both axes (ratios 1, 1/2, 1/4, 2, or a 1-pixel source axis)."""
    cases = {}
    for i, wd in enumerate(PRE_WIDTHS):
        hd = (1, 2, 3, 5)[i % 4]
        cases["identity_w%d" % wd] = (hd, wd, hd, wd)
        cases["reduce2_w%d" % wd] = (2 * hd, 2 * wd, hd, wd)
        if wd % 2 == 0:
            cases["magnify2_w%d" % wd] = (hd, wd // 2, 2 * hd, wd)
        if wd % 4 == 0:
            cases["magnify4_w%d" % wd] = (hd, wd // 4, 4 * hd, wd)
    cases["magnify4_w4_from_ws1"] = (2, 1, 8, 4)
    for wd in (1, 2, 3, 5, 257):
        cases["ws1_w%d" % wd] = (3, 1, 3, wd)                   # Ws == 1: every pixel is source column 0 with weight 1
    cases["hs1_w5"] = (1, 10, 4, 5)                             # Hs == 1, 2x reduction in x
    cases["hs1_w258"] = (1, 129, 3, 258)                        # Hs == 1, 2x magnification in x
    cases["hs1_ws1"] = (1, 1, 2, 3)
    return cases


# non-integer ratios: (Hs, Ws, Hd, Wd)
PRE_GENERAL = {"1242_to_177": (5, 1242, 7, 177), "53_to_259": (6, 53, 9, 259), "640_to_1242": (9, 640, 12, 1242), "vertical_7.3x": (73, 40, 10, 37)}


def preproc_image(hs, ws, seed=0):
    return np.random.RandomState(hs * 7919 + ws + seed).randint(0, 256, size=(PRE_N, hs, ws, 3)).astype(np.uint8)


def preproc_oracle(im, hd, wd):
    return np.stack([PO.preprocess_bgr(im[i], hd, wd, MEANS) for i in range(im.shape[0])])


def preproc_float64(im_u8, hd, wd):
    """The oracle's algorithm (its float32 source coordinates included: they are part of cv2's specification) with every
    interpolation operation and the mean subtraction in float64: (resized, resized - means), float64, one image."""
    im = np.asarray(im_u8).astype(np.float64)
    sy, sy1, fy = PO._coords(hd, im.shape[0])
    sx, sx1, fx = PO._coords(wd, im.shape[1])
    fx, fy = fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
    h0 = im[sy][:, sx] * (1.0 - fx) + im[sy][:, sx1] * fx
    h1 = im[sy1][:, sx] * (1.0 - fx) + im[sy1][:, sx1] * fx
    out = h0 * (1.0 - fy) + h1 * fy
    return out, out - np.asarray(MEANS, np.float32).astype(np.float64).reshape(1, 1, 3)


def check_preproc_general(out, ref):
    """The project's criteria (tests/test_gpu_preproc.py): max abs error <= 2e-4 and more than 99 % of the elements equal.
    Returns the share of equal elements."""
    assert out.shape == ref.shape and out.dtype == np.float32
    share = float((out == ref).mean())
    assert np.abs(out - ref).max() <= 2e-4, "max abs error %g" % np.abs(out - ref).max()
    assert share > 0.99, "only %.4f of the elements are equal" % share
    return share


def _preproc_call(im, hd, wd, dtype, off=0, trailing=0):
    """sqdet_preprocess_bgr on a source that is a slice of a larger buffer (16 bytes in front, 64 bytes of `trailing` behind) into
    a view that starts `off` elements into the sentinel-filled destination; asserts the sentinels around the view; NumPy result."""
    from squeezedet_amd import _lib
    n, hs, ws, _ = im.shape
    sbuf = torch.full((16 + im.size + 64,), trailing, dtype=torch.uint8, device=DEV)
    sbuf[16:16 + im.size] = _t(im.reshape(-1))
    m = n * hd * wd * 3
    lo = GUARD + off
    if dtype == torch.float16:
        raw = torch.full((lo + m + GUARD,), SENT16, dtype=torch.int16, device=DEV)
        dbuf = raw.view(torch.float16)
    else:
        dbuf = torch.full((lo + m + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        raw = dbuf.view(torch.int32)
    sentinel = int(raw[0].item())
    view = dbuf[lo:lo + m]
    _lib.check(_lib.lib().sqdet_preprocess_bgr(_ptr(sbuf[16:]), _ptr(view), n, hs, ws, hd, wd, MEANS[0], MEANS[1], MEANS[2],
                                               _lib.dtype_code(dtype), _lib.stream_ptr()), "sqdet_preprocess_bgr")
    torch.cuda.synchronize()
    what = "preprocess %s -> %s %s off %d" % ((hs, ws), (hd, wd), dtype, off)
    assert bool((raw[:lo] == sentinel).all()), "%s: a cell in front of the view was written" % what
    assert bool((raw[lo + m:] == sentinel).all()), "%s: a cell behind the view was written" % what
    return view.cpu().numpy().reshape(n, hd, wd, 3)


def _check_f16(h16, out32, ref, what):
    """float16 output: bitwise the float32 output rounded to float16 (the kernel converts the same float32 value), beside the
    project's <= 0.07."""
    assert h16.dtype == np.float16
    _same_bits(h16, out32.astype(np.float16), what + " float16 vs float32 output .half()")
    assert np.abs(h16.astype(np.float32) - ref).max() <= 0.07


_EXACT = preproc_exact_cases()


@pytest.mark.parametrize("name", list(_EXACT))
def test_preprocess_exact_cases_bitwise(name):
    """Dyadic weights: every product and sum of the interpolation is exact in float32, the mean subtraction is the one rounding
    -- the kernel must give the oracle's bits (tests/test_support_kernels_host.py shows each case is exact)."""
    hs, ws, hd, wd = _EXACT[name]
    im = preproc_image(hs, ws)
    ref = preproc_oracle(im, hd, wd)
    out = _preproc_call(im, hd, wd, torch.float32)
    _same_bits(out, ref, name)
    _check_f16(_preproc_call(im, hd, wd, torch.float16), out, ref, name)


@pytest.mark.parametrize("name", list(PRE_GENERAL))
def test_preprocess_general_cases(name):
    hs, ws, hd, wd = PRE_GENERAL[name]
    im = preproc_image(hs, ws)
    ref = preproc_oracle(im, hd, wd)
    out = _preproc_call(im, hd, wd, torch.float32)
    share = check_preproc_general(out, ref)
    print("PREPROC %-14s %s -> %s: %.5f of %d elements equal, max abs error %.3g" % (name, (hs, ws), (hd, wd), share, out.size, np.abs(out - ref).max()))
    _check_f16(_preproc_call(im, hd, wd, torch.float16), out, ref, name)
    _same_bits(_ops().preprocess_bgr(_t(im), hd, wd, MEANS, torch.float32), out, name + " (ops)")


# (Hs, Ws, Hd, Wd): 256 -- 8-byte stores at offsets 0 / 4 (float32: every even offset); 258 at offset 2 -- float16 dword stores on every
# second row; 257 and 6 -- rows of odd / short width; odd offsets -- scalar stores everywhere
PRE_ALIGN_CASES = [(3, 256, 3, 256), (3, 129, 3, 258), (4, 514, 2, 257), (2, 3, 4, 6), (5, 177, 4, 259)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", PRE_ALIGN_CASES, ids=["%dx%d_to_%dx%d" % c for c in PRE_ALIGN_CASES])
def test_preprocess_store_paths_do_not_depend_on_alignment(dtype, case):
    hs, ws, hd, wd = case
    im = preproc_image(hs, ws, seed=1)
    base = _preproc_call(im, hd, wd, dtype, off=0)
    assert not np.isnan(base).any()
    for off in (1, 2, 3, 4, 5):
        _same_bits(_preproc_call(im, hd, wd, dtype, off=off), base, "%s offset %d" % (case, off))
    if dtype == torch.float32:
        ref = preproc_oracle(im, hd, wd)
        assert np.abs(base - ref).max() <= 2e-4


@pytest.mark.parametrize("case", [(3, 256, 3, 256), (2, 1, 2, 3), (1, 10, 4, 5), (5, 53, 7, 259), (6, 177, 3, 40)],
                         ids=["identity", "ws1", "hs1", "magnify", "reduce"])
def test_preprocess_trailing_bytes_have_no_weight(case):
    """The neighbour of the last column has weight 0 and the masked tail path must not pull the bytes behind the source in: the
    output is the same whether they are 0 or 255."""
    hs, ws, hd, wd = case
    im = preproc_image(hs, ws, seed=2)
    for dtype in (torch.float32, torch.float16):
        a = _preproc_call(im, hd, wd, dtype, trailing=0)
        b = _preproc_call(im, hd, wd, dtype, trailing=255)
        _same_bits(a, b, "%s %s trailing 0 vs 255" % (case, dtype))
        assert not np.isnan(a).any()
