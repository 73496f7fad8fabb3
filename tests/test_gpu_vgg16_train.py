"""GPU tests of VGG16+ConvDet training (nets/vgg16_convDet.py:31-90 + nn_skeleton.py:285-361): the 2x2/s2 window-index pool
forward and backward, the fused 3x3 conv + 2x2 pool launch that also writes the index, and VGG16ConvDetTrainer against a
PyTorch-CPU autograd oracle assembled here from oracle.train_oracle's _conv / _q / loss_graph / apply_gradients and
oracle.sqdet_oracle.pooling_layer."""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O
from oracle import train_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [torch.float16, torch.float32]
DT_IDS = ["fp16", "fp32"]

VGG16 = [("conv1/conv1_1", 3, 64), ("conv1/conv1_2", 64, 64), ("conv2/conv2_1", 64, 128), ("conv2/conv2_2", 128, 128),
         ("conv3/conv3_1", 128, 256), ("conv3/conv3_2", 256, 256), ("conv3/conv3_3", 256, 256),
         ("conv4/conv4_1", 256, 512), ("conv4/conv4_2", 512, 512), ("conv4/conv4_3", 512, 512),
         ("conv5/conv5_1", 512, 512), ("conv5/conv5_2", 512, 512), ("conv5/conv5_3", 512, 512), ("conv6", 512, 72)]
POOL_AFTER = {"conv1/conv1_2": "pool1", "conv2/conv2_2": "pool2", "conv3/conv3_3": "pool3", "conv4/conv4_3": "pool4"}
FROZEN = ("conv1/", "conv2/")


def _opt(name, value):
    from squeezedet_amd import ops
    ops.set_option(name, value)


@pytest.fixture
def options():
    """Options a test sets are reset to their defaults afterwards."""
    yield _opt
    for k, v in (("conv_pool", 1), ("dbg", 0)):
        _opt(k, v)


# ------------------------------------------------------------------ host references
def _idx_ref(x, padding):
    """Row-major FIRST maximum of every 2x2/s2 window (strict '>' from -inf; a window nothing wins names its first valid
    cell), index 2 * row + col, as uint8 [n, ho, wo, c]."""
    x = x.float().cpu().numpy()
    n, h, w, c = x.shape
    ho, wo = (-(-h // 2), -(-w // 2)) if padding == "SAME" else (h // 2, w // 2)
    hh, ww = min(h, 2 * ho), min(w, 2 * wo)
    xp = np.full((n, 2 * ho, 2 * wo, c), np.nan, np.float32)
    xp[:, :hh, :ww] = x[:, :hh, :ww]
    ok = np.zeros((1, 2 * ho, 2 * wo, 1), bool)
    ok[:, :hh, :ww] = True
    best = np.full((n, ho, wo, c), -np.inf, np.float32)
    pos = np.full((n, ho, wo, c), 255, np.int32)
    for t in range(4):
        v, valid = xp[:, t >> 1::2, t & 1::2], np.broadcast_to(ok[:, t >> 1::2, t & 1::2], best.shape)
        pos = np.where(valid & (pos == 255), t, pos)
        win = valid & (v > best)
        best = np.where(win, v, best)
        pos = np.where(win, t, pos)
    return pos.astype(np.uint8)


def _relu_like(shape, dtype, seed, levels=4):
    """Quantised ReLU-like values: many exact zeros and many ties."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-levels, levels + 1, shape, generator=g).clamp(min=0).float() * 0.25
    return v.to(DEV, dtype)


# ------------------------------------------------------------------ 2x2 index forward / backward
POOL_SHAPES = [(2, 94, 311, 64), (1, 47, 156, 128), (2, 7, 9, 16), (1, 5, 5, 8), (3, 2, 3, 32), (1, 1, 1, 8), (1, 8, 6, 24)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("padding,shape", [(p, s) for p in ("SAME", "VALID") for s in POOL_SHAPES if p == "SAME" or min(s[1:3]) >= 2],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_maxpool2_idx_forward(dtype, padding, shape):
    from squeezedet_amd import ops
    x = _relu_like(shape, dtype, seed=sum(shape))
    y, idx = ops.maxpool_nhwc_idx(x, 2, 2, padding)
    assert torch.equal(y, ops.maxpool_nhwc(x, 2, 2, padding))
    np.testing.assert_array_equal(idx.cpu().numpy(), _idx_ref(x, padding))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_maxpool2_idx_forward_nan_and_inf(dtype):
    from squeezedet_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 9, 11, 16, generator=g)
    x[0, :2, :2, :] = float("-inf")                      # a window of -inf
    x[0, 2:4, 2:4, :] = float("nan")                     # a window of NaN
    x[1, 0:2, 0:2, :3] = float("nan")
    x[1, 0, 1, :3] = float("-inf")                       # NaN and -inf only
    x[1, 4, 4, :] = float("nan")                         # NaN beside finite values: never wins
    x = x.to(DEV, dtype)
    for padding in ("SAME", "VALID"):
        y, idx = ops.maxpool_nhwc_idx(x, 2, 2, padding)
        ref = ops.maxpool_nhwc(x, 2, 2, padding)
        assert torch.equal(y.view(torch.int16 if dtype == torch.float16 else torch.int32),
                           ref.view(torch.int16 if dtype == torch.float16 else torch.int32)), padding
        i = idx.cpu().numpy()
        np.testing.assert_array_equal(i, _idx_ref(x, padding))
        assert (i[0, 0, 0] == 0).all() and (i[0, 1, 1] == 0).all() and (i[1, 0, 0, :3] == 0).all()


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("shape", [(2, 94, 311, 64), (1, 47, 156, 128), (2, 7, 9, 16), (1, 5, 4, 8), (2, 4, 7, 24)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_maxpool2_idx_backward(dtype, padding, shape, relu):
    from squeezedet_amd import ops
    x = _relu_like(shape, dtype, seed=3 + sum(shape))
    y, idx = ops.maxpool_nhwc_idx(x, 2, 2, padding)
    g = torch.Generator().manual_seed(7)
    dy = torch.randn(tuple(y.shape), generator=g).to(DEV, dtype)
    dy.view(-1)[::7] = -0.0                                # signed zeros: the generic kernel's sum makes them +0
    dx = ops.maxpool_bwd_idx(idx, y, dy, x.shape[1:3], 2, 2, padding, relu=relu)
    ref = ops.maxpool_bwd(x, dy, 2, 2, padding, relu=relu)
    iv = torch.int16 if dtype == torch.float16 else torch.int32
    assert torch.equal(dx.view(iv), ref.view(iv))
    if padding == "VALID":
        if shape[1] % 2:
            assert bool((dx[:, -1] == 0).all())
        if shape[2] % 2:
            assert bool((dx[:, :, -1] == 0).all())


# ------------------------------------------------------------------ fused conv + pool + index
PAIRS = [(128, 256), (256, 256), (256, 512), (512, 512)]     # conv2_2's input .. conv4_3: the four VGG16 pair shapes (cin, cout)


def _pair_inputs(cin, cout, dtype, h, w, n=2, seed=0):
    from squeezedet_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(n, h, w, cin, generator=g)).to(DEV, dtype)
    k = torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.2).to(DEV)
    return x, k, b, ops.pack_conv_weights(k.to(DEV), dtype)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("dbg", [0, 97], ids=["dma", "regs"])
def test_conv_maxpool2_idx_fused(dtype, pair, relu, dbg, options):
    from squeezedet_amd import ops
    options("dbg", dbg)
    cin, cout = pair
    for (h, w) in ((11, 37), (16, 32), (9, 17)):
        x, _, b, pk = _pair_inputs(cin, cout, dtype, h, w, seed=h * w)
        assert ops.conv2d_maxpool2_supported(2, h, w, cin, cout, dtype)
        y, idx = ops.conv2d_maxpool2_nhwc_idx(x, pk, b, relu)
        assert torch.equal(y, ops.conv2d_maxpool2_nhwc(x, pk, b, relu)), (h, w)
        full = ops.conv2d_nhwc(x, pk, b, 1, "SAME", relu)
        y2, idx2 = ops.maxpool_nhwc_idx(full, 2, 2, "SAME")
        assert torch.equal(y, y2), (h, w)
        assert torch.equal(idx, idx2), (h, w)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_conv_maxpool2_idx_planted_ties(dtype):
    """Zero kernels, positive bias: every window is a four-way tie and must name cell 0."""
    from squeezedet_amd import ops
    x, k, b, _ = _pair_inputs(256, 256, dtype, 13, 21)
    pk = ops.pack_conv_weights(torch.zeros_like(k).to(DEV), dtype)
    b = torch.rand(256, device=DEV) + 0.1
    y, idx = ops.conv2d_maxpool2_nhwc_idx(x, pk, b, True)
    assert bool((idx == 0).all())
    assert torch.equal(y, ops.conv2d_maxpool2_nhwc(x, pk, b, True))


def test_conv_maxpool2_idx_fp16_rounding_ties():
    """Values one float32 ulp-group apart that round to the SAME float16: the stored tensor ties, so the first cell wins --
    the index is ranked on the rounded values, not the float32 accumulators."""
    from squeezedet_amd import ops
    cin, cout, h, w = 128, 256, 8, 16
    x = torch.zeros(1, h, w, cin)
    # input channel 0 carries a per-pixel value; kernel tap (1, 1) of channel 0 passes it to every output channel
    base = 1.0 + 2.0 ** -10 * torch.arange(h * w).reshape(h, w).remainder(4)          # exact float16 values
    x[0, :, :, 0] = base
    k = torch.zeros(3, 3, cin, cout)
    k[1, 1, 0, :] = 1.0
    # bias offsets below half a float16 ulp at 1.0 (2^-11): e.g. cell 0 reads 1 + 2^-13, cell 1 reads 1 + 2^-12 -- distinct
    # float32 values that round to the same float16
    b = torch.zeros(cout)
    b[1::2] = 2.0 ** -12
    x, b = x.to(DEV, torch.float16), b.to(DEV)
    pk = ops.pack_conv_weights(k.to(DEV), torch.float16)
    y, idx = ops.conv2d_maxpool2_nhwc_idx(x, pk, b, True)
    full = ops.conv2d_nhwc(x, pk, b, 1, "SAME", True)
    y2, idx2 = ops.maxpool_nhwc_idx(full, 2, 2, "SAME")
    assert torch.equal(y, y2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_conv_maxpool2_idx_off(dtype, options):
    from squeezedet_amd import ops
    from squeezedet_amd._lib import SqdetUnsupported
    x, _, b, pk = _pair_inputs(256, 256, dtype, 9, 17)
    options("conv_pool", 0)
    with pytest.raises(SqdetUnsupported):
        ops.conv2d_maxpool2_nhwc_idx(x, pk, b, True)


# ------------------------------------------------------------------ trainer
def vgg16_params(seed=0):
    """He-normal kernels (conv6 scaled down), small biases."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, cin, cout in VGG16:
        w = torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5
        if name == "conv6":
            w = w * 0.05
        p[name + "/kernels"] = w
        p[name + "/biases"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
    return p


def oracle_forward(params, x, dm, keep, storage="fp32", override=None):
    """nets/vgg16_convDet.py:33-90 in training mode (dropout before conv6) with train_oracle's layers; storage "fp16" rounds
    every stored activation (_q); override pins stored activations to given values, straight-through."""
    def ov(name, t):
        if override is not None and name in override:
            v = override[name].to(torch.float32)
            assert v.shape == t.shape, name
            return t + (v - t).detach()
        return t
    t = TO._q(torch.as_tensor(x, dtype=torch.float32), storage)
    for name, _, _ in VGG16:
        if name == "conv6":
            t = ov("drop", TO._q(t * dm / keep, storage))
        t = ov(name, TO._conv(t, params[name + "/kernels"], params[name + "/biases"], 1, "SAME", name != "conv6", storage))
        if name in POOL_AFTER:
            t = ov(POOL_AFTER[name], O.pooling_layer(t, 2, 2, "SAME"))
    return t


def oracle_loss_and_grads(mc, params, x, dm, mask, delta, box, labels, storage="fp32", override=None):
    names = [n for n in params if not n.startswith(FROZEN)]
    p = {k: v.clone().requires_grad_(k in names) for k, v in params.items()}
    preds = oracle_forward(p, x, dm, 0.5, storage, override)
    parts = TO.loss_graph(mc, preds, mask, delta, box, labels)
    wd = sum(mc.WEIGHT_DECAY * (p[k] ** 2).sum() / 2 for k in names if k.endswith("/kernels"))
    main = parts["class_loss"] + parts["conf_loss"] + parts["bbox_loss"]
    grads = torch.autograd.grad(main + wd, [p[k] for k in names])
    return dict(class_loss=float(parts["class_loss"].detach()), conf_loss=float(parts["conf_loss"].detach()),
                bbox_loss=float(parts["bbox_loss"].detach()), grads=dict(zip(names, [g.detach() for g in grads])),
                preds=preds.detach())


def _close(got, ref, dtype, what):
    got = got.float().cpu().numpy()
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    tol = 1e-3 * scale + 1e-5 if dtype == torch.float32 else 1e-2 * scale + 1e-3
    assert err <= tol, "%s: max err %g vs scale %g" % (what, err, scale)


def _trainer(size, B, dtype=torch.float32, seed=0, **kw):
    import squeezedet_amd as S
    from squeezedet_amd import nets
    from squeezedet_amd.train import VGG16ConvDetTrainer
    mc = S.kitti_vgg16_config_for_input(*size)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.BATCH_SIZE = B
    mc.IS_TRAINING = True
    m = nets.VGG16ConvDet(mc, gpu_id="0", dtype=dtype)
    params = vgg16_params(seed)
    m.load_params(params)
    return VGG16ConvDetTrainer(m, **kw), mc, params


def _batch(tr, mc, size, B, seed=31):
    x = O.synthetic_images(B, size[0], size[1], seed=seed)
    mask, delta, box, labels = TO.synthetic_labels(mc, B, seed=seed + 1)
    gh, gw = tr.model.preds.get_shape()[1:3]
    dm = torch.from_numpy((np.random.RandomState(seed + 2).uniform(size=(B, gh, gw, 512)) < 0.5).astype(np.float32))
    return x, mask, delta, box, labels, dm


def _check_grads(tr, mc, params, grads, rel, ref32=None):
    for name, gref in grads.items():
        wdg = mc.WEIGHT_DECAY * params[name] if name.endswith("/kernels") else 0.0   # added by the optimizer kernel
        got = tr.gview[name].cpu() + wdg
        scale = float(gref.abs().max())
        err = float((got - gref).abs().max())
        assert err <= rel * scale + 1e-7, "%s: grad err %g vs scale %g" % (name, err, scale)
        if ref32 is not None:
            g32 = ref32["grads"][name]
            cos = float((got * g32).sum() / (got.norm() * g32.norm() + 1e-30))
            assert cos >= 0.99, "%s: cos %g vs the float32 oracle" % (name, cos)


def test_vgg16_training_step_vs_oracle():
    size, B = (67, 101), 2                  # -> a 5 x 7 grid, odd maps at every pool
    tr, mc, params = _trainer(size, B)
    x, mask, delta, box, labels, dm = _batch(tr, mc, size, B)
    ref = oracle_loss_and_grads(mc, params, x, dm, mask, delta, box, labels)
    out = tr.step(x, mask, delta, box, labels, dropout_mask=dm, apply_update=False)
    torch.cuda.synchronize()
    for k in ("class_loss", "conf_loss", "bbox_loss"):
        np.testing.assert_allclose(float(out[k]), ref[k], rtol=5e-4)
    _close(out["preds"], ref["preds"], torch.float32, "preds (training forward)")
    assert set(tr.names) == set(ref["grads"])
    assert all(n.startswith(("conv3/", "conv4/", "conv5/", "conv6/")) for n in tr.names) and len(tr.names) == 20
    _check_grads(tr, mc, params, ref["grads"], 2e-3)
    mom = {k: torch.zeros_like(v) for k, v in params.items()}
    p_ref, _ = TO.apply_gradients(mc, params, mom, ref["grads"], step=0)
    tr.opt.step(tr.flat_params, tr.flat_grads, tr.flat_accum, tr.learning_rate(), mc.MOMENTUM, mc.MAX_GRAD_NORM, 1.0)
    torch.cuda.synchronize()
    for name in ref["grads"]:
        got, want = tr.view[name].cpu(), p_ref[name]
        assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-7, name


def _mixed_step(size, B):
    tr, mc, params = _trainer(size, B, dtype=torch.float16, loss_scale=1024.0)
    x, mask, delta, box, labels, dm = _batch(tr, mc, size, B)
    for _ in range(24):
        out = tr.step(x, mask, delta, box, labels, dropout_mask=dm, apply_update=False, keep_activations=True)
        if bool(torch.isfinite(tr.flat_grads).all()):
            break
        tr.loss_scale /= 4.0
    torch.cuda.synchronize()
    assert out["preds"].dtype == torch.float16 and bool(torch.isfinite(tr.flat_grads).all()), tr.loss_scale
    ref = oracle_loss_and_grads(mc, params, x, dm, mask, delta, box, labels, storage="fp16")
    ref32 = oracle_loss_and_grads(mc, params, x, dm, mask, delta, box, labels)
    for k in ("class_loss", "conf_loss", "bbox_loss"):
        np.testing.assert_allclose(float(out[k]), ref[k], rtol=2e-2)
    _close(out["preds"], ref["preds"], torch.float16, "preds (float16 training forward)")
    acts = {k: v.float().cpu() for k, v in out["activations"].items()}
    assert {"pool2", "pool3", "pool4", "drop", "conv3/conv3_1", "conv4/conv4_3", "conv5/conv5_3", "conv6"} <= set(acts)
    pinned = oracle_loss_and_grads(mc, params, x, dm, mask, delta, box, labels, storage="fp16", override=acts)
    _check_grads(tr, mc, params, pinned["grads"], 1e-2, ref32)


def test_vgg16_mixed_precision_training_step_vs_oracle():
    _mixed_step((67, 101), 2)


def test_vgg16_full_size_mixed_precision_training_step_vs_oracle():
    _mixed_step((375, 1242), 2)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _state(tr, out):
    return (_bits(tr.flat_grads.clone()), _bits(out["preds"].clone()), [float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")])


def _finite_scale(tr, batch):
    """float16: lower the loss scale until a step's gradients are finite (the synthetic weights make large activation
    gradients), as the trainer's overflow handling would."""
    for _ in range(24):
        tr.step(*batch, apply_update=False)
        if bool(torch.isfinite(tr.flat_grads).all()):
            return
        tr.loss_scale /= 4.0
    raise AssertionError("no finite loss scale")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_vgg16_fused_and_unfused_pairs_agree(dtype, options):
    from squeezedet_amd import ops
    size, B = (75, 130), 2
    tr, mc, params = _trainer(size, B, dtype=dtype, loss_scale=8.0)
    x, mask, delta, box, labels, dm = _batch(tr, mc, size, B)
    assert ops.conv2d_maxpool2_supported(B, 18, 32, 256, 256, dtype)        # conv3_3 + pool3 takes the fused index launch
    _finite_scale(tr, (x, mask, delta, box, labels, dm))
    a = _state(tr, tr.step(x, mask, delta, box, labels, dropout_mask=dm, apply_update=False))
    options("conv_pool", 0)
    b = _state(tr, tr.step(x, mask, delta, box, labels, dropout_mask=dm, apply_update=False))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_vgg16_wgrad_overlap_is_bitwise(dtype):
    size, B = (67, 101), 2
    res = []
    for overlap in (True, False):
        tr, mc, params = _trainer(size, B, dtype=dtype, overlap_wgrad=overlap, loss_scale=8.0)
        x, mask, delta, box, labels, dm = _batch(tr, mc, size, B)
        _finite_scale(tr, (x, mask, delta, box, labels, dm))
        st = []
        for _ in range(2):
            st.append(_state(tr, tr.step(x, mask, delta, box, labels, dropout_mask=dm)))
        tr.flush()
        st.append(tr.flat_params.clone())
        res.append(st)
    torch.cuda.synchronize()
    for s0, s1 in zip(res[0][:2], res[1][:2]):
        assert torch.equal(s0[0], s1[0]) and torch.equal(s0[1], s1[1]) and s0[2] == s1[2]
    assert torch.equal(_bits(res[0][2]), _bits(res[1][2]))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_vgg16_graphed_step_equals_the_eager_step(dtype):
    """GraphedStep (its dropout-mask shape derived from preds.inputs[0]) against the eager step on device-built labels: four
    steps from the same start, masks from the same counter stream, leave bit-identical variables, momentum and losses."""
    from squeezedet_amd import ops
    from squeezedet_amd.train import GraphedStep
    size, B, M = (67, 101), 2, 5
    rs = np.random.RandomState(31)
    gt = torch.from_numpy(np.stack([rs.uniform(0, size[1], (B, M)), rs.uniform(0, size[0], (B, M)), rs.uniform(20, 60, (B, M)),
                                    rs.uniform(20, 50, (B, M))], 2)).to(DEV)
    cls = torch.from_numpy(rs.randint(0, 3, (B, M)).astype(np.int32)).to(DEV)
    cnt = torch.from_numpy(np.array([5, 3], np.int32)).to(DEV)
    xs = [O.synthetic_images(B, size[0], size[1], seed=60 + i).to(DEV, dtype) for i in range(4)]
    res = []
    for graphed in (False, True):
        tr, mc, params = _trainer(size, B, dtype=dtype, seed=9, loss_scale=8.0)
        tr.seed = 1234
        anchors = torch.from_numpy(np.asarray(mc.ANCHOR_BOX, np.float64)).to(DEV)
        gs = GraphedStep(tr, anchors, mc.CLASSES) if graphed else None
        hist = []
        for x in xs:
            if graphed:
                out = gs.step(x, gt, cls, cnt)
            else:
                out = tr.step(x, *ops.build_labels(anchors, gt, cls, cnt, mc.CLASSES)[:4])
            hist.append([float(out[k]) for k in ("class_loss", "conf_loss", "bbox_loss")])
        tr.flush()
        torch.cuda.synchronize()
        res.append((tr.flat_params.clone(), tr.flat_accum.clone(), hist))
    assert res[0][2] == res[1][2]
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))


def test_vgg16_training_reduces_the_loss():
    size, B = (67, 101), 2
    tr, mc, params = _trainer(size, B)
    mc.LEARNING_RATE = 0.002
    x, mask, delta, box, labels, dm = _batch(tr, mc, size, B)
    hist = []
    for _ in range(10):
        o = tr.step(x, mask, delta, box, labels, dropout_mask=dm)
        hist.append(float(o["class_loss"]) + float(o["conf_loss"]) + float(o["bbox_loss"]))
    tr.flush()
    assert tr.global_step == 10 and np.isfinite(hist).all()
    assert hist[-1] < hist[0], hist
    preds = tr.model.run([tr.model.preds], {tr.model.image_input: x})[0]
    assert bool(torch.isfinite(preds).all())


def test_other_trainers_still_reject_vgg16():
    from squeezedet_amd.train import ResNet50ConvDetTrainer, SqueezeDetTrainer
    import squeezedet_amd as S
    from squeezedet_amd import nets
    mc = S.kitti_vgg16_config_for_input(67, 101)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.IS_TRAINING = True
    m = nets.VGG16ConvDet(mc, gpu_id="0", dtype=torch.float32)
    for cls in (SqueezeDetTrainer, ResNet50ConvDetTrainer):
        with pytest.raises(NotImplementedError, match="VGG16ConvDetTrainer"):
            cls(m)
