"""GPU tests of VGG16+ConvDet (nets/vgg16_convDet.py:20-90): the fused 3x3 conv + 2x2/s2 max-pool launch (conv3x3_tile's POOL2 form)
bitwise against the separate conv and pool, maxpool2_kernel bitwise against the generic pool kernel, and the whole net -- op by op
and as the native plan (SQDET_ARCH_VGG16) -- against an oracle assembled here from oracle.sqdet_oracle.conv_layer / pooling_layer."""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (scope/layer, cin, cout) of the reference's convs; pools behind conv1_2, conv2_2, conv3_3, conv4_3
VGG16 = [("conv1/conv1_1", 3, 64), ("conv1/conv1_2", 64, 64), ("conv2/conv2_1", 64, 128), ("conv2/conv2_2", 128, 128),
         ("conv3/conv3_1", 128, 256), ("conv3/conv3_2", 256, 256), ("conv3/conv3_3", 256, 256),
         ("conv4/conv4_1", 256, 512), ("conv4/conv4_2", 512, 512), ("conv4/conv4_3", 512, 512),
         ("conv5/conv5_1", 512, 512), ("conv5/conv5_2", 512, 512), ("conv5/conv5_3", 512, 512), ("conv6", 512, 72)]
POOL_AFTER = {"conv1/conv1_2": "pool1", "conv2/conv2_2": "pool2", "conv3/conv3_3": "pool3", "conv4/conv4_3": "pool4"}


def _st(dtype):
    return "fp16" if dtype == torch.float16 else "fp32"


def _close(got, ref, dtype, what):
    got = got.float().cpu().numpy()
    ref = ref.numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, what
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    tol = 1e-3 * scale + 1e-5 if dtype == torch.float32 else 1e-2 * scale + 1e-3
    assert err <= tol, "%s: max err %g vs scale %g" % (what, err, scale)


def vgg16_params(seed=0, storage="fp32"):
    """He-normal kernels (conv6 scaled down), small biases; kernels rounded to the storage type the device packs them into."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, cin, cout in VGG16:
        w = torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5
        if name == "conv6":
            w = w * 0.05
        p[name + "/kernels"] = O._round_storage(w, storage)
        p[name + "/biases"] = (torch.rand(cout, generator=g) - 0.5) * 0.2
    return p


def vgg16_oracle(params, x, storage="fp32", collect=None):
    """nets/vgg16_convDet.py:33-90 with the oracle's layer functions: 3x3/s1/SAME convs + ReLU, 2x2/s2 SAME pools, conv6 without ReLU."""
    for name, _, _ in VGG16:
        last = name == "conv6"
        x = O.conv_layer(x, params[name + "/kernels"], params[name + "/biases"], 1, "SAME", not last, storage)
        if collect is not None:
            collect[name] = x
        if name in POOL_AFTER:
            x = O.pooling_layer(x, 2, 2, "SAME")
            if collect is not None:
                collect[POOL_AFTER[name]] = x
    return x


def _model(dtype, batch, size, seed=0):
    import squeezedet_amd as S
    from squeezedet_amd import nets
    mc = S.kitti_vgg16_config_for_input(*size)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.BATCH_SIZE = batch
    m = nets.VGG16ConvDet(mc, gpu_id="0", dtype=dtype)
    params = vgg16_params(seed, _st(dtype))
    m.load_params(params)
    return m, mc, params


def _opt(name, value):
    from squeezedet_amd import ops
    ops.set_option(name, value)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("hw", [(8, 16), (9, 17), (16, 32), (13, 37), (20, 22), (47, 23)])
def test_maxpool2_bitwise_generic(dtype, hw):
    """sqdet_maxpool_nhwc_fwd with k = s = 2 (maxpool2_kernel) == the generic maxpool_kernel ("dbg" 95) bit for bit, == the oracle."""
    from squeezedet_amd import ops
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(3, hw[0], hw[1], 64, generator=g).to(DEV, dtype)
    x[0, 0, 0, :8] = float("-inf")
    for pad in ("SAME", "VALID"):
        y = ops.maxpool_nhwc(x, 2, 2, pad)
        _opt("dbg", 95)
        try:
            want = ops.maxpool_nhwc(x, 2, 2, pad)
        finally:
            _opt("dbg", 0)
        assert torch.equal(y, want), pad
        assert torch.equal(y.float().cpu(), O.pooling_layer(x.float().cpu(), 2, 2, pad)), pad


PAIRS = [(64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]


@pytest.mark.parametrize("staging", ["dma", "registers"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_conv_maxpool2_fused_bitwise(pair, dtype, staging):
    """ops.conv2d_maxpool2_nhwc == maxpool_nhwc(conv2d_nhwc(x), 2, 2, SAME) bit for bit: every VGG16 (Cin, Cout) pair, maps odd / even
    / not multiples of the 8 x 16 tile, batch 2; both staging paths of the tile kernel (LDS-DMA, and "dbg" 97: through registers)."""
    from squeezedet_amd import ops
    cin, cout = pair
    st = _st(dtype)
    g = torch.Generator().manual_seed(cin + cout)
    w = O._round_storage(torch.randn(3, 3, cin, cout, generator=g) * (2.0 / (9 * cin)) ** 0.5, st)
    b = torch.rand(cout, generator=g) * 0.5          # positive: out-of-image pixels are real positive numbers before the mask
    pk = ops.pack_conv_weights(w.to(DEV), dtype)
    bd = b.to(DEV)
    if staging == "registers":
        _opt("dbg", 97)
    try:
        for (h, wd) in [(8, 16), (16, 32), (9, 17), (13, 37), (47, 21)]:
            x = O._round_storage(torch.randn(2, h, wd, cin, generator=g), st)
            xd = x.to(DEV, dtype)
            assert ops.conv2d_maxpool2_supported(2, h, wd, cin, cout, dtype)
            y = ops.conv2d_maxpool2_nhwc(xd, pk, bd)
            want = ops.maxpool_nhwc(ops.conv2d_nhwc(xd, pk, bd, 1, "SAME", True), 2, 2, "SAME")
            torch.cuda.synchronize()
            assert tuple(y.shape) == (2, (h + 1) // 2, (wd + 1) // 2, cout)
            assert torch.equal(y, want), (h, wd)
            if h == 13:
                _close(y, O.pooling_layer(O.conv_layer(x, w, b, 1, "SAME", True, st), 2, 2, "SAME"), dtype, "fused vs oracle")
                y0 = ops.conv2d_maxpool2_nhwc(xd, pk, bd, relu=False)
                assert torch.equal(y0, ops.maxpool_nhwc(ops.conv2d_nhwc(xd, pk, bd, 1, "SAME", False), 2, 2, "SAME"))
    finally:
        _opt("dbg", 0)


def test_conv_maxpool2_unsupported_is_an_error():
    from squeezedet_amd import ops
    from squeezedet_amd._lib import SqdetError
    x = torch.randn(1, 16, 16, 3, device=DEV)
    pk = ops.pack_conv_weights(torch.randn(3, 3, 3, 64, device=DEV), torch.float32)
    assert not ops.conv2d_maxpool2_supported(1, 16, 16, 3, 64, torch.float32)
    with pytest.raises(SqdetError):
        ops.conv2d_maxpool2_nhwc(x, pk, torch.zeros(64, device=DEV))


# ------------------------------------------------------------------ whole net
def _nodes(m):
    nodes, stack, seen = {}, [m.preds], set()
    while stack:
        nd = stack.pop()
        if nd in seen:
            continue
        seen.add(nd)
        if nd.op in ("conv", "pool"):
            nodes[nd.name] = nd
        stack.extend(nd.inputs)
    return nodes


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_vgg16_layer_by_layer_vs_oracle(dtype):
    """Op-by-op graph at a small odd size (67 x 101 -> 5 x 7): every conv and pool output against the oracle (all fetched: the pairs
    run unfused); then the pools alone (the pairs take the fused launch) -- bitwise the unfused pools."""
    size = (67, 101)
    st = _st(dtype)
    m, mc, params = _model(dtype, 2, size)
    x = O.synthetic_images(2, size[0], size[1], seed=1, storage=st)
    col = {}
    vgg16_oracle(params, x, st, collect=col)
    nodes = _nodes(m)
    assert set(nodes) == set(col)
    names = list(col)
    outs = m.run([nodes[n] for n in names], {m.image_input: x}, use_plan=False)
    for n, got in zip(names, outs):
        _close(got, col[n], dtype, n)
    pools = ["pool1", "pool2", "pool3", "pool4"]
    fused = m.run([nodes[n] for n in pools], {m.image_input: x}, use_plan=False)
    for n, got in zip(pools, fused):
        assert torch.equal(got, outs[names.index(n)]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_vgg16_plan_equals_graph_and_oracle(dtype):
    """Native plan == op-by-op graph bit for bit (fused pairs on both sides), and the plan with "conv_pool" = 0 (18 launches) too;
    all within tolerance of the oracle."""
    size = (67, 101)
    st = _st(dtype)
    m, mc, params = _model(dtype, 2, size, seed=2)
    x = O.synthetic_images(2, size[0], size[1], seed=4, storage=st)
    ref = vgg16_oracle(params, x, st)
    (pg,) = m.run([m.preds], {m.image_input: x}, use_plan=False)
    (pp,) = m.run([m.preds], {m.image_input: x}, use_plan=True)
    assert tuple(pp.shape) == (2, 5, 7, 72)
    assert torch.equal(pg, pp)
    _close(pp, ref, dtype, "preds")
    assert sum("+pool" in n for n, _, _ in m._native_plan(2).layer_table()) == 4
    _opt("conv_pool", 0)
    try:
        m2, _, _ = _model(dtype, 2, size, seed=2)
        (po,) = m2.run([m2.preds], {m2.image_input: x}, use_plan=True)
        assert len(m2._native_plan(2).layer_table()) == 18
    finally:
        _opt("conv_pool", 1)
    assert torch.equal(po, pp)


def test_vgg16_full_size_vs_oracle_and_picks():
    """375 x 1242, batch 2, float16: preds against the oracle; the picks identical wherever tests/decision_margins.py finds every
    decision decidable."""
    from tests import decision_margins as DM
    import squeezedet_amd as S
    m, mc, params = _model(torch.float16, 2, (375, 1242), seed=3)
    omc = O.squeezeDet_config_for_input(375, 1242)          # the same 24 x 78 grid and anchor shapes (the oracle has no VGG16 config)
    assert np.allclose(np.asarray(omc.ANCHOR_BOX, np.float64), np.asarray(S.kitti_vgg16_config().ANCHOR_BOX, np.float64))
    x = O.synthetic_images(2, 375, 1242, seed=5, storage="fp16")
    xd = x.to(DEV, torch.float16)
    outs = m.run([m.preds, m.det_boxes, m.det_probs, m.det_class, m.pred_class_probs, m.pred_conf], {m.image_input: xd})
    ob, op, oc, oi, cnt = m.filter_prediction_batch(outs[1], outs[2], outs[3])
    torch.cuda.synchronize()
    ref = vgg16_oracle(params, x, "fp16")
    _close(outs[0], ref, torch.float16, "preds 375x1242")
    r = O.interpret_output(ref.numpy(), omc)
    g = [o.cpu().numpy() for o in outs[1:4]]
    oi, cnt, oc = oi.cpu().numpy(), cnt.cpu().numpy(), oc.cpu().numpy()
    for i in range(2):
        ri = {k: r[k][i] for k in ("det_boxes", "det_probs", "det_class", "pred_class_probs", "pred_conf")}
        row = DM.image_margins(omc, ri, dict(det_boxes=g[0][i], det_probs=g[1][i], det_class=g[2][i]))
        dets = O.filter_prediction(omc, r["det_boxes"][i], r["det_probs"][i], r["det_class"][i], return_index=True)
        print("image %d: %s" % (i, row))
        if row["decidable"]:
            assert oi[i, :cnt[i]].tolist() == list(dets[3])
            assert oc[i, :cnt[i]].tolist() == [int(c) for c in dets[2]]


def test_vgg16_serving_paths():
    """demo.py-shaped Session.run at batch 1, and detect_filter_pipelined on two lanes (deferred) == the sequential step."""
    from squeezedet_amd.nn_skeleton import Session
    m1, mc1, params = _model(torch.float16, 1, (375, 1242), seed=6)
    x = O.synthetic_images(1, 375, 1242, seed=7, storage="fp16")
    with Session() as sess:
        det_boxes, det_probs, det_class = sess.run([m1.det_boxes, m1.det_probs, m1.det_class], feed_dict={m1.image_input: [x[0].numpy()]})
    assert det_boxes.shape == (1, 16848, 4) and np.isfinite(det_boxes).all()
    fb, fp, fc = m1.filter_prediction(det_boxes[0], det_probs[0], det_class[0])
    assert len(fb) == len(fp) == len(fc) <= 64
    batch, lanes = 2, 2
    m, mc, _ = _model(torch.float16, batch, (375, 1242), seed=6)
    xs = [O.synthetic_images(batch, 375, 1242, seed=s, storage="fp16").to(DEV, torch.float16) for s in (3, 4, 5)]
    seq = []
    for xx in xs:
        b, p, c = m.detect(xx)
        seq.append([t.clone() for t in m.filter_prediction_batch(b, p, c)])
    torch.cuda.synchronize()
    outs, hist = [], []
    for xx in xs + xs[:1]:
        hist.append(m.detect_filter_pipelined(xx, to_host=True, defer=True, lanes=lanes))
        if len(hist) > lanes:
            torch.cuda.synchronize()
            outs.append([t.clone() for t in hist[-1 - lanes]])
    m.flush_pipeline()
    torch.cuda.current_stream().synchronize()
    for out in hist[-lanes:]:
        outs.append([t.clone() for t in out])
    seq = seq + seq[:1]
    assert len(outs) == 4
    for got, want in zip(outs, seq):
        n = want[4].cpu().numpy()
        assert np.array_equal(got[4].numpy(), n)
        for i in range(batch):
            for t in range(4):
                assert torch.equal(got[t][i, :n[i]], want[t][i, :n[i]].cpu())
