"""VGG16+ConvDet without a GPU (nets/vgg16_convDet.py:20-90): the native plan's parameter table against the reference's 28
variables, its grid against kitti_vgg16_config_for_input, the fused conv + pool launches of its layer table, the Python graph and
the pretrained-pickle conversion."""
import ctypes as C

import numpy as np
import pytest
import torch

import squeezedet_amd as S
from squeezedet_amd import _lib, nets, weights
from squeezedet_amd import build as sqbuild

# the reference's variables, in creation order: (tf.variable_scope / layer name, HWIO kernel shape)
VGG16_CONVS = [("conv1/conv1_1", (3, 3, 3, 64)), ("conv1/conv1_2", (3, 3, 64, 64)),
               ("conv2/conv2_1", (3, 3, 64, 128)), ("conv2/conv2_2", (3, 3, 128, 128)),
               ("conv3/conv3_1", (3, 3, 128, 256)), ("conv3/conv3_2", (3, 3, 256, 256)), ("conv3/conv3_3", (3, 3, 256, 256)),
               ("conv4/conv4_1", (3, 3, 256, 512)), ("conv4/conv4_2", (3, 3, 512, 512)), ("conv4/conv4_3", (3, 3, 512, 512)),
               ("conv5/conv5_1", (3, 3, 512, 512)), ("conv5/conv5_2", (3, 3, 512, 512)), ("conv5/conv5_3", (3, 3, 512, 512)),
               ("conv6", (3, 3, 512, 72))]
VGG16_VARS = [v for n, s in VGG16_CONVS for v in ((n + "/kernels", s), (n + "/biases", (s[3],)))]


@pytest.fixture(scope="module")
def lib():
    sqbuild.build(verbose=False)
    return _lib.lib()


def _create(lib, h, w, batch=2, dtype=_lib.F16):
    net = C.c_void_p()
    assert lib.sqdet_net_create(C.byref(net), _lib.ARCH_VGG16, dtype, batch, h, w, 3, 9) == 0, lib.sqdet_last_error()
    return net


def _params(lib, net):
    name, shape, nd = C.create_string_buffer(128), (C.c_int * 4)(), C.c_int()
    out = []
    for i in range(lib.sqdet_net_num_params(net)):
        assert lib.sqdet_net_param_info(net, i, name, 128, shape, C.byref(nd)) == 0
        out.append((name.value.decode(), tuple(shape[j] for j in range(nd.value))))
    return out


def _layers(lib, net):
    name, fl, by = C.create_string_buffer(128), C.c_double(), C.c_double()
    out = []
    for i in range(lib.sqdet_net_num_layers(net)):
        assert lib.sqdet_net_layer_info(net, i, name, 128, C.byref(fl), C.byref(by)) == 0
        out.append((name.value.decode(), fl.value, by.value))
    return out


def _dims(lib, net):
    gh, gw, ch = C.c_int(), C.c_int(), C.c_int()
    assert lib.sqdet_net_output_dims(net, C.byref(gh), C.byref(gw), C.byref(ch)) == 0
    return gh.value, gw.value, ch.value


def test_arch_accepted_and_bad_arch_still_refused(lib):
    for h, w in [(375, 1242), (64, 64), (97, 131), (201, 333)]:
        net = _create(lib, h, w)
        mc = S.kitti_vgg16_config_for_input(h, w)
        gh, gw, ch = _dims(lib, net)
        assert (gh, gw, ch) == (-(-h // 16), -(-w // 16), 72)
        assert gh * gw * 9 == mc.ANCHORS
        lib.sqdet_net_destroy(net)
    h = C.c_void_p()
    assert lib.sqdet_net_create(C.byref(h), 7, 1, 1, 384, 1248, 3, 9) == -1


def test_parameter_table_is_the_reference_variables(lib):
    net = _create(lib, 375, 1242)
    assert _params(lib, net) == VGG16_VARS
    assert len(VGG16_VARS) == 28
    assert _dims(lib, net) == (24, 78, 72)
    lib.sqdet_net_destroy(net)


def test_grid_matches_config():
    mc = S.kitti_vgg16_config_for_input(375, 1242)
    ref = S.kitti_vgg16_config()
    assert mc.ANCHORS == ref.ANCHORS == 24 * 78 * 9
    assert np.array_equal(np.asarray(mc.ANCHOR_BOX), np.asarray(ref.ANCHOR_BOX))
    assert (mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH) == (375, 1242)
    assert S.kitti_vgg16_config_for_input(47, 311).ANCHORS == 3 * 20 * 9


def test_layer_table_fuses_the_four_conv_pool_pairs(lib):
    fused = ["conv1/conv1_2+pool1", "conv2/conv2_2+pool2", "conv3/conv3_3+pool3", "conv4/conv4_3+pool4"]
    for dt in (_lib.F16, _lib.F32):
        net = _create(lib, 375, 1242, batch=8, dtype=dt)
        lay = _layers(lib, net)
        names = [n for n, _, _ in lay]
        assert len(names) == 14 and [n for n in names if "+" in n] == fused
        assert not any(n.startswith("pool") for n in names) and names[-1] == "conv6"
        lib.sqdet_net_destroy(net)
        assert lib.sqdet_set_option(b"conv_pool", 0) == 0
        try:
            net = _create(lib, 375, 1242, batch=8, dtype=dt)
        finally:
            assert lib.sqdet_set_option(b"conv_pool", 1) == 0
        lay_off = _layers(lib, net)
        names_off = [n for n, _, _ in lay_off]
        assert len(names_off) == 18 and names_off.count("pool1") == 1 and not any("+" in n for n in names_off)
        lib.sqdet_net_destroy(net)
        # same arithmetic; the fused launches neither write nor re-read the convs' full-resolution outputs
        esz = 2 if dt == _lib.F16 else 4
        assert sum(f for _, f, _ in lay) == sum(f for _, f, _ in lay_off)
        hw = [(375, 1242)] * 2 + [(188, 621)] * 2 + [(94, 311)] * 3 + [(47, 156)] * 3 + [(24, 78)] * 4
        assert abs(sum(f for _, f, _ in lay) - sum(2.0 * 8 * h * w * np.prod(s) for (h, w), (_, s) in zip(hw, VGG16_CONVS))) < 1e3
        saved = 0.0
        for (h, w, c) in [(375, 1242, 64), (188, 621, 128), (94, 311, 256), (47, 156, 512)]:
            saved += 2.0 * 8 * h * w * c * esz      # conv output written + read back by the pool
        assert abs((sum(b for _, _, b in lay_off) - sum(b for _, _, b in lay)) - saved) < 1.0


def test_conv_pool_supported_query(lib):
    # every VGG16 conv + pool pair at 375x1242, both dtypes; conv1_1 (Cin 3) and odd channel counts are not covered
    for dt in (_lib.F16, _lib.F32):
        for h, w, cin, cout in [(375, 1242, 64, 64), (188, 621, 128, 128), (94, 311, 256, 256), (47, 156, 512, 512)]:
            assert lib.sqdet_conv2d_maxpool2_supported(8, h, w, cin, cout, dt) == 1
        assert lib.sqdet_conv2d_maxpool2_supported(1, 375, 1242, 3, 64, dt) == 0
        assert lib.sqdet_conv2d_maxpool2_supported(1, 16, 16, 64, 66, dt) == 0
    assert lib.sqdet_conv2d_maxpool2_supported(1, 16, 16, 64, 64, 7) == 0
    assert lib.sqdet_set_option(b"conv_pool", 0) == 0
    try:
        assert lib.sqdet_conv2d_maxpool2_supported(8, 375, 1242, 64, 64, _lib.F16) == 0
    finally:
        assert lib.sqdet_set_option(b"conv_pool", 1) == 0
    assert lib.sqdet_conv2d_maxpool2_nhwc_fwd(None, None, None, None, 1, 8, 8, 64, 64, 1, 1, None) == -1


def _model():
    mc = S.kitti_vgg16_config()
    mc.LOAD_PRETRAINED_MODEL = False
    mc.BATCH_SIZE = 1
    return nets.VGG16ConvDet(mc, gpu_id="0", dtype=torch.float16)


def test_python_graph_matches_the_plan(lib):
    m = _model()
    assert [(k, tuple(v.shape)) for k, v in m.params.items()] == VGG16_VARS
    assert m.preds.get_shape() == (1, 24, 78, 72)
    assert m.NATIVE_ARCH == "vgg16" and S.VGG16ConvDet is nets.VGG16ConvDet
    assert m.trainable["conv1/conv1_1/kernels"] is False and m.trainable["conv2/conv2_2/biases"] is False
    assert m.trainable["conv3/conv3_1/kernels"] is True and m.trainable["conv6/kernels"] is True
    # the reference's analytical counters (nn_skeleton.py:549-561)
    assert sum(c for _, c in m.model_size_counter) == sum(int(np.prod(s)) + s[3] for _, s in VGG16_CONVS)
    from squeezedet_amd import train
    with pytest.raises(NotImplementedError):
        train.SqueezeDetTrainer(m)
    with pytest.raises(NotImplementedError):
        train.ResNet50ConvDetTrainer(m)


def test_caffe_pickle_maps_onto_every_backbone_variable():
    m = _model()
    rs = np.random.RandomState(0)
    cw = {}
    for n, s in VGG16_CONVS[:-1]:
        layer = n.split("/")[-1]
        cw[layer] = [rs.randn(s[3], s[2], s[0], s[1]).astype(np.float32), rs.randn(s[3]).astype(np.float32)]
    out = weights.from_caffe_weights(cw, m)
    assert set(out) == {v for v, _ in VGG16_VARS if not v.startswith("conv6/")}
    for n, s in VGG16_CONVS[:-1]:
        layer = n.split("/")[-1]
        assert np.array_equal(out[n + "/kernels"], np.transpose(cw[layer][0], [2, 3, 1, 0]))
        assert out[n + "/kernels"].shape == s
        assert np.array_equal(out[n + "/biases"], cw[layer][1])
