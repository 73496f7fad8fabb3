"""VGG16+ConvDet training without a GPU: the C-ABI of the fused conv + pool launch that writes the window index, the training
graph VGG16ConvDetTrainer walks (frozen conv1 / conv2, the dropout in front of conv6) and the synthetic benchmark weights."""
import math
import os
import re

import torch

import squeezedet_amd as S
from squeezedet_amd import _lib, nets, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_launch_is_bound_and_declared():
    assert "sqdet_conv2d_maxpool2_nhwc_fwd_idx" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["sqdet_conv2d_maxpool2_nhwc_fwd_idx"]
    assert len(args) == 13
    hdr = open(os.path.join(ROOT, "include", "sqdet.h")).read()
    assert re.search(r"int sqdet_conv2d_maxpool2_nhwc_fwd_idx\(", hdr)


def _training_model(h=67, w=101):
    mc = S.kitti_vgg16_config_for_input(h, w)
    mc.LOAD_PRETRAINED_MODEL = False
    mc.IS_TRAINING = True
    mc.BATCH_SIZE = 2
    return nets.VGG16ConvDet(mc, gpu_id="0", dtype=torch.float32)


def test_training_graph_is_a_linear_chain_with_the_dropout_before_conv6():
    m = _training_model()
    chain, n = [], m.preds
    while n.op != "placeholder":
        chain.append(n)
        n = n.inputs[0]
    chain.reverse()
    assert [c.op for c in chain].count("pool") == 4 and [c.op for c in chain].count("dropout") == 1
    drop = next(c for c in chain if c.op == "dropout")
    assert m.preds.inputs[0] is drop and drop.inputs[0].name == "conv5/conv5_3"
    first = next(c for c in chain if c.op == "conv" and m.trainable[c.name + "/kernels"])
    assert first.name == "conv3/conv3_1" and first.inputs[0].name == "pool2"
    assert all(p.attrs["size"] == 2 and p.attrs["stride"] == 2 and p.attrs["padding"] == "SAME" for p in chain if p.op == "pool")
    assert m.preds.get_shape()[1:3] == (5, 7)
    trainable = [k for k in m.params if m.trainable[k]]
    assert len(trainable) == 20 and not any(k.startswith(("conv1/", "conv2/")) for k in trainable)


def test_synthetic_vgg16_weights():
    m = _training_model()
    p = synthetic.synthetic_params(m, seed=0)
    he = lambda k: math.sqrt(2.0 / (k.shape[0] * k.shape[1] * k.shape[2]))
    std = lambda k: float(k.std())
    # conv1_1 reads pixels (/64); conv1_2 reads conv1_1's O(1) output: plain He (a normal clipped at 2 sigma: std ~0.88-0.96 sigma)
    assert 0.8 < std(p["conv1/conv1_1/kernels"]) / (he(p["conv1/conv1_1/kernels"]) / 64) < 1.0
    assert 0.8 < std(p["conv1/conv1_2/kernels"]) / he(p["conv1/conv1_2/kernels"]) < 1.0
    # the other nets' conv1 rule is unchanged
    mc = S.kitti_squeezeDet_config()
    mc.LOAD_PRETRAINED_MODEL = False
    sq = nets.SqueezeDet(mc, gpu_id="0", dtype=torch.float32)
    ps = synthetic.synthetic_params(sq, seed=0)
    assert 0.8 < std(ps["conv1/kernels"]) / (he(ps["conv1/kernels"]) / 64) < 1.0


def test_vgg16_trainer_is_the_linear_chain_trainer():
    from squeezedet_amd import train
    assert issubclass(train.VGG16ConvDetTrainer, train.SqueezeDetTrainer)
    assert train.VGG16ConvDetTrainer._chain_backward is train.SqueezeDetTrainer._chain_backward
