"""Host checks of tests/fused_launch_cases.py (no GPU): the batch sizes it computes really make every persistent launch
loop, at three CU counts; no case is larger than the stated byte cap; the float64 restatement of a fire module agrees with
the oracle (oracle/sqdet_oracle.py fire_layer / pooling_layer / conv_layer) within the tolerance tests/test_gpu_ops.py uses
for these modules (float32: rtol 1e-3, atol 1e-4; float16: rtol 2^-8, atol 2e-3)."""
import numpy as np
import pytest
import torch

from oracle import sqdet_oracle as O
from tests import fused_launch_cases as FC

CUS = (64, 256, 304)


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("case", FC.LOOP_CASES, ids=lambda c: c.name)
def test_batch_makes_every_workgroup_loop(case, cu):
    n = FC.batch_for(case, cu)
    h, w = case.hw
    st = case.geo.steps(n, h, w, cu)
    units = case.geo.units(n, h, w)
    tiles = n * case.geo.tiles(h, w)
    # restated here rather than trusted from LoopCase.looping()
    assert sum(st) == units and len(st) == (4 if case.geo.walk == "flat" else 1) * case.geo.grid(units, cu)
    assert min(st) >= 3 and max(st) >= 4, (n, min(st), max(st))
    assert tiles % 8 != 0
    assert 4 <= case.geo.tiles(h, w) <= 6, "every image is four to six ragged tiles"
    if case.geo.group == 4:
        assert tiles % 4 != 0 and units % 8 != 0
    assert n == 1 or not case.looping(n - 1, cu)[0], "not the smallest batch"
    # the chunks of the chunked run: nobody takes a second tile, and the launch is not degenerate
    c = FC.chunk_for(case, cu)
    assert 1 <= c < n and max(case.geo.steps(c, h, w, cu)) == 1
    assert case.geo.units(c, h, w) <= (4 if case.geo.walk == "flat" else 1) * case.geo.cap(cu)


def test_caps_at_256_cus_match_the_launch_code():
    """The per-kernel workgroup caps at 256 CUs, as read from the launchers (the table of the test plan)."""
    caps = {g.name: g.cap(256) for g in (FC.DMA_F2, FC.DMA_F3, FC.DMA_F4, FC.DMA_F5, FC.STREAM_E64, FC.STREAM_E128, FC.STREAM_POOL_E64,
                                         FC.STREAM_POOL_E128, FC.CHAIN, FC.STEM_PHASE, FC.STEM_PERS, FC.STEM_K7)}
    assert caps == {"fire_dma f2": 512, "fire_dma f3": 1024, "fire_dma f4": 512, "fire_dma f5": 512, "fire_stream E=64": 512,
                    "fire_stream E=128": 256, "fire_stream pooled E=64": 512, "fire_stream pooled E=128": 256, "fire_chain_stream": 256,
                    "stem_phase_dma": 512, "stem_pers": 1024, "stem_k7": 512}
    assert FC.cu_count(304) == 304 and FC.cu_count(255) == 248 and FC.cu_count(4) == 256
    # the largest op-level cases of tests/test_gpu_ops.py stay at one tile per workgroup (why the looped tests exist)
    assert max(FC.DMA_F2.steps(2, 94, 311, 256)) == 1 and max(FC.CHAIN.steps(3, 94, 311, 256)) == 1
    assert max(FC.STEM_PHASE.steps(2, 375, 1242, 256)) == 1 and max(FC.STEM_K7.steps(1, 375, 1242, 256)) == 1


@pytest.mark.parametrize("cu", CUS)
def test_cases_stay_below_the_byte_cap(cu):
    for case in FC.LOOP_CASES:
        n = FC.batch_for(case, cu)
        nbytes = case.spec.device_bytes(n, *case.hw)
        assert nbytes < FC.BYTES_CAP, "%s: batch %d is %.1f MB" % (case.name, n, nbytes / 1e6)
    assert FC.BYTES_CAP == 96 << 20


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_float64_restatement_agrees_with_the_oracle(dtype):
    spec = FC.Spec("fire_sqnext", dtype, 64, 16, 64, 16, pool=True)
    wt = FC.make_weights(spec, 11)
    rs = np.random.RandomState(12)
    x = torch.from_numpy((rs.randn(3, 3, 5, 64) - 0.3).astype(np.float32)).to(FC.TDT[dtype])
    got = FC.fire_ref64(x, wt, dtype, pool=True)
    p = {"f/squeeze1x1/kernels": wt["ws"], "f/squeeze1x1/biases": wt["bs"], "f/expand1x1/kernels": wt["w1"],
         "f/expand1x1/biases": wt["b1"], "f/expand3x3/kernels": wt["w3"], "f/expand3x3/biases": wt["b3"]}
    sq = O.conv_layer(x.float(), wt["ws"], wt["bs"], 1, "SAME", True, storage=dtype)
    y = O.pooling_layer(O.fire_layer(p, "f", x.float(), storage=dtype), 3, 2, "SAME")
    nxt = O.conv_layer(y, wt["wn"], wt["bn"], 1, "SAME", True, storage=dtype)
    tol = dict(rtol=1e-3, atol=1e-4) if dtype == "fp32" else dict(rtol=2 ** -8, atol=2e-3)
    assert tuple(got["y"].shape) == (3, 2, 3, 128) and tuple(got["sq_out"].shape) == (3, 2, 3, 16)
    for name, want in (("sq", sq), ("y", y), ("sq_out", nxt)):
        assert got[name].dtype == FC.TDT[dtype]
        assert float(want.abs().max()) > 0.1, name
        np.testing.assert_allclose(got[name].float().numpy(), want.numpy(), err_msg=name, **tol)
    # the form that starts from the squeeze tensor gives the same expand half
    spec2 = FC.Spec("fire_expand", dtype, 0, 16, 64, pool=True)
    wt2 = {k: v for k, v in wt.items() if k in ("w1", "b1", "w3", "b3")}
    assert spec2.from_squeeze and torch.equal(FC.fire_ref64(got["sq"], wt2, dtype, pool=True)["y"], got["y"])
