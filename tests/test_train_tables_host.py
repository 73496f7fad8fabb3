"""The host half of the training step's three "many" launches, without a GPU.

1. The tables that sqdet_conv_pack_many_prepare[_bn], sqdet_fold_batchnorm_bwd_many_prepare and sqdet_slab_reduce_many_prepare
   fill are, byte for byte and count for count, those of the commit the fixture was written from (tests/golden/
   make_train_tables.py -> tests/golden/train_tables.json): every item's layout, every block range and so every grid.
2. ops._ItemTable, the Python base of PackPlan / FoldBwdPlan / WgradPlan, on host tensors (a `*_prepare` entry only copies the
   pointers): NULL for None, the plans' own error texts, and a failing prepare raised through check."""
import ctypes as C
import importlib.util
import json
import os
import struct

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_train_tables", os.path.join(HERE, "golden", "make_train_tables.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


G = _generator()
with open(G.OUT) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def tables():
    return G.tables()


def test_fixture_covers_the_case_matrix(tables):
    assert sorted(GOLDEN) == sorted(tables) and len(GOLDEN) == 24
    for table in ("pack", "fold", "reduce"):
        assert sum(name.startswith(table) for name in GOLDEN) >= 3
    # the smallest items own one workgroup each, so adjacent ranges of length 1 exist in every table (float16 packing has no
    # such item: a fragment group is 512 halves, two workgroups)
    assert GOLDEN["pack one f32 plain"]["counts"] == [1] and GOLDEN["pack one f16 plain"]["counts"] == [2]
    assert GOLDEN["fold run of single workgroups"]["counts"] == [5, 5] and GOLDEN["reduce run of single workgroups"]["counts"] == [5]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_tables_are_the_fixtures(tables, name):
    got, want = tables[name], GOLDEN[name]
    assert got["counts"] == want["counts"], name
    if got["table"] != want["table"]:
        a, b = bytes.fromhex(got["table"]), bytes.fromhex(want["table"])
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        pytest.fail("%s: %d bytes, the fixture has %d; the first difference is at byte %d" % (name, len(a), len(b), first))


# ------------------------------------------------------------------ ops._ItemTable and the plans on host tensors
def _ops():
    from squeezedet_amd import _lib, ops
    from squeezedet_amd import build as sqbuild
    sqbuild.build(verbose=False)
    return ops, _lib


def test_item_table_columns_and_fill():
    ops, _lib = _ops()
    a, b = torch.zeros(4), torch.zeros(4)
    t = ops._ItemTable(3, [a, b])
    col = t._ptrs([a, None, b])
    assert list(col) == [a.data_ptr(), None, b.data_ptr()]                      # None -> NULL
    assert list(t._ints([1, 2.0, 3])) == [1, 2, 3] and list(t._floats([0, 0.5, 1])) == [0.0, 0.5, 1.0]
    assert t._keep == [a, b] and t.n == 3
    # a fold table of three one-workgroup items through _fill: the counts come back, the table is uploaded as bytes
    cols = [t._ptrs([a, a, a]) for _ in range(3)] + [t._ptrs([None, b, None])] + [t._ptrs([a, a, a]) for _ in range(7)]
    cols += [t._ints([1, 1, 1]), t._ints([1, 1, 1]), t._ints([4, 4, 4])]
    counts = t._fill("sqdet_fold_batchnorm_bwd_many_table_bytes", "sqdet_fold_batchnorm_bwd_many_prepare", cols + [3], 2, "cpu")
    assert counts == [3, 3]
    assert t.table.dtype == torch.uint8 and t.table.numel() == _lib.lib().sqdet_fold_batchnorm_bwd_many_table_bytes(3)
    raw = bytes(t.table.numpy())
    item = len(raw) // 3
    cbias = [struct.unpack_from("<Q", raw, i * item + 3 * 8)[0] for i in range(3)]          # the 4th pointer of an item
    assert cbias == [0, b.data_ptr(), 0]
    # a prepare that fails (a NULL kernel pointer: -1, invalid argument) raises through check
    cols[0] = t._ptrs([a, None, a])
    with pytest.raises(_lib.SqdetError, match="sqdet_fold_batchnorm_bwd_many_prepare.*bad item 1"):
        t._fill("sqdet_fold_batchnorm_bwd_many_table_bytes", "sqdet_fold_batchnorm_bwd_many_prepare", cols + [3], 2, "cpu")


def test_plans_build_their_tables_on_the_host_and_keep_their_error_texts():
    ops, _lib = _ops()
    w = torch.zeros(1, 1, 16, 16)
    vec = lambda: torch.zeros(16)
    plan = ops.PackPlan({"a": w, "b": w}, torch.float32, bwd_names=("b",), bn={"b": (vec(), vec(), vec(), vec(), None)}, eps=1e-5)
    assert (plan.n, plan.blocks) == (3, 3) and sorted(plan.fwd) == ["a", "b"] and sorted(plan.bwd) == ["b"] and sorted(plan.bias) == ["b"]
    assert isinstance(plan.fwd["a"], ops.PackedConv) and isinstance(plan.bwd["b"], ops.PackedConvBwd)
    pb = plan.bwd["b"]
    assert (pb.k, pb.cin, pb.cout, pb.dtype) == (1, 16, 16, torch.float32)
    assert pb.data.numel() == _lib.lib().sqdet_conv_packed_bytes(1, 16, 16, _lib.F32)
    assert plan.table.numel() == _lib.lib().sqdet_conv_pack_many_table_bytes(3)
    with pytest.raises(_lib.SqdetError, match="PackPlan: a must be a contiguous float32 HWIO tensor"):
        ops.PackPlan({"a": w.double()}, torch.float32)
    with pytest.raises(_lib.SqdetError, match="PackPlan: a must be a contiguous float32 HWIO tensor"):
        ops.PackPlan({"a": torch.zeros(1, 1, 16, 32)[..., ::2]}, torch.float32)
    with pytest.raises(_lib.SqdetError, match=r"PackPlan: a: batch-norm vectors must be contiguous float32 \[cout\]"):
        ops.PackPlan({"a": w}, torch.float32, bn={"a": (vec(), vec().half(), vec(), vec(), None)})
    with pytest.raises(_lib.SqdetError, match=r"PackPlan: a: batch-norm vectors must be contiguous float32 \[cout\]"):
        ops.PackPlan({"a": w}, torch.float32, bn={"a": (vec(), vec(), torch.zeros(32)[::2], vec(), None)})
    # WgradPlan: its own message for dw, and sqdet_slab_reduce_many_prepare's -1 for a 5x5 conv through check
    dw = torch.zeros(1, 1, 4, 4)
    wp = ops.WgradPlan([("k", (1, 4, 4, 4, 4, 1), dw, None, None, 0.0), ("l", (1, 4, 4, 4, 4, 1), dw, torch.zeros(4), dw, 1e-3)])
    assert (wp.n, wp.blocks) == (2, 2) and wp.shape["k"] == (1, 4, 4, 4, 4, 1) and sorted(wp.ws) == ["k", "l"]
    with pytest.raises(_lib.SqdetError, match=r"WgradPlan: k: dw must be a contiguous float32 \[k,k,cin,cout\] tensor"):
        ops.WgradPlan([("k", (1, 4, 4, 4, 4, 1), dw.half(), None, None, 0.0)])
    with pytest.raises(_lib.SqdetError, match="sqdet_slab_reduce_many_prepare.*bad item 0"):
        ops.WgradPlan([("k", (1, 4, 4, 4, 4, 5), torch.zeros(5, 5, 4, 4), None, None, 0.0)])
    fp = ops.FoldBwdPlan([(dw, dw, vec(), None, vec(), vec(), vec(), dw, vec(), vec())] * 2, 1e-5)
    assert (fp.n, fp.blocks, fp.finish_blocks, len(fp.ws)) == (2, 2, 2, 2)
