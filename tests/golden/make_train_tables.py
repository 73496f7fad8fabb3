"""The host tables of the three training "many" launches -> tests/golden/train_tables.json (no GPU).

sqdet_conv_pack_many_prepare[_bn], sqdet_fold_batchnorm_bwd_many_prepare and sqdet_slab_reduce_many_prepare are host functions:
given pointers they never dereference and lists of dimensions they fill a table of items, one block range per item, and return
the grid.  The fixture keeps every table as hex beside the returned counts, written ONCE from the commit before a change to the
tables; tests/test_train_tables_host.py recomputes it from the library under test, which pins every item's layout, every block
range and so every grid.  (ctypes zero-fills the host buffer, so struct padding compares equal.)  Only the C ABI is used, so this
file runs unchanged on an older checkout:

    python tests/golden/make_train_tables.py [out.json]
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "train_tables.json")
EPS = 1e-5

# tests/test_gpu_train.py test_pack_many_equals_the_per_kernel_packers' shapes (k, cin, cout)
PACK_NINE = [(1, 64, 16), (1, 16, 64), (3, 16, 64), (1, 256, 48), (3, 48, 192), (1, 768, 96), (3, 96, 384), (3, 768, 72), (3, 24, 40)]
# the lookup's edges (tests/test_gpu_train.py test_pack_plan_lookup_at_one_workgroup_items): the smallest items next to each other.
# float32: one workgroup each.  float16: two -- a fragment group is 64 lanes x 8 halves = 512 elements however few channels it holds.
PACK_ONE = [(1, 16, 16)]
PACK_RUN = [(1, 16, 16)] * 5 + [(3, 24, 40)]
# tests/test_gpu_train.py test_wgrad_plan_one_reduction_for_many_convs' subset of BWD_CASES (its float32 selection), (n, h, w, cin, cout, k)
REDUCE_NAMES = ("e3_16_64", "convdet_768_72", "e3_32_128_9tap", "sq_512_96", "ragged_20_36", "ragged_40_24", "plus_e3_384_256", "e1_48_192")
REDUCE_ONE = [(1, 4, 4, 4, 4, 1)]                 # 16 + 4 sums: one workgroup
REDUCE_RUN = [(1, 4, 4, 4, 4, 1), (2, 3, 5, 8, 4, 1), (1, 4, 4, 4, 12, 1), (1, 2, 2, 4, 4, 1), (1, 4, 4, 4, 4, 1)]


def ptrs(col, n, absent=()):
    """Column `col` of fake device pointers (never dereferenced on the host), NULL at the indices in `absent`."""
    return (C.c_void_p * n)(*[None if i in absent else 0x1000000 * (col + 1) + 0x100 * (i + 1) for i in range(n)])


def ints(vals):
    return (C.c_int * len(vals))(*vals)


def dump(host, *counts):
    return {"table": bytes(host).hex(), "counts": [int(c.value) for c in counts]}


def pack_table(lib, shapes, orders, code, bn_every):
    """One item per (shape, order) pair; bn_every = 0: sqdet_conv_pack_many_prepare; m > 0: the _bn entry with batch-norm pointers
    on every m-th item (a conv bias on every second of those, a folded-bias output on the forward-order ones)."""
    items = [(k, ci, co, o) for (k, ci, co) in shapes for o in orders]
    n = len(items)
    host = (C.c_ubyte * int(lib.sqdet_conv_pack_many_table_bytes(n)))()
    blocks = C.c_int()
    cols = [ints([it[j] for it in items]) for j in range(4)]
    if not bn_every:
        rc = lib.sqdet_conv_pack_many_prepare(ptrs(0, n), ptrs(1, n), *cols, n, code, host, C.byref(blocks))
    else:
        plain = {i for i in range(n) if i % bn_every}
        rc = lib.sqdet_conv_pack_many_prepare_bn(ptrs(0, n), ptrs(1, n), *cols, ptrs(2, n, plain), ptrs(3, n, plain), ptrs(4, n, plain),
                                                 ptrs(5, n, plain), ptrs(6, n, plain | {i for i in range(n) if i % (2 * bn_every)}),
                                                 ptrs(7, n, plain | {i for i in range(n) if items[i][3]}), EPS, n, code, host,
                                                 C.byref(blocks))
    assert rc == 0, lib.sqdet_last_error()
    return dump(host, blocks)


def fold_table(lib, shapes, no_bias):
    n = len(shapes)
    host = (C.c_ubyte * int(lib.sqdet_fold_batchnorm_bwd_many_table_bytes(n)))()
    b1, b2 = C.c_int(), C.c_int()
    cols = [ptrs(j, n, no_bias if j == 3 else ()) for j in range(11)]
    rc = lib.sqdet_fold_batchnorm_bwd_many_prepare(*cols, *[ints([s[j] for s in shapes]) for j in range(3)], n, host, C.byref(b1),
                                                   C.byref(b2))
    assert rc == 0, lib.sqdet_last_error()
    return dump(host, b1, b2)


def reduce_table(lib, shapes):
    """Like the GPU test's items: no bias gradient on every third item, weight decay on every second."""
    n = len(shapes)
    host = (C.c_ubyte * int(lib.sqdet_slab_reduce_many_table_bytes(n)))()
    blocks = C.c_int()
    decays = (C.c_float * n)(*[1e-3 * i for i in range(n)])
    rc = lib.sqdet_slab_reduce_many_prepare(ptrs(0, n), ptrs(1, n), ptrs(2, n, {i for i in range(n) if i % 3 == 0}),
                                            ptrs(3, n, {i for i in range(n) if i % 2 == 0}), decays,
                                            *[ints([s[j] for s in shapes]) for j in range(6)], n, host, C.byref(blocks))
    assert rc == 0, lib.sqdet_last_error()
    return dump(host, blocks)


def tables():
    """name -> {"table": hex, "counts": [...]} from the library of the checkout this file lies in."""
    from squeezedet_amd import _lib
    from squeezedet_amd import build as sqbuild
    from tests.test_gpu_support_kernels import PLAN_21, PLAN_21_NO_BIAS
    from tests.test_gpu_train import BWD_CASES
    sqbuild.build(verbose=False)
    lib = _lib.lib()
    out = {}
    for dname, code in (("f16", _lib.F16), ("f32", _lib.F32)):
        for bn in (0, 1):
            out["pack one %s %s" % (dname, "bn" if bn else "plain")] = pack_table(lib, PACK_ONE, (0,), code, bn)
            for o in (0, 1):
                out["pack run order %d %s %s" % (o, dname, "bn on every second item" if bn else "plain")] = pack_table(lib, PACK_RUN, (o,), code, 2 * bn)
        out["pack nine both orders %s plain" % dname] = pack_table(lib, PACK_NINE, (0, 1), code, 0)
        out["pack nine both orders %s bn on every item" % dname] = pack_table(lib, PACK_NINE, (0, 1), code, 1)
        out["pack nine both orders %s bn on every third item" % dname] = pack_table(lib, PACK_NINE, (0, 1), code, 3)
    small = PLAN_21[0]
    out["fold one"] = fold_table(lib, [small], ())
    out["fold run of single workgroups"] = fold_table(lib, [small] * 5, {1, 3})
    out["fold PLAN_21"] = fold_table(lib, PLAN_21, PLAN_21_NO_BIAS)
    by_name = {c[0]: c[1:] for c in BWD_CASES}
    out["reduce one"] = reduce_table(lib, REDUCE_ONE)
    out["reduce run of single workgroups"] = reduce_table(lib, REDUCE_RUN)
    out["reduce BWD_CASES subset"] = reduce_table(lib, [by_name[name] for name in REDUCE_NAMES])
    return out


def main():
    out = OUT if len(sys.argv) < 2 else sys.argv[1]
    doc = tables()
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d tables to %s" % (len(doc), out))


if __name__ == "__main__":
    main()
