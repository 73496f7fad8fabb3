"""Generates tests/golden/net_plans.json: what ``sqdet_net_create`` plans for every arch, dtype, batch, image size and plan
option of MATRIX below.  Plan creation is host code (no device: ``cu_count()`` falls back to the MI355X's 256), so the file is
written on any machine that builds the library.  It pins the planner across refactors: it is written by the commit BEFORE
a change to squeezedet_amd/csrc/net.cpp, and tests/test_net_plans_host.py rebuilds every plan and compares.

Per plan: the ordered (layer name, flops, bytes), the ordered (param name, shape, ndim), param_bytes, workspace_bytes, the
output dims, sqdet_net_rider_capacity, sqdet_net_overlap_layer and sqdet_net_scores_supported, as text (plan_text).  Every
flops / bytes value is an integer-valued double below 2^53 (asserted), so they are written and compared as integers.  The
file holds a digest of that text for every key, and the whole text for the default options at 32x375x1242 and 1x384x1248.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_net_plans_golden.py                 # rewrites net_plans.json
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_net_plans_golden.py --show KEY      # prints one plan's full text
                                                                     (diff it against the same command in another checkout)
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from squeezedet_amd import _lib  # noqa: E402
from squeezedet_amd import build as sqbuild  # noqa: E402

PATH = os.path.join(HERE, "net_plans.json")
ARCHS = [("squeezedet", _lib.ARCH_SQUEEZEDET), ("squeezedet_plus", _lib.ARCH_SQUEEZEDET_PLUS), ("resnet50", _lib.ARCH_RESNET50),
         ("vgg16", _lib.ARCH_VGG16)]
DTYPES = [("f16", _lib.F16), ("f32", _lib.F32)]
BATCHES = [1, 8, 20, 32]
SIZES = [(375, 1242), (384, 1248), (192, 512), (97, 131)]      # the last two take the narrow-image stem fallbacks
# one option at a time; (name, value, value that restores the default)
OPTIONS = [None] + [("fire_fuse", v, 0) for v in range(2, 12)] + [("conv_pool", 0, 1), ("stem_algo", 2, 0), ("stem_algo", 3, 0),
                                                                  ("conv_algo", 1, 0)]
CLASSES, APG = 3, 9                                             # KITTI: every arch's config
FULL = [(32, (375, 1242)), (1, (384, 1248))]                    # default-option plans stored as text, per arch and dtype


def key_of(arch, dtype, batch, size, opt):
    return "%s/%s/b%d/%dx%d/%s" % (arch, dtype, batch, size[0], size[1], "default" if opt is None else "%s=%d" % opt[:2])


def matrix():
    """[(key, arch id, dtype id, batch, (h, w), option)] in a fixed order."""
    return [(key_of(an, dn, b, s, o), a, d, b, s, o)
            for an, a in ARCHS for dn, d in DTYPES for b in BATCHES for s in SIZES for o in OPTIONS]


def _exact(v):
    i = int(v)
    assert float(i) == v and 0 <= i < 2 ** 53, "not an exactly representable integer: %r" % v
    return i


def plan_text(lib, arch, dtype, batch, size, opt):
    """The plan as text, one record per line."""
    h = C.c_void_p()
    if opt is not None:
        assert lib.sqdet_set_option(opt[0].encode(), opt[1]) == 0
    try:
        rc = lib.sqdet_net_create(C.byref(h), arch, dtype, batch, size[0], size[1], CLASSES, APG)
    finally:
        if opt is not None:
            assert lib.sqdet_set_option(opt[0].encode(), opt[2]) == 0
    assert rc == 0, "sqdet_net_create failed: %s" % lib.sqdet_last_error().decode()
    try:
        out = []
        name = C.create_string_buffer(256)
        fl, by = C.c_double(), C.c_double()
        for i in range(lib.sqdet_net_num_layers(h)):
            assert lib.sqdet_net_layer_info(h, i, name, 256, C.byref(fl), C.byref(by)) == 0
            out.append("layer %s %d %d" % (name.value.decode(), _exact(fl.value), _exact(by.value)))
        shape, nd = (C.c_int * 4)(), C.c_int()
        for i in range(lib.sqdet_net_num_params(h)):
            assert lib.sqdet_net_param_info(h, i, name, 256, shape, C.byref(nd)) == 0
            out.append("param %s %s %d" % (name.value.decode(), "x".join(str(shape[j]) for j in range(4)), nd.value))
        gh, gw, ch = C.c_int(), C.c_int(), C.c_int()
        assert lib.sqdet_net_output_dims(h, C.byref(gh), C.byref(gw), C.byref(ch)) == 0
        out.append("param_bytes %d" % lib.sqdet_net_param_bytes(h))
        out.append("workspace_bytes %d" % lib.sqdet_net_workspace_bytes(h))
        out.append("output %d %d %d" % (gh.value, gw.value, ch.value))
        out.append("rider_capacity %d" % lib.sqdet_net_rider_capacity(h))
        out.append("overlap_layer %d" % lib.sqdet_net_overlap_layer(h))
        out.append("scores_supported %d" % lib.sqdet_net_scores_supported(h))
        return "\n".join(out)
    finally:
        lib.sqdet_net_destroy(h)


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:24]


def load_lib():
    sqbuild.build(verbose=False)
    return _lib.lib()


def main(argv):
    lib = load_lib()
    rows = matrix()
    if argv[:1] == ["--show"]:
        by_key = {r[0]: r for r in rows}
        print(plan_text(lib, *by_key[argv[1]][1:]))
        return
    digests, tables = {}, {}
    for key, arch, dtype, batch, size, opt in rows:
        text = plan_text(lib, arch, dtype, batch, size, opt)
        digests[key] = digest(text)
        if opt is None and (batch, size) in FULL:
            tables[key] = text.split("\n")
    with open(argv[0] if argv else PATH, "w") as f:
        json.dump({"digests": digests, "tables": tables}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d digests (%d distinct), %d full tables" % (len(digests), len(set(digests.values())), len(tables)))


if __name__ == "__main__":
    main(sys.argv[1:])
