"""Digests of BatchReader.next_plan under every augmentation policy -> tests/golden/reader_plans.json (no GPU).

The fixture pins the reader's host half bit for bit: every random draw in number and order, every array of a plan in dtype,
shape and bytes, every Python value in value and type.  It is written ONCE, from the commit before a change to the reader,
and tests/test_reader_plans_host.py recomputes it from the code under test.  Only the public API and tests/augment_policy_cases.py
are used, so this file runs unchanged on an older checkout:

    python tests/golden/make_reader_plans.py [out.json]

Per case the digest is a SHA-256 over PLANS consecutive plans, field by field (the field's name, then its value: an array as
dtype string, shape and bytes; a list or tuple as its length and elements; a float as float64 bytes, an int as int64 bytes, a
string as UTF-8, None as a marker; every value tagged with its type's name), followed by the reader's state_dict() key array,
position and cursor.  Beside it the "trail" keeps four hex digits of the running digest after every field, so that a mismatch
can be traced to the first plan and field that differ."""
import hashlib
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "reader_plans.json")
SEED, PLANS = 5, 6
MOSAICS = [(0.0, None), (0.5, None), (1.0, None), (1.0, (0.0, 0.0)), (1.0, (1.0, 1.0)), (1.0, (0.0, 1.0))]


def cases():
    """name -> (geometry, colour, mosaic probability, mosaic centre or None for the default, DATA_AUGMENTATION, shuffle)."""
    out = {}
    for geometry in ("drift", "ssd"):
        for color in (False, True):
            for prob, centre in MOSAICS:
                for shuffle in (True, False):
                    name = "%s colour=%d mosaic=%g centre=%s shuffle=%d" % (geometry, color, prob, "default" if centre is None else
                                                                             "%g,%g" % centre, shuffle)
                    out[name] = (geometry, color, prob, centre, True, shuffle)
    out["no augmentation, mosaic=1"] = ("drift", False, 1.0, None, False, True)
    return out


def feed(h, v):
    """Update the hash h with the value v."""
    h.update(("<%s>" % type(v).__name__).encode())
    if v is None:
        h.update(b"N")
    elif isinstance(v, np.ndarray):
        h.update(("A%s%r" % (v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)):
        h.update(b"L" + struct.pack("<q", len(v)))
        for e in v:
            feed(h, e)
    elif isinstance(v, str):
        h.update(b"S" + v.encode("utf-8"))
    elif isinstance(v, (bool, int, np.integer)):
        h.update(b"I" + struct.pack("<q", int(v)))
    elif isinstance(v, (float, np.floating)):
        h.update(b"F" + struct.pack("<d", float(v)))
    else:
        raise TypeError("a plan holds a %s" % type(v).__name__)


def run_case(geometry, color, prob, centre, augment, shuffle):
    """(sha256 hex, trail hex, [label of every trail entry]) of one case."""
    from squeezedet_amd import BatchReader
    from tests import augment_policy_cases as AC
    images, rois = AC.policy_dataset()
    mc = AC.policy_config(geometry=geometry, color=color)
    mc.DATA_AUGMENTATION, mc.AUG_MOSAIC_PROB = augment, prob
    if centre is not None:
        mc.AUG_MOSAIC_CENTER = centre
    reader = BatchReader(mc, images, rois, seed=SEED)
    h, trail, labels = hashlib.sha256(), [], []

    def put(label, name, v):
        h.update(name.encode() + b"=")
        feed(h, v)
        trail.append(h.hexdigest()[:4])
        labels.append(label)

    for k in range(PLANS):
        p = reader.next_plan(shuffle)
        h.update(("<%s>" % type(p).__name__).encode())
        for name, v in zip(p._fields, p):
            put("plan %d, field %s" % (k, name), name, v)
    state = reader.state_dict()
    for name in ("rs_keys", "rs_pos", "cur_idx"):
        put("the reader's state after %d plans, %s" % (PLANS, name), name, state[name])
    return h.hexdigest(), "".join(trail), labels


def main():
    out = OUT if len(sys.argv) < 2 else sys.argv[1]
    doc = {"seed": SEED, "plans": PLANS, "cases": {}}
    for name, case in cases().items():
        sha, trail, _ = run_case(*case)
        doc["cases"][name] = {"sha256": sha, "trail": trail}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(doc["cases"]), out))


if __name__ == "__main__":
    main()
