"""Records tests/golden/voc_ap.npz: for every case of voc_ap_cases.py, what the reference's own Pascal VOC evaluation computes.

    python tests/golden/make_voc_ap_golden.py          (only where the reference tree is present)

Per case the reference's pascal_voc.evaluate_detections is driven itself -- an instance made with __new__, the fields it reads
set by hand, all_boxes built as the reference's eval.py:90-91 builds them (bbox_transform of the float32 filter row + [score])
-- so the per-class detection files are the reference's too; then voc_eval is called on those files for rec / prec and both AP
forms.  Recorded: '<case>:annotations_sha256', '<case>:detections_sha256' (voc_ap_cases.digest_dir) and, per class,
'<case>:<cls>:rec', ':prec', ':ap07', ':ap_area' (a class without detections: empty curves, AP 0, as voc_eval.py:147-148).

Nothing of the reference is copied: its two modules are read at run time.  pascal_voc.py is executed unchanged, with in-memory
stand-ins for what it imports and cannot have here (cv2, utils.util, dataset.imdb -- none of them used by evaluate_detections)
and `xrange`.  voc_eval.py is Python 2; its text is adjusted in memory before it is compiled: the two print statements,
cPickle -> pickle, the cache file opened in binary mode, np.bool -> bool.

The generator asserts that no two detections of one class print the same score, in every case but `ties`: the reference's
np.argsort(-confidence) is not stable, so only untied cases (and `ties`, built so that the order cannot matter) pin it."""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import voc_ap_cases as VC  # noqa: E402
from oracle.ref_numpy_half import REFERENCE_ROOT  # noqa: E402
_mods = None


def available():
    return os.path.exists(os.path.join(REFERENCE_ROOT, "src", "dataset", "voc_eval.py"))


def _load():
    """(pascal_voc module, voc_eval module) of the reference."""
    global _mods
    if _mods is not None:
        return _mods
    sys.dont_write_bytecode = True
    src = os.path.join(REFERENCE_ROOT, "src", "dataset")
    with open(os.path.join(src, "voc_eval.py")) as f:
        text = f.read()
    for old, new in (("import cPickle\n", "import pickle as cPickle\n"),
                     ("print 'Reading annotation for {:d}/{:d}'.format(", "print('Reading annotation for {:d}/{:d}'.format("),
                     ("i + 1, len(imagenames))\n", "i + 1, len(imagenames)))\n"),
                     ("print 'Saving cached annotations to {:s}'.format(cachefile)", "print('Saving cached annotations to {:s}'.format(cachefile))"),
                     ("with open(cachefile, 'w') as f:", "with open(cachefile, 'wb') as f:"),
                     ("with open(cachefile, 'r') as f:", "with open(cachefile, 'rb') as f:"),
                     (".astype(np.bool)", ".astype(bool)")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    voc_eval = types.ModuleType("dataset.voc_eval")
    exec(compile(text, os.path.join(src, "voc_eval.py"), "exec"), voc_eval.__dict__)
    names = ("cv2", "utils", "utils.util", "dataset", "dataset.imdb", "dataset.voc_eval")
    saved = {k: sys.modules.get(k) for k in names}
    try:
        from squeezedet_amd.util import bbox_transform_inv
        stubs = {k: types.ModuleType(k) for k in names[:-1]}
        stubs["utils.util"].bbox_transform_inv = bbox_transform_inv
        stubs["dataset.imdb"].imdb = type("imdb", (object,), {})
        sys.modules.update(stubs)
        sys.modules["dataset.voc_eval"] = voc_eval
        spec = importlib.util.spec_from_file_location("sqdet_ref_pascal_voc", os.path.join(src, "pascal_voc.py"))
        pascal_voc = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(pascal_voc)
        pascal_voc.xrange = range
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    _mods = (pascal_voc, voc_eval)
    return _mods


def all_boxes_of(case):
    """all_boxes[cls][image] as the reference's eval.py:90-91 fills it: bbox_transform(b) + [s] of the float32 rows."""
    out = [[[] for _ in case["image_idx"]] for _ in case["names"]]
    for i, (b, p, c) in enumerate(case["rows"]):
        for k in range(len(p)):
            cx, cy, w, h = b[k]
            out[int(c[k])][i].append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2] + [p[k]])
    return out


def run_reference(name):
    """{key: value} of one case, as recorded in voc_ap.npz."""
    pascal_voc, voc_eval = _load()
    case = VC.make_case(name)
    out = {}
    with tempfile.TemporaryDirectory() as root:
        voc = VC.write_tree(case, root)
        db = pascal_voc.pascal_voc.__new__(pascal_voc.pascal_voc)
        db._classes, db._image_idx = case["names"], case["image_idx"]
        db._data_root_path, db._year, db._image_set = root, VC.YEAR, VC.IMAGE_SET
        eval_dir = os.path.join(root, "eval")
        os.makedirs(eval_dir)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            aps07, _ = db.evaluate_detections(eval_dir, "0", all_boxes_of(case))
        det_dir = os.path.join(eval_dir, "detection_files_0")
        out[name + ":annotations_sha256"] = np.array(VC.digest_dir(os.path.join(voc, "Annotations")))
        out[name + ":detections_sha256"] = np.array(VC.digest_dir(det_dir))
        for c, cls in enumerate(case["names"]):
            with open(os.path.join(det_dir, cls + ".txt")) as f:
                scores = [line.split(" ")[1] for line in f]
            assert name == "ties" or len(set(scores)) == len(scores), (name, cls, "equal score texts")
            args = (os.path.join(det_dir, "{:s}.txt"), os.path.join(voc, "Annotations", "{:s}.xml"),
                    os.path.join(voc, "ImageSets", "Main", VC.IMAGE_SET + ".txt"), cls, os.path.join(root, "annotations_cache"))
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                rec, prec, ap07 = voc_eval.voc_eval(*args, ovthresh=0.5, use_07_metric=True)
                _, _, ap_area = voc_eval.voc_eval(*args, ovthresh=0.5, use_07_metric=False)
            assert float(ap07) == float(aps07[c]) or (np.isnan(ap07) and np.isnan(aps07[c]))
            key = "%s:%s:" % (name, cls)
            out[key + "rec"] = np.atleast_1d(np.asarray(rec, np.float64)) if scores else np.zeros(0)
            out[key + "prec"] = np.atleast_1d(np.asarray(prec, np.float64)) if scores else np.zeros(0)
            out[key + "ap07"], out[key + "ap_area"] = np.float64(ap07), np.float64(ap_area)
    return out


def main():
    out = {}
    for name in VC.CASES:
        r = run_reference(name)
        out.update(r)
        case = VC.make_case(name)
        print(name, " ".join("%s %.4f/%.4f" % (c, r["%s:%s:ap07" % (name, c)], r["%s:%s:ap_area" % (name, c)]) for c in case["names"][:6]))
    np.savez_compressed(os.path.join(HERE, "voc_ap.npz"), **out)


if __name__ == "__main__":
    main()
