"""Records tests/golden/kitti_ap.npz: for every case of kitti_ap_cases.py, the sha256 of its detection files and the
stats files the reference's KITTI evaluator (oracle/_ref/evaluate_object, built by oracle/Makefile) wrote for them.

    python tests/golden/make_kitti_ap_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import cases, kitti_ap_cases as KC  # noqa: E402

TOOL = os.path.join(ROOT, "oracle", "_ref", "evaluate_object")


def run_evaluator(root, result_dir, n):
    subprocess.run([TOOL, os.path.join(root, "training"), os.path.join(root, "ImageSets", "val.txt"), result_dir, str(n)],
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
    return KC.stats_files(result_dir)


def main():
    out = {}
    for name in KC.CASES:
        with tempfile.TemporaryDirectory() as d:
            idxs, result_dir = KC.make_case(name, d)
            out[name + "_detections_sha256"] = cases.kitti_detection_digest(os.path.join(result_dir, "data"))
            stats = run_evaluator(d, result_dir, len(idxs))
            out[name + "_files"] = np.array(sorted(stats))
            for fn, text in stats.items():
                out["%s:%s" % (name, fn)] = np.array(text)
            print(name, len(idxs), "images:", ", ".join("%s %s" % (fn, stats[fn].split()) for fn in sorted(stats) if "_ap" in fn))
    np.savez_compressed(os.path.join(HERE, "kitti_ap.npz"), **out)


if __name__ == "__main__":
    main()
