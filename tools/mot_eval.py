#!/usr/bin/env python
"""Scores a tracking results file against labelled objects on the device (squeezedet_amd.mot; include/sqdet.h, "tracking
evaluation"): MOTA, MOTP, IDF1, identity switches, fragmentations, mostly tracked / mostly lost.

    python tools/mot_eval.py --gt gt.txt --results tracks.txt [--format mot|kitti] [--iou 0.5] [--json]

--results is the MOT-challenge text `demo.py --mode video --track --track_out FILE` writes (frame, id, left, top, w, h, score,
-1, -1, -1; frames count from 1).  --format mot: --gt is a MOTChallenge gt.txt (conf 0 and the distractor classes are ignored
regions); kitti: a KITTI tracking label file (DontCare and unlisted types are ignored regions; frames count from 0 there).  The
results carry no class, so everything is scored as one class."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--results", required=True)
    ap.add_argument("--format", choices=("mot", "kitti"), default="mot")
    ap.add_argument("--iou", type=float, default=0.5)
    ap.add_argument("--classes", default="car,pedestrian,cyclist", help="kitti: the types that are objects (the rest are ignored regions)")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="also print the overall counters and metrics as one JSON line")
    a = ap.parse_args(argv)
    from squeezedet_amd import mot
    result, names = mot.score_files(a.gt, a.results, "cuda:%d" % a.gpu, a.format, a.iou, tuple(a.classes.split(",")))
    print(mot.format_summary(result, names))
    if a.json:
        print(json.dumps(result["overall"]))
    return result


if __name__ == "__main__":
    main()
