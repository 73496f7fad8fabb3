#!/usr/bin/env python
"""Scores a COCO-format results file against a COCO-format annotation file on the GPU (squeezedet_amd.coco): any detector's
[{"image_id", "category_id", "bbox": [x, y, w, h], "score"}] list -- eval.py --coco_metrics writes one as coco_results.json --
and prints the twelve lines: AP over IoU 0.50:0.95, AP50, AP75, AP by object size, AR at 1 / 10 / 100 detections, AR by size.

    python tools/coco_eval.py --annotations instances_val.json --results detections.json [--gpu 0]

Limits (include/sqdet.h): 512 results and 128 annotations per image, 128 categories."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--annotations", required=True, metavar="A.json", help="COCO annotation file: images, annotations, categories")
    ap.add_argument("--results", required=True, metavar="R.json", help="COCO results file")
    ap.add_argument("--gpu", default="0", help="gpu id")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from squeezedet_amd import coco
    ev = coco.evaluate_results_file(a.annotations, a.results, torch.device("cuda", int(a.gpu)))
    for line in ev.summarize():
        print(line)
    print("Per-class AP @[ IoU=0.50:0.95 | area=all | maxDets=%d ]:" % int(ev.max_dets[-1]))
    for name, ap in ev.per_class_ap.items():
        print("    {}: {:0.3f}".format(name, ap))
    return ev


if __name__ == "__main__":
    main()
