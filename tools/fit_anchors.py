#!/usr/bin/env python
"""Fits anchor shapes to a dataset on the device and reports how the anchors cover it, before and after.

    python tools/fit_anchors.py --dataset PASCAL_VOC --data_path VOCdevkit --year 2007 --image_set trainval --out anchors.json
    python tools/fit_anchors.py --data_path KITTI --image_set train --net squeezeDet --out anchors.json
    python tools/fit_anchors.py --synthetic 40 --out anchors.json                # seeded synthetic data, no dataset needed

--dataset, --data_path, --year, --image_set, --net, --image_size and --synthetic mean what they mean to train.py, so the shapes
are fitted at the network input the training will use.  Only the annotations are read: no image is decoded, the image sizes
come from the image headers.  The object shapes go through squeezedet_amd.anchors.fit_anchor_shapes (k-means under the IoU
distance, --restarts seeded runs at once on the GPU); then the coverage report (squeezedet_amd.anchors.dataset_coverage) is
printed twice, side by side: for the config's current shapes and for the fitted ones.  --out receives the JSON file that
train.py / eval.py / demo.py --anchor_shapes read: shapes, input size, dataset, image set, k, seed, mean IoU.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squeezedet_amd import drivers  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    drivers.add_dataset_args(ap, image_set_default="train")
    drivers.add_model_args(ap, dtype_default=None)         # (--net: its config gives the input size and the grid)
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="the N seeded synthetic images of train.py --synthetic N")
    ap.add_argument("--k", type=int, default=9, help="anchor shapes per grid cell (the nets are built for 9)")
    ap.add_argument("--seed", type=int, default=0, help="seeds the initial centroids (and --synthetic, as train.py --seed does)")
    ap.add_argument("--restarts", type=int, default=8, help="independent k-means runs; the one of highest mean IoU wins")
    ap.add_argument("--max_iter", type=int, default=100, help="iterations per run")
    ap.add_argument("--out", default="anchors.json", help="the JSON file to write")
    a = ap.parse_args(argv)
    if a.dataset not in drivers.DATASETS:           # (a usage error here; train.py and eval.py keep the reference's assert)
        ap.error("--dataset must be KITTI or PASCAL_VOC")
    drivers.check_dataset_args(ap, a)
    if a.k < 1 or a.restarts < 1 or a.max_iter < 1:
        ap.error("--k, --restarts and --max_iter must be positive")
    return a


def load_annotations(a, mc):
    """(rois, sizes [(height, width)], dataset label): annotations and image headers only."""
    if a.synthetic:
        images, rois = drivers.synthetic_data(mc, a.synthetic, a.seed)
        return rois, [im.shape[:2] for im in images], "synthetic-%d" % a.synthetic
    from PIL import Image
    data = drivers.load_index(a.dataset, a.data_path, a.year, a.image_set, mc)
    sizes = []
    for p in data.image_paths:
        with Image.open(p) as im:                    # reads the header; the pixels are never decoded
            sizes.append((im.size[1], im.size[0]))
    return data.rois, sizes, a.dataset


def main(argv=None):
    a = parse_args(argv)
    import torch
    from squeezedet_amd import anchors, config
    mc = drivers.base_config(a.net, a.image_size, a.dataset)       # (before any head padding: the classes are the real ones)
    rois, sizes, label = load_annotations(a, mc)
    device = torch.device("cuda", int(a.gpu))
    wh = anchors.dataset_shapes(rois, sizes, mc)
    print("{} objects in {} images of {} ({}), network input {} x {}".format(len(wh), len(rois), label, a.image_set, mc.IMAGE_HEIGHT,
                                                                            mc.IMAGE_WIDTH))
    fit = anchors.fit_anchor_shapes(wh, k=a.k, seed=a.seed, restarts=a.restarts, max_iter=a.max_iter, device=device)
    print("restart {} of {} wins: mean IoU {:.6f} after {} iterations (all restarts: {})".format(
        fit.restart, a.restarts, fit.mean_iou, fit.iters, " ".join("%.6f" % v for v in fit.restart_mean_iou)))
    print("fitted shapes (w, h; members):")
    for (w, h), c in zip(fit.shapes, fit.counts):
        print("  {:9.3f} {:9.3f}   {:d}".format(w, h, int(c)))
    fitted_mc = config.with_anchor_shapes(mc, fit.shapes)
    before = anchors.dataset_coverage(mc, rois, sizes, device=device)
    after = anchors.dataset_coverage(fitted_mc, rois, sizes, device=device)
    print(anchors.format_reports([before, after], ["current", "fitted"]))
    anchors.save_anchor_shapes(a.out, fit.shapes, mc, dataset=label, image_set=a.image_set, k=a.k, seed=a.seed, mean_iou=fit.mean_iou,
                               restarts=a.restarts, iters=fit.iters, coverage_current=before.summary(), coverage_fitted=after.summary())
    print("Anchor shapes saved to {}".format(a.out))
    if a.k not in anchors.RUNNABLE_ANCHOR_COUNTS:
        print("note: train.py / eval.py / demo.py build nets for {} anchors per cell and will refuse this file".format(
            " or ".join(str(c) for c in anchors.RUNNABLE_ANCHOR_COUNTS)))
    return fit


if __name__ == "__main__":
    main()
