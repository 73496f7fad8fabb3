#!/usr/bin/env python
"""Evaluates SqueezeDet checkpoints on KITTI or Pascal VOC (the reference's src/eval.py) in batches, scored on the GPU.

    python eval.py --data_path KITTI --image_set val --checkpoint_path ckpt/model-20000.npz --run_once [--net squeezeDet]
    python eval.py --dataset PASCAL_VOC --data_path VOCdevkit --year 2007 --image_set test --checkpoint_path ... --run_once

The reference's order per image: det_boxes rescaled to the original image size (float32, eval.py:83-84), then
filter_prediction, then the rows added to the detection table -- here a whole batch at a time on the device
(filter_prediction_batch, squeezedet_amd.kitti_ap.KittiEvaluator).  The table is scored by the GPU KITTI evaluator
(or, with --eval_tool, by an external evaluate_object binary through kitti_eval.evaluate_detections).  Outputs under
--eval_dir: detection_files_<step>/data/*.txt, the evaluator's stats_<cls>_{ap,detection}.txt, error_analysis/
det_error_file.txt, and one JSON line per checkpoint in eval_log.jsonl (in place of TF summaries).  --visualize N: N example
detections per error type of that file, each drawn on the device over its original image (imdb.visualize_detections) to
error_analysis/<type>/<i>.png; the rows are chosen by a permutation seeded with --seed.

--dataset PASCAL_VOC reads <data_path>/VOC<year> (squeezedet_amd.voc.load_voc; any dataset in VOC XML format), runs
SqueezeDet with the 20-class config at --image_size and scores the table with the GPU VOC evaluator
(squeezedet_amd.voc.VocEvaluator): it prints '<cls>: AP = ...' and 'Mean AP = ...' as pascal_voc.evaluate_detections does
and writes detection_files_<step>/<cls>.txt and the eval_log.jsonl line.  --eval_tool, the error analysis and --visualize
are KITTI-only.  (The net's ConvDet head is padded from 20 to 23 classes, the padding pinned to probability 0: DESIGN.md section 3.9.)

--coco_metrics (either dataset): the same filter rows also fill a squeezedet_amd.coco.CocoEvaluator, and after the dataset's
own scoring the COCO-style AP over IoU 0.50:0.95 / AR at 1, 10, 100 detections are printed (twelve lines), added to the
eval_log.jsonl record as "coco" and the table written to detection_files_<step>/coco_results.json.  For KITTI this is a
localisation metric over KITTI's boxes, not KITTI's protocol (CocoGroundTruth.from_kitti).

--anchor_shapes FILE: the net's anchors take the shapes of that file (tools/fit_anchors.py, train.py --anchor_shapes); without
the flag an anchor_shapes.json beside the checkpoint -- train.py leaves one in its --train_dir -- is used, else the config's own.

--ema: evaluate the exponential moving average of the weights that train.py --ema_decay keeps: under
--run_once the file <dir>/ema/<name> of --checkpoint_path <dir>/<name>, which must exist; otherwise <checkpoint_path>/ema is polled.

Checkpoints are .npz files from squeezedet_amd.weights.save_params.  --run_once: --checkpoint_path is that file;
otherwise it is a directory polled every --eval_interval_secs for the newest '*-<step>.npz'.  Every image is scored
once (the last batch is padded; the reference's reader wraps around instead).
"""
import argparse
import glob
import json
import os
import time

import numpy as np

from squeezedet_amd import drivers


class EvalArgs(argparse.Namespace):
    """parse_args' result.  --coco_metrics is off through this class attribute, not through an argparse default, so vars() of
    a run without the flag holds exactly the options it held before the flag existed; with the flag it is an instance attribute."""
    coco_metrics = False
    ema = False                 # (--ema, likewise)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[1], formatter_class=argparse.RawDescriptionHelpFormatter)
    drivers.add_dataset_args(ap, image_set_default="test")
    drivers.add_model_args(ap, dtype_default="fp32")       # (--image_size: PASCAL_VOC only, main refuses it for KITTI)
    ap.add_argument("--eval_dir", default="/tmp/squeezeDet/eval", help="where results are written")
    ap.add_argument("--checkpoint_path", default="/tmp/squeezeDet/train", help="a .npz file (--run_once) or a directory")
    ap.add_argument("--eval_interval_secs", type=int, default=60, help="how often to look for a new checkpoint")
    ap.add_argument("--run_once", action="store_true", help="evaluate --checkpoint_path once and exit")
    ap.add_argument("--batch_size", type=int, default=0, help="images per forward pass (default: the config's)")
    ap.add_argument("--eval_tool", default="", help="score with this evaluate_object binary instead of the GPU evaluator")
    ap.add_argument("--synthetic_weights", action="store_true", help="seeded synthetic weights instead of a checkpoint")
    ap.add_argument("--visualize", type=int, default=0, metavar="N",
                    help="draw N example detections per error type of the error analysis (the reference draws 10; 0: none)")
    ap.add_argument("--seed", type=int, default=0, help="seeds the choice of the rows --visualize draws")
    ap.add_argument("--anchor_shapes", default="", metavar="FILE",
                    help="anchor shapes the checkpoint was trained with (default: anchor_shapes.json beside the checkpoint, else the config's)")
    ap.add_argument("--coco_metrics", action="store_true", default=argparse.SUPPRESS,
                    help="also score the detections COCO-style: AP over IoU 0.50:0.95 by object size, AR at 1 / 10 / 100 detections")
    ap.add_argument("--ema", action="store_true", default=argparse.SUPPRESS,
                    help="evaluate the averaged weights of a run trained with --ema_decay: <dir>/ema/<name> of the file under --run_once, "
                         "else the directory <checkpoint_path>/ema is polled")
    drivers.add_nms_args(ap)
    a = ap.parse_args(argv, namespace=EvalArgs())
    drivers.check_dataset_args(ap, a)
    drivers.check_nms_args(ap, a)
    return a


def make_model(net, gpu, dtype, batch_size=0, anchor_shapes=None, image_size=None, dataset="KITTI"):
    """(config, model) of --net for the dataset: drivers.make_config, then the nets class on it."""
    mc = drivers.make_config(net, image_size, dataset, anchor_shapes)
    return mc, drivers.build_model(mc, net, gpu, dtype, batch_size)


def read_image(path, model):
    """PIL -> BGR uint8 (what cv2.imread returns) -> ops.preprocess_bgr: network input [1,H,W,3] and (x_scale, y_scale)
    = network size / original size (imdb.read_image_batch)."""
    import torch
    from squeezedet_amd import ops
    mc = model.mc
    bgr = torch.from_numpy(drivers.read_bgr(path)).to(model.device)
    orig_h, orig_w = float(bgr.shape[0]), float(bgr.shape[1])
    x = ops.preprocess_bgr(bgr[None], mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, model.dtype)
    return x, (mc.IMAGE_WIDTH / orig_w, mc.IMAGE_HEIGHT / orig_h)


def detect_batch(model, paths):
    """Images of `paths` into one batch tensor of mc.BATCH_SIZE (padded with the last image) -> det_boxes, det_probs,
    det_class (device, BATCH_SIZE rows) and the real images' scales."""
    import torch
    mc = model.mc
    batch = torch.empty((mc.BATCH_SIZE, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, 3), dtype=model.dtype, device=model.device)
    scales = []
    for j, p in enumerate(paths):
        batch[j:j + 1], s = read_image(p, model)
        scales.append(s)
    if len(paths) < mc.BATCH_SIZE:
        batch[len(paths):] = batch[len(paths) - 1:len(paths)]
    return model.detect(batch) + (scales,)


def rescale_boxes(det_boxes, scales):
    """det_boxes[j, :, 0::2] /= scales[j][0]; det_boxes[j, :, 1::2] /= scales[j][1] (eval.py:83-84) on the device, float32
    divided by the float32 scale as NumPy does."""
    import torch
    n = len(scales)
    s = torch.tensor(np.tile(np.asarray(scales, np.float32).reshape(n, 1, 2), (1, 1, 2)), device=det_boxes.device)  # x, y, x, y
    return det_boxes[:n] / s


VIS_COLOR = (200, 200, 0)       # RGB (imdb.py:285)


def visualize_detections(image_dir, image_format, det_error_file, output_image_dir, num_det_per_type, seed, device):
    """imdb.visualize_detections (src/dataset/imdb.py:254-305): num_det_per_type rows per error type of det_error_file, each
    drawn over its original-size image -- rectangle and "<class> (<score>)" at its top-left corner, colour (200, 200, 0) RGB --
    to <output_image_dir>/<type>/<i>.png.  The image goes to the device as uint8 and is drawn there (squeezedet_amd.viz).  The
    reference shuffles the lines with random.shuffle; here their order is RandomState(seed).permutation, so that a run can
    be repeated.  Returns [(error type, i, line number)] of what was drawn."""
    import shutil
    import torch
    from PIL import Image
    from squeezedet_amd import viz
    with open(det_error_file) as f:
        lines = f.read().splitlines()
    dets_per_type = {}
    for k in np.random.RandomState(seed).permutation(len(lines)):
        obj = lines[k].strip().split(" ")
        dets_per_type.setdefault(obj[1], []).append((int(k), obj))
    drawn = []
    for error_type, dets in dets_per_type.items():
        det_im_dir = os.path.join(output_image_dir, error_type)
        if os.path.exists(det_im_dir):
            shutil.rmtree(det_im_dir)
        os.makedirs(det_im_dir)
        for i, (k, obj) in enumerate(dets[:num_det_per_type]):
            bgr = torch.from_numpy(drivers.read_bgr(os.path.join(image_dir, obj[0] + image_format))[None]).to(device)
            x0, y0, x1, y1 = (int(float(v)) for v in obj[2:6])
            label = "{:s} ({:.2f})".format(obj[6], float(obj[7]))
            items = viz.pack_items([[(x0, y0, x1, y1, VIS_COLOR[::-1], label, "top_left")]], device)
            pic = viz.draw(bgr, items, order="rgb")
            Image.fromarray(pic[0].cpu().numpy()).save(os.path.join(det_im_dir, str(i) + image_format))
            drawn.append((error_type, i, k))
    return drawn


def load_weights(a, model, ckpt_path):
    """Loads the checkpoint (or the seeded synthetic weights) into the model; returns the global step as text."""
    from squeezedet_amd import weights, synthetic
    from squeezedet_amd.config import pin_padding_classes
    if a.synthetic_weights:
        model.load_params(pin_padding_classes(model.mc, synthetic.synthetic_params(model, seed=0)))
        global_step = "0"
    else:
        from squeezedet_amd.kitti_ap import parse_checkpoint_step
        model.load_params(pin_padding_classes(model.mc, weights.load_params(ckpt_path)))
        global_step = parse_checkpoint_step(ckpt_path)
    return global_step


def detect_all(model, data, evaluator, coco=None):
    """Every image of the set through the detector and the filter into the evaluator's table, a batch at a time (coco: a second
    table that receives the same rows).  Returns (detections, seconds in detect, seconds in the rest, batches)."""
    import torch
    mc = model.mc
    n = len(data.image_idx)
    evaluator.reset()
    if coco is not None:
        coco.reset()
    t_detect = t_misc = 0.0
    counts = []
    for i0 in range(0, n, mc.BATCH_SIZE):
        paths = data.image_paths[i0:i0 + mc.BATCH_SIZE]
        t0 = time.time()
        det_boxes, det_probs, det_class, scales = detect_batch(model, paths)
        torch.cuda.synchronize(model.device)
        t1 = time.time()
        k = len(paths)
        boxes = rescale_boxes(det_boxes, scales)
        ob, op, oc, oi, cnt = model.filter_prediction_batch(boxes, det_probs[:k].contiguous(), det_class[:k].contiguous())
        evaluator.add_rows(ob, op, oc, cnt, i0)
        if coco is not None:
            coco.add_rows(ob, op, oc, cnt, i0)
        counts.append(cnt)
        torch.cuda.synchronize(model.device)
        t2 = time.time()
        t_detect += t1 - t0
        t_misc += t2 - t1
        print("im_detect: {:d}/{:d} detect: {:.3f}s misc: {:.3f}s".format(i0 + k, n, t_detect / (i0 // mc.BATCH_SIZE + 1),
                                                                         t_misc / (i0 // mc.BATCH_SIZE + 1)))
    num_detection = int(torch.cat(counts).clamp(min=0).sum().item())
    nb = max(1, (n + mc.BATCH_SIZE - 1) // mc.BATCH_SIZE)
    return num_detection, t_detect, t_misc, nb


def score_kitti(a, model, data, evaluator, result_dir, global_step):
    """The detection files, then the GPU evaluator and its stats files (or --eval_tool on the files) -> (aps, names)."""
    from squeezedet_amd import kitti_eval
    mc = model.mc
    evaluator.write_detection_files(os.path.join(result_dir, "data"), data.image_idx)
    if a.eval_tool:
        all_boxes = kitti_eval.new_all_boxes(len(mc.CLASS_NAMES), len(data.image_idx))
        for i, rows in enumerate(evaluator.tables()):
            for c, x1, y1, x2, y2, s in rows:
                all_boxes[c][i].append([x1, y1, x2, y2, s])
        return kitti_eval.evaluate_detections(a.eval_tool, a.data_path, a.image_set, a.eval_dir, global_step, data.image_idx,
                                              mc.CLASS_NAMES, all_boxes)
    aps, ap_names, _ = evaluator.evaluate()
    evaluator.write_stats(result_dir)
    return aps, ap_names


def analyze_kitti(a, model, data, evaluator, result_dir):
    """kitti.analyze_detections: det_error_file.txt, --visualize and the printed analysis -> the stats dict."""
    print("Analyzing detections...")
    stats = evaluator.analyze()
    det_error_file = os.path.join(result_dir, "error_analysis", "det_error_file.txt")
    evaluator.write_error_file(det_error_file, data.image_idx)
    if a.visualize > 0:
        drawn = visualize_detections(os.path.dirname(data.image_paths[0]), ".png", det_error_file, os.path.dirname(det_error_file),
                                     a.visualize, a.seed, model.device)
        print("Visualized {} detections under {}".format(len(drawn), os.path.dirname(det_error_file)))
    print("Detection Analysis:")
    print("    Number of detections: {}".format(stats["num of detections"]))
    print("    Number of objects: {}".format(stats["num of objects"]))
    print("    Percentage of correct detections: {}".format(stats["% correct detections"]))
    print("    Percentage of localization error: {}".format(stats["% localization error"]))
    print("    Percentage of classification error: {}".format(stats["% classification error"]))
    print("    Percentage of background error: {}".format(stats["% background error"]))
    print("    Percentage of repeated detections: {}".format(stats["% repeated error"]))
    print("    Recall: {}".format(stats["% recall"]))
    return stats


def score_voc(a, model, data, evaluator, result_dir, global_step):
    """pascal_voc.evaluate_detections (:81-137) on the device table: the per-class files and the 'AP =' lines -> (aps, names)."""
    from squeezedet_amd.voc import use_07_metric_for
    evaluator.write_detection_files(result_dir, data.image_idx)
    aps, ap_names = evaluator.evaluate(use_07_metric_for(a.year))
    for cls, ap in zip(ap_names, aps):
        print("{:s}: AP = {:.4f}".format(cls, ap))
    print("Mean AP = {:.4f}".format(np.mean(aps)))
    return aps, ap_names


def score_coco(coco, result_dir):
    """--coco_metrics: the twelve lines and coco_results.json -> the record's "coco" entry."""
    stats = coco.evaluate()
    print("COCO-style metrics:")
    for line in coco.summarize():
        print(line)
    os.makedirs(result_dir, exist_ok=True)
    coco.write_results_json(os.path.join(result_dir, "coco_results.json"))
    return {"stats": [float(v) for v in stats], "per_class_ap": coco.per_class_ap}


def eval_once(a, model, data, ckpt_path, evaluator, coco=None):
    """One checkpoint: its weights, every image into the evaluator's table, the dataset's scoring (score_kitti and
    analyze_kitti, or score_voc), the summary and the eval_log.jsonl record (KITTI's carries "analysis"; with coco, a
    CocoEvaluator, also "coco")."""
    voc = a.dataset == "PASCAL_VOC"
    global_step = load_weights(a, model, ckpt_path)
    n = len(data.image_idx)
    num_detection, t_detect, t_misc, nb = detect_all(model, data, evaluator, coco)

    print("Evaluating detections...")
    t0 = time.time()
    result_dir = os.path.join(a.eval_dir, "detection_files_{:s}".format(global_step))
    aps, ap_names = (score_voc if voc else score_kitti)(a, model, data, evaluator, result_dir, global_step)
    t_eval = time.time() - t0

    print("Evaluation summary:")
    print("  Average number of detections per image: {}:".format(num_detection / float(n)))
    policy = drivers.config_nms_policy(model.mc)         # (what the model filtered with: main set it from the --nms flags)
    print("  Suppression: {}".format(drivers.format_nms_policy(policy)))
    print("  Timing:")
    print("    detect: {:.3f}s misc: {:.3f}s eval: {:.3f}s".format(t_detect / nb, t_misc / nb, t_eval))
    print("  Average precisions:")
    for cls, ap in zip(ap_names, aps):
        print("    {}: {:.3f}".format(cls, ap))
    print("    Mean average precision: {:.3f}".format(np.mean(aps)))

    rec = {"global_step": global_step, "checkpoint": ckpt_path, "mAP": float(np.mean(aps)),
           "APs": dict(zip(ap_names, [float(v) for v in aps])), "num_det_per_image": num_detection / float(n),
           "timing": {"im_detect": t_detect / nb, "post_proc": t_misc / nb, "eval": t_eval}}
    if not voc:
        rec["analysis"] = analyze_kitti(a, model, data, evaluator, result_dir)
    if coco is not None:
        rec["coco"] = score_coco(coco, result_dir)
    if not policy["default"]:           # (a run without the --nms flags writes the record it always wrote)
        rec["nms"] = policy
    with open(os.path.join(a.eval_dir, "eval_log.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    return rec


def latest_checkpoint(directory):
    """The newest '*-<step>.npz' in directory (largest step), or None."""
    from squeezedet_amd.kitti_ap import parse_checkpoint_step
    best = None
    for p in glob.glob(os.path.join(directory, "*-*.npz")):
        step = parse_checkpoint_step(p)
        if step.isdigit() and (best is None or int(step) > best[0]):
            best = (int(step), p)
    return best[1] if best else None


def ema_checkpoint_path(checkpoint_path, run_once):
    """--ema: where the averaged weights of train.py --ema_decay lie.  A file (--run_once) <dir>/<name> resolves to
    <dir>/ema/<name> and must exist; a directory to poll becomes <dir>/ema."""
    from squeezedet_amd import checkpoint
    if not run_once:
        return os.path.join(checkpoint_path, checkpoint.EMA_DIR)
    path = checkpoint.ema_of(checkpoint_path)
    if not os.path.isfile(path):
        raise SystemExit("--ema: %s does not exist (train.py writes it beside a checkpoint when it runs with --ema_decay)" % path)
    return path


def main(argv=None):
    a = parse_args(argv)
    if a.ema:
        if a.synthetic_weights:
            raise SystemExit("--ema reads a checkpoint's averaged weights: not with --synthetic_weights")
    raw_checkpoint_path = a.checkpoint_path           # (anchor_shapes.json lies beside the raw checkpoint, not under ema/)
    if a.ema:
        a.checkpoint_path = ema_checkpoint_path(a.checkpoint_path, a.run_once)
    if a.dataset == "PASCAL_VOC":
        for flag, given in (("--eval_tool", a.eval_tool), ("--visualize", a.visualize)):
            if given:
                raise SystemExit("%s is KITTI-only: the external evaluator and the error analysis have no Pascal VOC form" % flag)
        from squeezedet_amd.voc import VocEvaluator as Evaluator
    else:
        if a.image_size is not None:
            raise SystemExit("--image_size is for --dataset PASCAL_VOC (the KITTI nets run at their configs' size)")
        from squeezedet_amd.kitti_ap import KittiEvaluator as Evaluator
    shapes = drivers.driver_anchor_shapes(a.anchor_shapes, raw_checkpoint_path)
    mc, model = make_model(a.net, a.gpu, a.dtype, a.batch_size, shapes, a.image_size, a.dataset)
    drivers.nms_policy(a, model.mc)         # --nms ...: the rule model.filter_prediction_batch thins every image's rows with
    data = drivers.load_index(a.dataset, a.data_path, a.year, a.image_set, mc)
    evaluator = Evaluator(mc, data.gt, model.device)
    coco = None
    if a.coco_metrics:
        from squeezedet_amd.coco import CocoEvaluator, CocoGroundTruth
        cgt = CocoGroundTruth.from_voc(data.gt, mc.CLASS_NAMES) if a.dataset == "PASCAL_VOC" else CocoGroundTruth.from_kitti(data.gt, mc)
        coco = CocoEvaluator(mc, cgt, model.device)
    os.makedirs(a.eval_dir, exist_ok=True)
    if a.run_once:
        return eval_once(a, model, data, a.checkpoint_path, evaluator, coco)
    seen = set()
    while True:
        ckpt = latest_checkpoint(a.checkpoint_path)
        if ckpt is None:
            print("No checkpoint file found")
        elif ckpt not in seen:
            seen.add(ckpt)
            print("Evaluating {}...".format(ckpt))
            eval_once(a, model, data, ckpt, evaluator, coco)
            continue
        print("Wait {:d}s for new checkpoints to be saved ... ".format(a.eval_interval_secs))
        time.sleep(a.eval_interval_secs)


if __name__ == "__main__":
    main()
