#!/usr/bin/env python
"""SqueezeDet demo on MI355X: the py3 / HIP counterpart of the reference's src/demo.py -- image_demo (:160-225) and
video_demo (:44-158) -- same call shape (`sess.run([det_boxes, det_probs, det_class], {image_input: [im]})`,
`model.filter_prediction`, PLOT_PROB_THRESH, class colours) with the image preparation (float cast, bilinear
resize to the network input, BGR mean subtraction, demo.py:186-190) done by sqdet_preprocess_bgr on the GPU.
cv2 is replaced by PIL for file I/O.

    python demo.py --input_path 'data/*.png' --out_dir out/ [--weights weights.npz] [--demo_net squeezeDet] [--draw gpu]
    python demo.py --mode video --input_path 'frames/*.png' --out_dir out/ [--crop 500 205 239 439] [--batch 8]
    python demo.py --mode video --input_path 'frames/*.png' --out_dir out/ --track [--track_out tracks.txt]

--draw pil (default): boxes and labels are drawn with PIL on a host-resized copy of the image.  --draw gpu: they are drawn on
the device into the preprocessed network input (squeezedet_amd.viz: one launch, the means added back), in the reference's
cls2clr colours.  --mode video takes a glob of FRAME FILES, sorted by name -- there is no video decoder here -- crops them
(--crop TOP BOTTOM LEFT RIGHT rows / columns cut off, the reference's frame[500:-205, 239:-439]), runs them in batches of
--batch with everything from the mean subtraction to the drawing on the device, and writes <out_dir>/%06d.jpg per frame.
--track (video only) runs the device tracker (squeezedet_amd.track) behind the filter, across batches: the boxes of confirmed
tracks are drawn as "<name> #<id>", one colour per id, in place of the per-detection boxes.  --track_out FILE writes them as
MOT-challenge text, `frame,id,left,top,width,height,score,-1,-1,-1` per confirmed row: frame 1-based, network-input pixels.
--track_opts iou_thresh=0.3,min_hits=3,...: the tracker's parameters (track.PARAMS).  --track_gt FILE scores the tracks against
labelled objects on the device (squeezedet_amd.mot: MOTA, MOTP, IDF1, switches, fragmentations) and prints the summary at the
end; FILE is a KITTI tracking label file (--track_gt_format kitti, per class) or a MOTChallenge gt.txt (mot, one class), its
boxes in network-input pixels, its first frame the first frame file.

--weights: a {variable name: array} file written by squeezedet_amd.weights.save_params (or converted from a
reference checkpoint with squeezedet_amd.weights.from_reference_names); without it seeded synthetic weights
are used (there is no network access to fetch the reference's checkpoint), so the boxes are meaningless but
the whole path runs.  --anchor_shapes FILE: the anchor shapes the weights were trained with (tools/fit_anchors.py, train.py
--anchor_shapes); without the flag an anchor_shapes.json beside --weights is used, else the config's own shapes.
"""
import argparse
import glob
import os
import time

import numpy as np

from squeezedet_amd import drivers

CLS2CLR = {"car": (255, 191, 0), "cyclist": (0, 191, 255), "pedestrian": (255, 0, 191)}      # BGR (demo.py:123-127)


def draw_boxes(img_rgb, boxes, labels, cdict):
    """_draw_box of src/demo.py / src/train.py:51-72 with PIL: cx,cy,w,h boxes, label at the top-left corner."""
    from PIL import ImageDraw
    d = ImageDraw.Draw(img_rgb)
    for (cx, cy, w, h), lab in zip(boxes, labels):
        x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
        bgr = cdict.get(lab.split(":")[0], (0, 255, 0))
        d.rectangle([x1, y1, x2, y2], outline=(bgr[2], bgr[1], bgr[0]), width=2)
        d.text((x1 + 2, y1 + 2), lab, fill=(bgr[2], bgr[1], bgr[0]))
    return img_rgb


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="image", choices=["image", "video"],
                    help="video: --input_path is a glob of frame files, sorted by name (there is no video decoder on this platform)")
    ap.add_argument("--input_path", default="./data/sample.png", help="glob of input images / frames")
    ap.add_argument("--out_dir", default="./data/out/")
    ap.add_argument("--demo_net", default="squeezeDet", choices=drivers.NETS)
    ap.add_argument("--weights", default="")
    ap.add_argument("--anchor_shapes", default="", metavar="FILE",
                    help="anchor shapes the weights were trained with (default: anchor_shapes.json beside --weights, else the config's)")
    ap.add_argument("--gpu", default="0")
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--draw", default="pil", choices=["pil", "gpu"], help="image mode: draw with PIL on the host, or on the device")
    ap.add_argument("--crop", type=int, nargs=4, default=[500, 205, 239, 439], metavar=("T", "B", "L", "R"),
                    help="video: rows cut off the top / bottom and columns off the left / right of every frame")
    ap.add_argument("--batch", type=int, default=1, help="video: frames per forward pass")
    # (the tracking flags exist on the namespace only when given: a run without them has the arguments it always had)
    ap.add_argument("--track", action="store_true", default=argparse.SUPPRESS,
                    help="video: track the detections across frames and draw the confirmed tracks")
    ap.add_argument("--track_out", default=argparse.SUPPRESS, metavar="FILE",
                    help="video, with --track: write the confirmed rows as MOT-challenge text")
    ap.add_argument("--track_opts", default=argparse.SUPPRESS, metavar="K=V,...",
                    help="video, with --track: tracker parameters, e.g. min_hits=2,max_age=10")
    ap.add_argument("--track_gt", default=argparse.SUPPRESS, metavar="FILE",
                    help="video, with --track: labelled objects to score the tracks against (MOTA, MOTP, IDF1), printed at the end")
    ap.add_argument("--track_gt_format", default=argparse.SUPPRESS, choices=["kitti", "mot"],
                    help="video, with --track_gt: a KITTI tracking label file (default) or a MOTChallenge gt.txt")
    drivers.add_nms_args(ap)        # (these too exist on the namespace only when given)
    a = ap.parse_args(argv)
    drivers.check_nms_args(ap, a)
    if (hasattr(a, "track_gt") and not hasattr(a, "track")) or (hasattr(a, "track_gt_format") and not hasattr(a, "track_gt")):
        ap.error("--track_gt needs --track, --track_gt_format needs --track_gt")
    if hasattr(a, "track") and a.mode != "video":
        ap.error("--track needs --mode video")
    if (hasattr(a, "track_out") or hasattr(a, "track_opts")) and not hasattr(a, "track"):
        ap.error("--track_out / --track_opts need --track")
    if a.mode == "video":
        assert a.demo_net in ("squeezeDet", "squeezeDet+"), "Selected nueral net architecture not supported: {}".format(a.demo_net)
        if a.batch < 1 or min(a.crop) < 0:
            ap.error("--batch must be positive, --crop non-negative")
    return a


def make_model(a, batch):
    from squeezedet_amd import synthetic, weights
    mc = drivers.make_config(a.demo_net, anchor_shapes=drivers.driver_anchor_shapes(a.anchor_shapes, a.weights))
    model = drivers.build_model(mc, a.demo_net, a.gpu, a.dtype, batch)     # parameters are restored below (demo.py:171-172)
    drivers.nms_policy(a, model.mc)     # --nms ...: image, video and tracking modes all filter through the model
    model.load_params(weights.load_params(a.weights) if a.weights else synthetic.synthetic_params(model, seed=0))
    return mc, model, drivers.torch_dtype(a.dtype)


def detect_and_draw(model, input_image, n):
    """The first n images of the network input with their detections above PLOT_PROB_THRESH drawn, all on the device: detect,
    filter_prediction, the item build (the reference's cls2clr as the per-class table, "<name>: (<prob>)") and one draw launch
    -> (uint8 RGB [n, H, W, 3] device tensor, counts of drawn boxes [n] device tensor)."""
    from squeezedet_amd import viz
    mc = model.mc
    det_boxes, det_probs, det_class = model.detect(input_image)
    ob, op, oc, _, cnt = model.filter_prediction_batch(det_boxes[:n].contiguous(), det_probs[:n].contiguous(), det_class[:n].contiguous())
    items = viz.make_items(ob, oc, cnt, list(mc.CLASS_NAMES), probs=op, plot_thresh=mc.PLOT_PROB_THRESH,
                           class_colors=[CLS2CLR.get(c, (0, 255, 0)) for c in mc.CLASS_NAMES], label="name: (p)")
    return viz.draw(input_image[:n].contiguous(), items, bgr_means=mc.BGR_MEANS, order="rgb"), items.counts


def image_demo(a):
    import torch
    from PIL import Image
    from squeezedet_amd import ops
    from squeezedet_amd.nn_skeleton import Session
    mc, model, dtype = make_model(a, 1)
    os.makedirs(a.out_dir, exist_ok=True)
    with Session() as sess:
        for f in glob.iglob(a.input_path):
            bgr_host = drivers.read_bgr(f)
            bgr = torch.from_numpy(bgr_host).to(model.device)
            input_image = ops.preprocess_bgr(bgr[None], mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, dtype)
            out = os.path.join(a.out_dir, "out_" + os.path.split(f)[1])
            if a.draw == "gpu":
                pics, counts = detect_and_draw(model, input_image, 1)
                Image.fromarray(pics[0].cpu().numpy()).save(out)
                nbox = int(counts[0])
            else:
                det_boxes, det_probs, det_class = sess.run([model.det_boxes, model.det_probs, model.det_class],
                                                           feed_dict={model.image_input: input_image})
                final_boxes, final_probs, final_class = model.filter_prediction(det_boxes[0], det_probs[0], det_class[0])
                keep = [i for i in range(len(final_probs)) if final_probs[i] > mc.PLOT_PROB_THRESH]
                labels = [mc.CLASS_NAMES[final_class[i]] + ": (%.2f)" % final_probs[i] for i in keep]
                # boxes are in network-input coordinates: draw on the resized image like the reference does
                im = Image.fromarray(np.ascontiguousarray(bgr_host[:, :, ::-1])).resize((mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT), Image.BILINEAR)
                draw_boxes(im, [final_boxes[i] for i in keep], labels, CLS2CLR)
                im.save(out)
                nbox = len(keep)
            print("Image detection output saved to {} ({} boxes above {:.2f})".format(out, nbox, mc.PLOT_PROB_THRESH))


def video_demo(a):
    """video_demo of src/demo.py:44-158 over frame files, --batch frames at a time.  A cropped frame that is not of the network's
    input size is resized to it by the preprocessing, and the boxes are drawn on that input (the reference feeds the crop as it is)."""
    import torch
    from PIL import Image
    from squeezedet_amd import ops
    mc, model, dtype = make_model(a, a.batch)
    os.makedirs(a.out_dir, exist_ok=True)
    frames = sorted(glob.glob(a.input_path))
    top, bottom, left, right = a.crop
    count = 0
    tracker = VideoTracker(a, mc, model.device) if getattr(a, "track", False) else None
    for i0 in range(0, len(frames), a.batch):
        t_start = time.time()
        crops = []
        for f in frames[i0:i0 + a.batch]:
            frame = drivers.read_bgr(f)
            frame = frame[top:frame.shape[0] - bottom, left:frame.shape[1] - right, :]
            assert frame.size, "--crop {} leaves nothing of {} ({} x {})".format(a.crop, f, *drivers.read_bgr(f).shape[:2])
            crops.append(frame)
        n = len(crops)
        crops += [crops[-1]] * (a.batch - n)               # the last batch is padded with its last frame
        batch = torch.from_numpy(np.stack(crops)).to(model.device)
        input_image = ops.preprocess_bgr(batch, mc.IMAGE_HEIGHT, mc.IMAGE_WIDTH, mc.BGR_MEANS, dtype)     # mean subtraction on the device
        torch.cuda.synchronize(model.device)
        t_reshape = time.time()
        det = model.detect(input_image)
        torch.cuda.synchronize(model.device)
        t_detect = time.time()
        ob, op, oc, _, cnt = model.filter_prediction_batch(det[0][:n].contiguous(), det[1][:n].contiguous(), det[2][:n].contiguous())
        torch.cuda.synchronize(model.device)
        t_filter = time.time()
        from squeezedet_amd import viz
        if tracker is not None:
            items = tracker.items(ob, op, oc, cnt, count)      # only the n real frames: the padding never reaches the tracker
        else:
            items = viz.make_items(ob, oc, cnt, list(mc.CLASS_NAMES), probs=op, plot_thresh=mc.PLOT_PROB_THRESH,
                                   class_colors=[CLS2CLR.get(c, (0, 255, 0)) for c in mc.CLASS_NAMES], label="name: (p)")
        pics = viz.draw(input_image[:n].contiguous(), items, bgr_means=mc.BGR_MEANS, order="rgb").cpu().numpy()
        for im in pics:
            count += 1
            Image.fromarray(im).save(os.path.join(a.out_dir, str(count).zfill(6) + ".jpg"))
        print("Total time: {:.4f}, detection time: {:.4f}, filter time: {:.4f}".format(time.time() - t_start, t_detect - t_reshape,
                                                                                        t_filter - t_detect))
    if tracker is not None and tracker.acc is not None:
        print(tracker.summary())


class VideoTracker:
    """--track: one stream of tracks across the batches of video_demo (S = 1, F = the batch's real frames)."""

    def __init__(self, a, mc, device):
        import torch
        from squeezedet_amd import track, viz
        opts = {}
        for kv in filter(None, getattr(a, "track_opts", "").split(",")):
            k, _, v = kv.partition("=")
            opts[k.strip()] = int(v) if k.strip() in ("min_hits", "max_age") else float(v)
        self.track, self.mc = track, mc
        self.tracker = track.Tracker(1, device, **opts)
        self.names = viz.pack_names(list(mc.CLASS_NAMES), device)
        self.palette = torch.tensor(np.asarray(track.PALETTE, np.uint8)).to(device)
        self.path = getattr(a, "track_out", "")
        if self.path:
            open(self.path, "w").close()           # truncated here, appended to batch by batch: no handle is held across the loop
        self.acc = None
        if getattr(a, "track_gt", ""):             # --track_gt: the tracks are scored where they are, batch by batch
            from squeezedet_amd import mot
            self.mot, self.per_class = mot, getattr(a, "track_gt_format", "kitti") == "kitti"
            self.gt = (mot.MotGroundTruth.from_kitti_tracking(a.track_gt, list(mc.CLASS_NAMES)) if self.per_class
                       else mot.MotGroundTruth.from_mot_text(a.track_gt))
            self.acc = mot.MotAccumulator(1, device, len(mc.CLASS_NAMES) if self.per_class else 1)

    def items(self, ob, op, oc, cnt, frames_before):
        """The draw items of this batch's confirmed tracks; appends their MOT lines (frame = frames_before + 1 + index)."""
        ids, states = self.tracker.update(ob, op, oc, cnt, frames_per_stream=int(ob.shape[0]))
        items = self.track.make_track_items(ob, op, oc, cnt, ids, states, self.names, plot_thresh=self.mc.PLOT_PROB_THRESH,
                                            palette=self.palette)
        if self.acc is not None:
            n = int(ob.shape[0])
            self.acc.update(ob, oc if self.per_class else oc * 0, cnt, ids, states,
                            self.gt.device(ob.device, frames_before + 1, n, self.gt.max_objects), frames_per_stream=n)
        if self.path:
            lines = []
            b, p, n, i, s = (t.cpu().numpy() for t in (ob, op, cnt, ids, states))
            for f in range(b.shape[0]):
                for j in range(min(max(int(n[f]), 0), b.shape[1])):
                    if s[f, j] == 2 and i[f, j] > 0:
                        cx, cy, w, h = (float(v) for v in b[f, j])
                        lines.append("%d,%d,%.2f,%.2f,%.2f,%.2f,%.4f,-1,-1,-1\n" % (frames_before + 1 + f, i[f, j], cx - w / 2, cy - h / 2, w, h,
                                                                                 float(p[f, j])))
            with open(self.path, "a") as out:
                out.writelines(lines)
        return items


    def summary(self):
        """--track_gt: the evaluation of everything seen so far, as text."""
        return self.mot.format_summary(self.acc.evaluate(), list(self.mc.CLASS_NAMES) if self.per_class else ["all"])


def main(argv=None):
    a = parse_args(argv)
    if a.mode == "video":
        video_demo(a)
    else:
        image_demo(a)


if __name__ == "__main__":
    main()
