"""train.py on the GPU at the small shape of the training tests (2 x 128 x 256), dropout on (the nets' training keep_prob):
bitwise resume through squeezedet_amd.checkpoint, summaries that do not perturb training, and the command line end to end
in child processes.  Every child is a fresh process under its own timeout; its exit status is checked before anything else
is started, and at most one of them has the GPU open at a time."""
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--image_size", "128", "256", "--batch_size", "2"]


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("train")


def _args(train_dir, *more):
    return T.parse_args(["--synthetic", "12", "--seed", "3", "--train_dir", str(train_dir), "--summary_step", "0"] + SMALL + list(more))


def _end_state(run):
    run.close()
    torch.cuda.synchronize()
    tr = run.tr
    return dict(flat_params=tr.flat_params.clone(), flat_accum=tr.flat_accum.clone(), global_step=tr.global_step,
                loss_scale=tr.loss_scale, skipped_steps=tr.skipped_steps, mask_calls=tr._mask_calls,
                next_batch=list(run.reader.next_plan().batch_idx))


def _bits(t):
    return t.view(torch.int32)


def _assert_same(a, b):
    for k in ("global_step", "loss_scale", "skipped_steps", "mask_calls", "next_batch"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert torch.equal(_bits(a["flat_params"]), _bits(b["flat_params"])), "flat_params differ"
    assert torch.equal(_bits(a["flat_accum"]), _bits(b["flat_accum"])), "flat_accum differ"


# float16: the run starts from a loss scale of 2^16.  Established on an MI355X: at this shape and seed the float16 gradients
# overflow at every scale above 8192 (a run started at 2^24 skipped its first 11 steps), so the first steps here are skipped,
# the scale halved each time, and the steps behind them update: the checkpoint at step k - 1 carries a lowered scale,
# skipped_steps > 0 AND real updates.  Asserted below, on the straight run and at the save.
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_resume_is_bitwise(tmp_path, dtype):
    """N steps straight against k steps, checkpoint.save, a NEW model, trainer and reader, checkpoint.load, N - k steps."""
    N, k = 12, 5
    more = ["--dtype", dtype] + (["--loss_scale", str(2.0 ** 16)] if dtype == "fp16" else [])
    a = T.Run(_args(tmp_path / "straight", *more))
    for s in range(N):
        a.step(s)
    want = _end_state(a)
    print("straight run: global_step %d, loss_scale %g, skipped_steps %d" % (want["global_step"], want["loss_scale"], want["skipped_steps"]))
    if dtype == "fp16":
        assert want["skipped_steps"] > 0 and want["loss_scale"] < 2.0 ** 16
    assert want["global_step"] + want["skipped_steps"] == N and want["global_step"] > 0
    del a
    args = _args(tmp_path / "resumed", *more)
    os.makedirs(args.train_dir)
    b = T.Run(args)
    for s in range(k):
        b.step(s)
    b.save(k - 1)
    if dtype == "fp16":
        assert b.tr.skipped_steps > 0 and b.tr.global_step > 0, "the saved state must carry a lowered loss scale and real updates"
    b.close()
    del b
    from squeezedet_amd import checkpoint
    assert checkpoint.latest(args.train_dir) == k - 1
    c = T.Run(args, resume_step=k - 1)
    assert c.first == k
    for s in range(k, N):
        c.step(s)
    _assert_same(want, _end_state(c))


def test_trainer_state_rejects_another_model(tmp_path):
    from squeezedet_amd._lib import SqdetError
    a = T.Run(_args(tmp_path / "a", "--no_graph"))
    d = a.tr.state_dict()
    bad = dict(d, names=d["names"][:-1], shapes=d["shapes"][:-1])
    with pytest.raises(SqdetError):
        a.tr.load_state_dict(bad)
    with pytest.raises(SqdetError):
        a.tr.load_state_dict(dict(d, half=True))
    a.tr.load_state_dict(d)                           # and its own state loads


def test_summaries_do_not_perturb_training(tmp_path):
    """The same run with summary_step 2 and with 0: the final variables are bitwise equal -- which also pins the eager summary
    steps (activations kept, conv1 and pool1 as separate launches) against the graph-replayed ones inside one run.  float32:
    every float32 form of the stem is bitwise the conv -> pool pair (tests/test_gpu_ops.py)."""
    N = 6
    res = []
    for ss in ("2", "0"):
        args = _args(tmp_path / ("s" + ss))
        args.summary_step = int(ss)
        os.makedirs(args.train_dir)
        r = T.Run(args)
        for s in range(N):
            r.step(s)
        res.append(_end_state(r))
        if ss == "2":
            lines = [json.loads(l) for l in open(os.path.join(args.train_dir, "summaries.jsonl"))]
            assert [l["step"] for l in lines] == [0, 2, 4]
        del r
    _assert_same(res[0], res[1])


# ------------------------------------------------------------------------------------------- the command line, end to end --
def _kitti_tree(root, n=6, seed=5):
    from PIL import Image
    rs = np.random.RandomState(seed)
    for d in ("training/image_2", "training/label_2", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    names = []
    for i in range(n):
        h, w = [(122, 250), (126, 254), (131, 262), (134, 266)][i % 4]
        im = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        name = "%06d" % i
        Image.fromarray(im).save(os.path.join(root, "training", "image_2", name + ".png"))
        rows = []
        for j in range(int(rs.randint(1, 4))):
            bw, bh = rs.uniform(30, 70), rs.uniform(25, 50)
            x0, y0 = rs.uniform(16, w - bw - 2), rs.uniform(8, h - bh - 2)
            rows.append("%s 0.00 0 0.00 %.2f %.2f %.2f %.2f 1.50 1.60 3.90 1.00 1.00 10.00 0.00"
                        % (("Car", "Pedestrian", "Cyclist")[int(rs.randint(3))], x0, y0, x0 + bw, y0 + bh))
        with open(os.path.join(root, "training", "label_2", name + ".txt"), "w") as f:
            f.write("\n".join(rows) + "\n")
        names.append(name)
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")


def _child(args, timeout=300):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    print(r.stdout[-3000:])
    print(r.stderr[-3000:])
    return r


def _tree_listing(d):
    return sorted((os.path.relpath(os.path.join(p, f), d), os.path.getsize(os.path.join(p, f)), os.path.getmtime(os.path.join(p, f)))
                  for p, _, fs in os.walk(d) for f in fs)


def test_command_line_end_to_end(tmp_path):
    import squeezedet_amd as S
    from squeezedet_amd import nets, synthetic, weights
    ev = _load("eval")
    data = str(tmp_path / "KITTI")
    _kitti_tree(data)
    d1, d2 = str(tmp_path / "run"), str(tmp_path / "straight")
    common = ["--data_path", data, "--image_set", "train", "--checkpoint_step", "3", "--summary_step", "2"] + SMALL
    r = _child(common + ["--train_dir", d1, "--max_steps", "6"])
    assert r.returncode == 0, "train.py failed"
    assert "step 0, loss = " in r.stdout and "conf_loss: " in r.stdout
    for s in (0, 3, 5):
        assert os.path.exists(os.path.join(d1, "model.ckpt-%d.npz" % s)) and os.path.exists(os.path.join(d1, "state", "step-%d.npz" % s))
    assert ev.latest_checkpoint(d1) == os.path.join(d1, "model.ckpt-5.npz")
    # the checkpoint loads into a fresh inference model, and detect runs
    mc = S.kitti_squeezeDet_config_for_input(128, 256)
    mc.LOAD_PRETRAINED_MODEL, mc.BATCH_SIZE = False, 2
    model = nets.SqueezeDet(mc, "0", dtype=torch.float32)
    params = weights.load_params(ev.latest_checkpoint(d1))
    assert set(params) == set(model.params)                     # ALL variables, the frozen conv1 included
    model.load_params(params)
    boxes, probs, cls = model.detect(synthetic.synthetic_images(2, 128, 256, seed=1).to(DEV))
    torch.cuda.synchronize()
    assert tuple(boxes.shape) == (2, mc.ANCHORS, 4) and bool(torch.isfinite(probs).all())
    # the training changed the trainable variables and left the frozen conv1 alone
    p0 = weights.load_params(os.path.join(d1, "model.ckpt-0.npz"))
    assert np.array_equal(p0["conv1/kernels"], params["conv1/kernels"]) and not np.array_equal(p0["conv12/kernels"], params["conv12/kernels"])
    # summaries: steps 0, 2, 4, every trainable variable, its gradient, every activation
    lines = [json.loads(l) for l in open(os.path.join(d1, "summaries.jsonl"))]
    assert [l["step"] for l in lines] == [0, 2, 4]
    fires = ["fire%d" % i for i in range(2, 12)]
    act_names = ["conv1", "pool1", "pool3", "pool5", "drop", "conv12"] + fires + [f + "/squeeze1x1" for f in fires]
    trainable = [n for n in model.params if model.trainable[n]]
    assert "conv1/kernels" not in trainable and len(trainable) > 40
    for l in lines:
        for key in ("learning_rate", "loss", "class_loss", "conf_loss", "bbox_loss"):
            assert np.isfinite(l[key]), key
        assert l["learning_rate"] == mc.LEARNING_RATE
        for n in trainable:
            for name in (n, n + "/gradients"):
                e = l["variables"][name]
                assert e["count"] == model.params[n].numel(), name
                assert e["under"] + sum(e["hist"]) + e["over"] == e["count"] - e["nonfinite"]
            g = l["variables"][n + "/gradients"]
            assert g["grad_norm"] == math.sqrt(g["sumsq"]) and 0 < g["clip_scale"] <= 1
        assert len(l["variables"]) == 2 * len(trainable)
        assert set(l["activations"]) == set("activation_summary/" + n for n in act_names)
        for e in l["activations"].values():
            assert e["count"] > 0 and 0.0 <= e["sparsity"] <= 1.0 and e["min"] <= e["average"] <= e["max"]
    # model_metrics.txt: three sections, each total the sum of its rows
    text = open(os.path.join(d1, "model_metrics.txt")).read()
    sections = text.split("\n\n")
    assert [s.split("\n")[0] for s in sections] == ["Number of parameter by layer:", "Activation size by layer:", "Number of flops by layer:"]
    for s in sections:
        rows = [r.strip().split(": ") for r in s.strip().split("\n")[1:]]
        assert rows[-1][0] == "total" and int(rows[-1][1]) == sum(int(v) for _, v in rows[:-1]) and len(rows) > 10
    # resume to 8 steps against 8 steps straight
    r = _child(common + ["--train_dir", d1, "--max_steps", "8", "--resume"])
    assert r.returncode == 0 and "Resuming from step 5" in r.stdout
    r = _child(common + ["--train_dir", d2, "--max_steps", "8"])
    assert r.returncode == 0
    a, b = weights.load_params(os.path.join(d1, "model.ckpt-7.npz")), weights.load_params(os.path.join(d2, "model.ckpt-7.npz"))
    assert set(a) == set(b)
    for n in a:
        assert np.array_equal(a[n].view(np.int32), b[n].view(np.int32)), n
    # a used directory without --resume / --overwrite: refused, nothing touched
    before = _tree_listing(d1)
    r = _child(common + ["--train_dir", d1, "--max_steps", "8"], timeout=120)
    assert r.returncode != 0 and "--resume" in r.stderr
    assert _tree_listing(d1) == before
