"""The host half of resumable training: BatchReader.state_dict / load_state_dict, the checkpoint directory's pairing rule
against eval.latest_checkpoint, the summary edge table and train.py's command line.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_root_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dataset(n, seed, classes=3):
    rs = np.random.RandomState(seed)
    images, rois = [], []
    for i in range(n):
        h, w = [(370, 1224), (374, 1238), (376, 1241), (375, 1242)][i % 4]
        images.append(np.zeros((h, w, 3), np.uint8))
        k = rs.randint(1, 6)
        bw, bh = rs.uniform(20, 300, k), rs.uniform(20, 200, k)
        x0, y0 = rs.uniform(0, w - bw - 1), rs.uniform(0, h - bh - 1)
        rois.append([[x0[j] + bw[j] / 2, y0[j] + bh[j] / 2, bw[j], bh[j], int(rs.randint(classes))] for j in range(k)])
    return images, rois


def _reader(n=11, batch=3, seed=5):
    import squeezedet_amd as S
    mc = S.kitti_squeezeDet_config()
    mc.BATCH_SIZE = batch
    assert mc.DATA_AUGMENTATION and mc.DRIFT_X > 0 and mc.DRIFT_Y > 0
    return S.BatchReader(mc, *_dataset(n, seed=17), seed=seed)


def _same(p, q):
    assert list(p.batch_idx) == list(q.batch_idx)
    assert np.array_equal(p.aug, q.aug)
    assert p.label_per_batch == q.label_per_batch
    assert len(p.bbox_per_batch) == len(q.bbox_per_batch)
    for a, b in zip(p.bbox_per_batch, q.bbox_per_batch):
        assert np.array_equal(a, b)


def test_batch_reader_state_round_trip_across_a_reshuffle():
    """k plans, state_dict, m more -- against a second reader built the same way that loads the state and takes m.  11 images in
    batches of 3: a reshuffle every 3 batches (imdb.py:121-123), so with k = 2 the first reshuffle falls on the 2nd of the m."""
    k, m = 2, 7
    a = _reader()
    for _ in range(k):
        a.next_plan()
    state = a.state_dict()
    perm_at_save = list(a._perm_idx)
    want, reshuffled = [], False
    for _ in range(m):
        want.append(a.next_plan())
        reshuffled = reshuffled or list(a._perm_idx) != perm_at_save
    assert reshuffled, "the case must cross a reshuffle"
    # through the file form checkpoint.py uses (np.savez without pickle)
    import io
    buf = io.BytesIO()
    np.savez(buf, **{key: np.asarray(v) for key, v in state.items()})
    buf.seek(0)
    with np.load(buf, allow_pickle=False) as z:
        loaded = {key: (z[key].item() if z[key].ndim == 0 else z[key]) for key in z.files}
    b = _reader()
    b.load_state_dict(loaded)
    for p in want:
        _same(p, b.next_plan())


def test_batch_reader_rejects_the_state_of_another_dataset():
    state = _reader(n=11).state_dict()
    with pytest.raises(ValueError):
        _reader(n=12).load_state_dict(state)


def test_checkpoint_latest_needs_both_files_and_eval_never_sees_state(tmp_path):
    from squeezedet_amd import checkpoint
    ev = _load("eval")
    d = str(tmp_path)
    os.makedirs(os.path.join(d, "state"))
    touch = lambda p: np.savez(p, x=np.zeros(1))
    assert checkpoint.latest(d) is None and ev.latest_checkpoint(d) is None
    touch(os.path.join(d, "model.ckpt-3.npz")); touch(os.path.join(d, "state", "step-3.npz"))
    touch(os.path.join(d, "model.ckpt-7.npz"))                       # no state: not resumable
    touch(os.path.join(d, "state", "step-9.npz"))                    # no model file: the pair was never completed
    touch(os.path.join(d, "state", ".tmp-123.npz")); touch(os.path.join(d, ".tmp-123.npz"))      # writes in flight
    assert checkpoint.latest(d) == 3 and checkpoint.steps(d) == [3]
    assert ev.latest_checkpoint(d) == os.path.join(d, "model.ckpt-7.npz")        # eval needs the model file only
    touch(os.path.join(d, "state", "step-7.npz"))
    assert checkpoint.latest(d) == 7
    touch(os.path.join(d, "state", "step-100.npz"))
    got = ev.latest_checkpoint(d)
    assert got == os.path.join(d, "model.ckpt-7.npz") and os.sep + "state" + os.sep not in got


def test_default_edges_table():
    from squeezedet_amd import summary
    e = summary.default_edges()
    assert e.dtype == np.float32 and e.ndim == 1 and len(e) % 2 == 1
    assert (np.diff(e) > 0).all() and np.isfinite(e).all()
    assert np.array_equal(e, -e[::-1]) and e[len(e) // 2] == 0.0
    assert np.array_equal(e, summary.default_edges())               # fixed: the same table every call
    assert summary.record_dtype(len(e) - 1).itemsize == 48 + 8 * (len(e) + 1)
    # geometric in magnitude: a constant ratio of sqrt(2) between neighbours
    pos = e[len(e) // 2 + 1:].astype(np.float64)
    np.testing.assert_allclose(pos[1:] / pos[:-1], np.sqrt(2.0), rtol=2e-7)


def test_train_parse_args_takes_the_reference_flags():
    tr = _load("train")
    a = tr.parse_args(["--dataset", "KITTI", "--data_path", "/data/KITTI", "--image_set", "trainval", "--train_dir", "/tmp/x",
                       "--max_steps", "77", "--net", "resnet50", "--pretrained_model_path", "w.npz", "--summary_step", "5",
                       "--checkpoint_step", "50", "--gpu", "1"])
    assert (a.dataset, a.data_path, a.image_set, a.train_dir, a.max_steps, a.net, a.pretrained_model_path, a.summary_step,
            a.checkpoint_step, a.gpu) == ("KITTI", "/data/KITTI", "trainval", "/tmp/x", 77, "resnet50", "w.npz", 5, 50, "1")
    d = tr.parse_args([])                                             # the reference's defaults (train.py:27-48)
    assert (d.dataset, d.image_set, d.max_steps, d.net, d.summary_step, d.checkpoint_step, d.gpu) == \
        ("KITTI", "train", 1000000, "squeezeDet", 10, 1000, "0")
    b = tr.parse_args(["--dtype", "fp16", "--batch_size", "2", "--seed", "3", "--resume", "--keep_checkpoints", "2", "--no_graph",
                       "--synthetic", "12", "--image_size", "128", "256"])
    assert (b.dtype, b.batch_size, b.seed, b.resume, b.overwrite, b.keep_checkpoints, b.no_graph, b.synthetic, b.image_size) == \
        ("fp16", 2, 3, True, False, 2, True, 12, [128, 256])
    for net in ("squeezeDet", "squeezeDet+", "resnet50", "vgg16"):
        assert tr.parse_args(["--net", net]).net == net
    with pytest.raises(AssertionError, match="Currently only supports KITTI dataset"):
        tr.parse_args(["--dataset", "VOC"])


def test_train_dir_policy(tmp_path):
    tr = _load("train")
    d = str(tmp_path / "run")
    assert tr.prepare_train_dir(tr.parse_args(["--train_dir", d]), 0) is None and os.path.isdir(d)
    open(os.path.join(d, "note.txt"), "w").write("x")
    with pytest.raises(SystemExit):
        tr.prepare_train_dir(tr.parse_args(["--train_dir", d]), 0)
    assert os.path.exists(os.path.join(d, "note.txt"))
    with pytest.raises(SystemExit):                                   # nothing to resume from
        tr.prepare_train_dir(tr.parse_args(["--train_dir", d, "--resume"]), 0)
    assert tr.prepare_train_dir(tr.parse_args(["--train_dir", d, "--overwrite"]), 0) is None and os.listdir(d) == []
