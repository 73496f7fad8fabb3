"""What Tracker (track.py) and MotAccumulator (mot.py) share through stream_tables.StreamTables, and viz.make_items and
track.make_track_items through viz._item_tables: every error a caller can meet, with its type and its whole text written out
here; checkpoints in the layout that has been saved so far; a reset of some of the streams.  S = 1 .. 3, rows = 1, F = 1."""
import numpy as np
import pytest
import torch

from squeezedet_amd import _lib, mot, track, viz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E, U = _lib.SqdetError, _lib.SqdetUnsupported
PARAMS_TEXT = "{'iou_thresh': %s, 'high_thresh': 0.5, 'low_thresh': 0.1, 'min_hits': 3, 'max_age': 30, 'w_pos': 0.05, 'w_vel': 0.00625}"


def raises(kind, message, fn, *args, **kw):
    with pytest.raises(kind) as e:
        fn(*args, **kw)
    assert type(e.value) is kind and str(e.value) == message


def z(shape, dtype, device=DEV):
    return torch.zeros(shape, dtype=dtype, device=device)


def track_shapes(S):
    """The tracker's tables as they have been saved so far."""
    d = {"x": ((S, 64, 4, 2), torch.float64), "P": ((S, 64, 4, 3), torch.float64)}
    d.update({f: ((S, 64), torch.int32) for f in ("cls", "id", "state", "hits", "miss", "age")})
    d.update({"score": ((S, 64), torch.float32), "next_id": ((S,), torch.int32), "dropped": ((S,), torch.int32)})
    return d


def mot_shapes(S, classes):
    d = {f: ((S, 256), torch.int32) for f in ("obj_id", "obj_cls", "obj_last", "obj_present", "obj_tracked", "obj_frag", "obj_run")}
    d.update({f: ((S, 1024), torch.int32) for f in ("hyp_id", "hyp_cls", "hyp_frames")})
    d.update({"n_obj": ((S,), torch.int32), "n_hyp": ((S,), torch.int32), "status": ((S,), torch.int32),
              "counts": ((S, classes, 5), torch.int64), "iou_sum": ((S, classes), torch.float64), "overlap": ((S, 256, 1024), torch.int32)})
    return d


def filled(shapes, seed):
    """Host tensors of these shapes with no zero and no one in them."""
    rs = np.random.RandomState(seed)
    return {f: torch.from_numpy(rs.randint(2, 1000, size=shape)).to(dt) for f, (shape, dt) in shapes.items()}


def same_bits(got, want, what):
    got, want = got.cpu().contiguous().numpy(), want.cpu().contiguous().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


# ------------------------------------------------------------------------------------------------ constructors, tables --
def test_constructor_errors():
    raises(E, "Tracker: streams must be positive", track.Tracker, 0, DEV)
    raises(E, "Tracker: unknown parameter(s) ['bogus'] (known: ['high_thresh', 'iou_thresh', 'low_thresh', 'max_age', 'min_hits', "
              "'w_pos', 'w_vel'])", track.Tracker, 1, DEV, bogus=1)
    raises(E, "MotAccumulator: streams and classes must be positive", mot.MotAccumulator, 0, DEV, 1)
    raises(E, "MotAccumulator: streams and classes must be positive", mot.MotAccumulator, 1, DEV, 0)
    raises(U, "MotAccumulator: 129 classes (at most 128)", mot.MotAccumulator, 1, DEV, 129)
    raises(E, "MotAccumulator: iou_thresh 0.0 must be in (0, 1]", mot.MotAccumulator, 1, DEV, 1, iou_thresh=0.0)


def test_a_callers_table_of_the_wrong_shape_dtype_or_layout():
    def tables(shapes, **swap):
        return dict({f: z(shape, dt) for f, (shape, dt) in shapes.items()}, **swap)

    T = track_shapes(1)
    raises(E, "Tracker: table x must be a contiguous device float64 (1, 64, 4, 2)", track.Tracker, 1, DEV,
           tables=tables(T, x=z((1, 64, 4, 3), torch.float64)))
    raises(E, "Tracker: table score must be a contiguous device float32 (1, 64)", track.Tracker, 1, DEV,
           tables=tables(T, score=z((1, 64), torch.float64)))
    raises(E, "Tracker: table cls must be a contiguous device int32 (1, 64)", track.Tracker, 1, DEV,
           tables=tables(T, cls=z((1, 128), torch.int32)[:, ::2]))
    raises(E, "Tracker: table next_id must be a contiguous device int32 (1,)", track.Tracker, 1, DEV,
           tables=tables(T, next_id=z((1,), torch.int32, "cpu")))
    M = mot_shapes(1, 2)
    raises(E, "MotAccumulator: table obj_id must be a contiguous device int32 (1, 256)", mot.MotAccumulator, 1, DEV, 2,
           tables=tables(M, obj_id=z((1, 255), torch.int32)))
    raises(E, "MotAccumulator: table iou_sum must be a contiguous device float64 (1, 2)", mot.MotAccumulator, 1, DEV, 2,
           tables=tables(M, iou_sum=z((1, 2), torch.float32)))
    raises(E, "MotAccumulator: table counts must be a contiguous device int64 (1, 2, 5)", mot.MotAccumulator, 1, DEV, 2,
           tables=tables(M, counts=z((1, 2, 10), torch.int64)[:, :, ::2]))
    # and the caller's own tables are the ones used
    mine = tables(T)
    assert all(t.data_ptr() == mine[f].data_ptr() for f, t in track.Tracker(1, DEV, tables=mine).tables().items())
    mine = tables(M)
    assert all(t.data_ptr() == mine[f].data_ptr() for f, t in mot.MotAccumulator(1, DEV, 2, tables=mine).tables().items())


# ------------------------------------------------------------------------------------------------ update --
def test_tracker_update_errors():
    trk = track.Tracker(1, DEV)

    def rows(n=1, device=DEV):
        return [z((n, 1, 4), torch.float32, device), z((n, 1), torch.float32, device), z((n, 1), torch.int32, device),
                z((n,), torch.int32, device)]

    b, p, c, k = rows()
    raises(E, "Tracker.update: boxes must be [n, rows, 4]", trk.update, b[0], p, c, k)
    raises(E, "Tracker.update: boxes must be [n, rows, 4]", trk.update, z((1, 1, 5), torch.float32), p, c, k)
    raises(E, "Tracker.update: 2 images are not 1 streams x 1 frames", trk.update, *rows(2))
    raises(E, "Tracker.update: 1 images are not 1 streams x 0 frames", trk.update, b, p, c, k, frames_per_stream=0)
    raises(E, "Tracker.update: probs / cls must be [n, rows], counts [n]", trk.update, b, z((1, 2), torch.float32), c, k)
    raises(E, "Tracker.update: probs / cls must be [n, rows], counts [n]", trk.update, b, p, c, z((2,), torch.int32))
    raises(E, "Tracker.update: rows on cpu, tables on cuda:0", trk.update, *rows(device="cpu"))
    raises(E, "Tracker.update: out must be two int32 [1, 1]", trk.update, b, p, c, k, out=(z((1, 1), torch.int32), z((1, 2), torch.int32)))
    same_bits(trk.next_id, torch.ones(1, dtype=torch.int32), "a refused call changes nothing")


def test_accumulator_update_errors():
    acc = mot.MotAccumulator(1, DEV, 1)

    def gt(n=1, G=1, device=DEV):
        return (z((n, G, 4), torch.float64, device),) + tuple(z((n, G), torch.int32, device) for _ in range(3)) + (z((n,), torch.int32, device),)

    def rows(n=1, device=DEV):
        return [z((n, 1, 4), torch.float32, device), z((n, 1), torch.int32, device), z((n,), torch.int32, device),
                z((n, 1), torch.int32, device), z((n, 1), torch.int32, device)]

    b, c, k, i, s = rows()
    g = gt()
    raises(E, "MotAccumulator.update: boxes must be [n, rows, 4]", acc.update, b[0], c, k, i, s, g)
    raises(E, "MotAccumulator.update: 2 images are not 1 streams x 1 frames", acc.update, *rows(2), gt(2))
    raises(E, "MotAccumulator.update: ids must be [1, 1]", acc.update, b, c, k, z((1, 2), torch.int32), s, g)
    raises(E, "MotAccumulator.update: counts must be [1]", acc.update, b, c, z((2,), torch.int32), i, s, g)
    raises(E, "MotAccumulator.update: gt is (gt_box, gt_id, gt_cls, gt_flags, gt_count)", acc.update, b, c, k, i, s, g[:4])
    raises(E, "MotAccumulator.update: gt_box must be [1, G, 4]", acc.update, b, c, k, i, s, (g[0][0],) + g[1:])
    raises(E, "MotAccumulator.update: gt_cls must be [1, 1]", acc.update, b, c, k, i, s, g[:2] + (z((1, 2), torch.int32),) + g[3:])
    raises(E, "MotAccumulator.update: gt_count must be [1]", acc.update, b, c, k, i, s, g[:4] + (z((2,), torch.int32),))
    raises(E, "MotAccumulator.update: rows on cpu, ground truth on cpu, tables on cuda:0", acc.update, *rows(device="cpu"), gt(device="cpu"))
    raises(E, "MotAccumulator.update: rows on cuda:0, ground truth on cpu, tables on cuda:0", acc.update, b, c, k, i, s, gt(device="cpu"))


def test_mot_file_errors(tmp_path):
    many = mot.MotGroundTruth({1: [(j + 1, 0, 0, (10.0, 10.0, 4.0, 4.0)) for j in range(65)]})
    raises(U, "MotGroundTruth: 65 objects in a frame (at most 64)", many.arrays)
    path = tmp_path / "results.txt"
    path.write_text("".join("1,%d,0,0,4,4,1,-1,-1,-1\n" % (j + 1) for j in range(65)))
    raises(U, "load_mot_results: 65 rows in a frame (at most 64)", mot.load_mot_results, str(path))
    raises(ValueError, "format must be mot or kitti, not 'csv'", mot.score_files, str(path), str(path), DEV, fmt="csv")


# ------------------------------------------------------------------------------------------------ item wrappers --
def test_item_wrapper_errors_and_empty_tables():
    names = ["car", "pedestrian", "cyclist"]
    b, c, k, p = z((1, 1, 4), torch.float32), z((1, 1), torch.int32), z((1,), torch.int32), z((1, 1), torch.float32)
    two = viz.DrawItems(z((2, 1, viz.ITEM_BYTES), torch.uint8), z((2,), torch.int32))
    raises(E, "make_items: boxes must be [B, M, 4] float32 or float64", viz.make_items, z((1, 1, 4), torch.int32), c, k, names)
    raises(E, "make_items: boxes must be [B, M, 4] float32 or float64", viz.make_items, b[0], c, k, names)
    raises(E, "bounding box format not accepted: corner.", viz.make_items, b, c, k, names, form="corner")
    raises(E, "make_items: classes / probs must be [B, M], counts [B]", viz.make_items, b, z((1, 2), torch.int32), k, names)
    raises(E, "make_items: classes / probs must be [B, M], counts [B]", viz.make_items, b, c, k, names, probs=z((2, 1), torch.float32))
    raises(E, "make_items: classes / probs must be [B, M], counts [B]", viz.make_items, b, c, z((2,), torch.int32), names)
    raises(E, "make_items: 2 class colours for 3 names", viz.make_items, b, c, k, names, class_colors=[(1, 2, 3), (4, 5, 6)])
    raises(E, "make_items: out holds 2 images, boxes 1", viz.make_items, b, c, k, names, out=two)
    raises(E, "make_track_items: boxes must be [B, M, 4] float32", track.make_track_items, z((1, 1, 4), torch.float64), p, c, k, c, c, names)
    raises(E, "make_track_items: probs must be [1, 1]", track.make_track_items, b, z((1, 2), torch.float32), c, k, c, c, names)
    raises(E, "make_track_items: det_track_id must be [1, 1]", track.make_track_items, b, p, c, k, z((2, 1), torch.int32), c, names)
    raises(E, "make_track_items: det_track_state must be [1, 1]", track.make_track_items, b, p, c, k, c, z((1, 2), torch.int32), names)
    raises(E, "make_track_items: counts must be [1]", track.make_track_items, b, p, c, z((2,), torch.int32), c, c, names)
    raises(E, "make_track_items: out holds 2 images, boxes 1", track.make_track_items, b, p, c, k, c, c, names, out=two)
    # no rows: an empty table of one slot per image, whatever `out` is
    e0, e2 = z((2, 0, 4), torch.float32), z((2, 0), torch.int32)
    for empty in (viz.make_items(e0, e2, z((2,), torch.int32), names),
                  track.make_track_items(e0, z((2, 0), torch.float32), e2, z((2,), torch.int32), e2, e2, names)):
        assert (empty.n, empty.cap) == (2, 1) and empty.counts.cpu().tolist() == [0, 0] and empty.decode() == [[], []]


# ------------------------------------------------------------------------------------------------ checkpoints, reset --
def test_state_dict_keys():
    assert sorted(track.Tracker(1, DEV).state_dict()) == sorted(
        ["x", "P", "cls", "id", "state", "hits", "miss", "age", "score", "next_id", "dropped", "params"])
    assert sorted(mot.MotAccumulator(1, DEV, 1).state_dict()) == sorted(
        ["obj_id", "obj_cls", "obj_last", "obj_present", "obj_tracked", "obj_frag", "obj_run", "hyp_id", "hyp_cls", "hyp_frames", "n_obj",
         "n_hyp", "status", "counts", "iou_sum", "overlap", "iou_thresh", "classes"])


def _owners():
    """(owner at S = 3, a checkpoint of it built by hand, a checkpoint with another setting, that one's error)."""
    params = dict(iou_thresh=0.3, high_thresh=0.5, low_thresh=0.1, min_hits=3, max_age=30, w_pos=1.0 / 20, w_vel=1.0 / 160)
    saved = dict(filled(track_shapes(3), 1), params=dict(params))
    yield (track.Tracker(3, DEV), saved, dict(saved, params=dict(params, iou_thresh=0.4)),
           "Tracker.load_state_dict: saved with parameters " + PARAMS_TEXT % "0.4" + ", this tracker has " + PARAMS_TEXT % "0.3",
           dict(saved, x=saved["x"][:2]), "Tracker.load_state_dict: x is (2, 64, 4, 2), expected (3, 64, 4, 2)", {"next_id": 1})
    saved = dict(filled(mot_shapes(3, 2), 2), iou_thresh=0.5, classes=2)
    yield (mot.MotAccumulator(3, DEV, 2), saved, dict(saved, iou_thresh=0.25),
           "MotAccumulator.load_state_dict: saved with iou_thresh 0.25 and 2 classes",
           dict(saved, n_obj=saved["n_obj"][:1]), "MotAccumulator.load_state_dict: n_obj is (1,), expected (3,)", {})


def test_hand_built_checkpoints_load_and_a_subset_of_the_streams_resets():
    for owner, saved, other, other_error, short, short_error, reset_to in _owners():
        fields = [f for f in saved if f not in ("params", "iou_thresh", "classes")]
        before = {f: t.data_ptr() for f, t in owner.tables().items()}
        raises(E, other_error, owner.load_state_dict, other)
        raises(E, short_error, owner.load_state_dict, short)
        assert sorted(owner.tables()) == sorted(fields)
        for f, t in owner.tables().items():                     # a refused checkpoint loads nothing
            same_bits(t, torch.full(tuple(t.shape), reset_to.get(f, 0), dtype=t.dtype), "%s after a refused load" % f)
        owner.load_state_dict(saved)
        for f, t in owner.tables().items():
            assert t.data_ptr() == before[f]
            same_bits(t, saved[f], "%s loaded" % f)
        again = owner.state_dict()
        assert sorted(again) == sorted(saved) and all(again[k] == saved[k] for k in saved if k not in fields)
        owner.reset(streams=[1])
        for f, t in owner.tables().items():
            want = saved[f].clone()
            want[1] = reset_to.get(f, 0)
            same_bits(t, want, "%s after reset([1])" % f)
            assert not bool((want[0] == 0).any()) and not bool((want[2] == 0).any())        # (streams 0 and 2 held no zero to begin with)
        owner.reset()
        for f, t in owner.tables().items():
            same_bits(t, torch.full(tuple(t.shape), reset_to.get(f, 0), dtype=t.dtype), "%s after reset()" % f)
