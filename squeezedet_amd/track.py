"""Object identities for the filtered detection rows, on the device (csrc/track.hip; include/sqdet.h, "tracking"): the stage
behind ``filter_prediction`` for ``demo.py --mode video --track`` and for a serving caller with a bank of cameras.  The reference
has no counterpart; the definition is the header's (tests/track_reference.py restates it sequentially in NumPy).

  * ``Tracker(streams, device, **params)`` owns the state tables of `streams` independent streams (64 track slots each).
    ``update(boxes, probs, cls, counts, frames_per_stream=1)``: ONE asynchronous launch on the current stream over the
    ``S * frames_per_stream`` images of the call -> ``(det_track_id, det_track_state)`` int32 [n, rows]: per detection row the id
    of its track (-1: none) and the track's state (1 tentative, 2 confirmed; 0: none).  Nothing is allocated while shapes stay.
  * ``make_track_items(...)``: the confirmed rows as a ``viz.DrawItems`` -- "<name> #<id>", one colour per id -- for ``viz.draw``.

Parameters (PARAMS): iou_thresh, high_thresh, low_thresh, min_hits, max_age, w_pos, w_vel.
"""
import ctypes as C

from .stream_tables import StreamTables, tables_struct

CAP = 64
PARAMS = dict(iou_thresh=0.3, high_thresh=0.5, low_thresh=0.1, min_hits=3, max_age=30, w_pos=1.0 / 20, w_vel=1.0 / 160)
INT_FIELDS = ("cls", "id", "state", "hits", "miss", "age")
FIELDS = ("x", "P") + INT_FIELDS + ("score", "next_id", "dropped")
# BGR, one per id (id % len): distinct hues that read on road scenes
PALETTE = ((255, 191, 0), (0, 191, 255), (255, 0, 191), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 128, 255), (255, 0, 0),
           (128, 0, 255), (0, 255, 191), (191, 255, 0), (255, 128, 128))


_Tables = tables_struct(FIELDS)                  # sqdet_track_tables_t


class _Params(C.Structure):                      # sqdet_track_params_t
    _fields_ = [("iou_thresh", C.c_double), ("high_thresh", C.c_double), ("low_thresh", C.c_double), ("w_pos", C.c_double),
                ("w_vel", C.c_double), ("min_hits", C.c_int32), ("max_age", C.c_int32)]


def table_shapes(streams):
    """{name: (shape, torch dtype name)} of the state tables of `streams` streams."""
    S = int(streams)
    d = {"x": ((S, CAP, 4, 2), "float64"), "P": ((S, CAP, 4, 3), "float64")}
    d.update({f: ((S, CAP), "int32") for f in INT_FIELDS})
    d.update({"score": ((S, CAP), "float32"), "next_id": ((S,), "int32"), "dropped": ((S,), "int32")})
    return d


class Tracker(StreamTables):
    FIELDS, STRUCT, RESET = FIELDS, _Tables, {"next_id": 1}

    def __init__(self, streams, device, tables=None, **params):
        """tables: {name: device tensor} of the caller's own (a serving arena; tests' guarded buffers) in the shapes and dtypes of
        ``table_shapes(streams)``, already reset; None: the tracker allocates them."""
        from ._lib import SqdetError
        if int(streams) < 1:
            raise SqdetError("Tracker: streams must be positive")
        unknown = set(params) - set(PARAMS)
        if unknown:
            raise SqdetError("Tracker: unknown parameter(s) %s (known: %s)" % (sorted(unknown), sorted(PARAMS)))
        super().__init__(streams, device, table_shapes(streams), tables)
        p = self.params = dict(PARAMS, **params)
        self._params = _Params(float(p["iou_thresh"]), float(p["high_thresh"]), float(p["low_thresh"]), float(p["w_pos"]),
                               float(p["w_vel"]), int(p["min_hits"]), int(p["max_age"]))
        self._out = None

    def update(self, boxes, probs, cls, counts, frames_per_stream=1, stream=None, max_workgroups=0, out=None):
        """boxes float32 [n, rows, 4] (cx, cy, w, h), probs float32 [n, rows], cls int32 [n, rows], counts int32 [n] -- the
        outputs of ops.detect_filter / filter_prediction_batch -- with n = streams * frames_per_stream; image s*F + f is frame f
        of stream s.  stream: a torch stream (None: the current one).  max_workgroups > 0 bounds the launch's workgroups.
        -> (det_track_id, det_track_state), reused by the next call of the same shape (or `out`, a pair of int32 [n, rows])."""
        import torch
        from . import ops
        from ._lib import SqdetError, check, lib
        F, n, rows = self._frames(boxes, frames_per_stream)
        if tuple(probs.shape) != (n, rows) or tuple(cls.shape) != (n, rows) or tuple(counts.shape) != (n,):
            raise SqdetError("Tracker.update: probs / cls must be [n, rows], counts [n]")
        if boxes.device != self.device:
            raise SqdetError("Tracker.update: rows on %s, tables on %s" % (boxes.device, self.device))
        if out is None:
            if self._out is None or tuple(self._out[0].shape) != (n, rows):
                self._out = (torch.empty((n, rows), dtype=torch.int32, device=self.device),
                             torch.empty((n, rows), dtype=torch.int32, device=self.device))
            out = self._out
        if tuple(out[0].shape) != (n, rows) or tuple(out[1].shape) != (n, rows):
            raise SqdetError("Tracker.update: out must be two int32 [%d, %d]" % (n, rows))
        check(lib().sqdet_track_update(
            C.byref(self._tables), ops._dev(boxes, "boxes", torch.float32), ops._dev(probs, "probs", torch.float32),
            ops._dev(cls, "cls", torch.int32), ops._dev(counts, "counts", torch.int32), self.streams, F, rows, C.byref(self._params),
            ops._dev(out[0], "det_track_id", torch.int32), ops._dev(out[1], "det_track_state", torch.int32), int(max_workgroups),
            self._stream(stream)), "sqdet_track_update")
        return out

    def tracks(self, s):
        """The live slots of stream s on the host (synchronises): a list of dicts -- slot, id, cls, state, hits, miss, age, score,
        box (cx, cy, w, h), velocity -- in ascending slot."""
        t = {f: getattr(self, f)[s].cpu().numpy() for f in FIELDS[:-2]}
        return [dict(slot=k, id=int(t["id"][k]), cls=int(t["cls"][k]), state=int(t["state"][k]), hits=int(t["hits"][k]),
                     miss=int(t["miss"][k]), age=int(t["age"][k]), score=float(t["score"][k]),
                     box=tuple(float(v) for v in t["x"][k, :, 0]), velocity=tuple(float(v) for v in t["x"][k, :, 1]))
                for k in range(CAP) if t["state"][k] != 0]

    def _settings(self):
        return {"params": dict(self.params)}

    def _settings_error(self, d):
        return "saved with parameters %s, this tracker has %s" % (d["params"], self.params)


def make_track_items(boxes, probs, cls, counts, det_track_id, det_track_state, names, plot_thresh=0.0, palette=PALETTE,
                     anchor="bottom_left", out=None):
    """The rows of confirmed tracks -> viz.DrawItems, on the device (sqdet_track_build_items): image i keeps, in order, its rows
    j < counts[i] with det_track_state == 2, det_track_id > 0 and probs > plot_thresh; the label is "<name> #<id>", the colour
    palette[id % len(palette)] -- palette a list of (b, g, r) or a uint8 device tensor [k, 3]; names a list or pack_names(...)'s
    tensor."""
    import torch
    from . import ops, viz
    from ._lib import check, lib, stream_ptr
    B, M, names, palette, out = viz._item_tables(
        "make_track_items", boxes, ("float32",),
        [(t, what + " must be [%(B)d, %(M)d]") for t, what in ((probs, "probs"), (cls, "cls"), (det_track_id, "det_track_id"),
                                                               (det_track_state, "det_track_state"))],
        (counts, "counts must be [%(B)d]"), names, palette, out)
    if M == 0:
        return out
    check(lib().sqdet_track_build_items(
        ops._dev(boxes, "boxes", torch.float32), ops._dev(probs, "probs", torch.float32), ops._dev(cls, "cls", torch.int32),
        ops._dev(counts, "counts", torch.int32), ops._dev(det_track_id, "det_track_id", torch.int32),
        ops._dev(det_track_state, "det_track_state", torch.int32), B, M, float(plot_thresh), ops._dev(names, "names", torch.uint8),
        int(names.shape[0]), ops._dev(palette, "palette", torch.uint8), int(palette.shape[0]), viz.ANCHORS[anchor],
        ops._dev(out.rows, "items"), ops._dev(out.counts, "item counts", torch.int32), out.cap, stream_ptr()), "sqdet_track_build_items")
    return out
