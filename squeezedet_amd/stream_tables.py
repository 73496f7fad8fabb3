"""The per-stream device tables under the tracker and its evaluator (csrc/stream_wave.h: one wave per stream): ``Tracker``
(track.py) and ``MotAccumulator`` (mot.py) derive from ``StreamTables``, which holds the tables -- its own or the caller's --
their ctypes struct, reset and checkpointing, and the checks of a call over S streams x F frames; they add their settings,
their launches and what they read back."""
import ctypes as C

from ._lib import SqdetError, stream_ptr


def tables_struct(fields):
    """The C struct of one device pointer per field (sqdet_track_tables_t, sqdet_mot_tables_t)."""
    return type("_Tables", (C.Structure,), {"_fields_": [(f, C.c_void_p) for f in fields]})


class StreamTables:
    """Tables of `streams` independent streams on `device`, every one indexed by the stream first.  A subclass names them
    (FIELDS, STRUCT = tables_struct(FIELDS)), says what a reset leaves in those that are not zero (RESET) and supplies
    _settings(): what state_dict() stores beside the tables, and _settings_error(d) for a checkpoint whose settings differ."""
    FIELDS, STRUCT, RESET = (), None, {}

    def __init__(self, streams, device, shapes, tables=None):
        """shapes: {name: (shape, torch dtype name)}.  tables: {name: device tensor} of the caller's own (a serving arena; tests'
        guarded buffers) in those shapes and dtypes, already reset; None: allocated here."""
        import torch
        self.who = type(self).__name__
        self.streams, self.device = int(streams), torch.device(device)
        for f, (shape, dtype) in shapes.items():
            if tables is None:
                t = torch.full(shape, self.RESET.get(f, 0), dtype=getattr(torch, dtype), device=self.device)
            else:
                t = tables[f]
                if tuple(t.shape) != shape or t.dtype != getattr(torch, dtype) or not t.is_cuda or not t.is_contiguous():
                    raise SqdetError("%s: table %s must be a contiguous device %s %s" % (self.who, f, dtype, shape))
            setattr(self, f, t)
        self._tables = self.STRUCT(*[getattr(self, f).data_ptr() for f in self.FIELDS])

    def tables(self):
        """{name: device tensor}: the tables themselves."""
        return {f: getattr(self, f) for f in self.FIELDS}

    def reset(self, streams=None):
        """Forgets everything of `streams` (a list of stream indices; None: all): every table zero but for RESET's values."""
        import torch
        idx = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=self.device)
        for f in self.FIELDS:
            getattr(self, f)[idx] = self.RESET.get(f, 0)

    def state_dict(self):
        """Host copies of every table and the settings; continuing after load_state_dict is bitwise the uninterrupted run."""
        d = {f: getattr(self, f).cpu().clone() for f in self.FIELDS}
        d.update(self._settings())
        return d

    def load_state_dict(self, d):
        if any(d.get(k, v) != v for k, v in self._settings().items()):
            raise SqdetError("%s.load_state_dict: %s" % (self.who, self._settings_error(d)))
        for f in self.FIELDS:
            if tuple(d[f].shape) != tuple(getattr(self, f).shape):
                raise SqdetError("%s.load_state_dict: %s is %s, expected %s" % (self.who, f, tuple(d[f].shape), tuple(getattr(self, f).shape)))
        for f in self.FIELDS:
            getattr(self, f).copy_(d[f])          # in place: the tables keep their addresses

    def _frames(self, boxes, frames_per_stream):
        """update()'s first checks -> (F, n, rows): boxes [n, rows, 4] with n = streams * F, image s*F + f frame f of stream s."""
        F = int(frames_per_stream)
        if boxes.dim() != 3 or int(boxes.shape[2]) != 4:
            raise SqdetError("%s.update: boxes must be [n, rows, 4]" % self.who)
        n, rows = int(boxes.shape[0]), int(boxes.shape[1])
        if F < 1 or n != self.streams * F:
            raise SqdetError("%s.update: %d images are not %d streams x %d frames" % (self.who, n, self.streams, F))
        return F, n, rows

    @staticmethod
    def _stream(stream):
        """A torch stream (None: the current one) as the C calls take it."""
        return stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
