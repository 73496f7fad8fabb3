"""Training summaries on the device: the reference's tf.summary ops of the train graph (src/train.py:275-299,
src/nn_skeleton.py:340-358,736-755 -- learning rate, loss terms, a histogram of every trainable variable and of its gradient,
and per layer the activation histogram, sparsity, average, max and min) as calls of ONE statistics kernel family
(csrc/summary.hip, sqdet_tensor_stats_many) and one asynchronous copy per summary step.

  * ``default_edges()``: the histogram's bucket table.
  * ``tensor_stats(...)``: the Python face of the kernel; records stay on the device.
  * ``TrainSummary(trainer, train_dir)``: what train.py calls at a summary step; writes ``<train_dir>/summaries.jsonl``.

Divergence from the reference, on purpose: the reference histograms each gradient AFTER tf.clip_by_norm
(nn_skeleton.py:347-358).  Here the clip happens inside the optimizer kernel, so ``<var>/gradients`` describes the UNCLIPPED
gradient in the flat bucket (after the all-reduce); every gradient entry carries ``grad_norm = sqrt(sumsq)`` and
``clip_scale = MAX_GRAD_NORM / max(grad_norm, MAX_GRAD_NORM)`` so that a reader can rescale the edges.
"""
import json
import math
import os

import numpy as np

EDGE_MIN_EXP2, EDGE_MAX_EXP2 = -48, 16        # magnitudes 2^(k/2), k = -48 .. 16: 6e-8 (float16's smallest denormal) .. 256


def default_edges():
    """The fixed float32 bucket table of every histogram: 131 ascending edges, symmetric around 0 -- 0 itself and the
    magnitudes 2^(k/2), k = -48 .. 16, with both signs -- so 130 buckets, the same for every tensor and every step
    (histograms of different steps and tensors can be compared bucket by bucket).  This table is this project's own choice:
    the reference's histograms use TensorBoard's bucket limits, which live inside TensorFlow and are not part of the
    reference's tree.  Odd k is sqrt(2) (correctly rounded) times an exact power of two, so the table does not depend on a
    libm's pow."""
    mags = []
    for k in range(EDGE_MIN_EXP2, EDGE_MAX_EXP2 + 1):
        m = 2.0 ** (k // 2)
        mags.append(np.float32(m * math.sqrt(2.0)) if k % 2 else np.float32(m))
    mags = np.asarray(mags, np.float32)
    return np.concatenate([-mags[::-1], np.zeros(1, np.float32), mags]).astype(np.float32)


def record_dtype(n_bins):
    """NumPy view of one record of sqdet_tensor_stats_many (include/sqdet.h)."""
    return np.dtype([("count", "<i8"), ("nonfinite", "<i8"), ("zeros", "<i8"), ("min", "<f4"), ("max", "<f4"), ("sum", "<f8"),
                     ("sumsq", "<f8"), ("under", "<i8"), ("hist", "<i8", (int(n_bins),)), ("over", "<i8")])


def decode(raw, n_bins):
    """Host bytes of records (a uint8 array / tensor [n, record bytes]) -> structured array [n] of record_dtype(n_bins)."""
    a = raw.numpy() if hasattr(raw, "numpy") else np.asarray(raw)
    return np.ascontiguousarray(a).reshape(-1).view(record_dtype(n_bins))


class StatsPlan:
    """The fixed half of a statistics call over one buffer: edge table, segment table and workspace on the device, allocated
    once, so that run() only launches (no allocation, no synchronisation) and can sit behind a replayed training step.
    offsets / counts: host integers, in elements of the buffer's dtype; checked here against `base_count`, because the
    kernel reads them from the device."""

    def __init__(self, offsets, counts, base_count, device, edges=None):
        import torch
        from . import _lib
        from ._lib import lib
        offs, cnts = np.asarray(offsets, np.int64).reshape(-1), np.asarray(counts, np.int64).reshape(-1)
        if offs.shape != cnts.shape or offs.size == 0:
            raise _lib.SqdetError("tensor_stats: %d offsets for %d counts" % (offs.size, cnts.size))
        if (offs < 0).any() or (cnts < 0).any() or (offs + cnts > int(base_count)).any():
            raise _lib.SqdetError("tensor_stats: a segment leaves the buffer of %d elements" % int(base_count))
        e = default_edges() if edges is None else np.ascontiguousarray(edges, np.float32).reshape(-1)
        if e.size < 2 or not (np.diff(e) > 0).all() or not np.isfinite(e).all():
            raise _lib.SqdetError("tensor_stats: edges must be finite and strictly ascending, at least two")
        self.n, self.n_bins, self.base_count, self.device = int(offs.size), int(e.size) - 1, int(base_count), torch.device(device)
        self.record_bytes = int(lib().sqdet_tensor_stats_record_bytes(self.n_bins))
        ws = int(lib().sqdet_tensor_stats_workspace_bytes(self.n, self.n_bins))
        if not self.record_bytes or not ws:
            raise _lib.SqdetError("tensor_stats: %d bins are not supported" % self.n_bins)
        self.offsets, self.counts = torch.from_numpy(offs).to(self.device), torch.from_numpy(cnts).to(self.device)
        self.edges = torch.from_numpy(e).to(self.device)
        self.workspace = torch.empty(ws // 8 + 1, dtype=torch.int64, device=self.device)

    def run(self, base, out=None):
        """Launches over `base` (a contiguous device tensor of float32 / float16, at least base_count elements) on the
        current stream; returns the records, uint8 [n, record_bytes] on the device (`out` when given)."""
        import torch
        from . import ops
        from ._lib import check, dtype_code, lib, stream_ptr
        if out is None:
            out = torch.empty((self.n, self.record_bytes), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.numel() != self.n * self.record_bytes or int(base.numel()) < self.base_count:
            raise ops._lib.SqdetError("tensor_stats: bad output or buffer size")
        check(lib().sqdet_tensor_stats_many(ops._dev(base, "base"), self.base_count, ops._dev(self.offsets, "offsets"),
                                            ops._dev(self.counts, "counts"), self.n, ops._dev(self.edges, "edges"), self.n_bins,
                                            ops._dev(out, "records"), ops._dev(self.workspace, "workspace"), dtype_code(base.dtype),
                                            stream_ptr()), "sqdet_tensor_stats_many")
        return out


def tensor_stats(src, offsets=None, counts=None, edges=None):
    """Statistics records (include/sqdet.h, sqdet_tensor_stats_many) on the device, uint8 [n, record bytes]; read them with
    ``decode(records.cpu(), n_bins)``.

    ``tensor_stats(flat, offsets, counts)``: n segments [offsets[i], offsets[i] + counts[i]) of one contiguous device buffer,
    ONE launch.  ``tensor_stats([t0, t1, ...])``: one record per tensor, in the list's order; tensors that are views of one
    buffer (the trainers' view / gview) share a launch -- one call per distinct buffer and dtype.  float32 or float16."""
    import torch
    from . import _lib
    if isinstance(src, torch.Tensor):
        if offsets is None:
            offsets, counts = [0], [int(src.numel())]
        plan = StatsPlan(offsets, counts, int(src.numel()), src.device, edges)
        return plan.run(src.reshape(-1))
    tensors = list(src)
    if not tensors:
        raise _lib.SqdetError("tensor_stats: no tensors")
    groups = {}
    for i, t in enumerate(tensors):
        if not t.is_cuda or not t.is_contiguous():
            raise _lib.SqdetError("tensor_stats: tensor %d must be a contiguous device tensor" % i)
        groups.setdefault((t.untyped_storage().data_ptr(), t.dtype, t.device), []).append(i)
    n_bins = (len(default_edges()) if edges is None else int(np.asarray(edges).size)) - 1
    out = None
    for (sptr, dt, dev), idx in groups.items():
        es = tensors[idx[0]].element_size()
        offs = [(tensors[i].data_ptr() - sptr) // es for i in idx]
        cnts = [int(tensors[i].numel()) for i in idx]
        total = tensors[idx[0]].untyped_storage().nbytes() // es
        whole = torch.empty(0, dtype=dt, device=dev).set_(tensors[idx[0]].untyped_storage(), 0, (total,))
        rec = StatsPlan(offs, cnts, total, dev, edges).run(whole)
        if out is None:
            out = torch.empty((len(tensors), rec.shape[1]), dtype=torch.uint8, device=dev)
        out[torch.tensor(idx, device=dev)] = rec
    assert out.shape[1] == record_dtype(n_bins).itemsize
    return out


def _entry(r, hist=True):
    """One record as the JSON entry of summaries.jsonl; the histogram trimmed to its non-empty range."""
    finite = int(r["count"]) - int(r["nonfinite"])
    e = dict(count=int(r["count"]), nonfinite=int(r["nonfinite"]), zeros=int(r["zeros"]), min=float(r["min"]), max=float(r["max"]),
             sum=float(r["sum"]), sumsq=float(r["sumsq"]), average=(float(r["sum"]) / finite if finite else 0.0))
    if hist:
        h = np.asarray(r["hist"])
        nz = np.flatnonzero(h)
        lo, hi = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
        e.update(under=int(r["under"]), over=int(r["over"]), hist_first=lo, hist=[int(v) for v in h[lo:hi]])
    return e


def _json_safe(o):
    """inf / NaN are not JSON: written as strings."""
    if isinstance(o, float) and not math.isfinite(o):
        return repr(o)
    if isinstance(o, dict):
        return {k: _json_safe(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_json_safe(v) for v in o]
    return o


LOSS_TERMS = ("class_loss", "conf_loss", "bbox_loss")
DISTILL_TERMS = ("distill_class_loss", "distill_conf_loss", "distill_bbox_loss")       # a trainer with a teacher adds them to its step's outputs


class TrainSummary:
    """``TrainSummary(trainer, train_dir)``; at a summary step ``record(step, out, learning_rate)`` with the dict of the eager
    ``trainer.step(..., keep_activations=True)``.  It issues one statistics call over ``flat_params``, one over ``flat_grads``
    (entries ``<var>`` and ``<var>/gradients``, the reference's names), one per kept activation
    (``activation_summary/<layer>``: histogram, sparsity = zeros / count, average, max, min) and ONE asynchronous copy of all
    records and the three loss terms into pinned memory behind an event -- no host synchronisation per tensor.  The line goes to
    ``<train_dir>/summaries.jsonl`` once the event has completed: at ``poll()``, at the latest at the next ``record()`` or at
    ``close()``.  The edge table is written once, to ``<train_dir>/summary_edges.json``.

    ``loss`` = class_loss + conf_loss + bbox_loss + the weight decay term (the reference's total of the 'losses'
    collection), the decay from the variables' sumsq records, i.e. of the variables AFTER the step's update."""

    def __init__(self, trainer, train_dir, edges=None, write=True):
        import torch
        self.tr, self.dir, self.write = trainer, train_dir, bool(write)
        self.edges = default_edges() if edges is None else np.ascontiguousarray(edges, np.float32)
        self.n_bins = len(self.edges) - 1
        tr = trainer
        offs = [(tr.view[n].data_ptr() - tr.flat_params.data_ptr()) // 4 for n in tr.names]
        cnts = [int(tr.view[n].numel()) for n in tr.names]
        self.plan = StatsPlan(offs, cnts, tr.total, tr.dev, self.edges)         # serves flat_params and flat_grads: same layout
        self.rb = self.plan.record_bytes
        self._act_plans, self._rows, self._dev, self._host, self._loss_host = {}, 0, None, None, None
        self._event, self._pending = torch.cuda.Event(), None
        self.lines = 0
        if self.write:
            os.makedirs(train_dir, exist_ok=True)
            with open(os.path.join(train_dir, "summary_edges.json"), "w") as f:
                json.dump({"edges": [float(v) for v in self.edges]}, f)

    def _buffers(self, rows):
        import torch
        if rows != self._rows:
            self._dev = torch.empty((rows, self.rb), dtype=torch.uint8, device=self.tr.dev)
            self._host = torch.empty((rows, self.rb), dtype=torch.uint8).pin_memory()
            self._loss_host = torch.zeros(6, dtype=torch.float32).pin_memory()      # (three terms; six under a teacher)
            self._rows = rows

    def record(self, step, out, learning_rate):
        import torch
        self.drain()                                    # the pinned buffers are free again
        tr, nv = self.tr, len(self.tr.names)
        acts = list(out.get("activations", {}).items())
        with torch.cuda.device(tr.dev):
            self._buffers(2 * nv + len(acts))
            self.plan.run(tr.flat_params, out=self._dev[:nv])
            self.plan.run(tr.flat_grads, out=self._dev[nv:2 * nv])
            for k, (name, t) in enumerate(acts):
                n = int(t.numel())
                plan = self._act_plans.get(n)
                if plan is None:
                    plan = self._act_plans[n] = StatsPlan([0], [n], n, tr.dev, self.edges)
                plan.run(t.reshape(-1) if t.is_contiguous() else t.contiguous().reshape(-1), out=self._dev[2 * nv + k:2 * nv + k + 1])
            # (a trainer with a teacher -- DESIGN.md 3.20 -- reports three more terms; without one the three, as ever)
            terms = LOSS_TERMS + (DISTILL_TERMS if DISTILL_TERMS[0] in out else ())
            losses = torch.stack([out[k].reshape(()) for k in terms]).float()
            self._host.copy_(self._dev, non_blocking=True)
            self._loss_host[:len(terms)].copy_(losses, non_blocking=True)
            self._event.record(torch.cuda.current_stream())
        meta = dict(step=int(step), learning_rate=float(learning_rate))
        if tr.half:
            meta.update(loss_scale=float(tr.loss_scale), skipped_steps=int(tr.skipped_steps))
        self._pending = (meta, [a[0] for a in acts], losses)

    def poll(self):
        """Writes the pending line if its copy has landed; never waits."""
        if self._pending is not None and self._event.query():
            self._emit()

    def drain(self):
        if self._pending is not None:
            self._event.synchronize()
            self._emit()

    def close(self):
        self.drain()

    def _emit(self):
        meta, act_names, losses = self._pending
        self._pending, self._pending_terms = None, losses
        tr, nv, mc = self.tr, len(self.tr.names), self.tr.mc
        rec = decode(self._host, self.n_bins)
        cl, co, bb = [float(v) for v in self._loss_host[:3]]
        distill = {k: float(v) for k, v in zip(DISTILL_TERMS, self._loss_host[3:])} if len(self._pending_terms) > 3 else {}
        variables, wd = {}, 0.0
        for i, n in enumerate(tr.names):
            variables[n] = _entry(rec[i])
            if n.endswith("/kernels"):
                wd += float(rec[i]["sumsq"]) * mc.WEIGHT_DECAY / 2
            g = _entry(rec[nv + i])
            norm = math.sqrt(g["sumsq"]) if not g["nonfinite"] else float("nan")
            g["grad_norm"] = norm
            g["clip_scale"] = mc.MAX_GRAD_NORM / max(norm, mc.MAX_GRAD_NORM) if math.isfinite(norm) else float("nan")
            variables[n + "/gradients"] = g
        activations = {}
        for k, n in enumerate(act_names):
            e = _entry(rec[2 * nv + k])
            e["sparsity"] = e["zeros"] / e["count"] if e["count"] else 0.0
            activations["activation_summary/" + n] = e
        line = dict(meta, loss=cl + co + bb + sum(distill.values()) + wd, class_loss=cl, conf_loss=co, bbox_loss=bb, **distill,
                    weight_decay_loss=wd, n_bins=self.n_bins, variables=variables, activations=activations)
        self.last = line
        self.lines += 1
        if self.write:
            with open(os.path.join(self.dir, "summaries.jsonl"), "a") as f:
                f.write(json.dumps(_json_safe(line)) + "\n")
