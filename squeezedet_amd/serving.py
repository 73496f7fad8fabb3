"""The serving step behind ModelSkeleton.detect_filter_pipelined / warm_up_lanes / flush_pipeline: the network forward and the decode
+ filter of the previous batch as a two-stage pipeline.  A Pipe is one pipeline (two Slots of static buffers used alternately, a
post-processing side stream); a Lane is a HIP stream with a Pipe and a native plan of its own; the model's Serving object holds the
single-lane Pipe and the current set of Lanes.  None of them refers to the model: it is passed to every call and read for `mc`,
`anchors_f32()`, `_native_plan`, `_to_input`, `run`, `serve_lanes` and `_latency_probe`; nothing is installed on it."""
import os

import numpy as np
import torch

from . import nms, ops
from ._lib import SqdetError

# Every environment knob of the serving step and its default.  Read through knob() at each use, never cached: callers (bench.py,
# the tests) change them between calls.
KNOBS = {
    "SQDET_SERVE_LANES": "2",       # batches in flight where neither the `lanes` argument nor model.serve_lanes names a count
    "SQDET_LANE_CHECK": "1",        # 0: warm_up skips the timed check that the lanes' HIP streams run concurrently
    "SQDET_POST_DEFER": "ride",     # deferred decode + filter: riders of the next forward | signal: side stream behind its mid-forward event
    "SQDET_POST_WGS": "16",         # workgroups of a gated (signal) filter launch at batch > 16
    "SQDET_POST_INLINE": None,      # 1: side work goes to the stream current at enqueue time, not the side stream (A/B)
    "SQDET_POST_PRIORITY": "-1",    # priority of a pipe's side stream, read when the stream is created
    "SQDET_SPLIT_POST": None,       # 1: interpret_output + filter_prediction as two launches, not the fused detect_filter (A/B)
    "SQDET_SCORE_EPILOGUE": "1",    # 0: the stand-alone score kernel on the side stream, not ConvDet's score epilogue (A/B)
}


def knob(name):
    return os.environ.get(name, KNOBS[name])


def out_layout(B, M):
    """-> (bytes, views): the filtered rows (boxes [B,M,4] f32, probs [B,M] f32, cls [B,M] i32, anchor index [B,M] i32, count [B] i32)
    as views(flat) of ONE uint8 buffer of `bytes`, each at a 256-byte-aligned offset, so the rows leave the device in a single copy."""
    f32, i32 = torch.float32, torch.int32
    fields, end = [], 0
    for shape, dt in (((B, M, 4), f32), ((B, M), f32), ((B, M), i32), ((B, M), i32), ((B,), i32)):
        nb = int(np.prod(shape)) * 4
        fields.append((end, nb, dt, shape))
        end += (nb + 255) // 256 * 256
    return end, lambda flat: tuple(flat[o:o + nb].view(dt).view(shape) for o, nb, dt, shape in fields)


def _probed(probe, which, call, *args):
    """call(*args); with a probe list (model._latency_probe, bench.py's latency_ms_per_batch) also appends (lane index, (event ahead
    of the call's device work, event behind it)), both recorded on the current stream -- the one the call runs on."""
    if probe is None:
        return call(*args)
    evs = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    evs[0].record()
    out = call(*args)
    evs[1].record()
    probe.append((which, evs))
    return out


class Slot:
    """One set of a pipe's static buffers, its events, and the flags of the call that last used it."""
    __slots__ = ("preds", "det", "flat", "out", "views", "host_flat", "host", "fwd_done", "post_done", "sig",
                 "fused_post", "scored", "to_host", "ride", "post_wgs", "used", "nms")

    def __init__(self, model, plan, B, cur):
        A, N, f32, dev = model.mc.ANCHORS, model.mc.TOP_N_DETECTION, torch.float32, model.device
        nbytes, self.views = out_layout(B, N if 0 < N < A else min(A, 1024))
        self.flat = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.sig = torch.cuda.Event()
        self.sig.record(cur)                        # (creates the handle sqdet_net_set_signal is given)
        self.preds = torch.empty((B, plan.gh, plan.gw, plan.out_ch), dtype=model.dtype, device=dev)
        self.det = (torch.empty((B, A, 4), dtype=f32, device=dev), torch.empty((B, A), dtype=f32, device=dev),
                    torch.empty((B, A), dtype=torch.int64, device=dev))
        self.out, self.host_flat, self.host = self.views(self.flat), None, None
        self.fwd_done, self.post_done = torch.cuda.Event(), torch.cuda.Event()
        self.fused_post = self.scored = self.to_host = self.ride = self.used = False
        self.post_wgs, self.nms = 0, None           # (nms: the suppression policy of the call that last used the slot)


class Pipe:
    """One two-stage pipeline on native plan `which`: the forward on the stream current at the call, decode + filter + row copy of a
    slot behind it -- on `post_stream`, as riders of the next forward, or at flush().  Nothing is allocated before the first step;
    the slots are rebuilt when the batch size changes."""

    def __init__(self, which=0):
        self.which, self.k = which, 0
        self.post_stream = self.post_event = self.batch = self.slots = self.pending = None

    def step(self, model, serving, images, to_host, defer):
        cur = torch.cuda.current_stream()
        if model.NATIVE_ARCH is None:
            return self._step_graph(model, images, to_host, cur)
        mc = model.mc
        x = model._to_input(images)
        B = int(x.shape[0])
        plan = model._native_plan(B, self.which)
        if self.batch != B:                         # what flush_pipeline() does, with this pipe in the single-lane pipe's place
            serving._flush_lanes(model, cur)
            if self.post_stream is None:
                # high priority: the two small post-processing kernels are dispatched as soon as CUs free up at a kernel
                # boundary of the forward instead of waiting for its queue to drain
                self.post_stream = torch.cuda.Stream(device=model.device, priority=int(knob("SQDET_POST_PRIORITY")))
            self.flush(model)
            cur.wait_stream(self.post_stream)
            self.batch, self.k, self.slots = B, 0, [Slot(model, plan, B, cur), Slot(model, plan, B, cur)]
        s = self.slots[self.k & 1]
        self.k += 1
        if s.used:
            cur.wait_event(s.post_done)             # the side stream has finished reading this slot's preds
        s.fused_post = ops.detect_filter_supported(mc.ANCHORS, mc.TOP_N_DETECTION) and knob("SQDET_SPLIT_POST") != "1"
        # the score half of interpret_output rides in the ConvDet launch's epilogue where the plan has it (float16
        # SqueezeDet head): what is left for the side stream is ONE filter launch + the row copy
        s.scored = s.fused_post and plan.scores_supported() and knob("SQDET_SCORE_EPILOGUE") != "0"
        mode = knob("SQDET_POST_DEFER") if defer and s.scored else None
        # a non-default suppression policy (nms.py) is a second launch behind the filter: the riders write their rows straight into
        # pinned host memory, where it cannot follow, so the post work then runs on the side stream
        s.nms = nms.nms_options(mc)
        s.ride = mode == "ride" and plan.rider_capacity() >= B and nms.is_default(s.nms)
        s.to_host, s.post_wgs = to_host, int(knob("SQDET_POST_WGS")) if B > 16 else 0
        if to_host and s.host is None:
            s.host_flat = torch.empty(s.flat.shape, dtype=torch.uint8).pin_memory()
            s.host = s.views(s.host_flat)
        if s.ride:
            self._step_ride(model, plan, x, s)
        else:
            self._step_side(model, plan, x, s, cur, plan.overlap_layer() if mode == "signal" else -1)
        return s.host if to_host else s.out

    def _step_ride(self, model, plan, x, s):
        """Everything on the caller's stream: the previous call's decode + filter rides in this forward's fire_chain launches and
        writes its rows where the caller reads them (no post_done wait either: a slot's preds / scores are next overwritten by the
        ConvDet launch of the second-next forward, behind its riders in stream order)."""
        mc, prev = model.mc, self.pending
        if prev is not None:
            if prev.ride:
                plan.set_post_job(prev.preds, prev.det[1], model.anchors_f32(), prev.host if prev.to_host else prev.out,
                                  mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT, mc.EXP_THRESH,
                                  mc.TOP_N_DETECTION, mc.NMS_THRESH)
            else:
                self._post(model, prev, None)
        plan.set_signal(-1, None)
        plan.forward(x, s.preds, scores=s.det[1])
        self.pending = s
        s.used = False                              # (no side-stream reader to wait for)

    def _step_side(self, model, plan, x, s, cur, ov):
        """Decode + filter on the side stream behind the forward: this call's at once (ov < 0), or deferred to the next call and gated
        on the event that forward signals at its launch `ov` ("signal").  The previous call's pending side work goes beside THIS
        forward's fire_chain launches."""
        prev, deferred = self.pending, ov >= 0
        plan.set_signal(ov, s.sig if (deferred and prev is not None) else None)
        plan.forward(x, s.preds, scores=s.det[1] if s.scored else None)
        s.fwd_done.record(cur)
        if prev is not None:
            if prev.ride:
                self._post(model, prev, None, stream=cur)
            else:
                self._post(model, prev, s.sig if deferred else None)
        self.pending = s if deferred else None
        if not deferred:
            self._post(model, s, None)
        s.used = True

    def _step_graph(self, model, images, to_host, cur):
        """Models without a native plan: the graph evaluation's preds, decode + filter on the side stream behind an event."""
        mc = model.mc
        if self.post_stream is None:
            self.post_stream = torch.cuda.Stream(device=model.device, priority=int(knob("SQDET_POST_PRIORITY")))
            self.post_event = torch.cuda.Event()
        (preds,) = model.run([model.preds], {model.image_input: images})
        self.post_event.record(cur)
        with torch.cuda.stream(self.post_stream):
            self.post_stream.wait_event(self.post_event)
            boxes, probs, cls = ops.interpret_output(preds, model.anchors_f32(), mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH,
                                                     mc.IMAGE_HEIGHT, mc.EXP_THRESH)[:3]
            out = model.filter_prediction_batch(boxes, probs, cls)
            preds.record_stream(self.post_stream)   # the allocator must not hand preds' memory out before the side stream is done
            if to_host:
                out = tuple(t_.to("cpu", non_blocking=True) for t_ in out)
        return out

    def _post(self, model, s, gate, stream=None):
        """Decode + filter + row copy of slot s on the side stream, behind its forward (and `gate`, an event of a later forward)."""
        mc = model.mc
        thresh = nms.first_stage_thresh(s.nms, mc)          # (mc.NMS_THRESH itself under the default policy)
        pstream = stream if stream is not None else (torch.cuda.current_stream() if knob("SQDET_POST_INLINE") == "1" else self.post_stream)
        with torch.cuda.stream(pstream):
            pstream.wait_event(s.fwd_done)
            if gate is not None:
                pstream.wait_event(gate)
            if s.fused_post:
                # decode + top-N + NMS in one call (score kernel unless scored + filter kernel): boxes / classes are decoded for the selected anchors only
                ops.detect_filter(s.preds, model.anchors_f32(), mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH, mc.IMAGE_HEIGHT,
                                  mc.EXP_THRESH, mc.TOP_N_DETECTION, thresh, scratch=s.det[1], out=s.out,
                                  scores_ready=s.scored, max_workgroups=s.post_wgs if gate is not None else 0)
            else:
                ops.interpret_output(s.preds, model.anchors_f32(), mc.CLASSES, mc.ANCHOR_PER_GRID, mc.IMAGE_WIDTH,
                                     mc.IMAGE_HEIGHT, mc.EXP_THRESH, out=s.det)
                ops.filter_prediction(s.det[0], s.det[1], s.det[2], mc.CLASSES, mc.TOP_N_DETECTION, thresh,
                                      mc.PROB_THRESH, out=s.out)
            if not nms.is_default(s.nms):
                nms.apply(s.nms, mc, s.out)                             # the second stage, ahead of the row copy on the same stream
            if s.to_host:
                ops.copy_to_pinned_host(s.flat, s.host_flat)            # all five outputs in one launch (never blocks the host)
            s.post_done.record(pstream)

    def flush(self, model):
        """Enqueues the pending slot's side work now."""
        s, self.pending = self.pending, None
        if s is not None:
            cur = torch.cuda.current_stream() if s.ride else None
            if s.ride:                              # same stream as the forward: stream order is all the synchronisation there is
                s.fwd_done.record(cur)
            self._post(model, s, None, stream=cur)


class Lane:
    """A serving lane: native plan `which`, its HIP stream, the event that orders it behind the caller, its pipeline."""
    __slots__ = ("which", "stream", "in_ev", "pipe")

    def __init__(self, which, device):
        self.which, self.pipe, self.stream, self.in_ev = which, Pipe(which), torch.cuda.Stream(device=device), torch.cuda.Event()

    def __getitem__(self, name):                    # (bench.py reads ln["stream"])
        return getattr(self, name)


class Serving:
    """The serving state of one model (ModelSkeleton.serving): the single-lane pipe and the current lane set.  Creating it touches
    neither the model nor the device."""

    def __init__(self):
        self.pipe, self.lanes, self.lane_next, self.lanes_checked, self.lane_check = Pipe(), None, 0, False, None

    def step(self, model, images, to_host=False, defer=False, lanes=None):
        """One step of the serving loop as a two-stage pipeline: the network forward runs on the caller's stream,
        interpret_output + filter_prediction (a few dozen microseconds of latency-bound work on 32 workgroups)
        run on a side HIP stream behind an event, so the NEXT batch's forward starts while this batch's boxes
        are being decoded and suppressed.  Returns filter_prediction_batch's tuple; the tensors are complete once
        flush_pipeline() has been called and the caller's stream (or the device) is synchronised.

        Models with a native plan run it on TWO static sets of buffers (preds, det_*, outputs) used alternately, with
        explicit events in both directions -- no allocation per step.  (Per-step torch allocations were the first
        version: preds had to be record_stream'ed for the side stream, so the caching allocator could not reuse a
        block until its event had completed; a host running a hundred steps ahead then asked for a hundred preds
        buffers, i.e. hipMalloc inside the serving loop -- the same binary measured 0.77 or 1.0-1.2 ms per step from
        one run to the next.)  The returned tensors are those of the slot: valid until the second-next call of the lane.
        to_host=True: the filtered rows (<= TOP_N per image: boxes, probs, classes, anchor indices, counts) are also copied
        to the slot's PINNED host buffers on the side stream -- what sess.run + filter_prediction hand the reference's
        caller -- and those host tensors are returned.

        defer=True (plans with the score epilogue and fire_chain launches: float16 SqueezeDet): the decode + filter of this
        call is carried out BY THE NEXT CALL's forward (or by flush_pipeline()): it is handed to the plan as a post job
        (sqdet_net_set_post_job) and runs in rider workgroups of that forward's fire_chain launches, one image per
        otherwise idle CU, writing the rows straight into the slot's pinned host buffer -- no side stream, no events, no
        extra launch.  Every launch of the forward fills the chip exactly once (persistent kernels with a static share of
        tiles per workgroup), so side work on another stream costs a whole round of whatever it lands beside, and every
        event ordering the two streams drains the forward's queue: measured 35 us per 0.49 ms step wherever the filter
        launch was placed (side stream, same stream, with or without the score kernel, beside the stem or beside the
        fire_chain launches) -- whereas the six fire_chain launches occupy 240 of the 256 CUs at batch 32.
        (SQDET_POST_DEFER=signal: the previous form -- the side stream's launch gated on a mid-forward event.)

        lanes (deferred calls on native plans; None = the model attribute `serve_lanes`, whose default is 2, or the environment's
        SQDET_SERVE_LANES): the number of BATCHES IN FLIGHT.  Consecutive calls alternate between `lanes` serving lanes -- each its
        own plan (workspace), HIP stream and pipeline slots, nothing ordering the lanes against each other -- so one lane's launch
        ramps and tails are filled by the other lanes' launches (throughput +20 % at batch 32 with two; three pay at batch 1).
        THE COMPLETION CONTRACT DEPENDS ON IT: the rows a deferred call returns are complete after the next call OF ITS LANE, i.e.
        after `lanes` further calls -- or after flush_pipeline() -- plus a synchronisation of the caller's stream behind that
        call; lanes=1 is the single-stream behaviour (complete after the NEXT call).  The result latency of a steady serving
        loop is therefore `lanes` step times (bench.py reports it as latency_ms_per_batch)."""
        with torch.cuda.device(model.device):
            lane_set = self.lanes_for(model, defer, lanes)
            if lane_set is None:
                return _probed(model._latency_probe, 0, self.pipe.step, model, self, images, to_host, defer)
            # A lane starts behind the caller's stream (the input may have been produced there).
            if not self.lanes_checked:
                self.warm_up(model, images, lanes=len(lane_set))
            lane = lane_set[self.lane_next % len(lane_set)]
            self.lane_next = (self.lane_next + 1) % len(lane_set)
            lane.in_ev.record(torch.cuda.current_stream())
            with torch.cuda.stream(lane.stream):
                lane.stream.wait_event(lane.in_ev)
                out = _probed(model._latency_probe, lane.which, lane.pipe.step, model, self, images, to_host, defer)
                if isinstance(images, torch.Tensor) and images.is_cuda:
                    images.record_stream(lane.stream)
            return out

    def warm_up(self, model, images, lanes=None):
        """Builds the serving lanes' plans for this batch and makes sure their HIP streams really run CONCURRENTLY; called by the
        first deferred detect_filter_pipelined of a lane set (a caller that must not pay ~20-40 ms inside its first serving call,
        or that captures streams, calls it ahead of time).  Which hardware queue a HIP stream lands on is the runtime's business,
        and two streams that share one serialise -- measured on this stack: of ten streams of torch's pool, the pairs containing
        one particular stream gave 0.468 ms per forward (= one stream) where every other pair gave 0.371.  For every lane k >= 1:
        16 forwards alternating between lane 0's stream and lane k's are timed with HIP events against 16 on lane 0's stream
        alone (median of three repetitions each, plans built and warmed on the lane streams first); a pair that gains less than
        6 % has lane k's stream replaced (up to four candidates, the best kept).  Result: self.lane_check (model._lane_check)."""
        with torch.cuda.device(model.device):
            lane_set = self.lanes_for(model, True, lanes)
            self.lanes_checked = True
            if lane_set is None or knob("SQDET_LANE_CHECK") == "0":
                return None
            x = model._to_input(images)
            B = int(x.shape[0])
            cur = torch.cuda.current_stream()
            plans, pre = [], []
            for lane in lane_set:
                lane.stream.wait_stream(cur)
                with torch.cuda.stream(lane.stream):
                    plans.append(model._native_plan(B, lane.which))
                    pre.append(torch.empty((B, plans[0].gh, plans[0].gw, plans[0].out_ch), dtype=model.dtype, device=model.device))
            NF, REPS = 16, 3
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def timed(k, sb):
                """ms per forward: NF forwards alternating between lane 0 (plan 0, its stream) and lane k's plan on stream sb"""
                sa = lane_set[0].stream
                ts = []
                for rep in range(REPS + 1):               # (first repetition: warm-up of streams / plans)
                    torch.cuda.synchronize(model.device)
                    e0.record(sa)
                    if sb is not sa:
                        sb.wait_event(e0)
                    for i in range(NF):
                        j, st = (0, sa) if i % 2 == 0 else (k, sb)
                        with torch.cuda.stream(st):
                            plans[j].forward(x, pre[j])
                    if sb is not sa:
                        sa.wait_stream(sb)
                    e1.record(sa)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) / NF)
                return float(np.median(ts[1:]))

            single = timed(0, lane_set[0].stream)
            report = dict(single_ms=single, forwards_per_sample=NF, repetitions=REPS, pairs=[])
            for k in range(1, len(lane_set)):
                best, best_t, cand = None, None, lane_set[k].stream
                for attempt in range(4):
                    t = timed(k, cand)
                    if best_t is None or t < best_t:
                        best, best_t = cand, t
                    if t < 0.94 * single:
                        break
                    cand = torch.cuda.Stream(device=model.device)
                lane_set[k].stream = best
                report["pairs"].append(dict(lane=k, pair_ms=best_t, attempts=attempt + 1))
            report["pair_ms"] = max(p["pair_ms"] for p in report["pairs"])
            report["attempts"] = max(p["attempts"] for p in report["pairs"])
            cur.wait_stream(lane_set[0].stream)
            self.lane_check = report
            return report

    def lanes_for(self, model, defer, lanes=None):
        """The serving lanes of a step (None: single-lane operation).  Used for deferred steps on native plans.
        Count: the `lanes` argument, else the attribute serve_lanes (None = SQDET_SERVE_LANES from the environment, default 2).
        At batch 32 three lanes are no better than two (0.396 against 0.390 ms per step); at batch 1, where a forward leaves most of
        the chip idle, three give 11.1-11.8 k img/s against 8.3 k with two and four fall back to 8.4 k (bench.py's sqdet_sample_b1
        config asks for three); SqueezeDet+ at batch 8 loses 11 % with three (1.147 against 1.018 ms).  A change of the count
        flushes the old lanes first; the new set's streams are checked again at its first use (warm_up)."""
        n = lanes if lanes is not None else model.serve_lanes
        n = int(knob("SQDET_SERVE_LANES") if n is None else n)
        if n < 1:
            raise SqdetError("detect_filter_pipelined: lanes must be >= 1, got %r" % (n,))
        if not defer or model.NATIVE_ARCH is None or n < 2:
            if self.lanes is not None and defer and any(ln.pipe.pending is not None for ln in self.lanes):
                # the lane set holds pending rows of earlier multi-lane calls: carried out ONCE, ahead of the first single-lane call (the
                # set is kept).  The single-lane pipe's own pending job is left alone -- it rides in this call's forward as ever.
                with torch.cuda.device(model.device):
                    self._flush_lanes(model, torch.cuda.current_stream())
            return None
        if self.lanes is None or len(self.lanes) != n:
            if self.lanes is not None:
                self.flush(model)
            self.lanes = [Lane(k, model.device) for k in range(n)]
            self.lane_next, self.lanes_checked, self.lane_check = 0, False, None
        return self.lanes

    def flush(self, model):
        """Enqueues the side work of the last call(s) now (nothing to overlap it with) and makes the CALLER's stream wait for all of
        it: every serving lane's stream AND every post-processing side stream (a lane's own, and the single-lane one).  After
        flush_pipeline() a synchronisation of the caller's stream alone (torch.cuda.current_stream().synchronize()) is enough to
        read every returned row, device or pinned host."""
        with torch.cuda.device(model.device):
            cur = torch.cuda.current_stream()
            self._flush_lanes(model, cur)
            self.pipe.flush(model)
            if self.pipe.post_stream is not None:
                cur.wait_stream(self.pipe.post_stream)

    def _flush_lanes(self, model, cur):
        """The serving lanes' half of flush: every lane's pending side work enqueued on its own stream, `cur` waits for it."""
        for lane in self.lanes or ():
            with torch.cuda.stream(lane.stream):
                lane.pipe.flush(model)
            cur.wait_stream(lane.stream)
            if lane.pipe.post_stream is not None:
                cur.wait_stream(lane.pipe.post_stream)
