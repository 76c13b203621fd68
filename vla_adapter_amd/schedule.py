"""Segment schedules: how every GPU step of this package is enqueued and captured.

A step is a list of single-stream segments, ordered so that every event is recorded before it is waited on.  Eagerly a segment is
a Python call under its stream; captured, every segment is its own single-stream (linear) hipGraph replayed on that stream, and
the cross-stream edges are plain hipEvents between graph launches.  (One multi-stream hipGraph of the whole step was measured to
serialise the two backward chains in the runtime's graph executor - rocprofv3 trace, tools/timeline.py: LLM backward started only
after the head backward's last kernel - so the overlap is not left to it.)

The part every step shares - the LLM in layer chunks on "M" with the action head trailing it on "H", and the head's backward
running ahead of the LLM's over the reversed chunks - is built here, once: turnaround_chunks() cuts the layers, pipeline_forward()
and pipeline_backward() return the two halves.  engine.VLAEngine (adapter-only step, predict(), validation) and
trainers.BackboneTrainer (LoRA / full fine-tune step) supply the calls that are theirs, put their own segments (vision, gradient
hand-overs) around the halves, and run and capture the lists here; they share StepControls (accumulation, clipping) and captured_validation() too.
"""
from __future__ import annotations

import contextlib
import gc
import time
from typing import Any, Callable, List, NamedTuple, Optional, Tuple

import torch

from .scratch import ARENA


class Segment(NamedTuple):
    """stream: kind of the segment's stream ("M": the caller's); fn: its call, or None; wait: None, one event key or a list of
    keys; signal: key of the event recorded behind it; ranges: flat gradient ranges that are final when it ends (trainers.py)."""
    stream: str
    fn: Optional[Callable[[], Any]]
    wait: Any = None
    signal: Any = None
    ranges: Optional[list] = None


def chunks(n: int, sizes) -> List[Tuple[int, int]]:
    """[lo, hi) layer ranges covering 0..n with the given chunk sizes (last size repeats / is clipped)."""
    out, lo, k = [], 0, 0
    while lo < n:
        sz = sizes[min(k, len(sizes) - 1)]
        out.append((lo, min(n, lo + sz)))
        lo, k = out[-1][1], k + 1
    return out


def turnaround_chunks(n: int, body: int, tail, short: int) -> List[Tuple[int, int]]:
    """Layer ranges with `body`-layer chunks at the bottom and the short `tail` sizes at the top: the head's last forward chunk
    and first backward chunk - the serial forward -> backward turn-around - stay short, the rest costs few segments.  Stacks
    too shallow for two tails get uniform `short`-layer chunks."""
    t = sum(tail)
    return chunks(n, [body] * max(0, (n - t) // body) + list(tail)) if n >= 2 * t else chunks(n, [short])


def pipeline_forward(head, ch, llm_fwd, head_args, at_end, *, wait=None, signal=None, refresh: bool = False) -> List[Segment]:
    """Forward half of the LLM-and-head pipeline: per chunk c = [lo, hi) of ``ch`` an "M" segment running llm_fwd(c, lo, hi) and
    signalling ("f", c), and an "H" segment behind it with the head's blocks lo .. min(hi, head.nb) - 1 (block i reads hidden
    state i + 1).  The first "H" segment begins with head.fwd_begin(*head_args()) and, with ``refresh``, head.refresh_transposes() (the
    W^T operands of the head's backward, rebuilt beside the LLM forward instead of on the turn-around, which the LLM backward
    waits for: -0.09 ms on the adapter step, same box); the last one ends with at_end().  wait: of the first "M" segment; signal:
    of the last "H" segment."""
    segs = []
    for c, (lo, hi) in enumerate(ch):
        def h_fwd(c=c, lo=lo, hi=hi):
            if c == 0:
                head.fwd_begin(*head_args())
                if refresh:
                    head.refresh_transposes()
            for i in range(lo, min(hi, head.nb)):
                head.fwd_layer(i)
            if c == len(ch) - 1:
                at_end()
        segs.append(Segment("M", lambda c=c, lo=lo, hi=hi: llm_fwd(c, lo, hi), wait if c == 0 else None, ("f", c)))
        segs.append(Segment("H", h_fwd, ("f", c), signal if c == len(ch) - 1 else None))
    return segs


def pipeline_backward(head, ch, llm_bwd, dhs, handover=None) -> List[Segment]:
    """Backward half: over the reversed chunks, k = 0 at the top, an "H" segment running head.bwd_layer(i, dhs()) from block
    min(hi, head.nb) - 1 down to lo and signalling ("b", k), and an "M" segment behind it running llm_bwd(k, lo, hi).  A chunk above
    the head's last block receives no gradient from it: no "H" segment, and its "M" segment waits for nothing.  handover(k, lo,
    hi) -> the segment that follows chunk k's "M" segment (the trainers' gradient work), which then signals ("m", k)."""
    segs = []
    for k, (lo, hi) in enumerate(reversed(ch)):
        wait = None
        if min(hi, head.nb) > lo:
            segs.append(Segment("H", lambda lo=lo, hi=hi: [head.bwd_layer(i, dhs()) for i in range(min(hi, head.nb) - 1, lo - 1, -1)], None, ("b", k)))
            wait = ("b", k)
        segs.append(Segment("M", lambda k=k, lo=lo, hi=hi: llm_bwd(k, lo, hi), wait, ("m", k) if handover else None))
        if handover:
            segs.append(handover(k, lo, hi))
    return segs


class GradAccumulator:
    """Gradient accumulation over ``ga`` micro-steps (vla-scripts/finetune.py:1039-1042, 1078-1082): one accumulator per flat
    gradient buffer, summed in the buffers' own precision as autograd accumulates ``.grad``.  copy(dst, src) and add(dst, src)
    are the caller's kernels."""

    def __init__(self, copy, add):
        self.ga, self._micro, self._copy, self._add, self._pairs = 1, 0, copy, add, []

    def reset(self, ga: int, grads):
        self.ga, self._micro = int(ga), 0
        self._pairs = [(torch.zeros_like(g), g) for g in grads] if ga > 1 else []

    def fold(self) -> bool:
        """Fold the micro-step's gradients into the accumulators; True on the boundary micro-step (the gradient buffers then hold
        the sums).  ga == 1: nothing to do."""
        if self.ga == 1:
            return True
        for acc, g in self._pairs:
            (self._copy if self._micro == 0 else self._add)(acc, g)
        self._micro += 1
        if self._micro < self.ga:
            return False
        self._micro = 0
        for acc, g in self._pairs:
            self._copy(g, acc)
        return True


def check_max_grad_norm(max_norm) -> Optional[float]:
    """None (no clipping) or a float > 0; +inf is allowed: it clips nothing and the norm is still taken."""
    if max_norm is None:
        return None
    max_norm = float(max_norm)
    if not max_norm > 0.0:                           # (NaN fails the comparison too)
        raise ValueError(f"max_grad_norm must be > 0 (inf: report the norm, clip nothing), got {max_norm}")
    return max_norm


class GradClip:
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) over ranges of flat gradient buffers, without a host sync
    (prismatic/training/strategies/ddp.py:127-128; base_strategy.py:389).  Every range owns fp32 slots for the partial sums of
    squares of its elements (ops.grad_sumsq_): the pass of a range can run as soon as that range is final, on any stream.
    finalise() adds the slots in a fixed order and leaves ``out`` = (total_norm, clip coefficient) on the device, where
    ops.adamw_clipped_ reads the coefficient.  The slot layout depends on the set of ranges alone - buffers in the order given,
    ranges by first element, slots per range by its length - so the norm has the same bits whichever stream schedule ran the
    passes, eager or captured, and on every data-parallel rank."""

    def __init__(self, max_norm: float, bufs):
        self.max_norm = check_max_grad_norm(max_norm)
        assert self.max_norm is not None
        self.bufs = list(bufs)
        self._buf_index = {id(b): i for i, b in enumerate(self.bufs)}
        self.out = torch.zeros(2, device=self.bufs[0].device, dtype=torch.float32)
        self._layouts, self._seen, self._slot_of, self._slots = {}, {}, None, None

    def _index(self, buf) -> int:
        return self._buf_index[id(buf)]

    def begin(self, ranges, check=None) -> list:
        """Choose the slot layout of ``ranges`` = [(buffer, first element, end element)] for the passes that follow -> the ranges
        as sorted (buffer index, first, end), empty ones dropped.  A list of ranges seen before costs one dictionary lookup; a new
        one builds its layout and allocates its slots, so an owner hands its lists over once where it is set up (set_max_grad_norm,
        capture) and no step allocates.  check(sorted ranges) runs once per new list (the owner's coverage assertion)."""
        from . import ops
        seen = tuple((id(buf), lo, hi) for buf, lo, hi in ranges)
        hit = self._seen.get(seen)
        if hit is None:
            key = tuple(sorted((self._index(buf), lo, hi) for buf, lo, hi in ranges if hi > lo))
            if check is not None:
                check(list(key))
            lay = self._layouts.get(key)
            if lay is None:
                assert all(a[0] != b[0] or a[2] <= b[1] for a, b in zip(key, key[1:])), "gradient ranges overlap"
                slot_of, n = {}, 0
                for r in key:
                    slot_of[r], n = n, n + ops.grad_sumsq_slots(r[2] - r[1])
                lay = self._layouts[key] = (slot_of, torch.zeros(max(n, 1), device=self.out.device, dtype=torch.float32))
            hit = self._seen[seen] = (key, lay)
        key, (self._slot_of, self._slots) = hit
        return list(key)

    def sumsq(self, buf, lo: int, hi: int, gscale: float = 1.0):
        """The pass over buf[lo:hi] into that range's slots, on the current stream (gscale: as AdamW will be given it)."""
        from . import ops
        if hi > lo:
            ops.grad_sumsq_(buf[lo:hi], self._slots[self._slot_of[(self._index(buf), lo, hi)]:], gscale)

    def finalise(self):
        from . import ops
        ops.grad_norm_finalise_(self._slots, self.max_norm, self.out)

    @property
    def total_norm(self) -> torch.Tensor:
        return self.out[0]

    @property
    def coef(self) -> torch.Tensor:
        return self.out[1:2]


class StepControls:
    """Gradient accumulation and gradient-norm clipping of whoever owns a step (engine.VLAEngine, trainers.BackboneTrainer): the
    GradAccumulator, the GradClip and the public members around them.  The owner calls _init_step_controls(), keeps ``_graphs``
    (None until its capture()) and supplies _grad_buffers() -> its flat gradient buffers and _set_clip(clip), which settles
    what belongs to the old setting, stores ``self._clip = clip`` (a new GradClip, or None: off) and lays out its slots."""

    def _init_step_controls(self, copy, add):
        self._accum = GradAccumulator(copy, add)     # gradient accumulation (set_grad_accumulation)
        self._clip: Optional[GradClip] = None        # global gradient-norm clipping (set_max_grad_norm)

    def set_grad_accumulation(self, n: int):
        """finetune.py:1039-1042, 1078-1082: loss / n on every micro-batch, gradients summed over n micro-batches (in bf16, as
        autograd accumulates ``.grad``; over every flat gradient buffer of the owner), one optimizer step per n.  The
        data-parallel exchange runs once, on the boundary micro-step's sums (the reference's DDP all-reduces on every
        micro-step; same result, n-1 exchanges saved).  Call before capture(): the captured loss kernel carries the 1/n."""
        assert n >= 1 and self._graphs is None, "set_grad_accumulation() before capture()"
        self._accum.reset(n, self._grad_buffers())

    @property
    def ga(self) -> int:
        return self._accum.ga

    def set_max_grad_norm(self, max_norm: Optional[float]):
        """torch.nn.utils.clip_grad_norm_(trainable parameters, max_norm) in front of every optimizer step, as the reference's
        native trainer does it (base_strategy.py:389, ddp.py:127-128; every shipped configuration: 1.0; its L1 fine-tune script
        does not clip); None: off, inf: take the norm, clip nothing.  The norm covers exactly what AdamW updates - the engine:
        head.P.grad (action head, proprio projector, action queries); a trainer: _adam_ranges() and the head's buffer - as AdamW
        consumes it (averaged over the ranks, bf16), and it stays on the device with the coefficient (``grad_norm``).  A
        trainer takes it before capture() only."""
        max_norm = check_max_grad_norm(max_norm)
        self._set_clip(None if max_norm is None else GradClip(max_norm, self._grad_buffers()))

    @property
    def max_grad_norm(self) -> Optional[float]:
        return None if self._clip is None else self._clip.max_norm

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """Device scalar (f32): the global gradient norm of the last applied optimizer step, before clipping; None without
        set_max_grad_norm().  Reading its value is the only host sync clipping can cause."""
        return None if self._clip is None else self._clip.total_norm

    @property
    def clip_coef(self) -> Optional[torch.Tensor]:
        """Device f32 [1]: min(1, max_grad_norm / (grad_norm + 1e-6)) of the last applied optimizer step."""
        return None if self._clip is None else self._clip.coef

    # ---- optimizer state (train_state.py: --save_train_state / --resume_train_state / --log_state_digest) ------------------------------
    # The owner supplies _state_buffers() -> [(name, FlatParams)] of everything its optimizer step moves, keeps ``step_count``, and
    # may keep device counters of its own (_device_counters / _load_device_counters: LoRA dropout's mask counter).
    def _device_counters(self) -> dict:
        return {}

    def _load_device_counters(self, counters: dict) -> None:
        pass

    def state_digests_device(self) -> torch.Tensor:
        """ops.state_digest of data, m and v of every flat buffer -> int64 [3 * buffers] on the device, launched on the current stream
        (the caller has applied a pending update: flush()); nothing synchronises."""
        from . import train_state as TS
        return TS.digests_device(self._state_buffers())

    def state_digest_dict(self, values) -> dict:
        """{buffer: {data, m, v: hex}} from the values of state_digests_device()."""
        from . import train_state as TS
        return TS.digest_dict(self._state_buffers(), values)

    def optimizer_state(self) -> dict:
        """What the optimizer carries from one gradient step to the next, on the host: per flat buffer m and v, the hash of its
        offsets table and the digests of data, m and v (the weights themselves stay in the checkpoint files); the AdamW step count;
        the owner's device counters.  Between two gradient steps only: every update applied (flush()), no micro-step folded."""
        from . import train_state as TS
        assert self._accum._micro == 0, "optimizer_state() inside a gradient step: the accumulators hold a partial sum"
        bufs = self._state_buffers()
        dg = TS.read_digests(bufs)
        return dict(step_counts={type(self).__name__: int(self.step_count)}, counters=self._device_counters(),
                    buffers={name: dict(m=P.m.detach().cpu().clone(), v=P.v.detach().cpu().clone(), numel=int(P.numel), offsets=TS.offsets_hash(P),
                                        digest=dg[name]) for name, P in bufs})

    def verify_data_digests(self, state: dict) -> None:
        """The loaded weights against the digests recorded when they were written: ValueError naming the buffers that differ (the
        checkpoint round trip lost bits, or the files are another checkpoint's)."""
        from . import train_state as TS
        bufs = self._state_buffers()
        self._check_tables(state, bufs)
        got = TS.read_digests(bufs)
        bad = [f"{name}.data: recorded {state['buffers'][name]['digest']['data']}, loaded {got[name]['data']}"
               for name, _ in bufs if got[name]["data"] != state["buffers"][name]["digest"]["data"]]
        if bad:
            raise ValueError("--resume_train_state: the loaded weights are not the ones the state was written beside - " + "; ".join(bad))

    def _check_tables(self, state: dict, bufs) -> None:
        from . import train_state as TS
        if sorted(state["buffers"]) != sorted(name for name, _ in bufs):
            raise ValueError(f"--resume_train_state: offsets-table mismatch - the state holds the buffers {sorted(state['buffers'])}, this "
                             f"run trains {sorted(name for name, _ in bufs)}")
        for name, P in bufs:
            rec = state["buffers"][name]
            if rec["offsets"] != TS.offsets_hash(P) or int(rec["numel"]) != P.numel:
                raise ValueError(f"--resume_train_state: offsets-table mismatch in buffer {name!r} (names, shapes or order of the trainable "
                                 f"tensors differ: {int(rec['numel'])} elements recorded, {P.numel} here)")

    def load_optimizer_state(self, state: dict) -> None:
        """The inverse of optimizer_state(): m, v and the step count, each moment buffer verified against its recorded digest
        (the device counters follow capture() and its warm-up: load_device_counters)."""
        from . import train_state as TS
        bufs = self._state_buffers()
        self._check_tables(state, bufs)
        counts = state["step_counts"]
        if list(counts) != [type(self).__name__]:
            raise ValueError(f"--resume_train_state: the state holds the step counts of {list(counts)}, this run's optimizer is {type(self).__name__}")
        for name, P in bufs:
            rec = state["buffers"][name]
            P.m.copy_(rec["m"].to(P.m.device))
            P.v.copy_(rec["v"].to(P.v.device))
        self.step_count = int(counts[type(self).__name__])
        got = TS.read_digests(bufs)
        bad = [f"{name}.{part}" for name, _ in bufs for part in ("m", "v") if got[name][part] != state["buffers"][name]["digest"][part]]
        if bad:
            raise ValueError(f"--resume_train_state: the optimizer moments do not reproduce their recorded digests: {bad}")

    def load_device_counters(self, state: dict) -> None:
        """Device counters of the owner (behind capture() and its warm-up, which move them)."""
        self._load_device_counters(state.get("counters", {}))


def captured_validation(model, batch, noise, make, replay):
    """val_step_graphed of an engine / trainer: on the first call two eager model.val_forward() (every buffer allocated and
    kernel attribute set outside the capture), then make() -> (graphs, segs, the workspace they were captured on), timed into
    model.val_capture_seconds and kept; every call replay(graphs, segs, workspace) -> model._val_loss3.  The graphs write the loss and the prediction (model._val_pred) of the
    capture; an eager val_forward in between rebinds both names, so every replay binds them back to the captured tensors."""
    if model._val_graphs is None:
        for _ in range(2):
            model.val_forward(batch, noise)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model._val_graphs = make()
        torch.cuda.synchronize()
        model.val_capture_seconds = time.perf_counter() - t0
        model._val_graph_outs = (model._val_loss3, model._val_pred)
    replay(*model._val_graphs)
    model._val_loss3, model._val_pred = model._val_graph_outs
    return model._val_loss3


@contextlib.contextmanager
def graph_capture(g, *, stream, **kw):
    """``torch.cuda.graph(g, stream=stream, **kw)``: the one place this package enters a capture.  The kernels' scratch of ``stream``
    is reserved first (scratch.ARENA.reserve: allocated outside the capture, at the size the warm-up needed, and kept from then on),
    and Python's cyclic garbage collector is paused for the capture.  A dead reference cycle (an
    earlier engine / trainer with its graphs, events and memory pools) collected in the middle of a capture runs destructors
    (hipEventDestroy, hipGraphExecDestroy, frees of a graph pool) that this thread may not call while it captures: the runtime
    refuses, the destructor cannot raise, and the process aborts.  Paused, such cycles are collected after the capture."""
    ARENA.reserve(stream)
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, stream=stream, **kw):
            yield
    finally:
        if was:
            gc.enable()


def capture_graph(fn, pool, stream) -> torch.cuda.CUDAGraph:
    """fn() captured as one hipGraph on ``stream`` into the memory pool ``pool``.  thread_local: other host threads (the RCCL
    watchdog of a multi-rank job) may touch the HIP runtime meanwhile."""
    g = torch.cuda.CUDAGraph()
    with graph_capture(g, pool=pool, stream=stream, capture_error_mode="thread_local"):
        fn()
    return g


def _call(kind: str, fn):
    fn()


def run(segs, stream_of, graphs=None, *, fork=None, join: bool = False, call=_call, after=None, timeline=None) -> dict:
    """Enqueue the segments in order, eagerly or as replays of their ``graphs`` -> {signal key: event}.  stream_of(kind, caller's
    stream) -> stream.  fork: the streams that first wait for the caller's (default: those of the kinds other than "M"); join:
    the caller's stream waits for them at the end.  call(kind, fn) runs a call.  after(index, segment, event) runs on the
    segment's stream behind the event recorded after a segment that signals or finishes ranges.  timeline: receives (kind,
    index, start event, end event) per segment with a call."""
    main = torch.cuda.current_stream()
    if fork is None:
        fork = [stream_of(k, main) for k in {sg.stream for sg in segs} - {"M"}]
    for st in fork:
        st.wait_stream(main)                         # inputs / the previous update are ordered before every segment
    ev = {}
    for k, sg in enumerate(segs):
        kind, fn, wait, signal, ranges = sg
        stream = stream_of(kind, main)
        with torch.cuda.stream(stream):
            for w in ([] if wait is None else wait if isinstance(wait, list) else [wait]):
                stream.wait_event(ev[w])
            if fn is not None:
                if timeline is not None:
                    t0 = torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                if graphs is not None:
                    graphs[k].replay()
                else:
                    call(kind, fn)
                if timeline is not None:
                    t1 = torch.cuda.Event(enable_timing=True)
                    t1.record(stream)
                    timeline.append((kind, k, t0, t1))
            if signal is not None or ranges:
                e = torch.cuda.Event()
                e.record(stream)
                if signal is not None:
                    ev[signal] = e
                if after is not None:
                    after(k, sg, e)
    if join:
        for st in fork:
            main.wait_stream(st)
    return ev


def capture(segs, pools: dict, capture_stream_of, call=_call) -> list:
    """One linear hipGraph per segment with a call (None for the others), captured on capture_stream_of(kind) into that capture
    stream's pool in ``pools`` (created on first use).  A capture stream stands for one replay stream, so graphs that share a pool
    replay strictly in capture order on ONE stream: the allocator's reuse of freed capture-time temporaries stays race-free while
    the streams overlap.  call: as in run()."""
    graphs = []
    for sg in segs:
        if sg.fn is None:
            graphs.append(None)
            continue
        stream = capture_stream_of(sg.stream)
        pool = pools.setdefault(stream, torch.cuda.graph_pool_handle())
        graphs.append(capture_graph(lambda: call(sg.stream, sg.fn), pool, stream))
    return graphs
