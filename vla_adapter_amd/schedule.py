"""Segment schedules: how every GPU step of this package is enqueued and captured.

A step is a list of single-stream segments, ordered so that every event is recorded before it is waited on.  Eagerly a segment is
a Python call under its stream; captured, every segment is its own single-stream (linear) hipGraph replayed on that stream, and
the cross-stream edges are plain hipEvents between graph launches.  (One multi-stream hipGraph of the whole step was measured to
serialise the two backward chains in the runtime's graph executor - rocprofv3 trace, tools/timeline.py: LLM backward started only
after the head backward's last kernel - so the overlap is not left to it.)  engine.VLAEngine builds the adapter-only step and
batch-1 predict() as such lists, trainers.BackboneTrainer the LoRA / full fine-tune step; both run and capture them here.
"""
from __future__ import annotations

import contextlib
import gc
from typing import Any, Callable, List, NamedTuple, Optional, Tuple

import torch


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


@contextlib.contextmanager
def graph_capture(g, **kw):
    """``torch.cuda.graph(g, **kw)`` with Python's cyclic garbage collector paused for the capture.  A dead reference cycle (an
    earlier engine / trainer with its graphs, events and memory pools) collected in the middle of a capture runs destructors
    (hipEventDestroy, hipGraphExecDestroy, frees of a graph pool) that this thread may not call while it captures: the runtime
    refuses, the destructor cannot raise, and the process aborts.  Paused, such cycles are collected after the capture."""
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):
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
