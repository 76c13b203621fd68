#!/usr/bin/env python3
"""Measures the JPEG encoder (include/vla_jpeg_encode.h, ops.jpeg_encode, jpeg_store.encode_tables) against the Pillow path of
tools/pack_episodes_jpeg.py on the same frames and the same machine: warm-up first, then ``--rounds`` rounds, medians with the spread
(min - max) beside them.  Every frame is SYNTHETIC - bench_jpeg_store.py's smooth pattern under mild noise - so bytes per frame and
times are those of these frames and say nothing about a real dataset.

  (a) ``encode``: HIP-event milliseconds of one ops.jpeg_encode call (both entry points and the read-back of the byte count between
      them) for 32 and 1024 frames at 224 x 224 and 256 x 256, q95, one restart marker per MCU row; the frames are on the device.
      ``plan_ms`` / ``write_ms``: the two entry points alone, on the workspace of the same call.
  (b) ``pillow``: host seconds of pack() - Pillow, one thread - over the same 1024 frames; ``identical``: the device's bytes and
      offsets equal pack()'s.
  (c) ``load``: host seconds (ending in a device synchronise) of EpisodeStore.load of one raw shard of ``--load_frames`` frames at
      256 x 256 without and with jpeg_quality=95, the two alternating; and the bytes of frames each leaves on the device.
One JSON line per measurement.  ``--parts`` selects them."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
from bench_jpeg_store import synthetic_frames  # noqa: E402
from pack_episodes_jpeg import pack  # noqa: E402

DEV = "cuda:0"


def med(col, digits=3):
    return round(statistics.median(col), digits), [round(min(col), digits), round(max(col), digits)]


def event_ms(fn, calls: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def encode_times(args, frames_by_size):
    from vla_adapter_amd import native as N, ops
    lib = ops._lib()
    for size, host in frames_by_size.items():
        for n in (32, 1024):
            fr = host[:n].to(DEV)
            calls = 20 if n == 32 else 3
            ops.jpeg_encode(fr, 95, 1)                               # warm-up: code objects, the allocator's blocks
            ops.jpeg_encode(fr, 95, 1)
            whole = [event_ms(lambda: ops.jpeg_encode(fr, 95, 1), calls) for _ in range(args.rounds)]
            # the two entry points alone
            need = lib.vla_jpeg_encode_workspace_bytes(n, size, size, 1)
            ws, off = torch.empty(need, dtype=torch.uint8, device=DEV), torch.empty(n + 1, dtype=torch.int64, device=DEV)
            qtab = ops._encode_qtab(95, fr.device)
            plan = lambda: N.check(lib.vla_jpeg_encode_plan(ops._st(), ops._p(fr), size * size * 3, n, size, size, ops._p(qtab), 1, ops._p(ws), need, ops._p(off)))
            plan()
            total = int(off[-1].item())
            out = torch.empty(total, dtype=torch.uint8, device=DEV)
            write = lambda: N.check(lib.vla_jpeg_encode_write(ops._st(), n, size, size, ops._p(qtab), 1, ops._p(ws), need, ops._p(off), ops._p(out), total))
            write()
            plan_ms, write_ms = [], []
            for _ in range(args.rounds):
                plan_ms.append(event_ms(plan, calls))
                write_ms.append(event_ms(write, calls))
            rec = dict(part="encode", device=torch.cuda.get_device_name(0), synthetic=True, frames=n, size=size, quality=95, restart_rows=1,
                       jpeg_bytes_per_frame=total // n, raw_bytes_per_frame=size * size * 3, workspace_bytes=need, rounds=args.rounds, calls=calls)
            for name, col in (("encode_ms", whole), ("plan_ms", plan_ms), ("write_ms", write_ms)):
                rec[name], rec[name + ".spread"] = med(col)
            rec["frames_per_s"] = round(n / (rec["encode_ms"] * 1e-3))
            print(json.dumps(rec), flush=True)


def pillow_times(args, frames_by_size):
    from vla_adapter_amd import ops
    for size, host in frames_by_size.items():
        n = host.shape[0]
        d = dict(frames_u8=host.view(n, 1, size, size, 3))
        pack(dict(frames_u8=d["frames_u8"][:32]), 95, "4:2:0", 1)          # warm-up
        col, packed = [], None
        for _ in range(args.pillow_rounds):
            t0 = time.perf_counter()
            packed = pack(d, 95, "4:2:0", 1)
            col.append(time.perf_counter() - t0)
        data, off = ops.jpeg_encode(host.to(DEV), 95, 1)
        same = torch.equal(data.cpu(), packed["frames_jpeg"]) and torch.equal(off.cpu(), packed["frame_off"])
        rec = dict(part="pillow", synthetic=True, frames=n, size=size, quality=95, restart_rows=1, threads=1, rounds=args.pillow_rounds, identical=bool(same))
        rec["pack_s"], rec["pack_s.spread"] = med(col)
        rec["frames_per_s"] = round(n / rec["pack_s"])
        print(json.dumps(rec), flush=True)


def load_times(args, frames_by_size):
    from vla_adapter_amd.episodes import EpisodeStore
    size = 256
    fr = frames_by_size[size][:args.load_frames]
    T = fr.shape[0]
    d = dict(frames_u8=fr.view(T, 1, size, size, 3), actions_raw=torch.zeros(T, 7), proprio_raw=torch.zeros(T, 8),
             episode_off=torch.tensor([0, T], dtype=torch.int64), prompt_flat=torch.arange(30, dtype=torch.int64),
             prompt_off=torch.tensor([0, 30], dtype=torch.int32), dataset_name="bench")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "raw.pt")
        torch.save(d, path)

        def load(q):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = EpisodeStore.load(path, DEV, jpeg_quality=q)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            held = int(st.jpeg.bytes.numel()) if st.jpeg is not None else int(st.frames_u8.numel())
            del st
            return dt, held
        for q in (None, 95):
            load(q)                                                  # warm-up: the page cache holds the file, the kernels are loaded
        cols, held = {None: [], 95: []}, {}
        for _ in range(args.pillow_rounds):
            for q in (None, 95):
                dt, held[q] = load(q)
                cols[q].append(dt)
    rec = dict(part="load", synthetic=True, frames=T, size=size, rounds=args.pillow_rounds, raw_frame_bytes_on_device=held[None], jpeg_frame_bytes_on_device=held[95])
    rec["load_raw_s"], rec["load_raw_s.spread"] = med(cols[None])
    rec["load_jpeg_quality_95_s"], rec["load_jpeg_quality_95_s.spread"] = med(cols[95])
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pillow_rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--load_frames", type=int, default=1024)
    ap.add_argument("--parts", default="encode,pillow,load")
    args = ap.parse_args()
    args.parts = args.parts.split(",")
    assert torch.cuda.is_available(), "bench_jpeg_encode needs a GPU"
    frames_by_size = {size: synthetic_frames(args.frames, size) for size in (224, 256)}
    if "encode" in args.parts:
        encode_times(args, frames_by_size)
    if "pillow" in args.parts:
        pillow_times(args, frames_by_size)
    if "load" in args.parts:
        load_times(args, frames_by_size)


if __name__ == "__main__":
    main()
