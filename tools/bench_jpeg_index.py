#!/usr/bin/env python3
"""Measures the scan index of the JPEG frame store (vla_adapter_amd/jpeg_store.py: build_scan_index, csrc/jpeg_index.hip,
vla_jpeg_decode_rows_at) by the method of bench_jpeg_store.py: the same SYNTHETIC frames, alternating rounds, medians with the spread
(min - max) beside them.

  (a) ``decode``: HIP-event milliseconds of the decode alone at B = ``--batch``, q95 4:2:0, for n_img in {1, 2}, 224 x 224 and
      256 x 256: files without restart markers un-indexed and indexed (one MCU row a piece; with ``--piece_mcus half_row``, or a
      number of MCUs, also at that piece length), against the restart-per-row twin of the same images; both decode mappings.  All
      of them alternate inside every round.  ``indexed_faster``: per mapping, the indexed range (min - max) lies wholly below the un-indexed range.
  (b) ``step``: the captured adapter-only step of ``--backbone`` fed from the marker-less episode file with --jpeg_scan_index, without
      it, and from the raw twin (the decoded frames as frames_u8), on one engine and one graph.
  (c) ``build``: build_scan_index of the store of (b) as seconds per 10 000 frames, both build mappings (the parse is not in it).
  (d) ``size``: the index's bytes per frame and as a share of the JPEG bytes.
One JSON line per part.  ``--parts`` selects them."""
import argparse
import io
import json
import os
import statistics
import tempfile
import time

import _episode_bench as EB
import numpy as np
import torch
from bench_jpeg_store import synthetic_frames
from pack_episodes_jpeg import pack


def med(col):
    return round(statistics.median(col), 4), [round(min(col), 4), round(max(col), 4)]


def decode_times(args):
    from vla_adapter_amd import jpeg_store as JS
    dev, B, T = "cuda:0", args.batch, 64
    for size in (224, 256):
        for n_img in (1, 2):
            raw = synthetic_frames(T * n_img, size).view(T, n_img, size, size, 3)
            plain, rows = pack(dict(frames_u8=raw), 95, "4:2:0", 0), pack(dict(frames_u8=raw), 95, "4:2:0", 1)
            stores = {"markerless": JS.JpegFrames(plain, dev), "markerless_indexed": JS.JpegFrames(plain, dev), "restart_rows": JS.JpegFrames(rows, dev)}
            stores["markerless_indexed"].build_scan_index()
            if args.piece_mcus:
                name = f"markerless_indexed_{args.piece_mcus}"
                stores[name] = JS.JpegFrames(plain, dev)
                stores[name].build_scan_index(piece_mcus=size // 32 if args.piece_mcus == "half_row" else int(args.piece_mcus))
            eo = torch.tensor([0, T], dtype=torch.int64, device=dev)
            ep = torch.zeros(B, dtype=torch.int32, device=dev)
            row = (torch.arange(B, dtype=torch.int64, device=dev) * 7) % T
            out = {k: torch.empty(B, n_img, size, size, 3, dtype=torch.uint8, device=dev) for k in stores}

            def run(k, mapping, calls=10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    stores[k].decode(eo, T, ep, row, out[k], mapping=mapping)
                b.record()
                b.synchronize()
                return a.elapsed_time(b) / calls
            keys = [(k, m) for k in stores for m in (0, 1)]
            for k, m in keys:
                run(k, m, 3)
            for k in stores:                                        # the same pixels from all of them
                assert torch.equal(out[k], out["markerless"]), k
            samples = {km: [] for km in keys}
            for _ in range(args.rounds):
                for km in keys:
                    samples[km].append(run(*km))
            rec = dict(part="decode", batch=B, n_img=n_img, size=size, rounds=args.rounds, max_seg={k: s.max_seg for k, s in stores.items()},
                       jpeg_bytes_per_frame=int(plain["frames_jpeg"].numel() // (T * n_img)))
            for (k, m), col in samples.items():
                name = f"{k}.{('lane_per_segment', 'wave_per_segment')[m]}"
                rec[f"{name}.ms"], rec[f"{name}.ms.spread"] = med(col)
            rec["indexed_faster"] = {("lane_per_segment", "wave_per_segment")[m]: max(samples[("markerless_indexed", m)]) < min(samples[("markerless", m)])
                                     for m in (0, 1)}
            print(json.dumps(rec), flush=True)


def store_parts(args):
    from PIL import Image
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd import jpeg_store as JS
    mcfg = EB.model_config(args)
    rng, g = EB.generators()
    d = dict(EB.synthetic_episodes(mcfg, args, rng, g), dataset_name="bench")
    T, size = d["frames_u8"].shape[0], mcfg.vit[0].img
    d["frames_u8"] = synthetic_frames(T * args.n_img, size).view(T, args.n_img, size, size, 3)
    jd = pack(d, 95, "4:2:0", 0)
    n = T * args.n_img
    if set(args.parts) & {"build", "size"}:
        rec = None
        col = {0: [], 1: []}
        for r in range(args.rounds + 1):                            # (the first round warms up)
            for m in (0, 1):
                jf = JS.JpegFrames(jd, "cuda:0")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pieces = jf.build_scan_index(mapping=m)
                torch.cuda.synchronize()
                if r:
                    col[m].append((time.perf_counter() - t0) / n * 1e4)
                rec = dict(part="size", synthetic=True, frames=n, size=size, pieces_per_frame=round(pieces / n, 2), index_bytes_per_frame=round(jf.index_bytes() / n, 1),
                           jpeg_bytes_per_frame=int(jd["frames_jpeg"].numel() // n), index_share_of_jpeg_bytes=round(jf.index_bytes() / int(jd["frames_jpeg"].numel()), 4),
                           bad_scans=int((jf.index_status != 0).sum()))
                del jf
        if "build" in args.parts:
            out = dict(part="build", frames=n, size=size, slice_segments=JS.BUILD_SLICE, rounds=args.rounds)
            for m, name in ((0, "lane_per_segment"), (1, "wave_per_segment")):
                out[f"{name}.build_s_per_10k_frames"], out[f"{name}.build_s_per_10k_frames.spread"] = med(col[m])
            print(json.dumps(out), flush=True)
        if "size" in args.parts:
            print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    if "step" in args.parts:
        off, data = jd["frame_off"].tolist(), jd["frames_jpeg"].numpy().tobytes()
        twin = np.stack([np.asarray(Image.open(io.BytesIO(data[off[i]:off[i + 1]])).convert("RGB")) for i in range(len(off) - 1)])
        rd = dict(d, frames_u8=torch.from_numpy(twin).view(T, args.n_img, size, size, 3))
        with tempfile.TemporaryDirectory() as tmp:
            torch.save(jd, os.path.join(tmp, "jpeg.pt"))
            torch.save(rd, os.path.join(tmp, "raw.pt"))
            common = EB.common_flags(args)
            cfgs = {"raw_episode_file": F.parse_args(common + ["--episode_file", os.path.join(tmp, "raw.pt")]),
                    "markerless_jpeg": F.parse_args(common + ["--episode_file", os.path.join(tmp, "jpeg.pt")]),
                    "markerless_jpeg_indexed": F.parse_args(common + ["--episode_file", os.path.join(tmp, "jpeg.pt"), "--jpeg_scan_index", "True"])}
            samples, _ = EB.time_sources(args, mcfg, cfgs, base="raw_episode_file")
        out = dict(part="step", device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=args.max_seq_len,
                   steps=args.steps, rounds=args.rounds)
        out = EB.report(out, samples, "step_ms", base="raw_episode_file", other="markerless_jpeg_indexed")
        out["indexed_faster"] = max(samples["markerless_jpeg_indexed"]) < min(samples["markerless_jpeg"])
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    EB.add_common_args(ap)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--piece_mcus", default=None, help="(decode) also an indexed store with pieces of this many MCUs; half_row: half an MCU row")
    ap.add_argument("--parts", default="decode,build,size,step")
    args = ap.parse_args()
    args.parts = args.parts.split(",")
    assert torch.cuda.is_available(), "bench_jpeg_index needs a GPU"
    if "decode" in args.parts:
        decode_times(args)
    if set(args.parts) & {"build", "size", "step"}:
        store_parts(args)


if __name__ == "__main__":
    main()
