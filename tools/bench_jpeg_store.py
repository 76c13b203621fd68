#!/usr/bin/env python3
"""Measures the JPEG frame store (vla_adapter_amd/jpeg_store.py, csrc/jpeg.hip) by the method of bench_episodes.py: alternating
rounds, medians with the spread (min - max) beside them.  Every frame here is SYNTHETIC - a smooth pattern under mild noise - so the
byte ratio reported is that of these frames and says nothing about a real dataset.

  (a) ``decode``: HIP-event milliseconds of vla_jpeg_decode_rows alone at B = ``--batch``, q95 4:2:0, for n_img in {1, 2}, 224 x 224
      and 256 x 256, without restart markers and with one per MCU row, and both lane mappings (0: a lane per segment, 1: a wave per
      segment), which alternate inside every round.
  (b) ``step``: the captured adapter-only step of ``--backbone`` fed from the JPEG episode file against the same step fed from its raw
      twin (the decoded frames as frames_u8), on one engine and one graph; ``not_slower`` as bench_episodes.py defines it.
  (c) ``verify``: EpisodeStore.verify_frames() of the store of (b), as seconds per 10 000 frames; the load-time parse likewise.
  (d) ``ratio``: raw bytes over JPEG bytes of the frames of (b).
One JSON line per part.  ``--parts`` selects them."""
import argparse
import json
import os
import statistics
import tempfile
import time

import _episode_bench as EB
import numpy as np
import torch
from pack_episodes_jpeg import pack


def synthetic_frames(n: int, size: int, seed: int = 0) -> torch.Tensor:
    """uint8 [n, size, size, 3]: two smooth gradients and a moving blob under noise of +-6."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / size
    out = np.empty((n, size, size, 3), dtype=np.uint8)
    for i in range(n):
        cx, cy = g.random(2)
        blob = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) * 30)
        img = np.stack([x * 200 + blob * 50, y * 180 + 40 * np.sin(8 * x + i), 120 + 100 * blob], -1) + g.integers(-6, 7, (size, size, 3))
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return torch.from_numpy(out)


def decode_times(args):
    from vla_adapter_amd import jpeg_store as JS
    dev, B, T = "cuda:0", args.batch, 64
    for size in (224, 256):
        for n_img in (1, 2):
            raw = synthetic_frames(T * n_img, size).view(T, n_img, size, size, 3)
            for restart_rows in (0, 1):
                d = pack(dict(frames_u8=raw), 95, "4:2:0", restart_rows)
                jf = JS.JpegFrames(d, dev)
                eo = torch.tensor([0, T], dtype=torch.int64, device=dev)
                ep = torch.zeros(B, dtype=torch.int32, device=dev)
                row = (torch.arange(B, dtype=torch.int64, device=dev) * 7) % T
                out = torch.empty(B, n_img, size, size, 3, dtype=torch.uint8, device=dev)

                def run(mapping, calls=10):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        jf.decode(eo, T, ep, row, out, mapping=mapping)
                    b.record()
                    b.synchronize()
                    return a.elapsed_time(b) / calls
                for m in (0, 1):
                    run(m, 3)
                samples = {0: [], 1: []}
                for _ in range(args.rounds):
                    for m in (0, 1):
                        samples[m].append(run(m))
                rec = dict(part="decode", batch=B, n_img=n_img, size=size, restart_rows=restart_rows, max_seg=jf.max_seg,
                           jpeg_bytes_per_frame=int(d["frames_jpeg"].numel() // (T * n_img)))
                for m, name in ((0, "lane_per_segment"), (1, "wave_per_segment")):
                    rec[f"{name}.ms"] = round(statistics.median(samples[m]), 4)
                    rec[f"{name}.ms.spread"] = [round(min(samples[m]), 4), round(max(samples[m]), 4)]
                print(json.dumps(rec), flush=True)


def step_times(args):
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd.episodes import EpisodeStore
    mcfg = EB.model_config(args)
    rng, g = EB.generators()
    d = dict(EB.synthetic_episodes(mcfg, args, rng, g), dataset_name="bench")
    T, size = d["frames_u8"].shape[0], mcfg.vit[0].img
    d["frames_u8"] = synthetic_frames(T * args.n_img, size).view(T, args.n_img, size, size, 3)
    jd = pack(d, 95, "4:2:0", args.restart_rows)
    from PIL import Image
    import io
    off, data = jd["frame_off"].tolist(), jd["frames_jpeg"].numpy().tobytes()
    twin = np.stack([np.asarray(Image.open(io.BytesIO(data[off[i]:off[i + 1]])).convert("RGB")) for i in range(len(off) - 1)])
    rd = dict(d, frames_u8=torch.from_numpy(twin).view(T, args.n_img, size, size, 3))
    ratio = dict(part="ratio", synthetic=True, frames=len(off) - 1, size=size, quality=95, subsampling="4:2:0", restart_rows=args.restart_rows,
                 raw_bytes=int(rd["frames_u8"].numel()), jpeg_bytes=len(data), ratio=round(rd["frames_u8"].numel() / len(data), 3))
    if "ratio" in args.parts:
        print(json.dumps(ratio), flush=True)
    if "verify" in args.parts:
        t0 = time.perf_counter()
        st = EpisodeStore.from_dict(jd, "cuda:0", chunk=mcfg.chunk)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t0
        st.verify_frames()                                      # warm: buffers allocated
        col = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            n = st.verify_frames()
            col.append((time.perf_counter() - t0) / n * 1e4)
        print(json.dumps({"part": "verify", "frames": n, "size": size, "restart_rows": args.restart_rows,
                          "verify_s_per_10k_frames": round(statistics.median(col), 3), "verify_s_per_10k_frames.spread": [round(min(col), 3), round(max(col), 3)],
                          "load_s_per_10k_frames": round(t_load / n * 1e4, 3)}), flush=True)
        del st
        torch.cuda.empty_cache()
    if "step" in args.parts:
        with tempfile.TemporaryDirectory() as tmp:
            torch.save(jd, os.path.join(tmp, "jpeg.pt"))
            torch.save(rd, os.path.join(tmp, "raw.pt"))
            common = EB.common_flags(args)
            cfgs = {"raw_episode_file": F.parse_args(common + ["--episode_file", os.path.join(tmp, "raw.pt")]),
                    "jpeg_episode_file": F.parse_args(common + ["--episode_file", os.path.join(tmp, "jpeg.pt")])}
            samples, _ = EB.time_sources(args, mcfg, cfgs, base="raw_episode_file")
        out = dict(part="step", device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=args.max_seq_len,
                   steps=args.steps, rounds=args.rounds, restart_rows=args.restart_rows)
        print(json.dumps(EB.report(out, samples, "step_ms", base="raw_episode_file", other="jpeg_episode_file")), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    EB.add_common_args(ap)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--restart_rows", type=int, default=1)
    ap.add_argument("--parts", default="decode,ratio,verify,step")
    args = ap.parse_args()
    args.parts = args.parts.split(",")
    assert torch.cuda.is_available(), "bench_jpeg_store needs a GPU"
    if "decode" in args.parts:
        decode_times(args)
    if set(args.parts) & {"ratio", "verify", "step"}:
        step_times(args)


if __name__ == "__main__":
    main()
