#!/usr/bin/env python3
"""Times the two batch producers of the GPU input stage on the same inputs: ``GPUInputStage.build()`` (binning on the device, id
bookkeeping on the host: one device-to-host read-back, Python loops, a host-to-device copy) against ``GPUInputStage.collate()``
(kernels only), at batch 32 with prompt lengths uniform in 27-51, an 8 x 7 action window and one 224 x 224 frame per sample that is
already on the device.  ``collate`` is timed twice: with prompts as Python lists (flattened and uploaded per call) and with
device-resident (prompt_flat, prompt_off) and a static L, the form the training loop can hold.

Per variant, per batch, in microseconds:
  wall_us    host clock around ``iters`` calls that end in a device synchronise, over ``iters``
  device_us  device events around the same kind of window (first kernel's start to last kernel's end)
  host_us    host clock around each call alone, queue drained before the window: how long the call keeps the host - for build()
             that includes waiting for the device at its read-back, for collate() it is the enqueue
The variants alternate over ``rounds`` rounds after a warm-up of every variant; the figures are medians over the rounds, with the
spread (min - max) beside them.  One JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from vla_adapter_amd.input_stage import GPUInputStage, collate_layout  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_collate needs a GPU"
    dev, B = "cuda", args.batch
    rng = random.Random(0)
    g = torch.Generator().manual_seed(0)
    lens = [rng.randint(27, 51) for _ in range(B)]
    prompts = [[rng.randrange(0, 151000) for _ in range(n)] for n in lens]
    stage = GPUInputStage(dev, backbones=("siglip",), image_size=224)
    frames = [torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)]
    actions = (torch.rand(B, 8, 7, generator=g) * 2 - 1).to(dev)
    proprio = (torch.rand(B, 8, generator=g) * 2 - 1).to(dev)
    off, L = collate_layout(lens, stage.max_len)
    flat_d = torch.tensor([t for r in prompts for t in r], dtype=torch.int64, device=dev)
    off_d = torch.tensor(off, dtype=torch.int32, device=dev)
    py_rng = random.Random(1)
    variants = {
        "build": lambda i: stage.build(frames, prompts, actions, proprio, rng=py_rng),
        "collate_lists": lambda i: stage.collate(frames, prompts, actions, proprio, step=i),
        "collate_device": lambda i: stage.collate(frames, (flat_d, off_d), actions, proprio, L=L, step=i),
    }

    def measure(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            fn(i)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.iters
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        device = e0.elapsed_time(e1) * 1e-3 / args.iters
        host = 0.0
        for i in range(args.iters):
            t0 = time.perf_counter()
            fn(i)
            host += time.perf_counter() - t0
        torch.cuda.synchronize()
        return wall * 1e6, device * 1e6, host / args.iters * 1e6

    for fn in variants.values():
        for i in range(args.warmup):
            fn(i)
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            samples[k].append(measure(fn))
    out = dict(device=torch.cuda.get_device_name(0), batch=B, prompt_lens=[min(lens), max(lens)], L=L, iters=args.iters, rounds=args.rounds)
    for k, rows in samples.items():
        for j, name in enumerate(("wall_us", "device_us", "host_us")):
            col = [r[j] for r in rows]
            out[f"{k}.{name}"] = round(statistics.median(col), 1)
            out[f"{k}.{name}.spread"] = [round(min(col), 1), round(max(col), 1)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
