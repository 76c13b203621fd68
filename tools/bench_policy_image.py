#!/usr/bin/env python3
"""Times the evaluator's frame pipeline on the device (GPUInputStage.policy_frames: JPEG round trip, then TF's lanczos3 resize) with
device events after warm-up, alone and followed by pixels(center_crop=True), at B in {1, 8, 32}, two cameras, 256 x 256 -> 224; and,
for scale, the host rule (tests/policy_image_rule_np.py, numpy) on the same frames.  Prints one JSON line per shape and writes them
to profiles/policy_image.json.  No threshold is set and no speed is claimed: the numbers go into DESIGN.md section 20 as measured."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import policy_image_rule_np as P  # noqa: E402
from vla_adapter_amd.input_stage import GPUInputStage  # noqa: E402


def timed(fn, iters: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters              # us per call


def run(stage: GPUInputStage, B: int, n_img: int, side: int, size: int, iters: int, warmup: int, host_frames: int) -> dict:
    g = torch.Generator().manual_seed(B)
    fr_host = torch.randint(0, 256, (B, n_img, side, side, 3), generator=g, dtype=torch.uint8)
    fr = fr_host.to(stage.device)
    flat = fr.view(B * n_img, side, side, 3)
    t_trip = timed(lambda: stage.jpeg_round_trip(flat), iters, warmup)
    tripped = stage.jpeg_round_trip(flat)
    t_resize = timed(lambda: stage.lanczos3_resize(tripped, size, size), iters, warmup)
    t_policy = timed(lambda: stage.policy_frames(fr), iters, warmup)
    t_both = timed(lambda: stage.pixels(stage.policy_frames(fr), center_crop=True), iters, warmup)
    # the host rule on a few of the same frames, scaled to the batch
    k = min(host_frames, B * n_img)
    t0 = time.perf_counter()
    want = [P.policy_frame(a, size) for a in fr_host.view(B * n_img, side, side, 3)[:k].numpy()]
    t_host = (time.perf_counter() - t0) / k * (B * n_img) * 1e6
    got = stage.policy_frames(fr).view(B * n_img, size, size, 3)[:k].cpu().numpy()
    return dict(B=B, n_img=n_img, side=side, size=size, us_round_trip=round(t_trip, 2), us_resize=round(t_resize, 2), us_policy_frames=round(t_policy, 2),
                us_policy_frames_and_pixels=round(t_both, 2), us_host_rule=round(t_host, 0), host_frames_timed=k,
                equals_host_rule=bool(np.array_equal(got, np.stack(want))), mbytes_in=round(B * n_img * side * side * 3 / 1e6, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host_frames", type=int, default=4, help="frames the host rule is timed on (its time is scaled to the batch)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_image.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_policy_image needs a GPU"
    stage = GPUInputStage("cuda", backbones=("dino", "siglip"))
    rows = []
    for B in (1, 8, 32):
        rows.append(run(stage, B, 2, 256, 224, args.iters, args.warmup, args.host_frames))
        print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), iters=args.iters, warmup=args.warmup, shapes=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
