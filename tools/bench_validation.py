"""Cost of the validation pass (--use_val_set) next to the training step it interleaves with, on one GPU:

    python tools/bench_validation.py --mode adapter --batch 32      # VLAEngine, config2
    python tools/bench_validation.py --mode lora --batch 16         # LoRAFinetune (rank 64), config2

Times the captured training step (ms per step, steady state), the one-off capture of the validation graphs, and a captured
validation batch as finetune's sweep runs it: copy into the static buffers, replay, wait for that batch's three fp32 values
on the host.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vla_adapter_amd import engine as E, synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["adapter", "lora"], default="adapter")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--backbone", default="config2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--val-batches", type=int, default=10)
    ap.add_argument("--lora-rank", type=int, default=64)
    args = ap.parse_args()
    dev, B = "cuda", args.batch
    cfg = E.NAMED_CONFIGS[args.backbone]()
    eng = E.VLAEngine(cfg, S.make_weights(cfg, dev, seed=0), dev)
    batch = S.make_batch(cfg, B, dev, seed=1, P=32)
    val = [S.make_batch(cfg, B, dev, seed=100 + i, P=32) for i in range(args.val_batches)]
    noise = (torch.randn(cfg.chunk, cfg.action_dim * cfg.llm.d, device=dev) * 0.02).to(torch.bfloat16)
    vnoise = noise.clone()
    if args.mode == "lora":
        from vla_adapter_amd.trainers import LoRAFinetune
        model = LoRAFinetune(eng, rank=args.lora_rank)
    else:
        model = eng
    model.capture(batch, noise)
    step = lambda: model.train_step_graphed(1e-4)
    for _ in range(3):
        step()
    eng.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    eng.flush()
    torch.cuda.synchronize()
    train_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    static = {k: v.clone() for k, v in val[0].items()}
    model.begin_validation()
    t0 = time.perf_counter()
    model.val_step_graphed(static, vnoise).tolist()
    first_ms = (time.perf_counter() - t0) * 1e3
    capture_ms = model.val_capture_seconds * 1e3
    times = []
    for rep in range(2):
        for b in val:
            t0 = time.perf_counter()
            for k in static:
                static[k].copy_(b[k])
            model.val_step_graphed(static, vnoise).tolist()
            times.append((time.perf_counter() - t0) * 1e3)
    model.end_validation()
    torch.cuda.synchronize()
    steady = sorted(times[len(val):])                    # second pass over the batches
    print(json.dumps(dict(mode=args.mode, backbone=args.backbone, batch=B, train_step_ms=round(train_ms, 3),
                          val_batch_ms_median=round(steady[len(steady) // 2], 3), val_batch_ms_min=round(steady[0], 3),
                          val_capture_ms=round(capture_ms, 1), val_first_call_ms=round(first_ms, 1))), flush=True)


if __name__ == "__main__":
    main()
