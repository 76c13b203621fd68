"""What --max_grad_norm costs: the captured LoRA and full fine-tune step at batch 16 (bench.py's workload and inputs), four variants
of each built side by side in one process and timed in interleaved rounds, so that every comparison is a same-box, same-minute one:

  off            the default step: AdamW range by range under the backward
  off_end        the default step with the update at the end of the step (VLA_NO_UPDATE_OVERLAP=1: trainer.overlap_update = False) -
                 the clipped step's schedule without the norm work
  clip_1.0       max_grad_norm = 1.0: sum-of-squares passes under the backward, finalise, AdamW with the device coefficient
  clip_inf       max_grad_norm = inf: the same launches, coefficient 1

Prints one JSON line per mode: median ms per step of every variant over the rounds, min / max, and the ratios clip / off_end (the norm
work; expected within the box spread of DESIGN section 6 if the passes hide under the backward) and off_end / off (what giving up
the early update costs - the price of any global-norm clip).

--variants names the variants to build, in build order.  Where a step's buffers land in memory moves its time by more than the norm
work costs (the third trainer built in a process ran 10 % slower than its neighbours, whichever variant it was), so the figures
to trust come from one variant per process (--variants off, --variants clip_1.0, ...): every variant then allocates alike.  A ratio
is printed where both of its variants ran.

  python tools/bench_grad_clip.py [--modes lora full] [--variants off off_end clip_1.0 clip_inf] [--batch 16] [--steps 10] [--rounds 3]
                                  [--warmup 3]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vla_adapter_amd import engine as E, synthetic as S  # noqa: E402
from vla_adapter_amd.trainers import FullFinetune, LoRAFinetune  # noqa: E402

VARIANTS = (("off", None, True), ("off_end", None, False), ("clip_1.0", 1.0, True), ("clip_inf", float("inf"), True))


def build(mode, cfg, batch, noise, max_norm, overlap, rank):
    eng = E.VLAEngine(cfg, S.make_weights(cfg, "cuda", seed=0), "cuda")
    tr = FullFinetune(eng) if mode == "full" else LoRAFinetune(eng, rank=rank)
    tr.overlap_update = overlap
    if max_norm is not None:
        tr.set_max_grad_norm(max_norm)
    tr.capture(batch, noise)
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["lora", "full"], choices=["lora", "full"])
    ap.add_argument("--variants", nargs="+", default=[v[0] for v in VARIANTS], choices=[v[0] for v in VARIANTS])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lora-rank", type=int, default=64)
    ap.add_argument("--backbone", default="config2", choices=sorted(E.NAMED_CONFIGS))
    args = ap.parse_args()
    cfg = E.NAMED_CONFIGS[args.backbone]()
    batch = S.make_batch(cfg, args.batch, "cuda", seed=1000, P=32)
    batch["pixel_values"] = batch["pixel_values"].to(torch.bfloat16)
    gen = torch.Generator(device="cuda").manual_seed(2000)
    noise = (torch.randn(cfg.chunk, cfg.action_dim * cfg.llm.d, device="cuda", generator=gen) * 0.02).to(torch.bfloat16)
    lr = 5e-4
    for mode in args.modes:
        spec = {name: (mn, ov) for name, mn, ov in VARIANTS}
        trs = {name: build(mode, cfg, batch, noise, *spec[name], args.lora_rank) for name in args.variants}
        ms = {name: [] for name in trs}
        for name, tr in trs.items():
            for _ in range(args.warmup):
                tr.train_step_graphed(lr)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, tr in trs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    tr.train_step_graphed(lr)
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({
            "tool": "bench_grad_clip", "mode": mode, "backbone": args.backbone, "batch": args.batch, "steps": args.steps, "rounds": args.rounds,
            "device": torch.cuda.get_device_name(0),
            "ms_per_step": {k: {"median": round(med[k], 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items()},
            **{f"{a}_over_{b}": round(med[a] / med[b], 4) for a, b in (("clip_1.0", "off_end"), ("clip_inf", "off_end"), ("off_end", "off"))
               if a in med and b in med},
            "grad_norm": {k: float(trs[k].grad_norm) for k in ("clip_1.0", "clip_inf") if k in trs},
            "clip_coef": {k: float(trs[k].clip_coef) for k in ("clip_1.0", "clip_inf") if k in trs},
        }), flush=True)
        del trs
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
