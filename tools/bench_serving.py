#!/usr/bin/env python3
"""Serving a batch: OpenVLAForActionPrediction.predict_actions (B observations, one device pass) against B sequential predict_action
calls of the same build - the only path there was before - for B in {1, 2, 4, 8, 16, 32} on `config2` (SigLIP-224 + Qwen2.5-0.5B, one
image) and `dinosiglip-0_5b` (DINOv2 + SigLIP fused, two images).  At B > 1 the batched call is timed with and without
ops.latency_hint() baked into its graphs (three alternating rounds, median with minimum and maximum); the engine's default per B
follows these numbers (VLAEngine.predict).

    tools/bench_serving.py --config config2 --batch 8          one step: one JSON line
    tools/bench_serving.py --all --out profiles/serving_batch.json

--all starts one child process per (config, B), each under its own `timeout -k 10`, and stops at the first step that fails: nothing
is started on a device after a step that faulted or hung.  Rows that did not run are absent from the table - no number is made up.
Random-init weights, synthetic inputs (a 48-id prompt per sample, +-4 ids so that the batch is ragged); replayed calls only.
Times: HIP events on the caller's stream around n calls (the batched call with return_tensors=True and inputs on the device does not
synchronise), and the host's wall clock around the same loop."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("config2", "dinosiglip-0_5b")
BATCHES = (1, 2, 4, 8, 16, 32)
P = 48          # LIBERO prompt with the Qwen chat template (~48 ids)
STATS = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]},
                    "proprio": {"q01": [-1.0] * 8, "q99": [1.0] * 8, "min": [-1.0] * 8, "max": [1.0] * 8}}}


def timed(fn, n):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n


def one(config: str, B: int, n: int) -> dict:
    import numpy as np
    import torch
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    dev = "cuda"
    cfg = E.NAMED_CONFIGS[config]()
    vla = OpenVLAForActionPrediction(cfg, S.make_weights(cfg, dev, seed=0), dev, norm_stats=STATS)
    g = torch.Generator().manual_seed(1)
    lens = [P] + [P - 4 + int(torch.randint(0, 9, (1,), generator=g)) for _ in range(B - 1)]
    prompts = [torch.randint(0, 151000, (m,), generator=g) for m in lens]
    img = cfg.vit[0].img
    px = torch.randn(B, 3 * len(cfg.vit) * cfg.n_img, img, img, generator=g).clamp_(-3, 3).to(torch.bfloat16).to(dev)
    proprio = np.zeros((B, 8), np.float32)
    res = dict(config=config, B=B, n_img=cfg.n_img, prompt_lens=[min(lens), max(lens)], calls_timed=n)

    # B sequential batch-1 calls: every sample at its own length, as a caller stepping B simulators had to queue them
    def sequential():
        for b in range(B):
            vla.predict_action(input_ids=prompts[b].view(1, -1), proprio=proprio[b], proprio_projector=True, action_head=True,
                               pixel_values=px[b:b + 1], attention_mask=torch.ones(1, lens[b], dtype=torch.bool))
    for _ in range(2):
        sequential()
    dev_ms, host_ms = timed(sequential, max(2, n // B))
    res["sequential_predict_action_ms"] = dict(device=round(dev_ms, 3), host=round(host_ms, 3), graphs=len(vla.engine._predict_graphs))

    flat = torch.cat(prompts).to(dev)
    off = torch.tensor([sum(lens[:i]) for i in range(B + 1)], dtype=torch.int32, device=dev)
    pr_dev = torch.from_numpy(proprio).to(dev)
    from vla_adapter_amd.input_stage import serve_layout
    L = serve_layout(lens)[1]
    res["L"] = L
    # both settings of the latency hint captured first (the setting is part of the engine's cache key), then timed in alternating
    # rounds: a difference between them is read against the spread of the rounds
    hints = (True,) if B == 1 else (False, True)

    def batched(hint):
        vla.serve_latency_hint = hint
        return vla.predict_actions((flat, off), pixel_values=px, proprio=pr_dev, proprio_normalized=True, L=L, return_tensors=True)
    for hint in hints:
        for _ in range(3):
            a, _ = batched(hint)
        assert bool(torch.isfinite(a).all())
    runs = {h: [] for h in hints}
    for _ in range(3):
        for h in hints:
            runs[h].append(timed(lambda: batched(h), n))
    for h in hints:
        d, w = sorted(r[0] for r in runs[h]), sorted(r[1] for r in runs[h])
        res["predict_actions_hint_on_ms" if h else "predict_actions_hint_off_ms"] = dict(
            device=round(d[1], 3), device_min=round(d[0], 3), device_max=round(d[2], 3), host=round(w[1], 3))
    best = min(v["device"] for k, v in res.items() if k.startswith("predict_actions_"))
    res["speedup_over_sequential_device"] = round(res["sequential_predict_action_ms"]["device"] / best, 2)
    res["observations_per_s"] = round(B / best * 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=CONFIGS)
    ap.add_argument("--batch", type=int)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--step_timeout", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.all:
        print(json.dumps(one(a.config, a.batch, a.calls)), flush=True)
        return 0
    rows, stopped = [], None
    for config in a.configs.split(","):
        for B in map(int, a.batches.split(",")):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--config", config, "--batch", str(B),
                   "--calls", str(a.calls)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                stopped = dict(config=config, B=B, returncode=r.returncode, stderr_tail=r.stderr[-800:])
                break
            rows.append(json.loads(line[-1]))
            print(line[-1], flush=True)
        if stopped:
            break
    table = dict(tool="tools/bench_serving.py", device="MI355X", weights="random init", rows=rows, stopped_at=stopped)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    if stopped:
        print(json.dumps(dict(stopped_at=stopped)), flush=True)
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
