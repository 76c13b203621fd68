#!/usr/bin/env python3
"""Serving a token-CE model: OpenVLAForActionPrediction.generate_actions (one prefill, T - 1 cached single-token steps, captured)
against the only way there was before it - T uncached passes of forward_vlm(action_queries=False) + token_ce on the growing sequence
with the argmax taken on the host - on `config2` (SigLIP-224 + Qwen2.5-0.5B, one image) for B in {1, 8}, T = 56.

    tools/bench_generate.py --batch 1                     one step: one JSON line
    tools/bench_generate.py --all --out profiles/generate.json
    tools/bench_generate.py --all --do_sample --baseline_repeats 0 --out profiles/generate_sample.json

--all starts one child process per B, each under its own `timeout -k 10`, and stops at the first step that fails: nothing is started
on a device after a step that faulted or hung.  Rows that did not run are absent from the table - no number is made up.
--do_sample also times, in the same process and on the same captured shapes, the sampled call (do_sample with temperature 0.8,
top-k 50, top-p 0.95 and with both filters off, each with return_logprobs) and the greedy call with return_logprobs, and reports
the per-token times side by side; --baseline_repeats 0 leaves the uncached baseline out.
Random-init weights, synthetic inputs (a 48-id prompt per sample, +-4 ids so that the batch is ragged); replayed calls only.
Times: HIP events on the caller's stream around one whole generation (generate_actions with return_tensors=True does not
synchronise), median of the repeats with minimum and maximum; the baseline synchronises once per token by construction."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 8)
P, T = 48, 56   # LIBERO prompt with the Qwen chat template (~48 ids); NUM_ACTIONS_CHUNK * ACTION_DIM
STATS = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}}}


def timed(fn, repeats):
    import torch
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return dict(median=round(out[len(out) // 2], 3), min=round(out[0], 3), max=round(out[-1], 3), repeats=repeats)


SAMPLED = {"greedy_logprobs": dict(return_logprobs=True),
           "sampled_t0.8_k50_p0.95": dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95, seed=1, return_logprobs=True),
           "sampled_t1_k0_p1": dict(do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=1, return_logprobs=True)}


def sample_tokens_alone(B: int, V: int, D: int, launches: int = 50) -> dict:
    """vla_sample_tokens with its advance on random logits (4 randn, bf16), alone on the stream: microseconds per call over `launches`
    back-to-back calls, per setting - where the sampled step's extra time goes."""
    import torch
    from vla_adapter_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(2)
    logits = (4.0 * torch.randn(B, V, generator=g)).to(torch.bfloat16).to(dev)
    embed, x_next = torch.zeros(V, D, dtype=torch.bfloat16, device=dev), torch.zeros(B, D, dtype=torch.bfloat16, device=dev)
    out_ids, logprobs = torch.zeros(B, launches, dtype=torch.int64, device=dev), torch.zeros(B, launches, device=dev)
    step, pos = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    out = {}
    for name, kw in (("greedy", dict(greedy=True)), ("t0.8_k50_p0.95", dict(temperature=0.8, top_k=50, top_p=0.95, seed=1)),
                     ("t1_k0_p0.95", dict(top_p=0.95, seed=1)), ("t1_k50_p1", dict(top_k=50, seed=1)), ("t1_k0_p1", dict(seed=1))):
        blk = ops.sample_params(**kw).to(dev)

        def run():
            step.zero_()
            for _ in range(launches):
                ops.sample_tokens(logits, blk, step, logprob_out=logprobs, advance=(out_ids, step, pos, embed, x_next))
        run()
        out[name] = round(1e3 * timed(run, 5)["median"] / launches, 2)
    return out


def one(B: int, repeats: int, baseline_repeats: int, do_sample: bool = False) -> dict:
    import torch
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    dev = "cuda"
    cfg = E.config2()
    vla = OpenVLAForActionPrediction(cfg, S.make_weights(cfg, dev, seed=0), dev, norm_stats=STATS)
    g = torch.Generator().manual_seed(1)
    lens = [P] + [P - 4 + int(torch.randint(0, 9, (1,), generator=g)) for _ in range(B - 1)]
    prompts = [torch.randint(0, 151000, (m,), generator=g).tolist() for m in lens]
    img = cfg.vit[0].img
    px = torch.randn(B, 3 * len(cfg.vit) * cfg.n_img, img, img, generator=g).clamp_(-3, 3).to(torch.bfloat16).to(dev)
    res = dict(config="config2", B=B, T=T, prompt_lens=[min(lens), max(lens)], n_patches=cfg.n_patches, vocab=cfg.llm.vocab)

    cached = lambda: vla.generate_actions(prompts, pixel_values=px, max_new_tokens=T, return_tokens=True, return_tensors=True)
    for _ in range(3):
        actions, tokens = cached()
    assert bool(torch.isfinite(actions).all())
    res["generate_actions_ms"] = timed(cached, repeats)
    res["ms_per_token"] = round(res["generate_actions_ms"]["median"] / T, 4)
    if do_sample:
        for name, kw in SAMPLED.items():
            call = lambda kw=kw: vla.generate_actions(prompts, pixel_values=px, max_new_tokens=T, return_tokens=True, return_tensors=True, **kw)
            for _ in range(3):
                _, _, logprobs = call()
            assert bool(torch.isfinite(logprobs).all())
            ms = timed(call, repeats)
            res[name] = dict(ms=ms, ms_per_token=round(ms["median"] / T, 4),
                             extra_us_per_token=round(1e3 * (ms["median"] - res["generate_actions_ms"]["median"]) / T, 2))
        res["generate_actions_again_ms"] = timed(cached, repeats)          # the greedy call once more: the run-to-run spread on this box
        res["sample_tokens_us"] = sample_tokens_alone(B, cfg.llm.vocab, cfg.llm.d)
    if baseline_repeats < 1:
        return res

    # the parent's way: the whole growing sequence through every layer and the lm_head over ALL rows, once per token
    eng, Np, pad = vla.engine, cfg.n_patches, vla.input_stage().pad

    def uncached():
        rows = [list(p) for p in prompts]
        for _ in range(T):
            L = -(-max(len(r) for r in rows) // 32) * 32
            ids = torch.tensor([r + [pad] * (L - len(r)) for r in rows], dtype=torch.int64, device=dev)
            am = torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows], dtype=torch.bool, device=dev)
            eng.forward_vlm(dict(input_ids=ids, attention_mask=am, pixel_values=px), action_queries=False)
            _, logits = eng.token_ce(ids)
            nxt = [int(logits[b, Np + len(r) - 1].float().argmax()) for b, r in enumerate(rows)]
            for r, t in zip(rows, nxt):
                r.append(t)
        return torch.tensor([r[-T:] for r in rows])

    base_tokens = uncached()
    res["uncached_forward_vlm_token_ce_ms"] = timed(uncached, baseline_repeats)
    res["tokens_equal_to_uncached"] = round(float((base_tokens == tokens.cpu()).float().mean()), 4)   # (near-ties may differ: other GEMM tiles)
    res["speedup"] = round(res["uncached_forward_vlm_token_ce_ms"]["median"] / res["generate_actions_ms"]["median"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--baseline_repeats", type=int, default=3)
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--do_sample", action="store_true")
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    ap.add_argument("--step_timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not a.all:
        print(json.dumps(one(a.batch, a.repeats, a.baseline_repeats, a.do_sample)), flush=True)
        return 0
    rows, stopped = [], None
    for B in map(int, a.batches.split(",")):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--batch", str(B), "--repeats", str(a.repeats),
               "--baseline_repeats", str(a.baseline_repeats)] + (["--do_sample"] if a.do_sample else [])
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            stopped = dict(B=B, returncode=r.returncode, stderr_tail=r.stderr[-800:])
            break
        rows.append(json.loads(line[-1]))
        print(line[-1], flush=True)
    table = dict(tool="tools/bench_generate.py", device="MI355X", weights="random init", rows=rows, stopped_at=stopped)
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
