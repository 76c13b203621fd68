#!/usr/bin/env python3
"""Times the captured adapter-only training step fed from ``--episode_mix`` (four equal datasets kept on the device, each batch drawn by
vla_mixture_sample + vla_episode_gather and normalised per sample by vla_normalize_bounds_rows) against the same step fed from
``--episode_file`` over the same episodes as ONE dataset (vla_episode_sample + vla_episode_gather, vla_normalize_bounds), on the same
box, in one process, on ONE engine and one captured graph: only the batch source - two small kernels - differs.

The tool writes ``--datasets`` synthetic episode files (``--episodes`` episodes of ``--episode_len`` steps each, ``--n_img`` views of
the model's image size, prompts of 27-51 ids) and one file that holds all of them as a single dataset into a temporary directory,
builds the engine of ``--backbone`` (random weights) and runs the loop of ``finetune()``'s captured adapter-only branch - one batch of
look-ahead, its vision stage staged for the next step - over ``finetune.batch_stream`` of either source.  Both go through the same
``collate_raw`` (token assembly, augmentation).

Per source, milliseconds per step: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps.
The sources alternate over ``--rounds`` rounds; the figures are the medians over the rounds with the spread (min - max) beside them.
``not_slower``: the mix-fed median exceeds the episode-fed median by no more than the episode-fed step's own run-to-run spread
(max - min).  One JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def write_inputs(tmp, mcfg, args):
    """The datasets' episode files and the file that holds their episodes as one dataset; returns (mix spec, episode file)."""
    from vla_adapter_amd.episodes import concat_shards
    rng = random.Random(0)
    g = torch.Generator().manual_seed(0)
    E, n, img = args.episodes, args.episode_len, mcfg.vit[0].img
    T = E * n
    parts, spec = [], []
    for i in range(args.datasets):
        lens = [rng.randint(27, 51) for _ in range(E)]
        d = dict(frames_u8=torch.randint(0, 256, (T, args.n_img, img, img, 3), generator=g, dtype=torch.uint8),
                 actions_raw=torch.randn(T, mcfg.action_dim, generator=g) * (1 + i), proprio_raw=torch.randn(T, mcfg.proprio_dim, generator=g) + i,
                 episode_off=torch.arange(E + 1, dtype=torch.int64) * n,
                 prompt_flat=torch.randint(0, min(151000, mcfg.llm.vocab - 1), (sum(lens),), generator=g, dtype=torch.int64),
                 prompt_off=torch.tensor(np.cumsum([0] + lens), dtype=torch.int32))
        parts.append(d)
        f = os.path.join(tmp, f"suite_{i}.pt")
        torch.save(dict(d, dataset_name=f"suite_{i}"), f)
        spec.append(f"{f}=1.0")
    ep_file = os.path.join(tmp, "episodes.pt")
    torch.save(dict(concat_shards(parts), dataset_name="bench"), ep_file)
    return ",".join(spec), ep_file


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--backbone", default="config2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n_img", type=int, default=1)
    ap.add_argument("--datasets", type=int, default=4)
    ap.add_argument("--episodes", type=int, default=4, help="episodes per dataset")
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max_seq_len", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixture needs a GPU"
    from vla_adapter_amd import engine as E, finetune as F, synthetic as S
    dev = "cuda:0"
    mcfg = E.NAMED_CONFIGS[args.backbone]()
    mcfg.n_img, mcfg.pro = args.n_img, True                      # as finetune() sets them (--use_pro_version defaults to True)
    with tempfile.TemporaryDirectory() as tmp:
        spec, ep_file = write_inputs(tmp, mcfg, args)
        common = ["--use_proprio", "True", "--use_fz", "True", "--batch_size", str(args.batch), "--max_seq_len", str(args.max_seq_len),
                  "--num_images_in_input", str(args.n_img)]
        cfgs = {"episode_file": F.parse_args(common + ["--episode_file", ep_file]),
                "episode_mix": F.parse_args(common + ["--episode_mix", spec])}
        for c in cfgs.values():
            F.check_supported(c, c._explicit)
        infos = {k: {} for k in cfgs}
        streams = {k: F.batch_stream(c, mcfg, dev, 0, None, c._explicit, world=1, info=infos[k]) for k, c in cfgs.items()}
        eng = E.VLAEngine(mcfg, S.make_weights(mcfg, dev, seed=0), dev)
        pad_id = min(S.PAD_ID, mcfg.llm.vocab - 1)
        L, lr = args.max_seq_len, 1e-4
        noise = torch.zeros(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, device=dev, dtype=torch.bfloat16)
        cur = {k: F._pad_to(next(s), L, pad_id) for k, s in streams.items()}
        static = {k: v.clone() for k, v in cur["episode_file"].items()}
        eng.capture(static, noise, conservative_rows=True)          # prompts of 27-51 ids: the action block moves from batch to batch

        def run(which, steps):
            """finetune()'s captured adapter-only loop: copy the current batch's small tensors, stage the next batch's pixels, replay."""
            stream = streams[which]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                nxt = F._pad_to(next(stream), L, pad_id)
                for k in static:
                    if k != "pixel_values":
                        static[k].copy_(cur[which][k])
                eng.stage_next_pixels(nxt["pixel_values"])
                loss3 = eng.train_step_graphed(lr)
                cur[which] = nxt
            eng.flush()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            assert bool(torch.isfinite(loss3).all()), f"{which}: non-finite loss"
            return dt * 1e3

        for which in streams:
            run(which, args.warmup)
        samples = {k: [] for k in streams}
        for _ in range(args.rounds):
            for which in streams:
                samples[which].append(run(which, args.steps))
    mi = infos["episode_mix"]["mixture"]
    out = dict(device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=L, steps=args.steps,
               rounds=args.rounds, datasets=args.datasets, quota=mi["quota"], period=mi["period"], windows=sum(mi["windows"]))
    for k, col in samples.items():
        out[f"{k}.step_ms"] = round(statistics.median(col), 3)
        out[f"{k}.step_ms.spread"] = [round(min(col), 3), round(max(col), 3)]
    base = samples["episode_file"]
    out["not_slower"] = statistics.median(samples["episode_mix"]) - statistics.median(base) <= max(base) - min(base)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
