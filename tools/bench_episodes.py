#!/usr/bin/env python3
"""Times the captured adapter-only training step fed from ``--episode_file`` (episodes kept on the device, each batch drawn by
vla_episode_sample + vla_episode_gather) against the same step fed from ``--raw_batch_file`` (one torch.load and a host-to-device copy
per step), on the same box, in one process, on ONE engine and one captured graph: only the batch source differs.

The tool writes a synthetic episode file (``--episodes`` episodes of ``--episode_len`` steps, ``--n_img`` views of the model's image
size, prompts of 27-51 ids) and ``--files`` raw batches drawn from it into a temporary directory, builds the engine of ``--backbone``
(random weights) and runs the loop of ``finetune()``'s captured adapter-only branch - one batch of look-ahead, its vision stage staged
for the next step - over ``finetune.batch_stream`` of either source.  Both go through the same ``collate_raw`` (normalisation, token
assembly, augmentation).

Per source, milliseconds per step: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps.
The sources alternate over ``--rounds`` rounds; the figures are the medians over the rounds with the spread (min - max) beside them.
``not_slower``: the episode-fed median exceeds the file-fed median by no more than the file-fed step's own run-to-run spread
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
    """The episode file and the raw batches drawn from it; returns (episode file, raw batch directory, statistics file)."""
    from vla_adapter_amd.episodes import EpisodeStore
    rng = random.Random(0)
    g = torch.Generator().manual_seed(0)
    E, n, img = args.episodes, args.episode_len, mcfg.vit[0].img
    T = E * n
    lens = [rng.randint(27, 51) for _ in range(E)]
    d = dict(frames_u8=torch.randint(0, 256, (T, args.n_img, img, img, 3), generator=g, dtype=torch.uint8),
             actions_raw=torch.randn(T, mcfg.action_dim, generator=g), proprio_raw=torch.randn(T, mcfg.proprio_dim, generator=g),
             episode_off=torch.arange(E + 1, dtype=torch.int64) * n,
             prompt_flat=torch.randint(0, min(151000, mcfg.llm.vocab - 1), (sum(lens),), generator=g, dtype=torch.int64),
             prompt_off=torch.tensor(np.cumsum([0] + lens), dtype=torch.int32), dataset_name="bench")
    ep_file = os.path.join(tmp, "episodes.pt")
    torch.save(d, ep_file)
    store = EpisodeStore.from_dict(d, "cuda", chunk=mcfg.chunk)
    raw_dir = os.path.join(tmp, "raw")
    os.makedirs(raw_dir)
    for i in range(args.files):
        b = store.sample(args.batch, 0, 0, 1, i)
        torch.save({k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}, os.path.join(raw_dir, f"batch_{i:04d}.pt"))
    stats_file = os.path.join(tmp, "dataset_statistics.json")
    json.dump(store.statistics(), open(stats_file, "w"))
    del store
    torch.cuda.empty_cache()
    return ep_file, raw_dir, stats_file


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--backbone", default="config2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n_img", type=int, default=1)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max_seq_len", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_episodes needs a GPU"
    from vla_adapter_amd import engine as E, finetune as F, synthetic as S
    dev = "cuda:0"
    mcfg = E.NAMED_CONFIGS[args.backbone]()
    mcfg.n_img, mcfg.pro = args.n_img, True                      # as finetune() sets them (--use_pro_version defaults to True)
    with tempfile.TemporaryDirectory() as tmp:
        ep_file, raw_dir, stats_file = write_inputs(tmp, mcfg, args)
        common = ["--use_proprio", "True", "--use_fz", "True", "--batch_size", str(args.batch), "--max_seq_len", str(args.max_seq_len),
                  "--num_images_in_input", str(args.n_img)]
        cfgs = {"raw_batch_file": F.parse_args(common + ["--raw_batch_file", raw_dir, "--dataset_statistics_file", stats_file]),
                "episode_file": F.parse_args(common + ["--episode_file", ep_file])}
        for c in cfgs.values():
            F.check_supported(c, c._explicit)
        streams = {k: F.batch_stream(c, mcfg, dev, 0, None, c._explicit, world=1) for k, c in cfgs.items()}
        eng = E.VLAEngine(mcfg, S.make_weights(mcfg, dev, seed=0), dev)
        pad_id = min(S.PAD_ID, mcfg.llm.vocab - 1)
        L, lr = args.max_seq_len, 1e-4
        noise = torch.zeros(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, device=dev, dtype=torch.bfloat16)
        cur = {k: F._pad_to(next(s), L, pad_id) for k, s in streams.items()}
        static = {k: v.clone() for k, v in cur["raw_batch_file"].items()}
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
    out = dict(device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=L, steps=args.steps,
               rounds=args.rounds, raw_files=args.files, windows=args.episodes * max(args.episode_len - (mcfg.chunk - 1), 0))
    for k, col in samples.items():
        out[f"{k}.step_ms"] = round(statistics.median(col), 3)
        out[f"{k}.step_ms.spread"] = [round(min(col), 3), round(max(col), 3)]
    file_col = samples["raw_batch_file"]
    out["not_slower"] = statistics.median(samples["episode_file"]) - statistics.median(file_col) <= max(file_col) - min(file_col)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
