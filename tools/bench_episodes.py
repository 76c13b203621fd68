#!/usr/bin/env python3
"""Times the captured adapter-only training step fed from ``--episode_file`` (episodes kept on the device, each batch drawn by
vla_episode_sample + vla_episode_gather) against the same step fed from ``--raw_batch_file`` (one torch.load and a host-to-device copy
per step), on the same box, in one process, on ONE engine and one captured graph: only the batch source differs.

The tool writes a synthetic episode file (``--episodes`` episodes of ``--episode_len`` steps, ``--n_img`` views of the model's image
size, prompts of 27-51 ids) and ``--files`` raw batches drawn from it into a temporary directory, builds the engine of ``--backbone``
(random weights) and runs the loop of ``finetune()``'s captured adapter-only branch - one batch of look-ahead, its vision stage staged
for the next step - over ``finetune.batch_stream`` of either source.  Both go through the same ``batches.Collator.raw`` (normalisation, token
assembly, augmentation).

Per source, milliseconds per step: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps.
The sources alternate over ``--rounds`` rounds; the figures are the medians over the rounds with the spread (min - max) beside them.
``not_slower``: the episode-fed median exceeds the file-fed median by no more than the file-fed step's own run-to-run spread
(max - min).  One JSON line."""
import argparse
import json
import os
import tempfile

import _episode_bench as EB
import torch


def write_inputs(tmp, mcfg, args):
    """The episode file and the raw batches drawn from it; returns (episode file, raw batch directory, statistics file)."""
    from vla_adapter_amd.episodes import EpisodeStore
    d = dict(EB.synthetic_episodes(mcfg, args, *EB.generators()), dataset_name="bench")
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
    EB.add_common_args(ap)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_episodes needs a GPU"
    from vla_adapter_amd import finetune as F
    mcfg = EB.model_config(args)
    with tempfile.TemporaryDirectory() as tmp:
        ep_file, raw_dir, stats_file = write_inputs(tmp, mcfg, args)
        common = EB.common_flags(args)
        cfgs = {"raw_batch_file": F.parse_args(common + ["--raw_batch_file", raw_dir, "--dataset_statistics_file", stats_file]),
                "episode_file": F.parse_args(common + ["--episode_file", ep_file])}
        samples, _ = EB.time_sources(args, mcfg, cfgs, base="raw_batch_file")
    out = dict(device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=args.max_seq_len,
               steps=args.steps, rounds=args.rounds, raw_files=args.files, windows=args.episodes * max(args.episode_len - (mcfg.chunk - 1), 0))
    print(json.dumps(EB.report(out, samples, "step_ms", base="raw_batch_file", other="episode_file")), flush=True)


if __name__ == "__main__":
    main()
