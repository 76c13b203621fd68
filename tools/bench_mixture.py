#!/usr/bin/env python3
"""Times the captured adapter-only training step fed from ``--episode_mix`` (four equal datasets kept on the device, each batch drawn by
vla_mixture_sample + vla_episode_gather and normalised per sample by vla_normalize_bounds_rows) against the same step fed from
``--episode_file`` over the same episodes as ONE dataset (vla_episode_sample + vla_episode_gather, vla_normalize_bounds), on the same
box, in one process, on ONE engine and one captured graph: only the batch source - two small kernels - differs.

The tool writes ``--datasets`` synthetic episode files (``--episodes`` episodes of ``--episode_len`` steps each, ``--n_img`` views of
the model's image size, prompts of 27-51 ids) and one file that holds all of them as a single dataset into a temporary directory,
builds the engine of ``--backbone`` (random weights) and runs the loop of ``finetune()``'s captured adapter-only branch - one batch of
look-ahead, its vision stage staged for the next step - over ``finetune.batch_stream`` of either source.  Both go through the same
``batches.Collator.raw`` (token assembly, augmentation).

Per source, milliseconds per step: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps.
The sources alternate over ``--rounds`` rounds; the figures are the medians over the rounds with the spread (min - max) beside them.
``not_slower``: the mix-fed median exceeds the episode-fed median by no more than the episode-fed step's own run-to-run spread
(max - min).  One JSON line."""
import argparse
import json
import os
import tempfile

import _episode_bench as EB
import torch


def write_inputs(tmp, mcfg, args):
    """The datasets' episode files and the file that holds their episodes as one dataset; returns (mix spec, episode file)."""
    from vla_adapter_amd.episodes import concat_shards
    rng, g = EB.generators()
    parts, spec = [], []
    for i in range(args.datasets):
        d = EB.synthetic_episodes(mcfg, args, rng, g)
        d["actions_raw"], d["proprio_raw"] = d["actions_raw"] * (1 + i), d["proprio_raw"] + i
        parts.append(d)
        f = os.path.join(tmp, f"suite_{i}.pt")
        torch.save(dict(d, dataset_name=f"suite_{i}"), f)
        spec.append(f"{f}=1.0")
    ep_file = os.path.join(tmp, "episodes.pt")
    torch.save(dict(concat_shards(parts), dataset_name="bench"), ep_file)
    return ",".join(spec), ep_file


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    EB.add_common_args(ap)
    ap.add_argument("--datasets", type=int, default=4)
    ap.add_argument("--episodes", type=int, default=4, help="episodes per dataset")
    ap.add_argument("--episode_len", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mixture needs a GPU"
    from vla_adapter_amd import finetune as F
    mcfg = EB.model_config(args)
    with tempfile.TemporaryDirectory() as tmp:
        spec, ep_file = write_inputs(tmp, mcfg, args)
        common = EB.common_flags(args)
        cfgs = {"episode_file": F.parse_args(common + ["--episode_file", ep_file]),
                "episode_mix": F.parse_args(common + ["--episode_mix", spec])}
        samples, infos = EB.time_sources(args, mcfg, cfgs, base="episode_file")
    mi = infos["episode_mix"]["mixture"]
    out = dict(device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=args.batch, n_img=args.n_img, L=args.max_seq_len,
               steps=args.steps, rounds=args.rounds, datasets=args.datasets, quota=mi["quota"], period=mi["period"], windows=sum(mi["windows"]))
    print(json.dumps(EB.report(out, samples, "step_ms", base="episode_file", other="episode_mix")), flush=True)


if __name__ == "__main__":
    main()
