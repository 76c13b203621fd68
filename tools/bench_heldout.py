#!/usr/bin/env python3
"""Times one validation sweep fed from the held-out split of a device-resident episode store (``--val_episode_fraction``:
heldout.HeldOutSweep - windows named and gathered on the device, sums kept on the device, one read-back per sweep) against the same
windows pre-collated into ``--val_batch_file`` batches and swept by ``validation.ValidationPass`` (one torch.load, a host-to-device copy
and a three-float read-back per batch), on the same box, in one process, on ONE captured engine and one set of captured validation
graphs: only the source and the reduction differ.

The tool writes a synthetic episode file (``--episodes`` episodes of ``--episode_len`` steps, ``--n_img`` views of the model's image
size, prompts of 27-51 ids), builds the engine of ``--backbone`` (random weights), captures the adapter-only training step as
``finetune()`` does, holds ``--fraction`` of the episodes out and saves every batch of the held-out sweep, collated, as a
``--val_batch_file`` directory.  The defaults give 256 held-out windows: 8 whole batches of 32, so both sources see the same samples.

Per source, milliseconds per sweep: host clock around one sweep, which ends with its results on the host.  The sources alternate over
``--rounds`` rounds after ``--warmup`` sweeps each; the figures are the medians over the rounds with the spread (min - max) beside them.
``not_slower``: the held-out median exceeds the file-fed median by no more than the file-fed sweep's own run-to-run spread (max - min).
One JSON line."""
import argparse
import json
import os
import tempfile
import time

import _episode_bench as EB
import torch


def write_episodes(tmp, mcfg, args):
    d = dict(EB.synthetic_episodes(mcfg, args, *EB.generators()), dataset_name="bench")
    path = os.path.join(tmp, "episodes.pt")
    torch.save(d, path)
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    EB.add_common_args(ap)
    ap.add_argument("--episodes", type=int, default=16)
    ap.add_argument("--episode_len", type=int, default=71)
    ap.add_argument("--fraction", type=float, default=0.25)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heldout needs a GPU"
    from vla_adapter_amd import finetune as F, synthetic as S
    from vla_adapter_amd.heldout import HeldOutSweep
    dev = "cuda:0"
    mcfg = EB.model_config(args)
    B, L = args.batch, args.max_seq_len
    with tempfile.TemporaryDirectory() as tmp:
        ep_file = write_episodes(tmp, mcfg, args)
        val_dir = os.path.join(tmp, "val")
        os.makedirs(val_dir)
        common = EB.common_flags(args) + ["--episode_file", ep_file, "--use_val_set", "True"]
        cfg_h = F.parse_args(common + ["--val_episode_fraction", str(args.fraction)])
        cfg_f = F.parse_args(common + ["--val_batch_file", val_dir])
        for c in (cfg_h, cfg_f):
            F.check_supported(c, c._explicit)
        info = {}
        stream = F.batch_stream(cfg_h, mcfg, dev, 0, None, cfg_h._explicit, world=1, info=info)
        pad_id = min(S.PAD_ID, mcfg.llm.vocab - 1)
        cur = F.pad_to(next(stream), L, pad_id)
        store = info["store"]
        assert store.Nv % B == 0, f"{store.Nv} held-out windows do not fill whole batches of {B}: the file-fed sweep would average a padded batch"
        eng = EB.new_engine(mcfg, dev)
        static = EB.capture_step(eng, mcfg, cur, dev).static
        sweeper = HeldOutSweep(cfg_h, mcfg, dev, 0, 1, eng, store, info["dataset_statistics"], static, L, True)
        for j in range(sweeper.n_batches):                           # the same windows, collated, as --val_batch_file batches
            b = sweeper.collate(sweeper.draw(j), j)
            torch.save({k: v.cpu() for k, v in b.items()}, os.path.join(val_dir, f"batch_{j:04d}.pt"))
        first = sweeper.sweep(1)                                     # captures the validation graphs on the sweeper's static batch
        files = F.ValidationPass(cfg_f, mcfg, dev, 0, eng, static, L, pad_id, True)
        files.feed.static, files.noise = sweeper.feed.static, sweeper.noise   # one set of captured graphs: both sources replay it on the same buffers
        runs = {"val_batch_file": files.sweep, "val_episode_fraction": sweeper.sweep}

        def run(which):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = runs[which](1)
            dt = (time.perf_counter() - t0) * 1e3
            assert out["loss_value"] == out["loss_value"], f"{which}: non-finite loss"
            return dt, out

        results = {}
        for which in runs:
            for _ in range(args.warmup):
                results[which] = run(which)[1]
        samples = {k: [] for k in runs}
        for _ in range(args.rounds):
            for which in runs:
                samples[which].append(run(which)[0])
    a, b = results["val_episode_fraction"], results["val_batch_file"]
    assert a == first and a["val_samples_count"] == store.Nv and b["val_batches_count"] == sweeper.n_batches
    out = dict(device=torch.cuda.get_device_name(0), backbone=args.backbone, batch=B, n_img=args.n_img, L=L, rounds=args.rounds,
               heldout_windows=store.Nv, batches_per_sweep=sweeper.n_batches,
               loss_value={"val_episode_fraction": a["loss_value"], "val_batch_file": b["loss_value"]})
    print(json.dumps(EB.report(out, samples, "sweep_ms", base="val_batch_file", other="val_episode_fraction")), flush=True)


if __name__ == "__main__":
    main()
