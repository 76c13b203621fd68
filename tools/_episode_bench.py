"""What bench_episodes.py, bench_mixture.py and bench_heldout.py share: the synthetic episode writer, the engine with its captured
adapter-only step, that step's run loop over ``finetune.batch_stream`` sources, and the median / spread / ``not_slower`` report."""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def add_common_args(ap):
    """The flags all three tools take with the same default; each adds --episodes, --episode_len, --warmup and its own beside them."""
    ap.add_argument("--backbone", default="config2")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n_img", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max_seq_len", type=int, default=128)


def model_config(args):
    from vla_adapter_amd import engine as E
    mcfg = E.NAMED_CONFIGS[args.backbone]()
    mcfg.n_img, mcfg.pro = args.n_img, True                      # as finetune() sets them (--use_pro_version defaults to True)
    return mcfg


def synthetic_episodes(mcfg, args, rng, g) -> dict:
    """``--episodes`` episodes of ``--episode_len`` steps, ``--n_img`` views of the model's image size, prompts of 27-51 ids; rng and
    g: the tool's random.Random and torch.Generator, drawn from in a fixed order."""
    E, n, img = args.episodes, args.episode_len, mcfg.vit[0].img
    T = E * n
    lens = [rng.randint(27, 51) for _ in range(E)]
    return dict(frames_u8=torch.randint(0, 256, (T, args.n_img, img, img, 3), generator=g, dtype=torch.uint8),
                actions_raw=torch.randn(T, mcfg.action_dim, generator=g), proprio_raw=torch.randn(T, mcfg.proprio_dim, generator=g),
                episode_off=torch.arange(E + 1, dtype=torch.int64) * n,
                prompt_flat=torch.randint(0, min(151000, mcfg.llm.vocab - 1), (sum(lens),), generator=g, dtype=torch.int64),
                prompt_off=torch.tensor(np.cumsum([0] + lens), dtype=torch.int32))


def generators():
    return random.Random(0), torch.Generator().manual_seed(0)


def common_flags(args):
    return ["--use_proprio", "True", "--use_fz", "True", "--batch_size", str(args.batch), "--max_seq_len", str(args.max_seq_len),
            "--num_images_in_input", str(args.n_img)]


def new_engine(mcfg, dev: str):
    """The engine of ``mcfg`` with random weights."""
    from vla_adapter_amd import engine as E, synthetic as S
    return E.VLAEngine(mcfg, S.make_weights(mcfg, dev, seed=0), dev)


def capture_step(eng, mcfg, first: dict, dev: str):
    """``finetune()``'s own runner of the adapter-only step, captured on a copy of the padded batch ``first`` (``runner.static``)."""
    from vla_adapter_amd.finetune import StepRunner
    runner = StepRunner(eng, None, mcfg, dev, True, conservative_rows=True)   # prompts of 27-51 ids: the action block moves from batch to batch
    runner.capture(first)
    return runner


def time_sources(args, mcfg, cfgs: dict, base: str, dev: str = "cuda:0"):
    """Milliseconds per captured adapter-only step for every batch source of ``cfgs`` (name -> parsed FinetuneConfig), on ONE engine
    and one graph captured on the first batch of ``base``: ``--warmup`` steps each, then ``--rounds`` rounds of ``--steps`` steps, the
    sources alternating.  -> (samples per source, the info dicts batch_stream filled)."""
    from vla_adapter_amd import finetune as F, synthetic as S
    for c in cfgs.values():
        F.check_supported(c, c._explicit)
    infos = {k: {} for k in cfgs}
    streams = {k: F.batch_stream(c, mcfg, dev, 0, None, c._explicit, world=1, info=infos[k]) for k, c in cfgs.items()}
    eng = new_engine(mcfg, dev)
    pad_id = min(S.PAD_ID, mcfg.llm.vocab - 1)
    L, lr = args.max_seq_len, 1e-4
    cur = {k: F.pad_to(next(s), L, pad_id) for k, s in streams.items()}
    runner = capture_step(eng, mcfg, cur[base], dev)

    def run(which, steps):
        """finetune()'s loop around its captured adapter-only step: one batch of look-ahead, whose pixels the step stages."""
        stream = streams[which]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            nxt = F.pad_to(next(stream), L, pad_id)
            loss3 = runner.step(cur[which], nxt, lr)
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
    return samples, infos


def report(out: dict, samples: dict, unit: str, base: str, other: str) -> dict:
    """Adds per source the median and the (min, max) spread under ``<source>.<unit>``, and ``not_slower``: the median of ``other``
    exceeds the median of ``base`` by no more than base's own run-to-run spread (max - min)."""
    for k, col in samples.items():
        out[f"{k}.{unit}"] = round(statistics.median(col), 3)
        out[f"{k}.{unit}.spread"] = [round(min(col), 3), round(max(col), 3)]
    col = samples[base]
    out["not_slower"] = statistics.median(samples[other]) - statistics.median(col) <= max(col) - min(col)
    return out
