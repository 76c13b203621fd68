"""Where the fine-tune driver's batches come from and how they are collated: the raw-batch contract (``RAW_BATCH_KEYS``, the statistics
entries a raw batch is normalised with), the one construction of the run's ``GPUInputStage``, the ``Collator`` that turns a raw /
frame / collated batch into the model's batch, one generator per batch source, and ``batch_stream``, which selects and composes them.
The data layer (episodes.py, heldout.py) and the driver (finetune.py, validation.py) both import from here."""
from __future__ import annotations

import json
import os
from pathlib import Path
from typing import Optional

import torch

RAW_BATCH_KEYS = ("frames_u8", "prompt_flat", "prompt_off", "actions_raw", "proprio_raw")

IMAGE_AUG_REFUSAL = ("--image_aug: already normalised pixel_values cannot be augmented; pass raw uint8 frames (frames_u8) with "
                     "--frame_batch_file, or in the batches handed to finetune()")


def pad_to(batch: dict, L: int, pad_id: int) -> dict:
    """Right-pad (collator semantics, data_utils.py:114-134) a batch to the static sequence length of the captured step."""
    cur = batch["input_ids"].shape[1]
    if cur == L:
        return batch
    if cur > L:
        raise ValueError(f"batch with {cur} tokens exceeds the captured sequence length {L}: raise --max_seq_len")
    out = dict(batch)
    pad = lambda t, v: torch.nn.functional.pad(t, (0, L - cur), value=v)
    out["input_ids"], out["labels"] = pad(batch["input_ids"], pad_id), pad(batch["labels"], -100)
    out["attention_mask"] = pad(batch["attention_mask"].to(torch.bool), False)
    return out


def raw_batch_stats(norm_stats: dict, dataset_name: Optional[str] = None) -> dict:
    """The dataset_statistics.json entry a raw batch is normalised with: the one its ``dataset_name`` names, else the file's only one."""
    if dataset_name is None and len(norm_stats) == 1:
        dataset_name = next(iter(norm_stats))
    if dataset_name not in norm_stats:
        raise KeyError(f"dataset statistics hold no entry {dataset_name!r} (the batch's dataset_name; without one the file must hold a "
                       f"single entry): its keys are {sorted(norm_stats)}")
    st = norm_stats[dataset_name]
    if "action" not in st or "proprio" not in st:
        raise KeyError(f"dataset statistics entry {dataset_name!r} needs 'action' and 'proprio', got {sorted(st)}")
    return st


def mixture_stats(norm_stats: dict, dataset_names) -> tuple:
    """(action entries, proprio entries) in the order of a mixed raw batch's ``dataset_names``: what its ``dataset_index`` indexes.
    KeyError naming the dataset the statistics hold no entry for."""
    for n in dataset_names:
        if n not in norm_stats:
            raise KeyError(f"dataset statistics hold no entry {n!r} (one of the batch's dataset_names {tuple(dataset_names)}): their keys "
                           f"are {sorted(norm_stats)}")
    sts = [raw_batch_stats(norm_stats, n) for n in dataset_names]
    return tuple(st["action"] for st in sts), tuple(st["proprio"] for st in sts)


def batch_stats(norm_stats: dict, names, mixed: bool) -> tuple:
    """(action_stats, proprio_stats) as ``GPUInputStage.collate`` takes them: of a mixture one entry per name, in the order
    ``stats_index`` indexes them; else the bare entry of the one dataset ``names`` holds (a None there: the statistics' only one)."""
    if mixed:
        return mixture_stats(norm_stats, names)
    st = raw_batch_stats(norm_stats, names[0])
    return st["action"], st["proprio"]


def input_stage(cfg, mcfg, dev: str):
    """The run's GPU input stage: per-backbone normalisation and image size of the model, frames resized by --frame_resize.  Every
    consumer (training collator, either validator) builds its own with this."""
    from .input_stage import GPUInputStage, backbone_norms
    return GPUInputStage(dev, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img, resize=getattr(cfg, "frame_resize", "bicubic"))


def check_frames(fr: torch.Tensor) -> torch.Tensor:
    if fr.dtype != torch.uint8 or fr.dim() != 5 or fr.shape[-1] != 3:
        raise ValueError(f"frames_u8 must be uint8 [B, n_img, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
    return fr


class Collator:
    """Turns what a source yields into the model's batch.  It owns what every batch of the stream shares: the input stage (built with
    the first batch that carries frames), this rank's micro-step counter - the augmentation's and the collator's step, from ``start``
    on, advanced by every batch that carries frames - and the statistics with the entry lists per tuple of dataset names."""

    def __init__(self, cfg, mcfg, dev: str, rank: int, explicit=(), start: int = 0):
        self.cfg, self.mcfg, self.dev, self.rank, self.explicit = cfg, mcfg, dev, rank, explicit
        self.stage, self.step, self.norm_stats, self.mix_stats = None, int(start), None, {}

    def _stage_and_augment(self):
        from .input_stage import ImageAugment
        if self.stage is None:
            self.stage = input_stage(self.cfg, self.mcfg, self.dev)
        cfg = self.cfg
        return self.stage, (ImageAugment(seed=cfg.seed, rank=self.rank, step=self.step) if cfg.image_aug else None)

    def raw(self, b: dict) -> dict:
        """A raw batch (RAW_BATCH_KEYS, optionally dataset_name, or dataset_index and dataset_names): ``GPUInputStage.collate``."""
        cfg, dev = self.cfg, self.dev
        missing = [k for k in RAW_BATCH_KEYS if k not in b]
        if missing:
            raise ValueError(f"raw batch lacks {missing}: it carries {RAW_BATCH_KEYS} and optionally dataset_name")
        mixed = "dataset_index" in b or "dataset_names" in b
        if mixed and not ("dataset_index" in b and "dataset_names" in b):
            raise ValueError("a raw batch of a dataset mixture carries both dataset_index (int32 [B]) and dataset_names")
        if self.norm_stats is None:
            if not cfg.dataset_statistics_file:
                raise ValueError("raw batches carry un-normalised actions / proprio: pass the statistics with --dataset_statistics_file")
            self.norm_stats = json.load(open(cfg.dataset_statistics_file))
        if mixed:               # every sample with its own dataset's statistics; the entry lists are built once per tuple of names
            names = tuple(b["dataset_names"])
            if names not in self.mix_stats:
                self.mix_stats[names] = batch_stats(self.norm_stats, names, True)
            act_st, pr_st = self.mix_stats[names]
            index = b["dataset_index"].to(dev, torch.int32)
        else:
            (act_st, pr_st), index = batch_stats(self.norm_stats, (b.get("dataset_name"),), False), None
        stage, aug = self._stage_and_augment()
        L = cfg.max_seq_len or None
        if L is None and b["prompt_off"].is_cuda:
            raise ValueError("raw batches with prompt offsets on the device need --max_seq_len (the natural length would be read back)")
        out = stage.collate(b["frames_u8"], (b["prompt_flat"], b["prompt_off"]), b["actions_raw"], b["proprio_raw"], action_stats=act_st,
                            proprio_stats=pr_st, L=L, seed=cfg.seed, rank=self.rank, step=self.step, augment=aug, stats_index=index)
        self.step += 1
        return out

    def frames(self, b: dict) -> dict:
        """A collated batch (on the device) whose ``frames_u8`` stand for ``pixel_values``: augmented under --image_aug, else normalised."""
        fr = check_frames(b.pop("frames_u8"))
        stage, aug = self._stage_and_augment()
        b["pixel_values"] = stage.pixels(fr, augment=aug)
        self.step += 1
        return b

    def collated(self, b: dict) -> dict:
        """An already-collated batch (on the device): nothing to do, and nothing that an explicit --image_aug could act on."""
        if "image_aug" in self.explicit:
            raise NotImplementedError(IMAGE_AUG_REFUSAL)
        return b

    def __call__(self, b: dict) -> dict:
        if "actions_raw" in b:
            return self.raw(b)
        b = {k: v.to(self.dev) for k, v in b.items()}
        return self.frames(b) if "frames_u8" in b else self.collated(b)


# ---------------------------------------------------------------------------------------------------------------- the sources
def pt_files(src: str) -> list:
    """The batch files of ``src``: a .pt dict, or a directory of them in sorted order."""
    return sorted(str(p) for p in Path(src).glob("*.pt")) if os.path.isdir(src) else [src]


def iterable_batches(batches, start: int):
    """An explicit iterable, cycled for ever; the first ``start`` batches are passed over without collating."""
    skip = start
    while True:
        n = 0
        for b in batches:
            n += 1
            if skip > 0:
                skip -= 1
                continue
            yield b
        if n == 0:
            raise ValueError("empty batch iterable")


def episode_batches(cfg, mcfg, dev: str, rank: int, world: int, info: Optional[dict], collator: Collator):
    """``--episode_file`` / ``--episode_mix``: loads the store / mix, checks it against the model and the statistics file, fills ``info``
    (dataset_statistics, store, mixture), prints rank 0's lines; then the raw batch of every micro-step, drawn on the device at the
    collator's own step and normalised with the source's own statistics where no file gives them."""
    jpeg_quality = int(getattr(cfg, "episode_jpeg_quality", 0)) or None          # (0: off - the frames stay in the form their files have)
    if cfg.episode_file:
        from .episodes import EpisodeStore
        where = cfg.episode_file
        src = EpisodeStore.load(cfg.episode_file, dev, chunk=mcfg.chunk, dataset_name=cfg.dataset_name, holdout=cfg.val_episode_fraction,
                                jpeg_scan_index=cfg.jpeg_scan_index, jpeg_quality=jpeg_quality)
    else:
        from .mixture import EpisodeMix, parse_mix
        where = "--episode_mix"
        src = EpisodeMix.load(parse_mix(cfg.episode_mix), dev, chunk=mcfg.chunk, balance_weights=cfg.episode_mix_balance,
                              holdout=cfg.val_episode_fraction, jpeg_scan_index=cfg.jpeg_scan_index, jpeg_quality=jpeg_quality)
    if (src.A, src.Pd) != (mcfg.action_dim, mcfg.proprio_dim):
        raise ValueError(f"{where}: actions_raw / proprio_raw have {src.A} / {src.Pd} columns, the model takes "
                         f"{mcfg.action_dim} / {mcfg.proprio_dim}")
    if src.frame_shape[0] != mcfg.n_img:
        raise ValueError(f"{where}: frames_u8 carries {src.frame_shape[0]} images per step, --num_images_in_input is {mcfg.n_img}")
    if not cfg.dataset_statistics_file:
        collator.norm_stats = src.statistics()
        if info is not None:
            info["dataset_statistics"] = collator.norm_stats
    elif src.mixed:
        mixture_stats(json.load(open(cfg.dataset_statistics_file)), src.names)        # a missing entry is refused before the first step
    if src.jpeg is not None and src.jpeg.seg_ent is not None and rank == 0:      # (a raw store, or a marker per row already: no index)
        j = src.jpeg
        print(json.dumps(dict(jpeg_scan_index=dict(pieces_per_frame=round(int(j.seg_tab.shape[0]) / j.N, 2), index_bytes=j.index_bytes(),
                                                   jpeg_index_bad_scans=int((j.index_status != 0).sum())))), flush=True)
    if cfg.verify_frames:                     # (a raw store has nothing to verify)
        src.verify_frames()
    if info is not None:
        info["store"] = src                   # (the held-out sweep walks the same device-resident tables)
    if src.mixed:
        if info is not None:
            info["mixture"] = src.mixture_info()
        if rank == 0:
            print(json.dumps(dict(mixture=src.mixture_info())), flush=True)
    while True:
        yield src.sample(cfg.batch_size, cfg.seed, rank, world, collator.step)


def file_batches(cfg, rank: int, start: int):
    """``--batch_file`` / ``--frame_batch_file`` / ``--raw_batch_file``, cycled in sorted order from this rank's own offset."""
    src = cfg.batch_file or cfg.frame_batch_file or cfg.raw_batch_file
    files = pt_files(src)
    if not files:
        raise FileNotFoundError(f"no .pt batch files under {src}")
    i = (rank + start) % len(files)
    while True:
        b = torch.load(files[i], weights_only=True)
        if cfg.frame_batch_file and "frames_u8" not in b:
            raise ValueError(f"{files[i]}: --frame_batch_file batches carry frames_u8 (uint8 [B, n_img, H, W, 3])")
        if cfg.raw_batch_file and "actions_raw" not in b:
            raise ValueError(f"{files[i]}: --raw_batch_file batches carry {RAW_BATCH_KEYS}")
        yield b
        i = (i + 1) % len(files)


def synthetic_batches(cfg, mcfg, dev: str, rank: int, start: int):
    """Seeded synthetic batches, collated as they are made: a new one every micro-step."""
    from . import synthetic as S
    i = start
    while True:
        yield S.make_batch(mcfg, cfg.batch_size, dev, seed=1_000_003 * cfg.seed + 7919 * rank + i, P=32, ragged=True)
        i += 1


def batch_stream(cfg, mcfg, dev: str, rank: int, batches=None, explicit=(), world: int = 1, info: Optional[dict] = None,
                 start: int = 0):
    """Endless iterator over collated batches: an explicit iterable, ``--batch_file`` / ``--frame_batch_file`` / ``--raw_batch_file``
    (one .pt dict, or a directory of them, cycled in sorted order; every rank starts at its own offset - the reference's ranks draw independent
    shuffles, finetune.py:988-994), ``--episode_file``, ``--episode_mix``, or seeded synthetic batches (a new one every micro-step).

    ``--episode_file``: the episodes are loaded once into an ``episodes.EpisodeStore`` on the device; micro-step s of this rank collates
    ``store.sample(batch_size, seed, rank, world, s)`` - a raw batch as below, keyed by the same (seed, rank, step).  Without
    --dataset_statistics_file it is normalised with ``store.statistics()``, which is then also left in ``info["dataset_statistics"]``
    (the caller's dict) for the checkpoints.

    ``--val_episode_fraction f``: store and mix are built with ``holdout=f`` - every dataset's last episodes are never drawn here (the
    training table counts no window of theirs) and wait for ``heldout.HeldOutSweep``; the statistics stay over all episodes.
    ``info["store"]`` hands the store / mix to the caller.

    ``--episode_mix``: the same over a weighted mixture of datasets (``mixture.EpisodeMix``): the raw batch then carries
    ``dataset_index`` (int32 [B]) and ``dataset_names``, and every sample is normalised with its own dataset's entry - of the mix's
    statistics, or of --dataset_statistics_file, which must then hold every name (KeyError naming the missing one).  Such a batch
    is collated the same way when it comes from ``--raw_batch_file`` or ``batches``.  ``info["mixture"]`` holds ``mixture_info()``.

    A batch carrying ``frames_u8`` (uint8 [B, n_img, H, W, 3]) instead of ``pixel_values`` goes through the GPU input stage here:
    with --image_aug (default True, as in the reference) the training augmentation of the reference's RLDS pipeline
    (datasets.py:204-218, drawn per image from --seed, the rank and this rank's micro-step counter), else a plain normalise.  The
    normalisation per backbone follows the model config (input_stage.backbone_norms: DINOv2-like ViTs ImageNet, others SigLIP).
    Frames not at the model's image size go through the resize --frame_resize names first.

    A raw batch (``actions_raw`` ...: RAW_BATCH_KEYS) is collated on the device by ``GPUInputStage.collate``: actions and proprio
    normalised with the statistics of ``--dataset_statistics_file`` (the entry named by the batch's ``dataset_name``, or the file's
    only one), token length --max_seq_len (0: the batch's own), filler tokens and augmentation keyed by the same (seed, rank, step).

    ``start`` (--resume_train_state): the micro-step the first batch belongs to.  Every source is a function of that position - the
    samplers', the augmentation's and the collator's step, the file sources' cyclic index, the synthetic source's counter - so the
    stream yields what the stream of a run from 0 yields from its ``start``-th batch on; an explicit iterable is advanced by
    cycling through it without collating."""
    start = int(start)
    assert start >= 0
    collator = Collator(cfg, mcfg, dev, rank, explicit, start)
    if batches is not None:
        yield from map(collator, iterable_batches(batches, start))
    elif cfg.episode_file or cfg.episode_mix:
        yield from map(collator.raw, episode_batches(cfg, mcfg, dev, rank, world, info, collator))
    elif cfg.batch_file or cfg.frame_batch_file or cfg.raw_batch_file:
        yield from map(collator, file_batches(cfg, rank, start))
    else:
        yield from synthetic_batches(cfg, mcfg, dev, rank, start)
