"""A weighted mixture of device-resident episode datasets: the reference's normal mode of feeding a fine-tune.

``RLDSDataset`` always builds a mixture (prismatic/vla/datasets/datasets.py:160-200); ``make_interleaved_dataset``
(rlds/dataset.py:490-585) normalises every dataset with its own q01 / q99 statistics, interleaves the datasets frame by frame with
``sample_weights`` - multiplied by each dataset's transition count under ``balance_weights`` - and lets every dataset run through its
own endless epochs.  ``EpisodeMix`` keeps D datasets back to back in one set of tables (``episodes.EpisodeTables``) and draws each
step's batch with ``vla_mixture_sample`` (csrc/mixture.hip, include/vla_mixture.h) and the unchanged ``vla_episode_gather``; the batch
carries ``dataset_index``, with which ``GPUInputStage.collate`` normalises every sample with its own dataset's statistics
(``vla_normalize_bounds_rows``).  No host work per step: nothing is read back, synchronised or, after the first call, allocated.

The sampling rule is stated here in plain Python - ``probabilities``, ``quotas``, ``sample_windows`` - and is the specification the
kernel is tested against, bit for bit.  It is stateless: sample b of (rank, step) is a function of the seed
and its position alone, so ranks need no communication and a batch may straddle periods and dataset epochs.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .constants import NUM_ACTIONS_CHUNK
from .episodes import _M64, EpisodeTables, epoch_key, load_tables, locate, permute_index, sample_position, splitmix64_key

MIX_STREAM = 0x313D0DA7A5E75            # csrc/mixture.hip: keeps the period shuffle apart from the window shuffle (EPISODE_STREAM), the
                                        # collator's (COLLATE_STREAM) and the augmentation's draws under equal seed words
DEFAULT_PERIOD = 65536


# ---------------------------------------------------------------------------------------------------------------- the sampling rule
def probabilities(weights: Sequence[float], transitions: Sequence[int], balance_weights: bool = True) -> np.ndarray:
    """rlds/dataset.py:514-517 in float64: p_d = w_d T_d / sum(w T) with balance_weights, else w_d / sum(w)."""
    w = np.asarray(weights, dtype=np.float64)
    if balance_weights:
        w = w * np.asarray(transitions, dtype=np.float64)
    return w / w.sum()


def quotas(p: Sequence[float], Q: int) -> List[int]:
    """The Q slots of one period shared out over the datasets as integers q_d >= 1 that sum to Q: floor(p Q), at least 1, then the
    largest remainders are served first (ties: lowest index); where the floor of 1 overdrew the period, the datasets furthest above
    their share give a slot back."""
    p = np.asarray(p, dtype=np.float64)
    D = p.size
    if D > Q:
        raise ValueError(f"period: {D} datasets do not fit a period of {Q} slots (every dataset gets at least one)")
    share = p * Q
    q = np.maximum(np.floor(share), 1.0).astype(np.int64)
    while q.sum() < Q:
        q[int(np.argmax(share - q))] += 1
    while q.sum() > Q:
        rest = np.where(q > 1, share - q, np.inf)
        q[int(np.argmin(rest))] -= 1
    return [int(x) for x in q]


def period_key(seed: int, period: int) -> int:
    return splitmix64_key((seed & _M64) ^ MIX_STREAM, period)


def sample_window(pos: int, valid_off, dataset_off, quota_off, seed: int) -> Tuple[int, int, int, int]:
    """Draw ``pos`` of the endless sequence -> (dataset, ordinal in that dataset's own stream, global episode, step inside it)."""
    D, Q = len(dataset_off) - 1, int(quota_off[-1])
    k, s = pos // Q, pos % Q
    s2 = permute_index(s, Q, period_key(seed, k))
    d = max(x for x in range(D) if int(quota_off[x]) <= s2)
    c = k * (int(quota_off[d + 1]) - int(quota_off[d])) + (s2 - int(quota_off[d]))
    v0 = int(valid_off[int(dataset_off[d])])
    N_d = int(valid_off[int(dataset_off[d + 1])]) - v0
    ep_d, i = c // N_d, c % N_d
    j = v0 + permute_index(i, N_d, splitmix64_key(epoch_key(seed, ep_d), d + 1))
    e, t = locate(j, valid_off)
    return d, c, e, t


def sample_windows(valid_off, dataset_off, quota_off, B: int, seed: int, rank: int, world: int, step: int) -> List[Tuple[int, int, int]]:
    """The (dataset, global episode, step inside it) of every sample of the batch of (rank, step): what vla_mixture_sample computes."""
    out = []
    for b in range(B):
        d, _, e, t = sample_window(sample_position(B, rank, world, step, b), valid_off, dataset_off, quota_off, seed)
        out.append((d, e, t))
    return out


# ---------------------------------------------------------------------------------------------------------------- the mix
def parse_mix(text: str) -> List[Tuple[str, float]]:
    """``"pathA=1.0,pathB=0.5"`` -> [(path, weight)]; a weight defaults to 1.0."""
    entries = []
    for part in str(text).split(","):
        part = part.strip()
        if not part:
            continue
        path, eq, w = part.rpartition("=")
        if not eq:
            path, w = part, "1.0"
        try:
            weight = float(w)
        except ValueError:
            raise ValueError(f"--episode_mix: the weight of {path!r} is {w!r}, not a number (path=weight,path=weight ...)") from None
        if not path:
            raise ValueError(f"--episode_mix: {part!r} names no path (path=weight,path=weight ...)")
        entries.append((path, weight))
    if not entries:
        raise ValueError("--episode_mix names no dataset (path=weight,path=weight ...)")
    return entries


class EpisodeMix(EpisodeTables):
    """D datasets on the device in one set of tables; ``sample()`` draws one raw batch of the weighted mixture.  Build with
    ``EpisodeMix.load`` or ``EpisodeMix.from_dicts``."""

    mixed = True

    def __init__(self, tables: List[dict], weights: Sequence[float], names: Sequence[str], device, chunk: int = NUM_ACTIONS_CHUNK,
                 period: int = DEFAULT_PERIOD, balance_weights: bool = True, *, holdout: Optional[float] = None, jpeg_scan_index: bool = False):
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        if not tables:
            raise ValueError("an episode mix needs at least one dataset")
        names = [str(n) for n in names]
        for n in names:
            if names.count(n) > 1:
                raise ValueError(f"dataset_name {n!r} is given by {names.count(n)} entries of the mix: every dataset needs its own name")
        for n, w in zip(names, weights):
            if not (isinstance(w, (int, float)) and float(w) > 0.0 and math.isfinite(float(w))):      # (NaN fails the comparison too)
                raise ValueError(f"{n}: weight must be a finite number > 0, got {w!r}")
        super().__init__(tables, names, device, chunk, holdout=holdout, jpeg_scan_index=jpeg_scan_index)
        # transitions, p and the quotas stay over ALL episodes under holdout=f (episodes.EpisodeTables); windows are the training
        # windows N_d, which the sampler reads from valid_off on the device
        self.weights, self.balance_weights, self.Q = [float(w) for w in weights], bool(balance_weights), int(period)
        self.transitions = [int(d["actions_raw"].shape[0]) for d in tables]
        ds_off, valid = self.episode_ranges, self.valid_off_host
        self.windows = [int(valid[ds_off[d + 1]]) - int(valid[ds_off[d]]) for d in range(self.D)]
        self.p = probabilities(self.weights, self.transitions, self.balance_weights)
        self.quota = quotas(self.p, self.Q)
        self.dataset_off_host = torch.tensor(ds_off, dtype=torch.int32)
        self.quota_off_host = torch.tensor(np.cumsum([0] + self.quota), dtype=torch.int64)
        self.dataset_off, self.quota_off = self._upload(self.dataset_off_host), self._upload(self.quota_off_host)

    # ---- construction --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dicts(cls, entries, device, chunk: int = NUM_ACTIONS_CHUNK, period: int = DEFAULT_PERIOD, balance_weights: bool = True, *,
                   holdout: Optional[float] = None, jpeg_scan_index: bool = False) -> "EpisodeMix":
        """``entries``: [(tables dict, weight)]; a dict without dataset_name is called dataset_<index>."""
        return cls.load(entries, device, chunk, period, balance_weights, holdout=holdout, jpeg_scan_index=jpeg_scan_index)

    @classmethod
    def load(cls, entries, device, chunk: int = NUM_ACTIONS_CHUNK, period: int = DEFAULT_PERIOD, balance_weights: bool = True, *,
             holdout: Optional[float] = None, jpeg_scan_index: bool = False, jpeg_quality: Optional[int] = None) -> "EpisodeMix":
        """``entries``: [(path or tables dict, weight)]; a path is anything ``EpisodeStore.load`` takes.  A dataset is called by its
        file's dataset_name, else by the path's stem.  ``holdout``: the fraction of every dataset's episodes - its last ones - set aside
        for validation (episodes.EpisodeStore); None: every table and batch is what it is without the argument.  ``jpeg_scan_index``:
        JPEG frames get a scan index at load (episodes.EpisodeTables).  ``jpeg_quality``: raw frames are coded on the device into the
        JPEG form, dataset by dataset (EpisodeStore.load); a dataset already in that form stays as it is."""
        tables, weights, names = [], [], []
        for i, entry in enumerate(entries):
            src, w = entry if isinstance(entry, (tuple, list)) else (entry, 1.0)
            if isinstance(src, dict):
                d, fallback = src, f"dataset_{i}"
                if jpeg_quality is not None:
                    from .jpeg_store import encode_tables
                    d = encode_tables(d, device, jpeg_quality, where=str(d.get("dataset_name") or fallback))
            else:
                d, fallback = load_tables(src, device, jpeg_quality=jpeg_quality), Path(str(src)).stem
            if not isinstance(d, dict):
                raise ValueError(f"entry {i} of the mix: an episode file is a dict")
            name = d.get("dataset_name")
            tables.append(d)
            weights.append(w)
            names.append(name if isinstance(name, str) and name else fallback)
        return cls(tables, weights, names, device, chunk, period, balance_weights, holdout=holdout, jpeg_scan_index=jpeg_scan_index)

    # ---- what the mix is -----------------------------------------------------------------------------------------------------
    def mixture_info(self) -> dict:
        """Names, probabilities, quotas, the period, and the reference's dataset_len (rlds/dataset.py:512-522): the draws until every
        primary dataset - weight == 1.0 - has completed an epoch; None when no weight is 1.0 (the reference fails there)."""
        primary = [t / p for t, p, w in zip(self.transitions, self.p.tolist(), self.weights) if w == 1.0]
        return dict(datasets=list(self.names), weights=list(self.weights), balance_weights=self.balance_weights, p=self.p.tolist(),
                    quota=list(self.quota), period=self.Q, num_transitions=list(self.transitions), windows=list(self.windows),
                    dataset_len=int(max(primary)) if primary else None)

    # ---- the batch -----------------------------------------------------------------------------------------------------------
    def sample_indices(self, B: int, seed: int, rank: int, world: int, step: int):
        """vla_mixture_sample into the mix's buffers of batch size B -> (ds int32 [B], ep int32 [B], row int64 [B], prompt_off int32 [B + 1])."""
        from . import ops
        self._check_draw(B, rank, world, step)
        o = self._buffers(B)
        ops.mixture_sample(self.valid_off, self.episode_off, self.prompt_off, self.dataset_off, self.quota_off, seed, rank, world, step, self.Pmax,
                           o["dataset_index"], o["ep"], o["row"], o["prompt_off"])
        return o["dataset_index"], o["ep"], o["row"], o["prompt_off"]

    def sample(self, B: int, seed: int, rank: int = 0, world: int = 1, step: int = 0) -> dict:
        """The raw batch of (rank, step): RAW_BATCH_KEYS on the device plus dataset_index int32 [B] (which dataset each sample came
        from) and dataset_names.  Every rank passes the same seed.  The tensors are the mix's own buffers of this batch size: the next
        call with the same B overwrites them (in stream order), so consume - collate - a batch before drawing the next, or clone it."""
        ds, ep, row, off = self.sample_indices(B, seed, rank, world, step)
        out = self.gather(ep, row, off, self._buffers(B))
        out["dataset_index"] = ds
        out["dataset_names"] = self.names
        return out
