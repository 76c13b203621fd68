"""A weighted mixture of device-resident episode datasets: the reference's normal mode of feeding a fine-tune.

``RLDSDataset`` always builds a mixture (prismatic/vla/datasets/datasets.py:160-200); ``make_interleaved_dataset``
(rlds/dataset.py:490-585) normalises every dataset with its own q01 / q99 statistics, interleaves the datasets frame by frame with
``sample_weights`` - multiplied by each dataset's transition count under ``balance_weights`` - and lets every dataset run through its
own endless epochs.  ``EpisodeMix`` keeps D datasets back to back in one set of the tables of ``episodes.EpisodeStore`` and draws each
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
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .constants import NUM_ACTIONS_CHUNK
from .episodes import (MAX_BATCH, _M64, _check_shard, check_holdout, check_position, check_split, concat_shards, dataset_statistics, epoch_key, load_tables, locate, permute_index,
                       sample_position, split_offsets, splitmix64_key, valid_offsets)
from .finetune import RAW_BATCH_KEYS

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


class EpisodeMix:
    """D datasets on the device in one set of tables; ``sample()`` draws one raw batch of the weighted mixture.  Build with
    ``EpisodeMix.load`` or ``EpisodeMix.from_dicts``."""

    def __init__(self, tables: List[dict], weights: Sequence[float], names: Sequence[str], device, chunk: int = NUM_ACTIONS_CHUNK,
                 period: int = DEFAULT_PERIOD, balance_weights: bool = True, *, holdout: Optional[float] = None):
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
        for d, n in zip(tables, names):
            _check_shard(d, n)
        self.device, self.chunk, self.names = device, int(chunk), tuple(names)
        self.weights, self.balance_weights = [float(w) for w in weights], bool(balance_weights)
        self.action_masks = [torch.as_tensor(d["action_mask"]).tolist() if "action_mask" in d else None for d in tables]
        ds_off, self.transitions, self.windows, stats = [0], [], [], {}
        for d, n, mask in zip(tables, names, self.action_masks):
            E_d = int(d["episode_off"].numel() - 1)
            N_d = int(valid_offsets(d["episode_off"].cpu(), self.chunk)[-1])
            if N_d < 1:
                raise ValueError(f"{n}: no valid window - every one of the {E_d} episodes is shorter than the action chunk of {self.chunk} "
                                 "steps (episode_off)")
            ds_off.append(ds_off[-1] + E_d)
            self.transitions.append(int(d["actions_raw"].shape[0]))
            self.windows.append(N_d)
            stats[n] = dataset_statistics(d["actions_raw"].cpu().numpy(), d["proprio_raw"].cpu().numpy(), E_d, mask)
        self._stats = stats
        # one set of tables: the datasets' rows and episodes back to back (names and masks are the mix's own business)
        bare = [{k: v for k, v in d.items() if k not in ("dataset_name", "action_mask")} for d in tables]
        all_ = concat_shards(bare, list(names), device)
        self.D, self.Q = len(tables), int(period)
        self.p = probabilities(self.weights, self.transitions, self.balance_weights)
        self.quota = quotas(self.p, self.Q)
        act, pr, eo, po = all_["actions_raw"], all_["proprio_raw"], all_["episode_off"], all_["prompt_off"]
        valid = valid_offsets(eo.cpu(), self.chunk)
        self.T, self.E = int(act.shape[0]), int(eo.numel() - 1)
        # holdout=f: every dataset sets its own last H_d episodes aside (episodes.EpisodeStore).  transitions, p, the quotas and the
        # statistics stay over ALL episodes - the reference balances and normalises over split="all" (rlds/dataset.py:209-211) -;
        # windows becomes the training windows N_d, which the sampler reads from valid_off on the device
        self.holdout, self.heldout, val = holdout, None, None
        if holdout is not None:
            held = torch.zeros(self.E, dtype=torch.bool)
            counts = [check_holdout(holdout, ds_off[d + 1] - ds_off[d], n) for d, n in enumerate(names)]
            for d, H in enumerate(counts):
                held[ds_off[d + 1] - H:ds_off[d + 1]] = True
            valid, val = split_offsets(eo.cpu(), self.chunk, held)
            self.heldout = {n: check_split(valid, val, ds_off[d], ds_off[d + 1], counts[d], self.chunk, n) for d, n in enumerate(names)}
            self.windows = [self.heldout[n]["train_windows"] for n in names]
        self.N = int(valid[-1])
        self.Nv = int(val[-1]) if val is not None else 0
        self.val_off_host = val
        self.A, self.Pd = int(act.shape[1]), int(pr.shape[1])
        self.frame_shape = tuple(all_["frames_u8"].shape[1:])
        self.row_bytes = int(np.prod(self.frame_shape))
        self.Pmax = int(po.diff().max())
        self.valid_off_host = valid
        self.dataset_off_host = torch.tensor(ds_off, dtype=torch.int32)
        self.quota_off_host = torch.tensor(np.cumsum([0] + self.quota), dtype=torch.int64)
        dv = lambda t: t.to(device).contiguous()
        self.frames_u8, self.actions_raw, self.proprio_raw = dv(all_["frames_u8"]), dv(act), dv(pr)
        self.episode_off, self.valid_off = dv(eo), dv(valid)
        self.val_off = dv(val) if val is not None else None
        self.prompt_flat, self.prompt_off = dv(all_["prompt_flat"]), dv(po)
        self.dataset_off, self.quota_off = dv(self.dataset_off_host), dv(self.quota_off_host)
        self._out: Dict[int, dict] = {}

    # ---- construction --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dicts(cls, entries, device, chunk: int = NUM_ACTIONS_CHUNK, period: int = DEFAULT_PERIOD, balance_weights: bool = True, *,
                   holdout: Optional[float] = None) -> "EpisodeMix":
        """``entries``: [(tables dict, weight)]; a dict without dataset_name is called dataset_<index>."""
        return cls.load(entries, device, chunk, period, balance_weights, holdout=holdout)

    @classmethod
    def load(cls, entries, device, chunk: int = NUM_ACTIONS_CHUNK, period: int = DEFAULT_PERIOD, balance_weights: bool = True, *,
             holdout: Optional[float] = None) -> "EpisodeMix":
        """``entries``: [(path or tables dict, weight)]; a path is anything ``EpisodeStore.load`` takes.  A dataset is called by its
        file's dataset_name, else by the path's stem.  ``holdout``: the fraction of every dataset's episodes - its last ones - set aside
        for validation (episodes.EpisodeStore); None: every table and batch is what it is without the argument."""
        tables, weights, names = [], [], []
        for i, entry in enumerate(entries):
            src, w = entry if isinstance(entry, (tuple, list)) else (entry, 1.0)
            if isinstance(src, dict):
                d, fallback = src, f"dataset_{i}"
            else:
                d, fallback = load_tables(src, device), Path(str(src)).stem
            if not isinstance(d, dict):
                raise ValueError(f"entry {i} of the mix: an episode file is a dict")
            name = d.get("dataset_name")
            tables.append(d)
            weights.append(w)
            names.append(name if isinstance(name, str) and name else fallback)
        return cls(tables, weights, names, device, chunk, period, balance_weights, holdout=holdout)

    # ---- what the mix is -----------------------------------------------------------------------------------------------------
    def statistics(self) -> dict:
        """One reference-shaped get_dataset_statistics entry per dataset, each from that dataset's rows alone: what
        make_interleaved_dataset returns as all_dataset_statistics and --dataset_statistics_file would hold."""
        return self._stats

    def mixture_info(self) -> dict:
        """Names, probabilities, quotas, the period, and the reference's dataset_len (rlds/dataset.py:512-522): the draws until every
        primary dataset - weight == 1.0 - has completed an epoch; None when no weight is 1.0 (the reference fails there)."""
        primary = [t / p for t, p, w in zip(self.transitions, self.p.tolist(), self.weights) if w == 1.0]
        return dict(datasets=list(self.names), weights=list(self.weights), balance_weights=self.balance_weights, p=self.p.tolist(),
                    quota=list(self.quota), period=self.Q, num_transitions=list(self.transitions), windows=list(self.windows),
                    dataset_len=int(max(primary)) if primary else None)

    # ---- the batch -----------------------------------------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        if B not in self._out:
            dev, e = self.device, torch.empty
            self._out[B] = dict(dataset_index=e(B, dtype=torch.int32, device=dev), ep=e(B, dtype=torch.int32, device=dev),
                                row=e(B, dtype=torch.int64, device=dev),
                                frames_u8=e((B,) + self.frame_shape, dtype=torch.uint8, device=dev),
                                actions_raw=e(B, self.chunk, self.A, dtype=torch.float32, device=dev),
                                proprio_raw=e(B, self.Pd, dtype=torch.float32, device=dev),
                                prompt_flat=e(B * self.Pmax, dtype=torch.int64, device=dev),
                                prompt_off=e(B + 1, dtype=torch.int32, device=dev))
        return self._out[B]

    def sample_indices(self, B: int, seed: int, rank: int, world: int, step: int):
        """vla_mixture_sample into the mix's buffers of batch size B -> (ds int32 [B], ep int32 [B], row int64 [B], prompt_off int32 [B + 1])."""
        from . import ops
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"sample: the batch size must lie in [1, {MAX_BATCH}] (one workgroup draws the batch), got {B}")
        if not (world >= 1 and 0 <= rank < world and step >= 0):
            raise ValueError(f"sample: need 0 <= rank < world and step >= 0, got rank {rank}, world {world}, step {step}")
        check_position(B, rank, world, step)
        o = self._buffers(B)
        ops.mixture_sample(self.valid_off, self.episode_off, self.prompt_off, self.dataset_off, self.quota_off, seed, rank, world, step, self.Pmax,
                           o["dataset_index"], o["ep"], o["row"], o["prompt_off"])
        return o["dataset_index"], o["ep"], o["row"], o["prompt_off"]

    def sample(self, B: int, seed: int, rank: int = 0, world: int = 1, step: int = 0) -> dict:
        """The raw batch of (rank, step): RAW_BATCH_KEYS on the device plus dataset_index int32 [B] (which dataset each sample came
        from) and dataset_names.  Every rank passes the same seed.  The tensors are the mix's own buffers of this batch size: the next
        call with the same B overwrites them (in stream order), so consume - collate - a batch before drawing the next, or clone it."""
        from . import ops
        _, ep, row, off = self.sample_indices(B, seed, rank, world, step)
        o = self._buffers(B)
        ops.episode_gather(self.frames_u8, self.actions_raw, self.proprio_raw, self.episode_off, self.prompt_flat, self.prompt_off, ep, row, off,
                           o["frames_u8"], o["actions_raw"], o["proprio_raw"], o["prompt_flat"], self.Pmax)
        out = {k: o[k] for k in RAW_BATCH_KEYS}
        out["dataset_index"] = o["dataset_index"]
        out["dataset_names"] = self.names
        return out
