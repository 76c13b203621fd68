"""Device-resident demonstration episodes: the part of the reference's batch producer that decides WHICH transitions form a batch.

The reference's RLDS stage cuts every episode into windows of one observation plus ``NUM_ACTIONS_CHUNK - 1`` future actions
(``chunk_act_obs``, prismatic/vla/datasets/rlds/traj_transforms.py:14-57, configured in prismatic/vla/datasets/datasets.py:183-189),
shuffles all windows of the dataset, and computes the q01 / q99 statistics both training and ``predict_action`` need
(``get_dataset_statistics``, rlds/utils/data_utils.py:176-262).  ``EpisodeStore`` loads the episodes once, keeps them on the device
and draws each step's batch with two kernels (csrc/episodes.hip, include/vla_episodes.h): ``vla_episode_sample`` picks the windows -
shuffled, every window exactly once per epoch across all ranks and steps - and ``vla_episode_gather`` copies them into the raw-batch
dict ``GPUInputStage.collate`` consumes.  No host work per step: nothing is read back, synchronised or, after the first call,
allocated.

An episode file is a ``.pt`` dict, or a directory of them (the shards are concatenated in sorted order):

  frames_u8     uint8   [T, n_img, H, W, 3]   all episodes back to back
  actions_raw   float32 [T, A]
  proprio_raw   float32 [T, Pd]
  episode_off   int64   [E + 1]               row offsets of the episodes
  prompt_flat   int64   [n]                   one tokenised prompt per episode (the instruction is constant within an episode)
  prompt_off    int32   [E + 1]
  dataset_name  str, optional
  action_mask   bool    [A], optional         the reference's action_normalization_mask

In place of ``frames_u8`` a file may carry its frames as JPEG files - ``frames_jpeg``, ``frame_off``, ``frame_shape`` (jpeg_store.py) -
which ``gather`` then decodes on the device, batch by batch, into the same ``frames_u8`` buffer; a dict carries
exactly one of the two forms, and the shards of a dataset and the datasets of a mix all the same one.

The sampling rule is stated here in plain Python - ``sample_position``, ``permute_index``, ``locate`` - and is the specification the
kernel is tested against, bit for bit.

``EpisodeTables`` is what the store shares with ``mixture.EpisodeMix``: the tables on the device, the window tables, the statistics,
the raw-batch buffers and the gather.

``holdout=f`` sets every dataset's last episodes aside for validation without copying or reordering anything - ``holdout_count``,
``split_offsets``: two complementary window tables - and ``heldout.HeldOutSweep`` walks them.
"""
from __future__ import annotations

import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .constants import NUM_ACTIONS_CHUNK
from .batches import RAW_BATCH_KEYS                 # what sample() returns: the raw batch batches.batch_stream collates
from .jpeg_store import JPEG_KEYS, STATUS_TEXT, JpegFrames, check_jpeg_shard, concat_jpeg, storage_form

EPISODE_KEYS = ("frames_u8", "actions_raw", "proprio_raw", "episode_off", "prompt_flat", "prompt_off")
EPISODE_STREAM = 0xE9150DE5A391E        # csrc/windows.h: keeps the shuffle apart from the augmentation's and the collator's draws
MAX_BATCH = 1024                        # vla_episode_sample, vla_mixture_sample and vla_heldout_sweep are one workgroup each
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- the sampling rule
def splitmix64_key(seed: int, idx: int) -> int:
    """csrc/common.h: splitmix64 finaliser of (seed + idx * golden ratio), in 64-bit wrap-around arithmetic."""
    z = (seed + idx * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_position(B: int, rank: int, world: int, step: int, b: int) -> int:
    """Where sample b of the batch of (rank, step) stands in the endless sequence of draws: the ranks' batches of one step are
    consecutive, so positions [k N, (k + 1) N) - epoch k - are shared out over all ranks and steps without gap or overlap."""
    return (step * world + rank) * B + b


def check_position(B: int, rank: int, world: int, step: int) -> None:
    """ValueError when the position of the batch's last sample does not fit 63 bits: the kernels form it in 64-bit wrap-around
    arithmetic, this rule in Python integers, and the two part ways there (the entry points refuse the same arguments)."""
    last = sample_position(B, rank, world, step, B - 1)
    if last > 2 ** 63 - 1:
        raise ValueError(f"sample: the stream position overflows 63 bits (rank {rank}, world {world}, step {step}, batch size {B}: the "
                         f"last sample stands at {last})")


def epoch_key(seed: int, epoch: int) -> int:
    return splitmix64_key((seed & _M64) ^ EPISODE_STREAM, epoch)


def _feistel4(x: int, key: int, half: int) -> int:
    """Four rounds (L, R) -> (R, L ^ F(R)) over two halves of ``half`` bits: a bijection on [0, 4^half) whatever F is, since every
    round is undone by (L, R) -> (R ^ F(L), L)."""
    mask = (1 << half) - 1
    l, r = x >> half, x & mask
    for rnd in range(4):
        l, r = r, l ^ (splitmix64_key(splitmix64_key(key, rnd), r) & mask)
    return (l << half) | r


def permute_index(i: int, N: int, key: int) -> int:
    """A keyed bijection on [0, N): a balanced Feistel network over 2 * ceil(bits(N - 1) / 2) bits, results >= N walked on along
    their cycle (cycle-walking).  It needs no table of N entries, so every sample of every rank computes its own index.

    Termination: i lies inside [0, N); the walk follows the cycle through i of a permutation of the domain [0, 4^half), so it comes
    back to i - an element of [0, N) - after at most 4^half steps, and stops at the first element below N it meets.  The domain is
    smaller than 4 N (N > 2^(bits - 1) and 2 * half <= bits + 1), so a walk takes fewer than four passes on average."""
    if not 0 <= i < N:
        raise ValueError(f"permute_index: i = {i} outside [0, {N})")
    if N == 1:
        return 0
    half = max(((N - 1).bit_length() + 1) // 2, 1)
    y = _feistel4(i, key, half)
    while y >= N:
        y = _feistel4(y, key, half)
    return y


def locate(j: int, valid_off) -> Tuple[int, int]:
    """Window j of the dataset -> (episode, step inside it): the episode with valid_off[e] <= j < valid_off[e + 1], by the kernel's
    binary search (the largest e below E with valid_off[e] <= j: episodes without a window are stepped over)."""
    lo, hi = 0, len(valid_off) - 2
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if int(valid_off[mid]) <= j:
            lo = mid
        else:
            hi = mid - 1
    return lo, j - int(valid_off[lo])


def sample_windows(valid_off, B: int, seed: int, rank: int, world: int, step: int) -> List[Tuple[int, int]]:
    """The (episode, step inside it) of every sample of the batch of (rank, step): what vla_episode_sample computes."""
    N = int(valid_off[-1])
    out = []
    for b in range(B):
        pos = sample_position(B, rank, world, step, b)
        out.append(locate(permute_index(pos % N, N, epoch_key(seed, pos // N)), valid_off))
    return out


def window_rows(row: int, episode_end: int, chunk: int) -> List[int]:
    """The action rows of the window that starts at global row ``row`` of an episode ending at ``episode_end`` (exclusive):
    chunk_act_obs' minimum(index, goal_timestep) - it cannot bind for a start the sampler chose."""
    return [min(row + k, episode_end - 1) for k in range(chunk)]


# ---------------------------------------------------------------------------------------------------------------- statistics
def dataset_statistics(actions: np.ndarray, proprio: np.ndarray, num_trajectories: int, action_mask=None) -> dict:
    """get_dataset_statistics (rlds/utils/data_utils.py:231-256) on the float32 arrays, written as the reference writes it."""
    def part(x):
        return {"mean": x.mean(0).tolist(), "std": x.std(0).tolist(), "max": x.max(0).tolist(), "min": x.min(0).tolist(),
                "q01": np.quantile(x, 0.01, axis=0).tolist(), "q99": np.quantile(x, 0.99, axis=0).tolist()}
    meta = {"action": part(actions), "proprio": part(proprio), "num_transitions": int(actions.shape[0]),
            "num_trajectories": int(num_trajectories)}
    if action_mask is not None:
        meta["action"]["mask"] = [bool(m) for m in np.asarray(action_mask).tolist()]
    return meta


# ---------------------------------------------------------------------------------------------------------------- the store
def _check_shard(d: dict, where: str) -> None:
    """ValueError naming the key for every table that does not fit the others."""
    if not isinstance(d, dict):
        raise ValueError(f"{where}: an episode file is a dict of {EPISODE_KEYS}")
    jpeg = storage_form(d, where) == "jpeg"             # (ValueError for both forms in one dict; neither: frames_u8 is missing, below)
    for k in EPISODE_KEYS[1:] if jpeg else EPISODE_KEYS:
        if k not in d or not isinstance(d[k], torch.Tensor):
            raise ValueError(f"{where}: {k} is missing (an episode file carries {EPISODE_KEYS}, or {JPEG_KEYS} in place of frames_u8)")
    act, pr, eo, pf, po = (d[k] for k in EPISODE_KEYS[1:])
    if jpeg:
        T = act.shape[0] if act.dim() == 2 else 0
        check_jpeg_shard(d, T, where)
    else:
        fr = d["frames_u8"]
        if fr.dtype != torch.uint8 or fr.dim() != 5 or fr.shape[-1] != 3 or fr.shape[0] < 1:
            raise ValueError(f"{where}: frames_u8 must be uint8 [T, n_img, H, W, 3] with T >= 1, got {fr.dtype} {tuple(fr.shape)}")
        T = fr.shape[0]
    if act.dtype != torch.float32 or act.dim() != 2 or act.shape[0] != T or act.shape[1] < 1:
        raise ValueError(f"{where}: actions_raw must be float32 [T = {T}, A], got {act.dtype} {tuple(act.shape)}")
    if pr.dtype != torch.float32 or pr.dim() != 2 or pr.shape[0] != T or pr.shape[1] < 1:
        raise ValueError(f"{where}: proprio_raw must be float32 [T = {T}, Pd], got {pr.dtype} {tuple(pr.shape)}")
    if eo.dtype != torch.int64 or eo.dim() != 1 or eo.numel() < 2:
        raise ValueError(f"{where}: episode_off must be int64 [E + 1] with E >= 1, got {eo.dtype} {tuple(eo.shape)}")
    E = eo.numel() - 1
    if int(eo[0]) != 0 or int(eo[-1]) != T or bool((eo.diff() < 0).any()):
        raise ValueError(f"{where}: episode_off must rise from 0 to T = {T} without a step back, got {eo.tolist()[:8]} ... {int(eo[-1])}")
    if pf.dtype != torch.int64 or pf.dim() != 1:
        raise ValueError(f"{where}: prompt_flat must be int64 [n], got {pf.dtype} {tuple(pf.shape)}")
    if po.dtype != torch.int32 or po.dim() != 1 or po.numel() != E + 1:
        raise ValueError(f"{where}: prompt_off must be int32 [E + 1 = {E + 1}] (one prompt per episode), got {po.dtype} {tuple(po.shape)}")
    if int(po[0]) != 0 or int(po[-1]) != pf.numel() or bool((po.diff() < 0).any()):
        raise ValueError(f"{where}: prompt_off must rise from 0 to len(prompt_flat) = {pf.numel()} without a step back")
    if "action_mask" in d:
        m = torch.as_tensor(d["action_mask"])
        if m.dtype != torch.bool or tuple(m.shape) != (act.shape[1],):
            raise ValueError(f"{where}: action_mask must be bool [A = {act.shape[1]}], got {m.dtype} {tuple(m.shape)}")
    if "dataset_name" in d and not isinstance(d["dataset_name"], str):
        raise ValueError(f"{where}: dataset_name must be a str")


def check_one_form(tables: Sequence[dict], names: Sequence[str]) -> bool:
    """True when every one of the tables keeps its frames as JPEG files, False when every one keeps raw pixels; ValueError naming
    the first that differs from the first (shards of a dataset, datasets of a mix: mixed storage is not supported)."""
    forms = [storage_form(d, n) for d, n in zip(tables, names)]
    for f, n in zip(forms[1:], names[1:]):
        if f != forms[0]:
            raise ValueError(f"{n}: stores its frames as {f}, {names[0]} as {forms[0]}: one run keeps all its frames in one form "
                             f"(frames_u8, or {JPEG_KEYS})")
    return forms[0] == "jpeg"


def valid_offsets(episode_off: torch.Tensor, chunk: int) -> torch.Tensor:
    """int64 [E + 1]: prefix sum of max(len_e - (chunk - 1), 0), the windows each episode yields (traj_transforms.py:27:
    effective_traj_len = traj_len - future_action_window_size; an episode shorter than the chunk yields none)."""
    n = (episode_off.diff() - (chunk - 1)).clamp_(min=0)
    return torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])


# ---------------------------------------------------------------------------------------------------------------- the held-out split
def holdout_count(E: int, f: float) -> int:
    """How many of a dataset's E episodes - its LAST ones - a hold-out fraction f sets aside: min(E - 1, max(1, floor(f E + 0.5)))."""
    return min(E - 1, max(1, int(math.floor(f * E + 0.5))))


def check_holdout(f, E: int, name: str) -> int:
    """H for dataset ``name``; ValueError naming it for a fraction outside (0, 1) or a dataset of fewer than 2 episodes."""
    if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 < float(f) < 1.0:         # (NaN fails the comparison too)
        raise ValueError(f"{name}: holdout must be a fraction inside (0, 1), got {f!r}")
    if E < 2:
        raise ValueError(f"{name}: holdout needs at least 2 episodes (one to train on, one to hold out), the dataset has {E}")
    return holdout_count(E, float(f))


def split_offsets(episode_off: torch.Tensor, chunk: int, held: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(training valid_off, val_off), both int64 [E + 1]: the prefix sums of the windows each episode yields (valid_offsets) in which
    the held-out episodes (held bool [E]) / the training episodes contribute 0.  Nothing is copied or reordered: the samplers step over
    an episode without windows, so the training samplers never draw a held-out episode and the sweep never a training one."""
    n = (episode_off.diff() - (chunk - 1)).clamp_(min=0)
    zero = torch.zeros(1, dtype=torch.int64)
    return (torch.cat([zero, torch.where(held, 0, n).cumsum(0)]), torch.cat([zero, torch.where(held, n, 0).cumsum(0)]))


def check_split(train_off, val_off, e_lo: int, e_hi: int, H: int, chunk: int, name: str) -> dict:
    """The split of dataset ``name`` (episodes [e_lo, e_hi), the last H held out) as info["heldout"] records it; ValueError naming the
    dataset when either side is left without a window."""
    n_train, n_val = int(train_off[e_hi]) - int(train_off[e_lo]), int(val_off[e_hi]) - int(val_off[e_lo])
    if n_train < 1:
        raise ValueError(f"{name}: holdout leaves no training window - every one of the {e_hi - e_lo - H} training episodes is shorter than "
                         f"the action chunk of {chunk} steps")
    if n_val < 1:
        raise ValueError(f"{name}: holdout leaves no held-out window - every one of the {H} held-out episodes (the last ones) is shorter "
                         f"than the action chunk of {chunk} steps")
    return dict(episodes=[e_hi - H, e_hi], num_episodes=H, train_windows=n_train, heldout_windows=n_val)


class EpisodeTables:
    """What a store and a mix have in common: D >= 1 datasets back to back in one set of tables on the device, the training window
    table ``valid_off`` (and, with ``holdout=f``, the complementary ``val_off``), the extents, the per-dataset statistics, the buffers
    of a raw batch and the one ``vla_episode_gather`` call site.  ``EpisodeStore`` (below) and ``mixture.EpisodeMix`` add what is
    their own: how the windows of a batch are drawn.

    ``tables``: one episode-file dict per dataset; ``names``: the datasets' names (statistics and hold-out entries are keyed by them);
    ``wheres``: what a ValueError about dataset d's tables calls them (default: its name).  ``jpeg_scan_index``: frames that are
    JPEG files without a restart marker per MCU row get a scan index at load (jpeg_store.JpegFrames.build_scan_index) - the same
    pixels, decoded a row per work item; nothing changes for raw frames."""

    mixed = False                           # a mix: the raw batch carries dataset_index, every sample its own dataset's statistics

    def __init__(self, tables: List[dict], names: Sequence[str], device, chunk: int = NUM_ACTIONS_CHUNK, *, holdout: Optional[float] = None,
                 wheres: Optional[Sequence[str]] = None, jpeg_scan_index: bool = False):
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        wheres = list(wheres or names)
        for d, w in zip(tables, wheres):
            _check_shard(d, w)
        check_one_form(tables, wheres)
        self.device, self.chunk, self.names, self.D = device, int(chunk), tuple(names), len(tables)
        self.action_masks = [torch.as_tensor(d["action_mask"]).tolist() if "action_mask" in d else None for d in tables]
        ranges, self._stats = [0], {}                  # dataset d holds the episodes [ranges[d], ranges[d + 1])
        for d, n, w, mask in zip(tables, self.names, wheres, self.action_masks):
            E_d = int(d["episode_off"].numel() - 1)
            if int(valid_offsets(d["episode_off"].cpu(), self.chunk)[-1]) < 1:
                raise ValueError(f"{w}: no valid window - every one of the {E_d} episodes is shorter than the action chunk of {self.chunk} "
                                 "steps (episode_off)")
            ranges.append(ranges[-1] + E_d)
            self._stats[n] = dataset_statistics(d["actions_raw"].cpu().numpy(), d["proprio_raw"].cpu().numpy(), E_d, mask)
        self.episode_ranges = ranges
        # one set of tables: the datasets' rows and episodes back to back (names and masks are kept per dataset, above)
        all_ = tables[0]
        if self.D > 1:
            all_ = concat_shards([{k: v for k, v in d.items() if k not in ("dataset_name", "action_mask")} for d in tables], wheres, device)
        act, pr, eo, po = all_["actions_raw"], all_["proprio_raw"], all_["episode_off"], all_["prompt_off"]
        self.T, self.E = int(act.shape[0]), int(eo.numel() - 1)
        # holdout=f: every dataset sets its own last H_d episodes aside.  The statistics (and a mix's transitions, p and quotas) stay
        # over ALL episodes - the reference balances and normalises over split="all" (rlds/dataset.py:209-211)
        valid, val = valid_offsets(eo.cpu(), self.chunk), None
        self.holdout, self.heldout = holdout, None
        if holdout is not None:
            counts = [check_holdout(holdout, ranges[d + 1] - ranges[d], n) for d, n in enumerate(self.names)]
            held = torch.zeros(self.E, dtype=torch.bool)
            for d, H in enumerate(counts):
                held[ranges[d + 1] - H:ranges[d + 1]] = True
            valid, val = split_offsets(eo.cpu(), self.chunk, held)
            self.heldout = {n: check_split(valid, val, ranges[d], ranges[d + 1], counts[d], self.chunk, n) for d, n in enumerate(self.names)}
        self.N = int(valid[-1])
        self.Nv = int(val[-1]) if val is not None else 0
        self.A, self.Pd = int(act.shape[1]), int(pr.shape[1])
        # the frames: raw pixels (frames_u8), or JPEG files that gather() decodes (jpeg: their bytes and tables on the device)
        self.jpeg = JpegFrames(all_, device, wheres[0] if self.D == 1 else "episode mix") if "frames_jpeg" in all_ else None
        if self.jpeg and jpeg_scan_index:
            self.jpeg.build_scan_index()
        self.frame_shape = (self.jpeg.n_img, self.jpeg.H, self.jpeg.W, 3) if self.jpeg else tuple(all_["frames_u8"].shape[1:])
        self.row_bytes = int(np.prod(self.frame_shape))
        self.Pmax = int(po.diff().max())
        self.valid_off_host, self.val_off_host = valid, val
        self.frames_u8 = None if self.jpeg else self._upload(all_["frames_u8"])
        self.actions_raw, self.proprio_raw = self._upload(act), self._upload(pr)
        self.episode_off, self.valid_off = self._upload(eo), self._upload(valid)
        self.val_off = self._upload(val) if val is not None else None
        self.prompt_flat, self.prompt_off = self._upload(all_["prompt_flat"]), self._upload(po)
        self._out: Dict[int, dict] = {}
        self._no_frames, self.decode_status = None, None   # (JPEG: the gather's zero-length frame table; the last batch's status)

    def _upload(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(self.device).contiguous()

    def statistics(self) -> dict:
        """One reference-shaped get_dataset_statistics entry per dataset, keyed by its name and taken from that dataset's rows alone:
        what make_interleaved_dataset returns as all_dataset_statistics and --dataset_statistics_file would hold."""
        return self._stats

    # ---- the batch -----------------------------------------------------------------------------------------------------------
    def _buffers(self, B: int) -> dict:
        if B not in self._out:
            dev, e = self.device, torch.empty
            o = dict(ep=e(B, dtype=torch.int32, device=dev), row=e(B, dtype=torch.int64, device=dev),
                     frames_u8=e((B,) + self.frame_shape, dtype=torch.uint8, device=dev),
                     actions_raw=e(B, self.chunk, self.A, dtype=torch.float32, device=dev),
                     proprio_raw=e(B, self.Pd, dtype=torch.float32, device=dev),
                     prompt_flat=e(B * self.Pmax, dtype=torch.int64, device=dev), prompt_off=e(B + 1, dtype=torch.int32, device=dev))
            if self.mixed:
                o["dataset_index"] = e(B, dtype=torch.int32, device=dev)
            if self.jpeg:                   # the decode's workspace and status of this batch size (gather takes them from there: the
                self.jpeg.buffers(B)        # held-out sweep gathers into buffers of its own)
            self._out[B] = o
        return self._out[B]

    def _check_draw(self, B: int, rank: int, world: int, step: int) -> None:
        """ValueError for a (B, rank, world, step) the samplers' entry points refuse."""
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"sample: the batch size must lie in [1, {MAX_BATCH}] (one workgroup draws the batch), got {B}")
        if not (world >= 1 and 0 <= rank < world and step >= 0):
            raise ValueError(f"sample: need 0 <= rank < world and step >= 0, got rank {rank}, world {world}, step {step}")
        check_position(B, rank, world, step)

    def gather(self, ep: torch.Tensor, row: torch.Tensor, prompt_off: torch.Tensor, into: dict) -> dict:
        """vla_episode_gather of the windows (ep, row, prompt_off) - a sampler's or the held-out sweep's - into the frames_u8 /
        actions_raw / proprio_raw / prompt_flat of ``into``; -> the raw batch, RAW_BATCH_KEYS on the device."""
        from . import ops
        if self.jpeg:                       # actions, proprio and prompts by the same gather over zero-length frame rows, then the frames
            if self._no_frames is None:
                self._no_frames = torch.empty(self.T, 0, dtype=torch.uint8, device=self.device)
            buf = self.jpeg.buffers(int(ep.numel()))
            frames, out_frames = self._no_frames, buf["no_frames"]
        else:
            frames, out_frames = self.frames_u8, into["frames_u8"]
        ops.episode_gather(frames, self.actions_raw, self.proprio_raw, self.episode_off, self.prompt_flat, self.prompt_off, ep, row,
                           prompt_off, out_frames, into["actions_raw"], into["proprio_raw"], into["prompt_flat"], self.Pmax)
        if self.jpeg:
            self.decode_status = self.jpeg.decode(self.episode_off, self.T, ep, row, into["frames_u8"], buf)
        return {k: prompt_off if k == "prompt_off" else into[k] for k in RAW_BATCH_KEYS}

    def bad_segments(self) -> torch.Tensor:
        """f32 [1] on the device: how many segments of the last gathered batch did not decode (no read-back here).  In a store with
        a scan index a segment is a piece, and this counts pieces."""
        return (self.decode_status != 0).sum().to(torch.float32).view(1)

    def verify_frames(self, batch: int = 64) -> int:
        """Decode every frame of a JPEG store once, ``batch`` steps at a time, and raise a ValueError that names the first frame with a
        segment that did not decode (one read-back, behind the last batch); -> the number of frames decoded.  0 for a raw store.
        In a store with a scan index the segment it names is the piece: pieces in front of a damaged one decode, those behind it
        report that they ran out of bytes."""
        if not self.jpeg:
            return 0
        j, dev = self.jpeg, self.device
        rows = torch.arange(self.T, dtype=torch.int64, device=dev)
        eps = (torch.bucketize(rows, self.episode_off, right=True) - 1).clamp_(0, self.E - 1).to(torch.int32)
        B = min(int(batch), self.T)
        buf = j.buffers(B)
        frames = torch.empty((B,) + self.frame_shape, dtype=torch.uint8, device=dev)
        first = torch.full((1,), self.T * j.n_img * j.max_seg, dtype=torch.int64, device=dev)       # smallest (frame, segment) with a status
        code = torch.zeros(1, dtype=torch.uint8, device=dev)
        for t0 in range(0, self.T, B):
            t0 = min(t0, self.T - B)                                                                # (the last batch overlaps the one before)
            st = j.decode(self.episode_off, self.T, eps[t0:t0 + B], rows[t0:t0 + B], frames, buf).view(-1)
            bad = st != 0
            idx = torch.where(bad, torch.arange(st.numel(), device=dev) + t0 * j.n_img * j.max_seg, first).min().view(1)
            hit = idx < first
            code = torch.where(hit, st[(idx - t0 * j.n_img * j.max_seg).clamp(0, st.numel() - 1)], code)
            first = torch.minimum(first, idx)
        at, c = int(first), int(code)                                                               # the one read-back
        if at < self.T * j.n_img * j.max_seg:
            frame, seg = divmod(at, j.max_seg)
            raise ValueError(f"verify_frames: frame {frame} (step {frame // j.n_img}, image {frame % j.n_img}), segment {seg}: "
                             f"{STATUS_TEXT.get(c, f'status {c}')}")
        return self.T * j.n_img


class EpisodeStore(EpisodeTables):
    """Episodes on the device; ``sample()`` draws one raw batch.  Build with ``EpisodeStore.load`` or ``EpisodeStore.from_dict``.

    ``holdout=f`` (0 < f < 1) sets the last ``holdout_count(E, f)`` episodes aside for validation (heldout.HeldOutSweep): the training
    table ``valid_off`` then counts no window of theirs - ``sample()`` never draws them, ``N`` is the number of training windows - and
    ``val_off`` / ``Nv`` are the complementary table and count.  ``statistics()`` stays over ALL episodes, as the reference takes them
    over split="all" (rlds/dataset.py:209-211): the split changes no dataset_statistics.json.  ``holdout=None``: every table and every
    batch is what it is without the argument."""

    def __init__(self, tables: dict, device, chunk: int = NUM_ACTIONS_CHUNK, dataset_name: Optional[str] = None, _where: str = "episode store",
                 *, holdout: Optional[float] = None, jpeg_scan_index: bool = False):
        name = (tables.get("dataset_name") if isinstance(tables, dict) else None) or dataset_name or "episodes"
        super().__init__([tables], [name], device, chunk, holdout=holdout, wheres=[_where], jpeg_scan_index=jpeg_scan_index)
        self.dataset_name, self.action_mask = self.names[0], self.action_masks[0]

    # ---- construction --------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dict(cls, tables: dict, device, chunk: int = NUM_ACTIONS_CHUNK, dataset_name: Optional[str] = None, *,
                  holdout: Optional[float] = None, jpeg_scan_index: bool = False) -> "EpisodeStore":
        return cls(tables, device, chunk, dataset_name, holdout=holdout, jpeg_scan_index=jpeg_scan_index)

    @classmethod
    def load(cls, path, device, chunk: int = NUM_ACTIONS_CHUNK, dataset_name: Optional[str] = None, *,
             holdout: Optional[float] = None, jpeg_scan_index: bool = False, jpeg_quality: Optional[int] = None) -> "EpisodeStore":
        """``path``: a .pt episode file or a directory of them (concatenated in sorted order).  Validates the tables (ValueError that
        names the key), moves everything to the device and builds valid_off; ``dataset_name``: used when the file names none;
        ``holdout``: the fraction of episodes - the last ones - set aside for validation (see the class); ``jpeg_scan_index``: JPEG
        frames get a scan index (EpisodeTables); ``jpeg_quality``: raw frames are coded on the device, shard by shard, into the JPEG
        form at that quality (jpeg_store.encode_tables: LOSSY, and the store tools/pack_episodes_jpeg.py would have written); nothing
        to do for a file already in the JPEG form."""
        return cls(load_tables(path, device, jpeg_quality=jpeg_quality), device, chunk, dataset_name, _where=str(path), holdout=holdout, jpeg_scan_index=jpeg_scan_index)

    # ---- the batch -----------------------------------------------------------------------------------------------------------
    def sample_indices(self, B: int, seed: int, rank: int, world: int, step: int):
        """vla_episode_sample into the store's buffers of batch size B -> (ep int32 [B], row int64 [B], prompt_off int32 [B + 1])."""
        from . import ops
        self._check_draw(B, rank, world, step)
        o = self._buffers(B)
        ops.episode_sample(self.valid_off, self.episode_off, self.prompt_off, seed, rank, world, step, self.Pmax, o["ep"], o["row"], o["prompt_off"])
        return o["ep"], o["row"], o["prompt_off"]

    def sample(self, B: int, seed: int, rank: int = 0, world: int = 1, step: int = 0) -> dict:
        """The raw batch of (rank, step): RAW_BATCH_KEYS on the device plus dataset_name, from the two kernels.  Every rank passes the
        same seed.  The tensors are the store's own buffers of this batch size: the next call with the same B overwrites them (in
        stream order), so consume - collate - a batch before drawing the next, or clone it."""
        out = self.gather(*self.sample_indices(B, seed, rank, world, step), self._buffers(B))
        out["dataset_name"] = self.dataset_name
        return out


def load_tables(path, device="cpu", jpeg_quality: Optional[int] = None) -> dict:
    """The tables of a .pt episode file or of a directory of them (validated shard by shard, concatenated in sorted order).
    ``jpeg_quality``: see concat_shards."""
    path = str(path)
    files = sorted(str(p) for p in Path(path).glob("*.pt")) if os.path.isdir(path) else [path]
    if not files:
        raise FileNotFoundError(f"no .pt episode files under {path}")
    shards = []
    for f in files:
        d = torch.load(f, weights_only=True, mmap=True)
        _check_shard(d, f)
        shards.append(d)
    return concat_shards(shards, files, device, jpeg_quality=jpeg_quality)


def concat_shards(shards: List[dict], names: Optional[List[str]] = None, device="cpu", jpeg_quality: Optional[int] = None) -> dict:
    """The shards' tables back to back: rows concatenated, both offset tables shifted; dataset_name / action_mask must agree.  The
    frames are assembled on ``device`` shard by shard (the host never holds a second copy of them).  ``jpeg_quality``: every shard
    of raw frames is first coded on ``device`` into the JPEG form (jpeg_store.encode_tables; ValueError naming the shard for sides that
    are no multiples of 16); shards already in that form stay as they are."""
    names = names or [f"shard {i}" for i in range(len(shards))]
    if jpeg_quality is not None:
        from .jpeg_store import encode_tables
        shards = [encode_tables(d, device, jpeg_quality, where=n) for d, n in zip(shards, names)]
    first = shards[0]
    jpeg = check_one_form(shards, names)
    for d, n in zip(shards[1:], names[1:]):
        for k in ("actions_raw", "proprio_raw") if jpeg else ("frames_u8", "actions_raw", "proprio_raw"):
            if d[k].shape[1:] != first[k].shape[1:]:
                raise ValueError(f"{n}: {k} has rows of shape {tuple(d[k].shape[1:])}, {names[0]} of {tuple(first[k].shape[1:])}")
        if d.get("dataset_name") != first.get("dataset_name"):
            raise ValueError(f"{n}: dataset_name {d.get('dataset_name')!r} differs from {names[0]}'s {first.get('dataset_name')!r}")
        if ("action_mask" in d) != ("action_mask" in first) or ("action_mask" in d and not torch.equal(torch.as_tensor(d["action_mask"]), torch.as_tensor(first["action_mask"]))):
            raise ValueError(f"{n}: action_mask differs from {names[0]}'s")
    if len(shards) == 1:
        return first
    out = {k: torch.cat([d[k] for d in shards]) for k in ("actions_raw", "proprio_raw", "prompt_flat")}
    if jpeg:
        out.update(concat_jpeg(shards, names, device))
    else:
        out["frames_u8"] = torch.empty((out["actions_raw"].shape[0],) + tuple(first["frames_u8"].shape[1:]), dtype=torch.uint8, device=device)
    eo, po, t0, p0 = [first["episode_off"][:1]], [first["prompt_off"][:1].to(torch.int64)], 0, 0
    for d in shards:
        if not jpeg:
            out["frames_u8"][t0:t0 + d["frames_u8"].shape[0]].copy_(d["frames_u8"])
        eo.append(d["episode_off"][1:] + t0)
        po.append(d["prompt_off"][1:].to(torch.int64) + p0)
        t0 += d["actions_raw"].shape[0]
        p0 += d["prompt_flat"].numel()
    if p0 > 2 ** 31 - 1:
        raise ValueError(f"prompt_off: {p0} prompt ids in all do not fit its int32 offsets")
    out["episode_off"], out["prompt_off"] = torch.cat(eo), torch.cat(po).to(torch.int32)
    for k in ("dataset_name", "action_mask"):
        if k in first:
            out[k] = first[k]
    return out
