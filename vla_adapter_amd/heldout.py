"""Validation on held-out episodes of a device-resident store: what the reference gets from its RLDS ``val`` split
(rlds/dataset.py:234-236) and ``run_validation`` (vla-scripts/finetune.py:605-685).

``EpisodeStore(..., holdout=f)`` / ``EpisodeMix(..., holdout=f)`` set every dataset's last episodes aside (episodes.py: the training
table counts no window of theirs, ``val_off`` is the complementary table).  ``HeldOutSweep`` walks the held-out windows in order - window
0, stride, 2 stride, ... below ``Nv``, shared out over the ranks batch by batch - with two kernels of its own (csrc/heldout.hip,
include/vla_heldout.h) around the existing ones: ``vla_heldout_sweep`` names the windows of a batch and which of them exist,
``vla_episode_gather`` and ``GPUInputStage.collate`` build the batch (never augmented, every row with its own dataset's statistics), the
existing validation forward predicts, and ``vla_heldout_l1_accumulate`` adds the valid rows' |pred - target| to f64 sums per dataset and
cell.  No host work per batch: nothing is read back until the sweep ends, the host waits on an event every ``SYNC_EVERY`` batches only
to honour --val_time_limit.  One sweep is one finite pass and reports exact sample-weighted means (the reference averages batch means
over an endless shuffled stream until its time limit: DESIGN.md section 16).

Both kernels' rules are stated here in plain Python and numpy - ``sweep_windows``, ``l1_accumulate_reference`` - and are the
specification the kernels are tested against, bit for bit.
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .batches import batch_stats, input_stage
from .episodes import MAX_BATCH, locate     # one workgroup names the batch, as one draws a training batch
from .validation import ValidationFeed, validation_noise

HELDOUT_STREAM = 0x4E1D0075EE9A1        # the sweep's seed word for the collator's filler ids: apart from the training batches' under equal seeds
SYNC_EVERY = 8                          # batches between two host waits (the --val_time_limit check): the overshoot is at most this many


# ---------------------------------------------------------------------------------------------------------------- the two rules
def sweep_windows(val_off, dataset_off, B: int, rank: int, world: int, j: int, stride: int = 1) -> List[Tuple[int, int, int, int]]:
    """The (valid, dataset, global episode, step inside it) of every sample of validation batch j of ``rank``: what vla_heldout_sweep
    computes.  Sample b is window w = ((j world + rank) B + b) stride of the held-out set; it is valid while w < Nv = val_off[-1], an
    invalid one takes window 0.  dataset_off: int [D + 1] episode ranges of the datasets, or None (one dataset: 0)."""
    Nv = int(val_off[-1])
    out = []
    for b in range(B):
        w = ((j * world + rank) * B + b) * stride
        ok = w < Nv
        e, t = locate(w if ok else 0, val_off)
        d = 0
        if dataset_off is not None:
            d = max(x for x in range(len(dataset_off) - 1) if x == 0 or int(dataset_off[x]) <= e)
        out.append((int(ok), d, e, t))
    return out


def sweep_batches(Nv: int, stride: int, B: int, rank: int, world: int) -> int:
    """How many batches of B the sweep of ``rank`` runs: the ceil(Nv / stride) visited windows fill ceil(. / B) batches, dealt to the
    ranks in turn (batch j of rank r is global batch j world + r); a batch without a valid sample is not run."""
    samples = -(-Nv // stride)
    batches = -(-samples // B)
    return max(0, -(-(batches - rank) // world))


def l1_accumulate_reference(pred: np.ndarray, target: np.ndarray, ds, valid, D: int, acc: np.ndarray, cnt: np.ndarray):
    """What vla_heldout_l1_accumulate adds, -> (acc + S, cnt + n) as new arrays.  pred / target: float32 [B, C, A] holding the bf16
    values; ds int [B] or None; valid [B]; acc float64 [D, C, A]; cnt int64 [D].  Per dataset d, S starts at 0.0 and takes the rows
    with valid != 0 and clamp(ds, 0, D - 1) == d in ascending order: S += float64(|float32(pred) - float32(target)|), then ONE add
    into acc.  A row with valid == 0 is never read."""
    pred, target = np.asarray(pred, dtype=np.float32), np.asarray(target, dtype=np.float32)
    acc, cnt = np.array(acc, dtype=np.float64), np.array(cnt, dtype=np.int64)
    for d in range(D):
        S = np.zeros(pred.shape[1:], dtype=np.float64)
        for b in range(pred.shape[0]):
            db = 0 if ds is None else min(max(int(ds[b]), 0), D - 1)
            if int(valid[b]) != 0 and db == d:
                S = S + np.abs(pred[b] - target[b]).astype(np.float64)       # the difference and |.| in f32, the sum in f64
                cnt[d] += 1
        acc[d] = acc[d] + S
    return acc, cnt


# ---------------------------------------------------------------------------------------------------------------- the report
def _raw_scale(action_stats: Optional[dict], A: int) -> List[float]:
    """Per action column: the factor from normalised to raw units, (q99 - q01 + 1e-8) / 2 where the dataset's mask normalises the
    column (no mask: every column), else 1 - the slope of what vla_unnormalize_actions applies."""
    if action_stats is None:
        return [1.0] * A
    mask = action_stats.get("mask", [True] * A)
    return [(float(action_stats["q99"][a]) - float(action_stats["q01"][a]) + 1e-8) / 2 if mask[a] else 1.0 for a in range(A)]


def _means(acc: np.ndarray, n: int) -> dict:
    """The sample-weighted means of one f64 sum table [C, A] over n samples; None where nothing was counted.  next_actions_l1_loss
    at C == 1 is 0.0, as vla_l1_loss has it."""
    C, A = acc.shape
    if n < 1:
        return dict(loss_value=None, loss=None, curr_action_l1_loss=None, next_actions_l1_loss=None, val_samples_count=0,
                    l1_by_chunk_step=[None] * C, l1_by_action_dim=[None] * A)
    loss = float(acc.sum()) / (n * C * A)
    return dict(loss_value=loss, loss=loss, curr_action_l1_loss=float(acc[0].sum()) / (n * A),
                next_actions_l1_loss=float(acc[1:].sum()) / (n * (C - 1) * A) if C > 1 else 0.0, val_samples_count=int(n),
                l1_by_chunk_step=[float(acc[c].sum()) / (n * A) for c in range(C)],
                l1_by_action_dim=[float(acc[:, a].sum()) / (n * C) for a in range(A)])


def report(acc, cnt, names: Sequence[str], action_stats: Optional[Sequence[Optional[dict]]], step: int, batches: int,
           windows: Sequence[int]) -> dict:
    """One sweep's entry from its sums: acc f64 [D, C, A], cnt int64 [D] (over all ranks), the datasets' names, their statistics'
    "action" entries (for l1_by_action_dim_raw; None: no scaling), the held-out windows per dataset.  Every mean is exact over the
    counted samples: sum / (count C A) for loss_value (= loss), chunk step 0 for curr_action_l1_loss, chunk steps >= 1 for
    next_actions_l1_loss; the overall line sums the datasets' tables, i.e. weighs every dataset by its count."""
    acc, cnt = np.asarray(acc, dtype=np.float64), np.asarray(cnt, dtype=np.int64)
    D, C, A = acc.shape
    total = acc[0].copy()
    for d in range(1, D):
        total = total + acc[d]
    out = dict(step=int(step))
    out.update(_means(total, int(cnt.sum())))
    out["val_batches_count"] = int(batches)
    out["val_windows_total"] = int(sum(windows))
    per = {}
    for d, name in enumerate(names):
        m = _means(acc[d], int(cnt[d]))
        m["val_windows_total"] = int(windows[d])
        scale = _raw_scale(action_stats[d] if action_stats is not None else None, A)
        m["l1_by_action_dim_raw"] = [None if v is None else v * s for v, s in zip(m["l1_by_action_dim"], scale)]
        per[name] = m
    out["per_dataset"] = per
    return out


def all_reduce_sums(acc: torch.Tensor, cnt: torch.Tensor, group=None, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sweep's ONE collective: the element-wise sum over the ranks of acc (f64) and cnt (int64), host tensors in and out.  Both
    travel in one f64 vector (a count is exact there below 2^53), staged through the host under gloo and through ``device`` otherwise.
    Every rank calls it once per sweep whether or not its time limit cut the sweep short."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return acc, cnt
    t = torch.cat([acc.reshape(-1).to(torch.float64), cnt.to(torch.float64)])
    if dist.get_backend(group) != "gloo":
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    t = t.cpu()
    return t[:acc.numel()].view(acc.shape), t[acc.numel():].round().to(torch.int64)


# ---------------------------------------------------------------------------------------------------------------- the sweep
class HeldOutSweep:
    """``sweep(log_step)`` -> the entry ``report`` builds, from one ordered pass over the held-out windows of ``store`` (an EpisodeStore
    or EpisodeMix built with holdout=) at the training batch size.  ``model``: the engine or a trainer (val_forward / val_step_graphed,
    val_pred); ``static``: the captured step's batch (its shapes are enforced); ``norm_stats``: the dataset statistics the training
    batches are normalised with.  The sweep owns its index, raw-batch, noise and sum buffers: the store's ``_out[B]`` buffers hold the
    next training batch at the same B and are not touched.  With use_graph the model's captured validation graphs hold the addresses
    of the first static batch they were replayed on: one sweeper (or ValidationPass) per model, or hand the same ``static`` buffers on
    (``sweeper.feed.static``)."""

    def __init__(self, cfg, mcfg, dev: str, rank: int, world: int, model, store, norm_stats: dict, static: dict, L: int,
                 use_graph: bool, group=None):
        if getattr(store, "val_off", None) is None:
            raise ValueError("HeldOutSweep: the store holds nothing out (build it with holdout=f)")
        B = int(cfg.batch_size)
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"HeldOutSweep: the batch size must lie in [1, {MAX_BATCH}] (one workgroup names the batch), got {B}")
        self.stride = int(getattr(cfg, "val_window_stride", 1) or 1)
        if self.stride < 1:
            raise ValueError("--val_window_stride must be >= 1")
        self.cfg, self.mcfg, self.dev, self.rank, self.world, self.model, self.store = cfg, mcfg, dev, int(rank), int(world), model, store
        self.B, self.L, self.group = B, int(L), group
        self.mixed, self.names, self.D = store.mixed, tuple(store.names), store.D
        self.C, self.A = int(mcfg.chunk), int(mcfg.action_dim)
        # per-dataset entries in the order ds indexes them; a single store's collate takes its one entry bare (no stats_index)
        self.action_stats, self.proprio_stats = batch_stats(norm_stats, self.names, self.mixed)
        self.windows = [store.heldout[n]["heldout_windows"] for n in self.names]
        self.Nv = int(store.Nv)
        self.n_batches = sweep_batches(self.Nv, self.stride, B, self.rank, self.world)
        self.feed = ValidationFeed(model, static, use_graph, "held-out")
        self.stage = input_stage(cfg, mcfg, dev)
        self.training_phase = cfg.phase == "Training"
        e = torch.empty
        self.idx = dict(ds=e(B, dtype=torch.int32, device=dev), ep=e(B, dtype=torch.int32, device=dev), row=e(B, dtype=torch.int64, device=dev),
                        prompt_off=e(B + 1, dtype=torch.int32, device=dev), valid=e(B, dtype=torch.uint8, device=dev))
        self.raw = dict(frames_u8=e((B,) + store.frame_shape, dtype=torch.uint8, device=dev),
                        actions_raw=e(B, store.chunk, store.A, dtype=torch.float32, device=dev),
                        proprio_raw=e(B, store.Pd, dtype=torch.float32, device=dev), prompt_flat=e(B * store.Pmax, dtype=torch.int64, device=dev))
        # acc f64 [D, C, A] and cnt int64 [D] are two views of one buffer: one copy reads both back when the sweep ends
        n = self.D * self.C * self.A
        self.sums = torch.zeros(n + self.D, dtype=torch.float64, device=dev)
        self.acc, self.cnt = self.sums[:n].view(self.D, self.C, self.A), self.sums[n:].view(torch.int64)
        self.sums_host = torch.empty(n + self.D, dtype=torch.float64).pin_memory()
        self.noise, self.noise_host, self.event = None, None, torch.cuda.Event()
        self.batches_run = 0

    # ---- one batch -------------------------------------------------------------------------------------------------------------
    def draw(self, j: int) -> dict:
        """Validation batch j of this rank as the raw-batch dict (the sweep's own buffers) plus ds / valid: two launches."""
        from . import ops
        s, i, r = self.store, self.idx, self.raw
        ops.heldout_sweep(s.val_off, s.episode_off, s.prompt_off, s.dataset_off if self.mixed else None, self.rank, self.world, j, self.stride,
                          s.Pmax, i["ds"], i["ep"], i["row"], i["prompt_off"], i["valid"])
        return dict(s.gather(i["ep"], i["row"], i["prompt_off"], r), dataset_index=i["ds"], valid=i["valid"])

    def collate(self, raw: dict, j: int) -> dict:
        """The model's batch of a drawn raw batch: never augmented, every row normalised with its own dataset's statistics, filler ids
        keyed by (seed ^ HELDOUT_STREAM, rank, j); the captured step's shapes are enforced."""
        b = self.stage.collate(raw["frames_u8"], (raw["prompt_flat"], raw["prompt_off"]), raw["actions_raw"], raw["proprio_raw"],
                               action_stats=self.action_stats, proprio_stats=self.proprio_stats, L=self.L,
                               seed=(int(self.cfg.seed) ^ HELDOUT_STREAM) & (2 ** 64 - 1), rank=self.rank, step=j, augment=None,
                               stats_index=raw["dataset_index"] if self.mixed else None)
        return self.feed.enforce(b)

    def _noise(self, log_step: int, j: int) -> Optional[torch.Tensor]:
        """validation.validation_noise of batch j, keyed by the batch's place in the whole sweep (global batch j world + rank, rank word 0):
        a batch's perturbation belongs to its windows, not to the rank that happens to run it, so a sweep gives the same sums on any
        number of ranks.  It goes through a ring of SYNC_EVERY pinned host buffers: the copy is asynchronous, and slot j % SYNC_EVERY
        is rewritten only behind the host wait that follows batch j."""
        if not self.training_phase:
            return None
        nz = validation_noise(self.cfg, self.mcfg, 0, log_step, j * self.world + self.rank)
        if self.noise is None:
            self.noise = torch.empty(nz.shape, device=self.dev, dtype=nz.dtype)
            self.noise_host = [torch.empty(nz.shape, dtype=nz.dtype).pin_memory() for _ in range(SYNC_EVERY)]
        slot = self.noise_host[j % SYNC_EVERY]
        slot.copy_(nz)
        self.noise.copy_(slot, non_blocking=True)
        return self.noise

    def step(self, log_step: int, j: int) -> None:
        """Batch j of the sweep at log_step: name the windows, gather, collate, forward, accumulate - device work only."""
        from . import ops
        model = self.model
        raw = self.draw(j)
        b = self.collate(raw, j)
        noise = self._noise(log_step, j)
        target = self.feed.forward(b, noise)[1]["actions"]
        to_bf16 = getattr(model, "eng", model)._to_bf16
        ops.heldout_l1_accumulate(model.val_pred.contiguous(), to_bf16(target), raw["dataset_index"] if self.mixed else None, raw["valid"], self.acc, self.cnt)

    # ---- the sweep -------------------------------------------------------------------------------------------------------------
    def launch(self, log_step: int) -> int:
        """Every batch of this rank's sweep, enqueued; the host waits on an event behind every SYNC_EVERY-th batch and stops there once
        --val_time_limit seconds have passed.  -> the batches run.  Nothing is read back."""
        t0 = time.time()
        self.model.begin_validation()
        self.sums.zero_()
        n = 0
        for j in range(self.n_batches):
            self.step(log_step, j)
            n += 1
            if n % SYNC_EVERY == 0 and n < self.n_batches:
                self.event.record()
                self.event.synchronize()
                if time.time() - t0 > self.cfg.val_time_limit:
                    break
        self.model.end_validation()
        self.batches_run = n
        return n

    def finish(self, log_step: int) -> dict:
        """The sweep's one read-back (acc and cnt in one copy), its one all-reduce on more than one rank, and the entry."""
        self.sums_host.copy_(self.sums, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        n = self.D * self.C * self.A
        acc, cnt = self.sums_host[:n].clone().view(self.D, self.C, self.A), self.sums_host[n:].clone().view(torch.int64)
        batches = torch.tensor([self.batches_run], dtype=torch.int64)
        acc, cnt = all_reduce_sums(acc, torch.cat([cnt, batches]), self.group, self.dev)
        stats = self.action_stats if self.mixed else (self.action_stats,)
        return report(acc.numpy(), cnt[:-1].numpy(), self.names, stats, log_step, int(cnt[-1]), self.windows)

    def sweep(self, log_step: int) -> dict:
        self.launch(log_step)
        return self.finish(log_step)

    def info(self) -> dict:
        """What info["heldout"] records: per dataset the held-out episode range and the window counts, and the sweep's geometry."""
        return dict(fraction=self.store.holdout, stride=self.stride, datasets={n: dict(self.store.heldout[n]) for n in self.names},
                    windows=self.Nv, samples=-(-self.Nv // self.stride), batches_per_rank=self.n_batches)
