"""The validation pass of the fine-tune driver (--use_val_set): when it is due, its head noise, what the file-fed ``ValidationPass``
and the device-resident ``heldout.HeldOutSweep`` share (``ValidationFeed``: the captured step's shape contract, the static batch of the
captured validation graph, the graph / eager dispatch), and ``ValidationPass`` itself."""
from __future__ import annotations

import os
import time

import torch

from .batches import check_frames, input_stage, pad_to, pt_files


def validation_due(cfg, item) -> bool:
    """Does the validation pass run behind this loop_plan item?  The reference: ``log_step > 0 and log_step % val_freq == 0``
    after the optimizer step and the checkpoint save (finetune.py:1101), on EVERY micro-batch of such a gradient step.  Here
    once per gradient step, as for the checkpoint: behind the optimizer step that completes it - or behind the last micro-batch
    of the run, where the reference breaks before that optimizer step (loop_plan)."""
    _, _, log_step, boundary, _, last = item
    return bool(cfg.use_val_set) and (boundary or last) and log_step > 0 and log_step % cfg.val_freq == 0


def validation_noise(cfg, mcfg, rank: int, log_step: int, j: int) -> torch.Tensor:
    """The head's N(0, 0.02^2) input perturbation (action_heads.py:64-72) of validation batch j of the sweep at log_step, phase
    "Training": bf16 [chunk, action_dim * D] on the host, from a generator of its own keyed by (seed, rank, log_step, j) - the
    training stream's draws do not depend on whether (or how long) validation ran.  (The reference draws both from torch's
    global generator.)"""
    key = (((int(cfg.seed) * 1_000_003 + int(rank)) * 1_000_033 + int(log_step)) * 10_007 + int(j)) % (2 ** 63 - 1)
    g = torch.Generator().manual_seed(key)
    return (torch.randn(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, generator=g) * 0.02).to(torch.bfloat16)


class ValidationFeed:
    """What both validators do with a batch once it is built: hold it to the captured training step's shapes, and run the model's
    validation forward on it - captured (the batch copied into one static batch, whose addresses the validation graphs keep) or eager.
    ``what`` names the batch in the refusals ("validation" / "held-out")."""

    def __init__(self, model, static: dict, use_graph: bool, what: str):
        self.model, self.use_graph, self.what = model, bool(use_graph), what
        self.shapes = {k: (tuple(v.shape), v.dtype) for k, v in static.items()}   # the captured step's batch: shape contract
        self.static = None

    def enforce(self, b: dict, cast: bool = False) -> dict:
        """The training batch's keys of ``b``, each of the training step's shape (``cast``: and dtype)."""
        out = {}
        for k, (shape, dt) in self.shapes.items():
            if k not in b:
                raise ValueError(f"{self.what} batch without {k!r} (the training batches carry {sorted(self.shapes)})")
            if tuple(b[k].shape) != shape:
                raise ValueError(f"{self.what} batch {k!r} of shape {tuple(b[k].shape)}: the training step's is {shape}")
            out[k] = b[k].to(dt) if cast and b[k].dtype != dt else b[k]
        return out

    def forward(self, b: dict, noise):
        """-> (the three L1 values on the device, the batch the model was fed: the static one under use_graph)."""
        if not self.use_graph:
            return self.model.val_forward(b, noise), b
        if self.static is None:
            self.static = {k: b[k].clone() if b[k].dtype == dt else b[k].to(dt) for k, (_, dt) in self.shapes.items()}
        else:
            for k in self.static:
                self.static[k].copy_(b[k])
        return self.model.val_step_graphed(self.static, noise), self.static


class ValidationPass:
    """The reference's run_validation (finetune.py:605-685) on held-out batches: eval mode (no LoRA dropout, no image
    augmentation), no gradient; per batch the three L1 values of run_forward_pass, each averaged over the batches of the sweep
    as the reference does (sum / count of Python floats).  A sweep is ONE pass over the source from this rank's own offset,
    ended early behind the first batch at which --val_time_limit seconds have passed; a finite source is not cycled to fill the
    time limit (the reference's RLDS val iterator repeats for ever: the same batches would count twice).  No collective: every
    rank validates on its own, as every rank of the reference does."""

    def __init__(self, cfg, mcfg, dev: str, rank: int, model, static: dict, L: int, pad_id: int, use_graph: bool, val_batches=None):
        self.cfg, self.mcfg, self.dev, self.rank, self.model, self.L, self.pad_id = cfg, mcfg, dev, rank, model, L, pad_id
        self.feed = ValidationFeed(model, static, use_graph, "validation")
        if val_batches is not None:
            self.items, self.files = list(val_batches), None
            if not self.items:
                raise ValueError("empty validation batch iterable")
        else:
            src = cfg.val_batch_file
            self.files = pt_files(src)
            if not self.files or not os.path.isfile(self.files[0]):
                raise FileNotFoundError(f"no .pt validation batch files under {src}")
            self.items = None
        self.stage, self.noise = None, None
        self.training_phase = cfg.phase == "Training"

    def _order(self):
        n = len(self.items if self.items is not None else self.files)
        o = self.rank % n
        for i in list(range(o, n)) + list(range(o)):
            yield self.items[i] if self.items is not None else torch.load(self.files[i], weights_only=True)

    def prepare(self, b: dict) -> dict:
        """Host collate of one validation batch: frames -> plain normalised pixels, right-padding to the captured length, the
        training batch's shapes enforced."""
        b = {k: v.to(self.dev) for k, v in b.items()}
        if "frames_u8" in b:
            fr = check_frames(b.pop("frames_u8"))
            if self.stage is None:
                self.stage = input_stage(self.cfg, self.mcfg, self.dev)
            b["pixel_values"] = self.stage.pixels(fr)              # never augmented (rlds/dataset.py:412: train=False)
        B = self.feed.shapes["input_ids"][0][0]
        if b["input_ids"].shape[0] != B:
            raise ValueError(f"validation batch of {b['input_ids'].shape[0]} samples: the validation pass runs at the training batch size "
                             f"({B}, --batch_size)")
        return self.feed.enforce(pad_to(b, self.L, self.pad_id), cast=True)

    def sweep(self, log_step: int) -> dict:
        model, t0 = self.model, time.time()
        model.begin_validation()
        values = []
        for j, b in enumerate(self._order()):
            b = self.prepare(b)
            noise = None
            if self.training_phase:
                nz = validation_noise(self.cfg, self.mcfg, self.rank, log_step, j)
                if self.noise is None:
                    self.noise = torch.empty(nz.shape, device=self.dev, dtype=nz.dtype)
                self.noise.copy_(nz)
                noise = self.noise
            loss3, _ = self.feed.forward(b, noise)
            values.append(loss3.tolist())              # host sync on this batch's completion (the reference's .item())
            if time.time() - t0 > self.cfg.val_time_limit:
                break
        model.end_validation()
        n = len(values)
        mean = [sum(v[i] for v in values) / n for i in range(3)]
        return dict(step=log_step, loss_value=mean[0], loss=mean[0], curr_action_l1_loss=mean[1], next_actions_l1_loss=mean[2],
                    val_batches_count=n)
