"""Native counterpart of vla-scripts/finetune.py for the accelerated path (adapter-only fine-tune).

Keeps the reference's flat ``FinetuneConfig`` (finetune.py:66-128) and its ``--flag value`` command line (draccus is
absent here: parsed with argparse from the dataclass fields), the per-step metric names (finetune.py:421-444), the LR
warm-up / MultiStepLR schedule (:903-921, 1061-1065) and the checkpoint file names (:527-572).  What is NOT here, on
purpose: HF-hub / network loaders (:752-754), the RLDS/TensorFlow input pipeline (out of scope) -
batches come from an iterable / ``--batch_file`` (a .pt dict or a directory of them: the collator's contract), from
``--frame_batch_file`` (the same with raw uint8 frames, augmented on the device under ``--image_aug``), from
``--raw_batch_file`` (raw transitions: frames, prompt ids, un-normalised actions / proprio, collated on the device with the
statistics of ``--dataset_statistics_file``), from ``--episode_file`` (demonstration episodes kept on the device: shuffled windows drawn and
chunked by two kernels, statistics computed at load - episodes.EpisodeStore), from ``--episode_mix`` (a weighted mixture of such
datasets, every sample normalised with its own dataset's statistics - mixture.EpisodeMix) or ``synthetic.make_batch``; weights are random-init unless ``--vlm_path`` / ``--resum_vla_path`` point at local state-dict
files.  ``--use_val_set`` runs the reference's validation pass (finetune.py:605-685, 1101-1117) on held-out batches of the same
form (``--val_batch_file`` / ``finetune(val_batches=...)``; ``ValidationPass``), or - with an episode source and
``--val_episode_fraction`` - on the episodes that fraction holds out of every dataset, swept on the device (``heldout.HeldOutSweep``); the
RLDS val split itself is not read.  Every reference flag is either honoured or refused with an error (``check_supported``); none is silently dropped.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import torch


@dataclass
class FinetuneConfig:
    # fmt: off
    config_file_path: str = "openvla/openvla-7b"
    vlm_path: str = "openvla/openvla-7b"
    use_minivlm: bool = False
    resum_vla_path: str = "openvla/openvla-7b"
    # Dataset
    data_root_dir: Path = Path("datasets/rlds")
    dataset_name: str = "aloha_scoop_x_into_bowl"
    run_root_dir: Path = Path("runs")
    shuffle_buffer_size: int = 100_000
    # Algorithm and architecture
    use_l1_regression: bool = True
    use_diffusion: bool = False
    num_diffusion_steps: int = 50
    use_film: bool = False
    num_images_in_input: int = 1
    use_proprio: bool = False
    phase1_path: str = "None"
    # Training configuration
    batch_size: int = 8
    learning_rate: float = 5e-4
    lr_warmup_steps: float = 0.1
    num_steps_before_decay: int = 100000
    grad_accumulation_steps: int = 1
    max_steps: int = 200000
    use_val_set: bool = False
    val_freq: int = 10_000
    val_time_limit: int = 180
    save_freq: int = 10_000
    save_latest_checkpoint_only: bool = False
    resume: bool = False
    resume_step: Optional[int] = None
    image_aug: bool = True
    diffusion_sample_freq: int = 50
    # LoRA
    use_lora: bool = False
    lora_rank: int = 32
    lora_dropout: float = 0.0
    merge_lora_during_training: bool = False
    # Full Finetune
    use_fz: bool = False
    # Logging
    wandb_entity: str = "your-wandb-entity"
    wandb_project: str = "your-wandb-project"
    run_id_note: Optional[str] = None
    run_id_override: Optional[str] = None
    wandb_log_freq: int = 10
    # revision version
    use_pro_version: bool = True
    phase: str = "Training"
    # native additions (not in the reference)
    tiny: bool = False                    # prismatic-tiny plumbing config (BASELINE configs[0])
    seed: int = 0
    batch_file: Optional[str] = None      # torch-saved dict with the collator's keys
    val_batch_file: Optional[str] = None  # --use_val_set: held-out batches (a .pt dict or a directory of them; pixel_values or frames_u8, never
                                          # augmented), one pass per validation sweep
    frame_batch_file: Optional[str] = None  # same, with raw frames: frames_u8 uint8 [B, n_img, H, W, 3] instead of pixel_values (the
                                          # input stage normalises them on the device, augmented under --image_aug)
    raw_batch_file: Optional[str] = None  # raw transitions (a .pt dict or a directory of them): frames_u8, prompt_flat int64 [n], prompt_off int32
                                          # [B + 1], actions_raw [B, chunk, action_dim], proprio_raw [B, Pd], optional dataset_name - normalised with
                                          # --dataset_statistics_file and collated on the device (GPUInputStage.collate), L = --max_seq_len
    episode_file: Optional[str] = None    # demonstration episodes (a .pt dict or a directory of them: episodes.py), loaded once and kept on the
                                          # device; every micro-step's raw batch is drawn there - shuffled, each window once per epoch across the
                                          # ranks, actions chunked as the reference's RLDS stage does - and collated like a --raw_batch_file batch
                                          # (needs --max_seq_len; without --dataset_statistics_file the store's own statistics are used and saved)
    episode_mix: Optional[str] = None     # a weighted mixture of episode datasets, "pathA=1.0,pathB=0.5" (a weight defaults to 1.0; each path as
                                          # --episode_file takes it): all kept on the device, every sample drawn from dataset d with probability
                                          # p_d and normalised with that dataset's own statistics, every dataset running through its own epochs
                                          # (mixture.EpisodeMix; needs --max_seq_len; without --dataset_statistics_file the mix's statistics are
                                          # used and saved, one entry per dataset)
    episode_mix_balance: bool = True      # the reference's balance_weights: p_d = w_d T_d / sum(w T) over the transition counts, else w_d / sum(w)
    val_episode_fraction: Optional[float] = None   # --use_val_set with --episode_file / --episode_mix: hold out this fraction of every dataset's
                                          # episodes (its last ones; never trained on) and sweep their windows on the device every --val_freq steps
                                          # (heldout.HeldOutSweep); the statistics stay over all episodes, as the reference's split="all"
    val_window_stride: int = 1            # the held-out sweep visits every k-th window (consecutive windows of an episode share 7 of 8 actions)
    use_graph: bool = True                # replay the captured hipGraphs
    max_seq_len: int = 0                  # static token length every batch is right-padded to (0: length of the first batch)
    conservative_rows: bool = False       # captured live-row window starts at the first text row instead of the first batch's action block
    dataset_statistics_file: Optional[str] = None   # JSON written next to every checkpoint (finetune.py:531)
    objective: str = "l1"                 # "l1": action head + L1 regression (the reference's finetune.py); "token_ce": the native VLM / VLA trainer's
                                          # token cross-entropy (base_strategy.py:257-417) - LoRA / full modes only, no action head in the loss
    fp8_base_weights: bool = False        # --use_lora: the frozen base weights' products (forward and dX) on OCP e4m3 operands, the rank-r branch in
                                          # bf16 inside the same accumulator (BASELINE configs[4] "fp8 MFMA weight path"; parity unpinned: the reference is bf16)
    ddp_algo: str = "allreduce"           # data-parallel exchange per gradient bucket: "allreduce", or "rs_ag" = reduce-scatter + all-gather
                                          # (every rank talks to every peer directly: all 7 xGMI links instead of a ring)
    sync_check_freq: int = 0              # > 0: every that many optimizer steps the ranks compare a checksum of their parameters (one 8-byte
                                          # all-reduce) and the run stops on a mismatch; 0 = off
    max_grad_norm: Optional[float] = None   # clip the global gradient norm in front of every optimizer step (torch's clip_grad_norm_, on the
                                          # device): the reference's native trainer uses 1.0 (prismatic/conf/vla.py:96), its L1 fine-tune script
                                          # does not clip - default off; inf: log grad_norm, clip nothing
    backbone: Optional[str] = None        # model geometry: a name of engine.NAMED_CONFIGS ("config2", "dinosiglip-0_5b", "config5",
                                          # "tiny", "tiny_fused") - default: inferred from the --vlm_path state dict, else "config2"
    save_train_state: bool = False        # next to every checkpoint also write train_state--{suffix} (train_state.py): optimizer moments and step
                                          # count, the position in the schedule and in the batch stream, generator / dropout / live-row state, the
                                          # digests of the flat buffers and a fingerprint of the flags that define the trajectory
    resume_train_state: bool = False      # with --resume: go on bit for bit where the checkpoint's run stood - the weights through the usual path,
                                          # verified against the recorded digests, everything else from the state file; plain --resume (the
                                          # reference's: weights only, everything else from zero) is unchanged
    log_state_digest: bool = False        # every logged step also carries state_digest: the 64-bit digests (ops.state_digest) of data, m and v of
                                          # every flat buffer as hex strings, read in the log line's own read-back
    verify_frames: bool = False           # --episode_file / --episode_mix whose frames are JPEG files (jpeg_store.py): decode every frame once at
                                          # load and refuse the run, naming the frame, when a scan does not decode (DESIGN.md section 18 has the cost)
    jpeg_scan_index: bool = False         # --episode_file / --episode_mix whose frames are JPEG files: walk every scan once at load and record
                                          # where each MCU row starts, so that files without restart markers decode a row per work item - the
                                          # same pixels, hence the same run; nothing to do for raw frames
    frame_resize: str = "bicubic"         # how frames that are not at the model's size get there (every GPUInputStage of the run): "bicubic", the
                                          # processor's Pillow resize, or "lanczos3", the RLDS stage's tf.image.resize(method="lanczos3",
                                          # antialias=True) (obs_transforms.py:75).  Frames at the model's size: no effect
    # fmt: on


def parse_args(argv=None) -> FinetuneConfig:
    ap = argparse.ArgumentParser(description="native VLA-Adapter fine-tune (same flags as the reference's FinetuneConfig)")
    for f in dataclasses.fields(FinetuneConfig):
        default = f.default
        t = type(default) if default is not None else str
        if t is bool:
            ap.add_argument(f"--{f.name}", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=default)
        elif t is type(Path(".")):
            ap.add_argument(f"--{f.name}", type=Path, default=default)
        else:
            ap.add_argument(f"--{f.name}", type=(int if f.name in ("resume_step",) else float if f.name in ("max_grad_norm", "val_episode_fraction") else t), default=default)
    ns = ap.parse_args(argv)
    cfg = FinetuneConfig(**vars(ns))
    import sys
    given = [a[2:].split("=")[0] for a in (sys.argv[1:] if argv is None else argv) if str(a).startswith("--")]
    cfg._explicit = tuple(given)          # flags the user passed: out-of-path ones are refused, not ignored (check_supported)
    return cfg


# Flags of the reference that only configure subsystems outside the accelerated path (RLDS/TensorFlow input pipeline,
# W&B, HF hub): the native entry point consumes pre-collated batches, so their DEFAULT values are inert - but a value the
# user passes explicitly cannot be honoured and is refused instead of ignored.  (--image_aug is honoured where batches carry
# raw frames, --frame_batch_file: check_supported / batch_stream; --val_freq / --val_time_limit under --use_val_set with a
# validation source: ValidationPass, or heldout.HeldOutSweep under --val_episode_fraction.)
OUT_OF_PATH_FLAGS = ("data_root_dir", "shuffle_buffer_size", "wandb_entity", "wandb_project", "run_id_note",
                     "config_file_path", "phase1_path", "num_diffusion_steps", "diffusion_sample_freq", "val_freq", "val_time_limit",
                     "use_minivlm")


def train_mode(cfg: FinetuneConfig) -> str:
    """Which parameters train.  Reference: use_lora -> peft adapters on every Linear of the VLM + action_queries + head
    (finetune.py:832-844); otherwise EVERY VLM parameter keeps requires_grad (:846-849) - ``use_fz`` only renames the run there
    (:183-184), freezing the VLM is its evident intent and what BASELINE configs[1] ("adapter-only") means: implemented."""
    return "lora" if cfg.use_lora else ("adapter" if cfg.use_fz else "full")


IMAGE_AUG_REFUSAL = ("--image_aug: already normalised pixel_values cannot be augmented; pass raw uint8 frames (frames_u8) with "
                     "--frame_batch_file, or in the batches handed to finetune()")


VAL_FLAGS = ("val_freq", "val_time_limit")
EPISODE_FLAGS = ("episode_file", "episode_mix")     # the two device-resident batch sources: what either needs is stated once


def check_supported(cfg: FinetuneConfig, explicit=(), frame_batches: bool = False, val_batches: bool = False) -> None:
    """Raise for every reference option this path does not implement (nothing is parsed and silently dropped).
    ``frame_batches``: finetune() was handed a batch iterable, which may carry raw frames (--image_aug is then checked per batch).
    ``val_batches``: finetune() was handed a validation batch iterable (a validation source besides --val_batch_file)."""
    if cfg.grad_accumulation_steps < 1:
        raise ValueError("grad_accumulation_steps must be >= 1")
    if cfg.use_lora and not 0.0 <= cfg.lora_dropout < 1.0:
        raise ValueError("--lora_dropout must lie in [0, 1)")
    if cfg.use_lora and cfg.lora_dropout > 0.0 and cfg.fp8_base_weights:
        raise NotImplementedError("--lora_dropout > 0 together with --fp8_base_weights: the dropped inputs are bf16 (use one or the other)")
    if cfg.fp8_base_weights and not cfg.use_lora:
        raise NotImplementedError("--fp8_base_weights needs --use_lora True (frozen base weights); the adapter-only forward has engine.enable_fp8_frozen()")
    if cfg.max_grad_norm is not None and not float(cfg.max_grad_norm) > 0.0:      # (NaN fails the comparison too)
        raise ValueError(f"--max_grad_norm must be > 0 (inf: log the norm, clip nothing), got {cfg.max_grad_norm}")
    if cfg.ddp_algo not in ("allreduce", "rs_ag"):
        raise ValueError("--ddp_algo is allreduce or rs_ag")
    if cfg.objective not in ("l1", "token_ce"):
        raise ValueError("--objective is l1 or token_ce")
    if cfg.frame_resize not in ("bicubic", "lanczos3"):
        raise ValueError(f"--frame_resize is bicubic or lanczos3, got {cfg.frame_resize!r}")
    if cfg.objective == "token_ce" and train_mode(cfg) == "adapter":
        raise NotImplementedError("--objective token_ce trains the VLM (LoRA or full fine-tune); --use_fz True freezes it")
    if cfg.backbone is not None:
        from .engine import NAMED_CONFIGS
        if cfg.backbone not in NAMED_CONFIGS:
            raise ValueError(f"--backbone {cfg.backbone!r}: known geometries are {sorted(NAMED_CONFIGS)}")
    if cfg.use_film or cfg.use_diffusion or not cfg.use_l1_regression:
        raise NotImplementedError("native path = L1-regression action head; --use_film / --use_diffusion are not built")
    validating = False
    heldout = cfg.val_episode_fraction is not None
    if heldout:
        if not cfg.use_val_set:
            raise ValueError("--val_episode_fraction without --use_val_set True would hold episodes out and never validate on them: pass both")
        if cfg.val_batch_file or val_batches:
            raise ValueError("--val_episode_fraction and --val_batch_file / val_batches are two validation sources: pass one")
        if not (cfg.episode_file or cfg.episode_mix):
            raise ValueError("--val_episode_fraction holds episodes out of --episode_file / --episode_mix: no other batch source has episodes")
        if not 0.0 < float(cfg.val_episode_fraction) < 1.0:            # (NaN fails the comparison too)
            raise ValueError(f"--val_episode_fraction must lie inside (0, 1), got {cfg.val_episode_fraction}")
        if cfg.val_window_stride < 1:
            raise ValueError("--val_window_stride must be >= 1")
    if cfg.use_val_set:
        for flag in EPISODE_FLAGS:
            if getattr(cfg, flag) and not (cfg.val_batch_file or val_batches or heldout):
                raise NotImplementedError(f"--use_val_set with --{flag}: no validation split is cut from the episodes (ValidationPass takes "
                                          "collated batches); pass held-out batches with --val_batch_file.  Or hold a fraction of the "
                                          "episodes out with --val_episode_fraction.")
        if not (cfg.val_batch_file or val_batches or heldout):
            raise NotImplementedError("--use_val_set needs held-out batches: pass --val_batch_file (a .pt dict or a directory of them) or "
                                      "finetune(val_batches=...); the RLDS val split is not read (out of scope, SURVEY section 2 #16)")
        if cfg.objective != "l1":
            raise NotImplementedError("--use_val_set with --objective token_ce: the reference validates the L1 action head only")
        if cfg.val_freq < 1:
            raise ValueError("--val_freq must be >= 1")
        validating = True
    elif cfg.val_batch_file or val_batches:
        raise ValueError("a validation source (--val_batch_file / val_batches) without --use_val_set True would be ignored: pass both")
    if not cfg.use_proprio:
        # the reference passes proprio_projector=None into predict_action, which calls it (action_heads.py:54): TypeError
        raise TypeError("use_proprio=False: 'NoneType' object is not callable (the reference's predict_action requires the "
                        "proprio projector, action_heads.py:53-55); pass --use_proprio True as every reference launch script does")
    if cfg.grad_accumulation_steps < 1:
        raise ValueError("grad_accumulation_steps must be >= 1")
    if cfg.resume_train_state and not cfg.resume:
        raise ValueError("--resume_train_state without --resume: the state continues the run of a checkpoint - pass --resume True, "
                         "--resume_step and --resum_vla_path")
    if cfg.resume and cfg.resume_step is None:
        raise ValueError("--resume needs --resume_step (finetune.py:1056 computes log_step = resume_step + gradient_step_idx)")
    sources = [n for n in ("batch_file", "frame_batch_file", "raw_batch_file", "episode_file", "episode_mix") if getattr(cfg, n)]
    if len(sources) > 1:
        raise ValueError(" and ".join("--" + n for n in sources) + f" are {len(sources)} batch sources: pass one")
    if cfg.raw_batch_file and not cfg.dataset_statistics_file:
        raise ValueError("--raw_batch_file carries un-normalised actions / proprio: pass the statistics with --dataset_statistics_file")
    for flag in EPISODE_FLAGS:
        if getattr(cfg, flag) and not cfg.max_seq_len:
            raise ValueError("raw batches with prompt offsets on the device need --max_seq_len (the natural length would be read back): "
                             f"--{flag} draws its prompt offsets on the device")
        if getattr(cfg, flag) and not 1 <= cfg.batch_size <= 1024:
            raise ValueError(f"--{flag} draws a batch in one workgroup: --batch_size must lie in [1, 1024]")
    if cfg.episode_mix:
        from .mixture import parse_mix
        parse_mix(cfg.episode_mix)                # ValueError for a weight that is no number or an entry without a path
    frames = bool(cfg.frame_batch_file or cfg.raw_batch_file or cfg.episode_file or cfg.episode_mix) or frame_batches
    if "image_aug" in explicit and not frames:
        raise NotImplementedError(IMAGE_AUG_REFUSAL)
    bad = [n for n in explicit if n in OUT_OF_PATH_FLAGS and not (validating and n in VAL_FLAGS)]
    if bad:
        raise NotImplementedError(f"flags {bad} configure parts of the reference outside the accelerated path (input pipeline / "
                                  "logging services / hub loaders): the native entry point takes pre-collated batches "
                                  "(--batch_file) and cannot honour them")


def lr_at(gradient_step_idx: int, cfg: FinetuneConfig) -> float:
    """Learning rate the optimizer step of gradient step g runs with (finetune.py:917, 1061-1065, 1078-1082).
    lr_warmup_steps > 0 (the default 0.1): the warm-up block overwrites param_group['lr'] with
    original_lr * (0.1 + 0.9 * min((g + 1) / warmup, 1)) on EVERY iteration before optimizer.step(), which also undoes the
    MultiStepLR decay applied after the previous step - the decay never takes effect.  lr_warmup_steps <= 0: plain
    MultiStepLR, factor 0.1 from optimizer step num_steps_before_decay on."""
    if cfg.lr_warmup_steps > 0:
        return cfg.learning_rate * (0.1 + 0.9 * min((gradient_step_idx + 1) / cfg.lr_warmup_steps, 1.0))
    return cfg.learning_rate * (0.1 if gradient_step_idx >= cfg.num_steps_before_decay else 1.0)


def loop_plan(cfg: FinetuneConfig, start=None):
    """The reference loop's bookkeeping (finetune.py:1018-1122) as a generator of
    (batch_idx, gradient_step_idx, log_step, optimizer_step?, save?, last?) - one item per micro-batch.  The reference breaks
    behind the FIRST micro-batch whose log_step == max_steps (:1119-1121): with grad_accumulation_steps == 1 that batch's
    optimizer step has run (max_steps + 1 gradient steps from a fresh start); with ga > 1 it is the first micro-batch of gradient
    step max_steps - its forward / backward run, its gradients are never applied (boundary False).  A checkpoint is due when
    gradient_step_idx > 0 and log_step % save_freq == 0 (the reference re-saves on every micro-batch of such a step; here once,
    behind the optimizer step that completes it).
    ``start`` = (first micro-step, log-step base) of --resume_train_state (train_state.resumed_position): the plan is the tail of the
    plan of the run it continues - batch_idx, gradient_step_idx (so lr_at) and log_step all go on where that run's next item stood."""
    ga = cfg.grad_accumulation_steps
    base = cfg.resume_step if cfg.resume else 0
    batch_idx = 0
    if start is not None:
        batch_idx, base = int(start[0]), int(start[1])
    while True:
        g = batch_idx // ga
        log_step = base + g
        boundary = (batch_idx + 1) % ga == 0
        save = boundary and g > 0 and log_step % cfg.save_freq == 0
        last = log_step >= cfg.max_steps
        yield batch_idx, g, log_step, boundary, save, last
        if last:
            return
        batch_idx += 1


def validation_due(cfg: FinetuneConfig, item) -> bool:
    """Does the validation pass run behind this loop_plan item?  The reference: ``log_step > 0 and log_step % val_freq == 0``
    after the optimizer step and the checkpoint save (finetune.py:1101), on EVERY micro-batch of such a gradient step.  Here
    once per gradient step, as for the checkpoint: behind the optimizer step that completes it - or behind the last micro-batch
    of the run, where the reference breaks before that optimizer step (loop_plan)."""
    _, _, log_step, boundary, _, last = item
    return bool(cfg.use_val_set) and (boundary or last) and log_step > 0 and log_step % cfg.val_freq == 0


def validation_noise(cfg: FinetuneConfig, mcfg, rank: int, log_step: int, j: int) -> torch.Tensor:
    """The head's N(0, 0.02^2) input perturbation (action_heads.py:64-72) of validation batch j of the sweep at log_step, phase
    "Training": bf16 [chunk, action_dim * D] on the host, from a generator of its own keyed by (seed, rank, log_step, j) - the
    training stream's draws do not depend on whether (or how long) validation ran.  (The reference draws both from torch's
    global generator.)"""
    key = (((int(cfg.seed) * 1_000_003 + int(rank)) * 1_000_033 + int(log_step)) * 10_007 + int(j)) % (2 ** 63 - 1)
    g = torch.Generator().manual_seed(key)
    return (torch.randn(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, generator=g) * 0.02).to(torch.bfloat16)


class ValidationPass:
    """The reference's run_validation (finetune.py:605-685) on held-out batches: eval mode (no LoRA dropout, no image
    augmentation), no gradient; per batch the three L1 values of run_forward_pass, each averaged over the batches of the sweep
    as the reference does (sum / count of Python floats).  A sweep is ONE pass over the source from this rank's own offset,
    ended early behind the first batch at which --val_time_limit seconds have passed; a finite source is not cycled to fill the
    time limit (the reference's RLDS val iterator repeats for ever: the same batches would count twice).  No collective: every
    rank validates on its own, as every rank of the reference does."""

    def __init__(self, cfg: FinetuneConfig, mcfg, dev: str, rank: int, model, static: dict, L: int, pad_id: int, use_graph: bool,
                 val_batches=None):
        self.cfg, self.mcfg, self.dev, self.rank, self.model, self.L, self.pad_id = cfg, mcfg, dev, rank, model, L, pad_id
        self.use_graph = use_graph
        self.shapes = {k: (tuple(v.shape), v.dtype) for k, v in static.items()}   # the captured step's batch: shape contract
        if val_batches is not None:
            self.items, self.files = list(val_batches), None
            if not self.items:
                raise ValueError("empty validation batch iterable")
        else:
            src = cfg.val_batch_file
            self.files = sorted(str(p) for p in Path(src).glob("*.pt")) if os.path.isdir(src) else [src]
            if not self.files or not os.path.isfile(self.files[0]):
                raise FileNotFoundError(f"no .pt validation batch files under {src}")
            self.items = None
        self.stage, self.static, self.noise = None, None, None
        self.training_phase = cfg.phase == "Training"

    def _order(self):
        n = len(self.items if self.items is not None else self.files)
        o = self.rank % n
        for i in list(range(o, n)) + list(range(o)):
            yield self.items[i] if self.items is not None else torch.load(self.files[i], weights_only=True)

    def prepare(self, b: dict) -> dict:
        """Host collate of one validation batch: frames -> plain normalised pixels, right-padding to the captured length, the
        training batch's shapes enforced."""
        from .input_stage import GPUInputStage, backbone_norms
        b = {k: v.to(self.dev) for k, v in b.items()}
        if "frames_u8" in b:
            fr = b.pop("frames_u8")
            if fr.dtype != torch.uint8 or fr.dim() != 5 or fr.shape[-1] != 3:
                raise ValueError(f"frames_u8 must be uint8 [B, n_img, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
            if self.stage is None:
                self.stage = GPUInputStage(self.dev, backbones=backbone_norms(self.mcfg), image_size=self.mcfg.vit[0].img, resize=self.cfg.frame_resize)
            b["pixel_values"] = self.stage.pixels(fr)              # never augmented (rlds/dataset.py:412: train=False)
        B = self.shapes["input_ids"][0][0]
        if b["input_ids"].shape[0] != B:
            raise ValueError(f"validation batch of {b['input_ids'].shape[0]} samples: the validation pass runs at the training batch size "
                             f"({B}, --batch_size)")
        b = _pad_to(b, self.L, self.pad_id)
        out = {}
        for k, (shape, dt) in self.shapes.items():
            if k not in b:
                raise ValueError(f"validation batch without {k!r} (the training batches carry {sorted(self.shapes)})")
            if tuple(b[k].shape) != shape:
                raise ValueError(f"validation batch {k!r} of shape {tuple(b[k].shape)}: the training step's is {shape}")
            out[k] = b[k] if b[k].dtype == dt else b[k].to(dt)
        return out

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
            if self.use_graph:
                if self.static is None:
                    self.static = {k: v.clone() for k, v in b.items()}
                else:
                    for k in self.static:
                        self.static[k].copy_(b[k])
                loss3 = model.val_step_graphed(self.static, noise)
            else:
                loss3 = model.val_forward(b, noise)
            values.append(loss3.tolist())              # host sync on this batch's completion (the reference's .item())
            if time.time() - t0 > self.cfg.val_time_limit:
                break
        model.end_validation()
        n = len(values)
        mean = [sum(v[i] for v in values) / n for i in range(3)]
        return dict(step=log_step, loss_value=mean[0], loss=mean[0], curr_action_l1_loss=mean[1], next_actions_l1_loss=mean[2],
                    val_batches_count=n)


def save_training_checkpoint(cfg: FinetuneConfig, run_dir: Path, step: int, eng, dataset_statistics: Optional[dict] = None,
                             trainer=None, train_state=None) -> Path:
    """File names / key layout of finetune.py:527-572 (rank 0).  Where the VLM goes follows the reference: ``use_fz`` ->
    ``vla.module.save_pretrained(checkpoint_dir)`` (the whole VLM incl. the trained action queries at the top level, :551-552);
    otherwise ``save_pretrained(adapter_dir)`` - peft's adapter under ``lora_adapter/`` with LoRA, and, a quirk kept, the whole
    VLM under ``lora_adapter/`` for the full fine-tune (:553-554); the LoRA-merged VLM at the top level (:579-601).
    ``action_queries--{suffix}`` is a native addition (peft's adapter file does not hold them; the reference patches them into the
    merged model, :586-587), read back by checkpoints.load_run_dir.
    ``train_state`` (--save_train_state): a callable -> the state dict, written as ``train_state--{suffix}`` beside the other files
    (train_state.py); False: this checkpoint cannot be resumed exactly - a state file an earlier save left under the same name is
    removed, it would describe other weights; None: nothing is written or removed."""
    suffix = "latest_checkpoint.pt" if cfg.save_latest_checkpoint_only else f"{step}_checkpoint.pt"
    d = run_dir if cfg.save_latest_checkpoint_only else Path(str(run_dir) + f"--{step}_chkpt")
    os.makedirs(d, exist_ok=True)
    torch.save({k: v.cpu() for k, v in eng.head.head_state_dict().items()}, d / f"action_head--{suffix}")
    torch.save({k: v.clone().cpu() for k, v in eng.head.proprio_views().items()}, d / f"proprio_projector--{suffix}")
    torch.save({"weight": eng.head.P.view("action_queries").clone().cpu()}, d / f"action_queries--{suffix}")
    from . import checkpoints as CK
    from safetensors.torch import save_file
    if cfg.use_lora and trainer is not None:    # peft's adapter directory (finetune.py:537-541: vla.module.save_pretrained(adapter_dir))
        ad = d / "lora_adapter"
        os.makedirs(ad, exist_ok=True)
        save_file({k: v.contiguous().cpu() for k, v in trainer.lora_state_dict().items()}, str(ad / "adapter_model.safetensors"))
        json.dump(dict(peft_type="LORA", r=cfg.lora_rank, lora_alpha=2 * cfg.lora_rank, lora_dropout=cfg.lora_dropout, target_modules="all-linear",
                       init_lora_weights="gaussian"), open(ad / "adapter_config.json", "w"), indent=2)
        if cfg.merge_lora_during_training:      # finetune.py:579-601: merge the adapter into a bf16 base and save the whole VLM
            merged = trainer.merged_weights()
            saved = {}
            for key, wm in merged.items():
                holder, wk = trainer._base(key)
                saved[key] = holder[wk].clone()
                holder[wk].copy_(wm)
            try:
                save_file({k: v.contiguous().cpu() for k, v in CK.engine_vlm_state_dict(eng).items()}, str(d / "model.safetensors"))
            finally:
                for key, w0 in saved.items():
                    holder, wk = trainer._base(key)
                    holder[wk].copy_(w0)
    elif trainer is not None:                   # full fine-tune: vla.module.save_pretrained(adapter_dir) (finetune.py:553-554)
        ad = d / "lora_adapter"
        os.makedirs(ad, exist_ok=True)
        save_file({k: v.contiguous().cpu() for k, v in CK.engine_vlm_state_dict(eng).items()}, str(ad / "model.safetensors"))
    else:                                       # adapter-only (use_fz): vla.module.save_pretrained(checkpoint_dir) (:551-552)
        save_file({k: v.contiguous().cpu() for k, v in CK.engine_vlm_state_dict(eng).items()}, str(d / "model.safetensors"))
    if dataset_statistics is not None:          # save_dataset_statistics (finetune.py:531): q01/q99 etc. used to un-normalise actions
        json.dump(dataset_statistics, open(d / "dataset_statistics.json", "w"), indent=2)
    if train_state is not None:
        from . import train_state as TS
        if train_state is False:
            stale = d / TS.file_name(step, cfg.save_latest_checkpoint_only)
            if stale.exists():
                os.remove(stale)
        else:
            TS.save(train_state(), d, step, cfg.save_latest_checkpoint_only)
    return d


def _pad_to(batch: dict, L: int, pad_id: int) -> dict:
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


RAW_BATCH_KEYS = ("frames_u8", "prompt_flat", "prompt_off", "actions_raw", "proprio_raw")


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


def batch_stream(cfg: FinetuneConfig, mcfg, dev: str, rank: int, batches=None, explicit=(), world: int = 1, info: Optional[dict] = None,
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
    Frames not at the model's image size go through the Pillow-exact bicubic resize of the processor first; the reference's RLDS
    stage resizes with TF's lanczos3 there, which is not reproduced.

    A raw batch (``actions_raw`` ...: RAW_BATCH_KEYS) is collated on the device by ``GPUInputStage.collate``: actions and proprio
    normalised with the statistics of ``--dataset_statistics_file`` (the entry named by the batch's ``dataset_name``, or the file's
    only one), token length --max_seq_len (0: the batch's own), filler tokens and augmentation keyed by the same (seed, rank, step).

    ``start`` (--resume_train_state): the micro-step the first batch belongs to.  Every source is a function of that position - the
    samplers', the augmentation's and the collator's step, the file sources' cyclic index, the synthetic source's counter - so the
    stream yields what the stream of a run from 0 yields from its ``start``-th batch on; an explicit iterable is advanced by
    cycling through it without collating."""
    from . import synthetic as S
    from .input_stage import GPUInputStage, ImageAugment, backbone_norms
    start = int(start)
    assert start >= 0
    stage, step, norm_stats, mix_stats = None, start, None, {}

    def collate_raw(b):
        nonlocal stage, step, norm_stats
        missing = [k for k in RAW_BATCH_KEYS if k not in b]
        if missing:
            raise ValueError(f"raw batch lacks {missing}: it carries {RAW_BATCH_KEYS} and optionally dataset_name")
        mixed = "dataset_index" in b or "dataset_names" in b
        if mixed and not ("dataset_index" in b and "dataset_names" in b):
            raise ValueError("a raw batch of a dataset mixture carries both dataset_index (int32 [B]) and dataset_names")
        if norm_stats is None:
            if not cfg.dataset_statistics_file:
                raise ValueError("raw batches carry un-normalised actions / proprio: pass the statistics with --dataset_statistics_file")
            norm_stats = json.load(open(cfg.dataset_statistics_file))
        if mixed:               # every sample with its own dataset's statistics; the entry lists are built once per tuple of names
            names = tuple(b["dataset_names"])
            if names not in mix_stats:
                mix_stats[names] = mixture_stats(norm_stats, names)
            act_st, pr_st = mix_stats[names]
            index = b["dataset_index"].to(dev, torch.int32)
        else:
            st = raw_batch_stats(norm_stats, b.get("dataset_name"))
            act_st, pr_st, index = st["action"], st["proprio"], None
        if stage is None:
            stage = GPUInputStage(dev, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img, resize=cfg.frame_resize)
        aug = ImageAugment(seed=cfg.seed, rank=rank, step=step) if cfg.image_aug else None
        L = cfg.max_seq_len or None
        if L is None and b["prompt_off"].is_cuda:
            raise ValueError("raw batches with prompt offsets on the device need --max_seq_len (the natural length would be read back)")
        out = stage.collate(b["frames_u8"], (b["prompt_flat"], b["prompt_off"]), b["actions_raw"], b["proprio_raw"], action_stats=act_st,
                            proprio_stats=pr_st, L=L, seed=cfg.seed, rank=rank, step=step, augment=aug, stats_index=index)
        step += 1
        return out

    def collate(b):
        nonlocal stage, step
        if "actions_raw" in b:
            return collate_raw(b)
        b = {k: v.to(dev) for k, v in b.items()}
        if "frames_u8" not in b:
            if "image_aug" in explicit:
                raise NotImplementedError(IMAGE_AUG_REFUSAL)
            return b
        fr = b.pop("frames_u8")
        if fr.dtype != torch.uint8 or fr.dim() != 5 or fr.shape[-1] != 3:
            raise ValueError(f"frames_u8 must be uint8 [B, n_img, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
        if stage is None:
            stage = GPUInputStage(dev, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img, resize=cfg.frame_resize)
        aug = ImageAugment(seed=cfg.seed, rank=rank, step=step) if cfg.image_aug else None
        b["pixel_values"] = stage.pixels(fr, augment=aug)
        step += 1
        return b

    if batches is not None:
        skip = start
        while True:
            n = 0
            for b in batches:
                n += 1
                if skip > 0:
                    skip -= 1
                    continue
                yield collate(b)
            if n == 0:
                raise ValueError("empty batch iterable")
    elif cfg.episode_file or cfg.episode_mix:
        if cfg.episode_file:
            from .episodes import EpisodeStore
            where = cfg.episode_file
            src = EpisodeStore.load(cfg.episode_file, dev, chunk=mcfg.chunk, dataset_name=cfg.dataset_name, holdout=cfg.val_episode_fraction,
                                    jpeg_scan_index=cfg.jpeg_scan_index)
        else:
            from .mixture import EpisodeMix, parse_mix
            where = "--episode_mix"
            src = EpisodeMix.load(parse_mix(cfg.episode_mix), dev, chunk=mcfg.chunk, balance_weights=cfg.episode_mix_balance,
                                  holdout=cfg.val_episode_fraction, jpeg_scan_index=cfg.jpeg_scan_index)
        if (src.A, src.Pd) != (mcfg.action_dim, mcfg.proprio_dim):
            raise ValueError(f"{where}: actions_raw / proprio_raw have {src.A} / {src.Pd} columns, the model takes "
                             f"{mcfg.action_dim} / {mcfg.proprio_dim}")
        if src.frame_shape[0] != mcfg.n_img:
            raise ValueError(f"{where}: frames_u8 carries {src.frame_shape[0]} images per step, --num_images_in_input is {mcfg.n_img}")
        if not cfg.dataset_statistics_file:
            norm_stats = src.statistics()
            if info is not None:
                info["dataset_statistics"] = norm_stats
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
            yield collate_raw(src.sample(cfg.batch_size, cfg.seed, rank, world, step))
    elif cfg.batch_file or cfg.frame_batch_file or cfg.raw_batch_file:
        src = cfg.batch_file or cfg.frame_batch_file or cfg.raw_batch_file
        files = sorted(str(p) for p in Path(src).glob("*.pt")) if os.path.isdir(src) else [src]
        if not files:
            raise FileNotFoundError(f"no .pt batch files under {src}")
        i = (rank + start) % len(files)
        while True:
            b = torch.load(files[i], weights_only=True)
            if cfg.frame_batch_file and "frames_u8" not in b:
                raise ValueError(f"{files[i]}: --frame_batch_file batches carry frames_u8 (uint8 [B, n_img, H, W, 3])")
            if cfg.raw_batch_file and "actions_raw" not in b:
                raise ValueError(f"{files[i]}: --raw_batch_file batches carry {RAW_BATCH_KEYS}")
            yield collate(b)
            i = (i + 1) % len(files)
    else:
        i = start
        while True:
            yield S.make_batch(mcfg, cfg.batch_size, dev, seed=1_000_003 * cfg.seed + 7919 * rank + i, P=32, ragged=True)
            i += 1


def finetune(cfg: FinetuneConfig, batches=None, explicit=(), val_batches=None, on_finish=None) -> dict:
    """``batches``: optional iterable of collated batch dicts (util/data_utils.py:165-172 contract); ``explicit``: names of
    the flags given on the command line (parse_args records them); ``val_batches``: optional held-out batches of the same form
    for --use_val_set (iterated once per validation sweep; instead of --val_batch_file); ``on_finish(engine, trainer or None)``:
    called once behind the last step and the final save, with every update applied and the device idle (a caller that wants
    to look at the trained model itself, not at its checkpoint files)."""
    from . import ddp, engine as E, synthetic as S
    explicit = explicit or getattr(cfg, "_explicit", ())
    check_supported(cfg, explicit, frame_batches=batches is not None, val_batches=val_batches is not None)
    rank, local, world = ddp.init_process_group_from_env()
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    from . import checkpoints as CK
    # model geometry: explicit --backbone, else read off the --vlm_path state dict (which backbones, widths, depths), else BASELINE
    # configs[1].  The reference builds the model from the checkpoint's config.json (finetune.py:777-816); --tiny is the plumbing size.
    vlm_sd = CK.load_file(cfg.vlm_path) if (cfg.vlm_path and os.path.isfile(cfg.vlm_path)) else None
    if cfg.tiny:
        mcfg = E.NAMED_CONFIGS[cfg.backbone or "tiny"]()
    elif cfg.backbone is not None:
        mcfg = E.NAMED_CONFIGS[cfg.backbone]()
    elif vlm_sd is not None:
        mcfg = CK.infer_config(vlm_sd)
    else:
        mcfg = E.config2()
    mcfg.n_img = cfg.num_images_in_input
    mcfg.pro = bool(cfg.use_pro_version)
    mode = train_mode(cfg)
    W = S.make_weights(mcfg, dev, seed=cfg.seed)                  # identical on all ranks == DDP's initial broadcast
    if vlm_sd is not None:                                        # local VLM state dict (HF-style or native Prismatic keys)
        W.update(CK.split_reference_state_dict(vlm_sd, mcfg))
    lora_sd = None
    from . import train_state as TS
    # the flags that define the trajectory (--save_train_state writes them, --resume_train_state compares them), and the state to go on from
    fp = TS.fingerprint(cfg, mode, world, mcfg.n_img, batches is not None) if (cfg.save_train_state or cfg.resume_train_state) else None
    ts, start = None, None
    if cfg.resume:                    # head / proprio (finetune.py:275-278) + the action queries + whatever else this mode trained
        if not (cfg.resum_vla_path and os.path.isdir(cfg.resum_vla_path)):
            raise FileNotFoundError(f"--resume: --resum_vla_path {cfg.resum_vla_path!r} is not a checkpoint directory")
        if cfg.resume_train_state:    # every rank reads the file rank 0 wrote; refused before a weight is loaded: no file, another step, other flags
            ts = TS.load(cfg.resum_vla_path, cfg.resume_step)
            TS.check(ts, fp=fp, mode=mode, resume_step=cfg.resume_step)
            start = TS.resumed_position(ts)
        W["head"], W["proprio"], aq = CK.load_run_dir(cfg.resum_vla_path, cfg.resume_step, with_action_queries=True)
        if aq is not None:
            W["action_queries"] = aq
        rd = Path(cfg.resum_vla_path)
        if mode == "full":            # the trained VLM lives under lora_adapter/ (save_training_checkpoint, reference quirk kept)
            f = rd / "lora_adapter" / "model.safetensors"
            if not f.exists():
                raise FileNotFoundError(f"--resume of a full fine-tune needs {f}")
            W.update(CK.split_reference_state_dict(CK.load_file(str(f)), mcfg))
        elif mode == "lora":
            f = rd / "lora_adapter" / "adapter_model.safetensors"
            if not f.exists():
                raise FileNotFoundError(f"--resume of a LoRA fine-tune needs {f}")
            lora_sd = CK.load_file(str(f))
    eng = E.VLAEngine(mcfg, W, dev)
    if world > 1:
        eng.reducer = ddp.FlatGradReducer(algo=cfg.ddp_algo)
    trainer = None
    if mode == "lora":
        from .trainers import LoRAFinetune
        trainer = LoRAFinetune(eng, rank=cfg.lora_rank, seed=cfg.seed, fp8=cfg.fp8_base_weights, dropout=cfg.lora_dropout)
        if lora_sd is not None:
            trainer.load_lora_state_dict(lora_sd)
    elif mode == "full":
        from .trainers import FullFinetune
        trainer = FullFinetune(eng)
    use_graph = cfg.use_graph
    (trainer or eng).set_grad_accumulation(cfg.grad_accumulation_steps)
    if cfg.objective != "l1":
        trainer.set_objective(cfg.objective)
    clip = cfg.max_grad_norm is not None
    if clip:
        (trainer or eng).set_max_grad_norm(cfg.max_grad_norm)
    owner = trainer or eng
    if ts is not None:                # the loaded weights are the ones the state was written beside (digests), then m, v and the step count
        owner.verify_data_digests(ts)
        owner.load_optimizer_state(ts)
    info = {}
    stream = batch_stream(cfg, mcfg, dev, rank, batches, explicit, world=world, info=info, start=start[0] if start else 0)
    pad_id = min(S.PAD_ID, mcfg.llm.vocab - 1)
    cur = next(stream)
    L = cfg.max_seq_len or cur["input_ids"].shape[1]
    cur = _pad_to(cur, L, pad_id)
    training = cfg.phase == "Training"
    gen = torch.Generator(device=dev).manual_seed(cfg.seed * 7919 + rank)
    noise = torch.zeros(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, device=dev, dtype=torch.bfloat16)
    run_dir = Path(cfg.run_root_dir) / (cfg.run_id_override or f"native+{cfg.dataset_name}+b{cfg.batch_size * world}+lr-{cfg.learning_rate}")
    stats = json.load(open(cfg.dataset_statistics_file)) if cfg.dataset_statistics_file else info.get("dataset_statistics")
    static = None
    if use_graph:
        static = {k: v.clone() for k, v in cur.items()}
        if trainer is not None:       # LoRA / full fine-tune: forward + backward as one captured graph (trainers.BackboneTrainer.capture)
            trainer.capture(static, noise if training else None)
        else:
            eng.capture(static, noise if training else None, conservative_rows=cfg.conservative_rows,
                        row0=ts["row0"] if ts is not None and ts["row0"] >= 0 else None)     # (the window of the run this one continues)
    if ts is not None:                # behind capture and its warm-up, which move the dropout counter: the counters, the head-noise generator
        owner.load_device_counters(ts)
        TS.restore_generator(gen, ts, writer=rank == 0)
    validator = None
    if cfg.use_val_set and cfg.val_episode_fraction is not None:
        from .heldout import HeldOutSweep
        validator = HeldOutSweep(cfg, mcfg, dev, rank, world, trainer or eng, info["store"], stats, static if static is not None else cur, L,
                                 use_graph)
        info["heldout"] = validator.info()
        if rank == 0:
            print(json.dumps(dict(heldout=info["heldout"])), flush=True)
    elif cfg.use_val_set:
        validator = ValidationPass(cfg, mcfg, dev, rank, trainer or eng, static if static is not None else cur, L, pad_id, use_graph,
                                   val_batches)
    log, val_log, t0, saved_at, steps_done, first = [], [], time.time(), None, 0, True

    def state_after(batch_idx, g, log_step):
        """--save_train_state: the state behind the optimizer step that closes micro-step batch_idx (every update applied)."""
        return lambda: TS.collect(owner, mode=mode, fp=fp, next_grad_step=g + 1, next_micro_step=batch_idx + 1, log_step=log_step,
                                  generator=gen, row0=eng.frozen_row0)
    for item in loop_plan(cfg, start):
        batch_idx, g, log_step, boundary, save, last = item
        nxt = _pad_to(next(stream), L, pad_id)                    # one batch of look-ahead: its vision stage runs inside this step
        if training:   # fresh N(0, 0.02^2) perturbation every call (action_heads.py:14-17, 69-72)
            noise.copy_((torch.randn(noise.shape, device=dev, generator=gen) * 0.02).to(torch.bfloat16))
        lr = lr_at(g, cfg)
        if trainer is not None and use_graph:
            for k in static:
                static[k].copy_(cur[k])
            loss3 = trainer.train_step_graphed(lr)
        elif trainer is not None:
            loss3 = trainer.train_step(cur, lr, noise if training else None)
        elif use_graph:
            for k in static:
                if k != "pixel_values" or first:
                    static[k].copy_(cur[k])
            eng.stage_next_pixels(nxt["pixel_values"])
            loss3 = eng.train_step_graphed(lr)
        else:
            loss3 = eng.train_step(cur, lr, noise if training else None)
        steps_done += int(boundary)
        first = False
        if boundary and world > 1 and cfg.sync_check_freq > 0 and steps_done % cfg.sync_check_freq == 0:
            eng.flush()                      # (the captured adapter step leaves its update pending: compare what the ranks really hold)
            flats = [eng.head.P.data] + ([trainer.P.data] if trainer is not None else [])
            ddp.assert_ranks_in_sync(flats, what=f"parameters after optimizer step {steps_done}")
        if boundary and (log_step % cfg.wandb_log_freq == 0 or last):          # the only host sync, every log_freq gradient steps
            ce = cfg.objective == "token_ce"
            # token-CE: the four metrics of the reference's trainer (base_strategy.py:350-356; this rank's batch, as there) ride the
            # loss's read-back - one copy, one sync
            parts = [loss3] + ([trainer.ce_metrics] if ce else [])
            store = info.get("store")
            jpeg = store is not None and store.jpeg is not None and store.decode_status is not None
            if jpeg:    # JPEG frames: how many segments of the batch drawn last did not decode rides the same read-back
                parts.append(store.bad_segments())
            if clip:    # the norm of this step's update rides the same read-back (the captured adapter step leaves its update pending: apply it)
                eng.flush()
                parts.append((trainer or eng).grad_norm.view(1))
            if cfg.log_state_digest:        # the digests ride it too, as 16-bit limbs (exact in f32); they are of the state behind this step's update
                eng.flush()
                parts.append(TS.limbs_f32(owner.state_digests_device()))
            l = (torch.cat(parts) if len(parts) > 1 else loss3).tolist()
            if cfg.log_state_digest:
                nd = parts[-1].numel()
                l, digests = l[:-nd], owner.state_digest_dict(TS.from_limbs(l[-nd:]))
            l, tm, gn, bad = l[:3], l[3:7] if ce else [], l[-1], l[7 if ce else 3] if jpeg else None
            if not all(x == x for x in l):
                raise FloatingPointError(f"non-finite loss at step {log_step}: {l} (a captured step replayed on a batch whose action "
                                         "block starts before the frozen live-row window poisons the loss: --conservative_rows true)")
            log.append(dict(step=log_step, loss_value=l[0], curr_action_l1_loss=l[1], next_actions_l1_loss=l[2], lr=lr))
            if ce:      # (next_actions_l1_loss: the reference's name for the decoded next-actions L1 replaces the copy of the loss)
                from .ops import TOKEN_METRIC_NAMES
                log[-1].update(zip(TOKEN_METRIC_NAMES, tm))
            if clip:
                log[-1]["grad_norm"] = gn
            if jpeg:
                log[-1]["jpeg_bad_segments"] = int(bad)
            if cfg.log_state_digest:
                log[-1]["state_digest"] = digests
            if rank == 0:
                print(json.dumps(log[-1]), flush=True)
        if save:
            eng.flush()                      # the graphed step leaves its parameter update pending (engine.capture)
            if rank == 0:
                save_training_checkpoint(cfg, run_dir, log_step, eng, stats, trainer,
                                         train_state=state_after(batch_idx, g, log_step) if cfg.save_train_state else None)
            saved_at = log_step
            if world > 1:
                torch.distributed.barrier()  # finetune.py:544, 575
        if validator is not None and validation_due(cfg, item):
            val_log.append(validator.sweep(log_step))
            if rank == 0:
                print(json.dumps(val_log[-1]), flush=True)
        cur = nxt
        final_step = log_step
    eng.flush()
    torch.cuda.synchronize()
    if saved_at != final_step and rank == 0:     # never discard a run: the reference only saves on save_freq multiples
        # a state only where it can be resumed exactly: with grad accumulation the run ends INSIDE a gradient step (loop_plan: the last
        # micro-batch's gradients are never applied, the accumulators hold a partial sum) - the weights are saved, no state is
        final_state = None if not cfg.save_train_state else (state_after(batch_idx, g, final_step) if boundary else False)
        save_training_checkpoint(cfg, run_dir, final_step, eng, stats, trainer, train_state=final_state)
    if on_finish is not None:
        on_finish(eng, trainer)
    model = dict(vit=[dict(v.as_oracle(), img=v.img) for v in mcfg.vit], llm=dict(mcfg.llm.as_oracle(), d=mcfg.llm.d, inter=mcfg.llm.inter, vocab=mcfg.llm.vocab),
                 n_img=mcfg.n_img, num_blocks=mcfg.num_blocks, pro=mcfg.pro)
    out = dict(log=log, val_log=val_log, seconds=time.time() - t0, steps=steps_done, world=world, final_step=final_step, run_dir=str(run_dir), mode=mode, model=model)
    if "mixture" in info:                        # --episode_mix: names, probabilities, quotas, period, the reference's dataset_len
        out["mixture"] = info["mixture"]
    if "heldout" in info:                        # --val_episode_fraction: per dataset the held-out episode range and the window counts
        out["heldout"] = info["heldout"]
    return out
