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
from types import SimpleNamespace
from typing import Optional

import torch

from .batches import IMAGE_AUG_REFUSAL, RAW_BATCH_KEYS, batch_stream, mixture_stats, pad_to, raw_batch_stats  # noqa: F401  (re-exported)
from .validation import ValidationPass, validation_due, validation_noise  # noqa: F401  (re-exported)

_pad_to = pad_to                      # the name it had here: callers written against it keep resolving


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
    episode_jpeg_quality: int = 0         # --episode_file / --episode_mix whose frames are raw: code them on the device at load into the JPEG
                                          # form at this quality (1 .. 100; jpeg_store.encode_tables) - a tenth of the bytes
                                          # in HBM, and the run tools/pack_episodes_jpeg.py's file of the same quality gives.  LOSSY; 0 = off
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
    if isinstance(cfg.episode_jpeg_quality, bool) or not isinstance(cfg.episode_jpeg_quality, int) or not 0 <= cfg.episode_jpeg_quality <= 100:
        raise ValueError(f"--episode_jpeg_quality is an int inside 0 .. 100 (0: off), got {cfg.episode_jpeg_quality!r}")
    if cfg.episode_jpeg_quality and not (cfg.episode_file or cfg.episode_mix):
        raise ValueError("--episode_jpeg_quality codes the frames of --episode_file / --episode_mix: no other batch source keeps frames on the device")
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


class StepRunner:
    """One training step in each of its four forms - trainer (LoRA / full fine-tune) or the adapter-only engine, captured or eager.
    It owns what the forms need between steps: the static batch of the captured step, the head-noise buffer (``training``: the caller
    refills it before a step; else no noise is fed) and whether a step has run."""

    def __init__(self, eng, trainer, mcfg, dev: str, use_graph: bool, training: bool = True, conservative_rows: bool = False):
        self.eng, self.trainer, self.owner = eng, trainer, trainer or eng
        self.use_graph, self.conservative_rows = bool(use_graph), conservative_rows
        self.noise = torch.zeros(mcfg.chunk, mcfg.action_dim * mcfg.llm.d, device=dev, dtype=torch.bfloat16)
        self.fed_noise = self.noise if training else None
        self.static, self.first = None, True

    def capture(self, first_batch: dict, resume_state: Optional[dict] = None) -> None:
        """use_graph: captures the step on a copy of the padded ``first_batch``, the static batch; eager: nothing to do."""
        if not self.use_graph:
            return
        self.static = {k: v.clone() for k, v in first_batch.items()}
        if self.trainer is not None:  # LoRA / full fine-tune: forward + backward as one captured graph (trainers.BackboneTrainer.capture)
            self.trainer.capture(self.static, self.fed_noise)
        else:
            ts = resume_state
            self.eng.capture(self.static, self.fed_noise, conservative_rows=self.conservative_rows,
                             row0=ts["row0"] if ts is not None and ts["row0"] >= 0 else None)    # (the window of the run this one continues)

    def step(self, cur: dict, nxt: dict, lr: float):
        """Trains on ``cur``; ``nxt`` is the batch after it, whose vision stage the captured adapter-only step runs inside this one.
        -> the three loss values on the device."""
        first, self.first = self.first, False
        if not self.use_graph:
            return self.owner.train_step(cur, lr, self.fed_noise)
        if self.trainer is not None:
            for k in self.static:
                self.static[k].copy_(cur[k])
            return self.trainer.train_step_graphed(lr)
        for k in self.static:         # (the pixels reach the vision stage through stage_next_pixels: the first step's copy is spare)
            if k != "pixel_values" or first:
                self.static[k].copy_(cur[k])
        self.eng.stage_next_pixels(nxt["pixel_values"])
        return self.eng.train_step_graphed(lr)


class LogReadback:
    """The logged step's one host read-back: 1-D device tensors added by name, concatenated in that order (a lone part as it is),
    read with one ``tolist`` and handed back by name."""

    def __init__(self):
        self.parts = {}

    def add(self, name: str, part) -> None:
        self.parts[name] = part

    def read(self) -> dict:
        parts = list(self.parts.values())
        flat = iter((torch.cat(parts) if len(parts) > 1 else parts[0]).tolist())
        return {name: [next(flat) for _ in range(part.numel())] for name, part in self.parts.items()}


def setup_run(cfg: FinetuneConfig, explicit, given_batches: bool, given_val_batches: bool) -> SimpleNamespace:
    """Everything in front of the first batch: the flags checked, the process group, the model config, the weights (random, --vlm_path,
    --resume), the --resume_train_state file, the engine and the trainer of the mode with their step controls and, resumed, their
    optimizer state.  -> what the loop needs, by name."""
    from . import checkpoints as CK, ddp, engine as E, synthetic as S, train_state as TS
    check_supported(cfg, explicit, frame_batches=given_batches, val_batches=given_val_batches)
    rank, local, world = ddp.init_process_group_from_env()
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    vlm_sd = CK.load_file(cfg.vlm_path) if (cfg.vlm_path and os.path.isfile(cfg.vlm_path)) else None
    # model geometry: explicit --backbone, else read off the --vlm_path state dict (which backbones, widths, depths), else BASELINE
    # configs[1].  The reference builds the model from the checkpoint's config.json (finetune.py:777-816); --tiny is the plumbing size.
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
    # the flags that define the trajectory (--save_train_state writes them, --resume_train_state compares them), and the state to go on from
    fp = TS.fingerprint(cfg, mode, world, mcfg.n_img, given_batches) if (cfg.save_train_state or cfg.resume_train_state) else None
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
    owner = trainer or eng
    owner.set_grad_accumulation(cfg.grad_accumulation_steps)
    if cfg.objective != "l1":
        trainer.set_objective(cfg.objective)
    if cfg.max_grad_norm is not None:
        owner.set_max_grad_norm(cfg.max_grad_norm)
    if ts is not None:                # the loaded weights are the ones the state was written beside (digests), then m, v and the step count
        owner.verify_data_digests(ts)
        owner.load_optimizer_state(ts)
    return SimpleNamespace(rank=rank, world=world, dev=dev, mcfg=mcfg, mode=mode, eng=eng, trainer=trainer, owner=owner, fp=fp, ts=ts,
                           start=start, pad_id=min(S.PAD_ID, mcfg.llm.vocab - 1))


def finetune(cfg: FinetuneConfig, batches=None, explicit=(), val_batches=None, on_finish=None) -> dict:
    """``batches``: optional iterable of collated batch dicts (util/data_utils.py:165-172 contract); ``explicit``: names of
    the flags given on the command line (parse_args records them); ``val_batches``: optional held-out batches of the same form
    for --use_val_set (iterated once per validation sweep; instead of --val_batch_file); ``on_finish(engine, trainer or None)``:
    called once behind the last step and the final save, with every update applied and the device idle (a caller that wants
    to look at the trained model itself, not at its checkpoint files)."""
    from . import ddp, train_state as TS
    explicit = explicit or getattr(cfg, "_explicit", ())
    run = setup_run(cfg, explicit, batches is not None, val_batches is not None)
    rank, world, dev, mcfg, mode, eng, trainer, owner, ts, start, pad_id = (run.rank, run.world, run.dev, run.mcfg, run.mode, run.eng,
                                                                          run.trainer, run.owner, run.ts, run.start, run.pad_id)
    info = {}
    stream = batch_stream(cfg, mcfg, dev, rank, batches, explicit, world=world, info=info, start=start[0] if start else 0)
    cur = next(stream)
    L = cfg.max_seq_len or cur["input_ids"].shape[1]
    cur = pad_to(cur, L, pad_id)
    training = cfg.phase == "Training"
    gen = torch.Generator(device=dev).manual_seed(cfg.seed * 7919 + rank)
    run_dir = Path(cfg.run_root_dir) / (cfg.run_id_override or f"native+{cfg.dataset_name}+b{cfg.batch_size * world}+lr-{cfg.learning_rate}")
    stats = json.load(open(cfg.dataset_statistics_file)) if cfg.dataset_statistics_file else info.get("dataset_statistics")
    runner = StepRunner(eng, trainer, mcfg, dev, cfg.use_graph, training, cfg.conservative_rows)
    runner.capture(cur, ts)
    if ts is not None:                # behind capture and its warm-up, which move the dropout counter: the counters, the head-noise generator
        owner.load_device_counters(ts)
        TS.restore_generator(gen, ts, writer=rank == 0)
    validator, shaped = None, runner.static if runner.static is not None else cur
    if cfg.use_val_set and cfg.val_episode_fraction is not None:
        from .heldout import HeldOutSweep
        validator = HeldOutSweep(cfg, mcfg, dev, rank, world, owner, info["store"], stats, shaped, L, cfg.use_graph)
        info["heldout"] = validator.info()
        if rank == 0:
            print(json.dumps(dict(heldout=info["heldout"])), flush=True)
    elif cfg.use_val_set:
        validator = ValidationPass(cfg, mcfg, dev, rank, owner, shaped, L, pad_id, cfg.use_graph, val_batches)
    clip, ce = cfg.max_grad_norm is not None, cfg.objective == "token_ce"
    store = info.get("store")
    log, val_log, t0, saved_at, steps_done = [], [], time.time(), None, 0

    def state_after(batch_idx, g, log_step):
        """--save_train_state: the state behind the optimizer step that closes micro-step batch_idx (every update applied)."""
        return lambda: TS.collect(owner, mode=mode, fp=run.fp, next_grad_step=g + 1, next_micro_step=batch_idx + 1, log_step=log_step,
                                  generator=gen, row0=eng.frozen_row0)

    def log_entry(log_step, lr, loss3) -> dict:
        """The log line of a step: the only host sync, one read-back that everything the line carries rides."""
        rb = LogReadback()
        rb.add("loss", loss3)
        if ce:      # the four metrics of the reference's trainer (base_strategy.py:350-356; this rank's batch, as there)
            rb.add("ce", trainer.ce_metrics)
        if store is not None and store.jpeg is not None and store.decode_status is not None:
            rb.add("jpeg", store.bad_segments())   # JPEG frames: how many segments of the batch drawn last did not decode
        if clip:    # the norm of this step's update (the captured adapter step leaves its update pending: apply it)
            eng.flush()
            rb.add("grad_norm", owner.grad_norm.view(1))
        if cfg.log_state_digest:        # the digests as 16-bit limbs (exact in f32); they are of the state behind this step's update
            eng.flush()
            rb.add("digest", TS.limbs_f32(owner.state_digests_device()))
        got = rb.read()
        l = got["loss"]
        if not all(x == x for x in l):
            raise FloatingPointError(f"non-finite loss at step {log_step}: {l} (a captured step replayed on a batch whose action "
                                     "block starts before the frozen live-row window poisons the loss: --conservative_rows true)")
        entry = dict(step=log_step, loss_value=l[0], curr_action_l1_loss=l[1], next_actions_l1_loss=l[2], lr=lr)
        if ce:      # (next_actions_l1_loss: the reference's name for the decoded next-actions L1 replaces the copy of the loss)
            from .ops import TOKEN_METRIC_NAMES
            entry.update(zip(TOKEN_METRIC_NAMES, got["ce"]))
        if clip:
            entry["grad_norm"] = got["grad_norm"][0]
        if "jpeg" in got:
            entry["jpeg_bad_segments"] = int(got["jpeg"][0])
        if cfg.log_state_digest:
            entry["state_digest"] = owner.state_digest_dict(TS.from_limbs(got["digest"]))
        return entry

    for item in loop_plan(cfg, start):
        batch_idx, g, log_step, boundary, save, last = item
        nxt = pad_to(next(stream), L, pad_id)                     # one batch of look-ahead: its vision stage runs inside this step
        if training:   # fresh N(0, 0.02^2) perturbation every call (action_heads.py:14-17, 69-72)
            runner.noise.copy_((torch.randn(runner.noise.shape, device=dev, generator=gen) * 0.02).to(torch.bfloat16))
        lr = lr_at(g, cfg)
        loss3 = runner.step(cur, nxt, lr)
        steps_done += int(boundary)
        if boundary and world > 1 and cfg.sync_check_freq > 0 and steps_done % cfg.sync_check_freq == 0:
            eng.flush()                      # (the captured adapter step leaves its update pending: compare what the ranks really hold)
            flats = [eng.head.P.data] + ([trainer.P.data] if trainer is not None else [])
            ddp.assert_ranks_in_sync(flats, what=f"parameters after optimizer step {steps_done}")
        if boundary and (log_step % cfg.wandb_log_freq == 0 or last):          # every log_freq gradient steps
            log.append(log_entry(log_step, lr, loss3))
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
