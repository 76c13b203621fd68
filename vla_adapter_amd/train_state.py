"""Training state beside a checkpoint: what a run needs, besides its weights, to go on bit for bit where it stopped.

``train_state--{suffix}`` is written next to the checkpoint files of finetune.save_training_checkpoint under ``--save_train_state`` and
read back under ``--resume_train_state``.  It is a dict of CPU tensors, ints, strings and lists (``torch.load(weights_only=True)``):

    version        FORMAT_VERSION
    mode           "adapter" | "lora" | "full"
    buffers        {name: {m, v: bf16 [numel]; numel; offsets: sha256 of the offsets table (names, offsets, shapes);
                           digest: {data, m, v: hex strings of ops.state_digest}}}     name: "head", and "backbone" where a trainer owns one
    step_counts    {owner: AdamW step count}
    next_grad_step, next_micro_step    the first gradient step / micro-step whose gradients have not been applied
    log_step       the step the checkpoint is named for
    generator      the head-noise generator's state (uint8 tensor), of the rank that wrote the file
    generator_offset   its Philox offset: every rank reseeds its own generator and takes this offset
    row0           the frozen live-row window (engine._row0), -1: none
    counters       {name: value} of the owner's device counters (LoRA: drop_step, the dropout masks' step counter)
    fingerprint    JSON of the flags that define the trajectory (fingerprint())

The weights are NOT in the file: they stay in the checkpoint's own files, and the file holds the digest of every flat ``data`` buffer
as it was when they were written.  A resume loads the weights through the usual path and compares digests: equal digests prove the
checkpoint round trip lossless, unequal ones stop the run."""
from __future__ import annotations

import hashlib
import json
import os
from typing import Optional

import torch

FORMAT_VERSION = 1
# not part of the fingerprint: how long a run goes on, what it writes and what it reports
NOT_FINGERPRINTED = ("max_steps", "save_freq", "val_freq", "val_time_limit", "wandb_log_freq", "log_state_digest", "run_root_dir")
PARTS = ("data", "m", "v")


def file_name(step, latest_only: bool = False) -> str:
    return "train_state--" + ("latest_checkpoint.pt" if latest_only or step in (None, "latest") else f"{step}_checkpoint.pt")


def offsets_hash(P) -> str:
    """sha256 over the flat buffer's table: every name with its offset and shape, in order, and the buffer's length."""
    h = hashlib.sha256()
    for name, (off, shape) in P.offsets.items():
        h.update(f"{name}:{off}:{tuple(int(s) for s in shape)};".encode())
    h.update(f"numel={P.numel}".encode())
    return h.hexdigest()


def hex64(v: int) -> str:
    return f"0x{int(v) & (2 ** 64 - 1):016x}"


def digests_device(buffers, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ops.state_digest of data, m and v of every (name, FlatParams) -> int64 [3 * len(buffers)] on the device, in that order.
    Launched on the current stream; nothing synchronises."""
    from . import ops
    dev = buffers[0][1].data.device
    if out is None:
        out = torch.empty(3 * len(buffers), device=dev, dtype=torch.int64)
    k = 0
    for _, P in buffers:
        for t in (P.data, P.m, P.v):
            ops.state_digest(t, 0, out=out[k:k + 1])
            k += 1
    return out


def limbs_f32(d: torch.Tensor) -> torch.Tensor:
    """int64 [k] -> f32 [4 k]: the 16-bit limbs of every value, least significant first - each exact in f32, so that digests can ride a
    read-back of f32 values (the log line's) without a copy of their own."""
    return (d.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)


def from_limbs(vals) -> list:
    """The inverse of limbs_f32 on the host: a list of 4 k floats -> k unsigned 64-bit ints."""
    vals = [int(x) for x in vals]
    return [vals[i] | vals[i + 1] << 16 | vals[i + 2] << 32 | vals[i + 3] << 48 for i in range(0, len(vals), 4)]


def digest_dict(buffers, values) -> dict:
    """{name: {data, m, v: hex}} from the values of digests_device (ints, in its order)."""
    it = iter(values)
    return {name: {part: hex64(next(it)) for part in PARTS} for name, _ in buffers}


def read_digests(buffers) -> dict:
    """digests_device read back (one host sync) -> digest_dict."""
    return digest_dict(buffers, [v & (2 ** 64 - 1) for v in digests_device(buffers).tolist()])


def source_of(cfg, batches_given: bool = False):
    """(kind, path) of the batch source."""
    if batches_given:
        return "batches", None
    for kind in ("batch_file", "frame_batch_file", "raw_batch_file", "episode_file", "episode_mix"):
        if getattr(cfg, kind):
            return kind, str(getattr(cfg, kind))
    return "synthetic", None


def fingerprint(cfg, mode: str, world: int, n_img: int, batches_given: bool = False) -> dict:
    """The flags that define the trajectory.  Two runs with equal fingerprints, equal weights and equal state take the same steps."""
    kind, path = source_of(cfg, batches_given)
    lora = mode == "lora"
    fp = dict(
        seed=int(cfg.seed), batch_size=int(cfg.batch_size), grad_accumulation_steps=int(cfg.grad_accumulation_steps),
        learning_rate=float(cfg.learning_rate), lr_warmup_steps=float(cfg.lr_warmup_steps), num_steps_before_decay=int(cfg.num_steps_before_decay),
        mode=mode, lora_rank=int(cfg.lora_rank) if lora else None, lora_dropout=float(cfg.lora_dropout) if lora else None,
        fp8_base_weights=bool(cfg.fp8_base_weights), objective=str(cfg.objective),
        max_grad_norm=None if cfg.max_grad_norm is None else float(cfg.max_grad_norm),
        batch_source=kind, batch_source_path=path, max_seq_len=int(cfg.max_seq_len), image_aug=bool(cfg.image_aug),
        episode_mix=cfg.episode_mix, episode_mix_balance=bool(cfg.episode_mix_balance),
        val_episode_fraction=None if cfg.val_episode_fraction is None else float(cfg.val_episode_fraction),
        dataset_statistics_file=cfg.dataset_statistics_file, dataset_name=str(cfg.dataset_name),
        world_size=int(world), phase=str(cfg.phase), use_graph=bool(cfg.use_graph), conservative_rows=bool(cfg.conservative_rows),
        backbone=cfg.backbone, tiny=bool(cfg.tiny), use_pro_version=bool(cfg.use_pro_version), num_images_in_input=int(n_img),
        ddp_algo=str(cfg.ddp_algo))
    if getattr(cfg, "frame_resize", "bicubic") != "bicubic":      # (only when it is not the default: a state written before the flag existed resumes)
        fp["frame_resize"] = str(cfg.frame_resize)
    if int(getattr(cfg, "episode_jpeg_quality", 0) or 0) != 0:    # (lossy, so it defines the trajectory; likewise only when it is set)
        fp["episode_jpeg_quality"] = int(cfg.episode_jpeg_quality)
    return fp


def fingerprint_differences(recorded: dict, current: dict) -> list:
    """["flag: recorded X, now Y", ...] for every flag that differs (a flag one side lacks counts)."""
    out = []
    for k in sorted(set(recorded) | set(current)):
        a, b = recorded.get(k, "<absent>"), current.get(k, "<absent>")
        if a != b:
            out.append(f"{k}: recorded {a!r}, now {b!r}")
    return out


def collect(model, *, mode: str, fp: dict, next_grad_step: int, next_micro_step: int, log_step: int, generator, row0) -> dict:
    """The state dict of a run that stands between two gradient steps (every update applied: the caller has flushed)."""
    opt = model.optimizer_state()
    gstate = generator.get_state().cpu().clone()
    return dict(version=FORMAT_VERSION, mode=str(mode), buffers=opt["buffers"], step_counts=opt["step_counts"], counters=opt["counters"],
                next_grad_step=int(next_grad_step), next_micro_step=int(next_micro_step), log_step=int(log_step),
                generator=gstate, generator_offset=int(generator_offset(generator)),
                row0=-1 if row0 is None else int(row0),
                fingerprint=json.dumps(fp, sort_keys=True))


def generator_offset(gen) -> int:
    """Philox offset of a device generator: how far the run has drawn from it."""
    return int(gen.get_offset())


def restore_generator(gen, state: dict, writer: bool) -> None:
    """The rank that wrote the file takes the recorded state whole; any other rank keeps its own seed and takes the recorded offset (the
    ranks draw the same shapes at the same steps: their positions are equal, their seeds are not)."""
    if writer:
        gen.set_state(state["generator"])
    else:
        gen.set_offset(int(state["generator_offset"]))


def save(state: dict, directory, step, latest_only: bool = False) -> str:
    path = os.path.join(str(directory), file_name(step, latest_only))
    torch.save(state, path)
    return path


def find(directory, step) -> Optional[str]:
    for name in (file_name(step), file_name(None)):
        p = os.path.join(str(directory), name)
        if os.path.isfile(p):
            return p
    return None


def load(directory, step) -> dict:
    """The state file of a checkpoint directory; ValueError where there is none or it is of another format."""
    p = find(directory, step)
    if p is None:
        raise ValueError(f"--resume_train_state: no state file in {str(directory)!r} ({file_name(step)} or {file_name(None)}): the run "
                         "that wrote this checkpoint did not pass --save_train_state True")
    st = torch.load(p, map_location="cpu", weights_only=True)
    if not isinstance(st, dict) or st.get("version") != FORMAT_VERSION:
        raise ValueError(f"--resume_train_state: {p} has format version {st.get('version') if isinstance(st, dict) else None!r}, this build reads {FORMAT_VERSION}")
    return st


def check(state: dict, *, fp: dict, mode: str, resume_step) -> None:
    """The refusals that need no model: the step, the mode and the fingerprint."""
    if int(state["log_step"]) != int(resume_step):
        raise ValueError(f"--resume_train_state: the state file records step {int(state['log_step'])}, --resume_step is {resume_step}")
    diff = fingerprint_differences(json.loads(state["fingerprint"]), fp)
    if state["mode"] != mode and not any(d.startswith("mode:") for d in diff):
        diff.append(f"mode: recorded {state['mode']!r}, now {mode!r}")
    if diff:
        raise ValueError("--resume_train_state: the flags that define the trajectory differ from the run that wrote the state - " + "; ".join(diff))


def resumed_position(state: dict) -> tuple:
    """(first micro-step, log-step base) for finetune.loop_plan(cfg, start=...): the plan goes on with gradient step
    next_grad_step = next_micro_step // ga at log_step = recorded log_step + 1."""
    return int(state["next_micro_step"]), int(state["log_step"]) + 1 - int(state["next_grad_step"])
