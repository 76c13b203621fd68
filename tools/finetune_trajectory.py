#!/usr/bin/env python3
"""Records what ``finetune()`` does on a fixed list of command lines, so that two versions of the driver can be compared bit for bit.

Every line runs at ``--tiny`` for a few steps with ``--log_state_digest`` and takes one path through the driver: the adapter-only
step captured and eager, LoRA captured with dropout and gradient clipping, the full fine-tune eager under gradient accumulation, the
token-CE objective, a JPEG ``--episode_file`` with held-out validation, ``--episode_mix``, ``--frame_batch_file`` with
``--val_batch_file``, and a ``--save_train_state`` run with its ``--resume_train_state`` continuation.  The toy inputs (episodes of
``_episode_bench.synthetic_episodes``, frame batches of ``synthetic.make_batch``) are written to the working directory from fixed seeds;
all paths on the command lines are relative to it, so nothing recorded depends on where it lies.

Per line the record holds the ``log``, the ``val_log``, the ``heldout`` / ``mixture`` info and, for every file of the run directory, the
sha256 of its bytes and - for .pt and .safetensors files - a sha256 over the tensors it holds (names, dtypes, shapes, bytes): should a
file format not repeat byte for byte, its content still compares.  ``seconds`` is left out.

  python tools/finetune_trajectory.py --out new.json [--label <commit>]        # on a GPU; vla_adapter_amd is taken from beside tools/
  python tools/finetune_trajectory.py --compare parent.json new.json             # one JSON line: identical, and what differs
"""
import argparse
import hashlib
import json
import os
import tempfile
from types import SimpleNamespace

import _episode_bench as EB
import torch

COMMON = ["--tiny", "true", "--use_proprio", "True", "--max_steps", "4", "--wandb_log_freq", "1", "--learning_rate", "1e-3", "--lr_warmup_steps", "8",
          "--seed", "5", "--log_state_digest", "True", "--save_freq", "3", "--run_root_dir", "runs"]
ADAPTER = ["--use_fz", "True", "--batch_size", "2"]
LORA = ["--use_lora", "True", "--lora_rank", "8", "--batch_size", "2"]
EPISODES = ADAPTER + ["--conservative_rows", "true", "--max_seq_len", "128"]       # prompts of 27-51 ids: the action block moves
STATE = ADAPTER + ["--save_train_state", "True", "--save_freq", "2"]
CASES = {
    "adapter_captured": ADAPTER + ["--use_graph", "true"],
    "adapter_eager": ADAPTER + ["--use_graph", "false"],
    "lora_captured_dropout_clip": LORA + ["--use_graph", "true", "--lora_dropout", "0.1", "--max_grad_norm", "1.0"],
    "full_eager_accumulation": ["--batch_size", "2", "--use_graph", "false", "--grad_accumulation_steps", "2"],
    "token_ce": LORA + ["--objective", "token_ce"],
    "jpeg_episodes_heldout": EPISODES + ["--episode_file", "data/jpeg.pt", "--verify_frames", "True", "--use_val_set", "True",
                                         "--val_episode_fraction", "0.25", "--val_freq", "2"],
    "episode_mix": EPISODES + ["--episode_mix", "data/suite_a.pt=1.0,data/suite_b.pt=0.5"],
    "frame_files_validation": ADAPTER + ["--batch_size", "3", "--frame_batch_file", "data/frames", "--max_seq_len", "96", "--use_val_set", "True",
                                         "--val_batch_file", "data/val", "--val_freq", "2"],
    "save_state": STATE,
    "resume_state": STATE + ["--resume", "True", "--resume_step", "2", "--resum_vla_path", "runs/save_state--2_chkpt", "--resume_train_state", "True",
                             "--run_root_dir", "runs_resumed"],
}


def write_inputs():
    """The toy inputs under data/ of the working directory."""
    from pack_episodes_jpeg import pack
    from vla_adapter_amd import engine as E, synthetic as S
    mcfg = E.NAMED_CONFIGS["tiny"]()
    os.makedirs("data")
    rng, g = EB.generators()
    shape = SimpleNamespace(episodes=6, episode_len=12, n_img=1)
    for name in ("suite_a", "suite_b"):
        torch.save(dict(EB.synthetic_episodes(mcfg, shape, rng, g), dataset_name=name), f"data/{name}.pt")
    d = dict(EB.synthetic_episodes(mcfg, shape, rng, g), dataset_name="jpeg")
    d["frames_u8"] = torch.randint(0, 256, (d["frames_u8"].shape[0], 1, 48, 64, 3), generator=g, dtype=torch.uint8)   # (JPEG: sides in 16s)
    torch.save(pack(d), "data/jpeg.pt")
    for name, seed0 in (("frames", 100), ("val", 200)):       # frame batches: the collated batch with raw frames for its pixels
        os.makedirs(f"data/{name}")
        for i in range(3):
            b = S.make_batch(mcfg, 3, "cpu", seed=seed0 + i, P=32, ragged=True)
            del b["pixel_values"]
            b["frames_u8"] = torch.randint(0, 256, (3, 1, mcfg.vit[0].img, mcfg.vit[0].img, 3), generator=g, dtype=torch.uint8)
            torch.save(b, f"data/{name}/{i:03d}.pt")


def content_digest(obj, h) -> None:
    """Feeds ``h`` everything a loaded checkpoint file holds: containers in key order, tensors with dtype, shape and bytes."""
    if isinstance(obj, torch.Tensor):
        h.update(f"{obj.dtype}{tuple(obj.shape)}".encode())
        h.update(obj.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            h.update(f"{k}:".encode())
            content_digest(obj[k], h)
    elif isinstance(obj, (list, tuple)):
        for x in obj:
            content_digest(x, h)
    else:
        h.update(repr(obj).encode())


def file_record(path: str) -> dict:
    rec = dict(sha256=hashlib.sha256(open(path, "rb").read()).hexdigest())
    if path.endswith((".pt", ".safetensors")):
        from safetensors.torch import load_file
        h = hashlib.sha256()
        content_digest(torch.load(path, weights_only=True) if path.endswith(".pt") else load_file(path), h)
        rec["content_sha256"] = h.hexdigest()
    return rec


def record() -> dict:
    from vla_adapter_amd import finetune as F
    write_inputs()
    out = {}
    for name, flags in CASES.items():
        res = F.finetune(F.parse_args(COMMON + ["--run_id_override", name] + flags))
        root = os.path.dirname(res["run_dir"])
        files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if os.path.relpath(d, root).startswith(name + "--"))
        assert files, f"{name}: the run left no file under {root}"
        out[name] = dict(log=res["log"], val_log=res["val_log"], heldout=res.get("heldout"), mixture=res.get("mixture"),
                         files={os.path.relpath(f, root): file_record(f) for f in files})
        print(json.dumps(dict(case=name, steps=res["steps"], final_step=res["final_step"], files=len(files))), flush=True)
    return out


def compare(a: dict, b: dict) -> dict:
    """identical: every case's log, val_log, info and file list are equal and every file has the same bytes - or, where only the bytes
    differ, the same content (those files are named under by_content)."""
    differing, by_content = [], []
    for name in sorted(set(a["cases"]) | set(b["cases"])):
        x, y = a["cases"].get(name, {}), b["cases"].get(name, {})
        differing += [f"{name}.{k}" for k in ("log", "val_log", "heldout", "mixture") if x.get(k, "<absent>") != y.get(k, "<absent>")]
        fx, fy = x.get("files", {}), y.get("files", {})
        for f in sorted(set(fx) | set(fy)):
            if fx.get(f) == fy.get(f):
                continue
            same = f in fx and f in fy and "content_sha256" in fx[f] and fx[f]["content_sha256"] == fy[f].get("content_sha256")
            (by_content if same else differing).append(f"{name}.files.{f}")
    return dict(identical=not differing, cases=sorted(a["cases"]), labels=[a.get("label"), b.get("label")], differing=differing, by_content=by_content)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="where the record is written")
    ap.add_argument("--label", default=None, help="recorded as it is: the commit the driver is of")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        print(json.dumps(compare(*(json.load(open(p)) for p in args.compare))), flush=True)
        return
    assert args.out, "--out or --compare"
    assert torch.cuda.is_available(), "finetune_trajectory needs a GPU"
    out = os.path.abspath(args.out)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        cases = record()
        os.chdir(EB.ROOT)
    json.dump(dict(label=args.label, device=torch.cuda.get_device_name(0), cases=cases), open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
