"""Two-rank run of finetune() with --use_val_set on ONE GPU (collectives through gloo), for tests/test_validation_gpu.py:
launched with torch.distributed.run --nproc-per-node 2.  Every rank trains the captured adapter step on the same batch list
twice - with a validation sweep every second step and without - and writes both logs and its val_log to <out>/rank<r>.json.
The sweeps run without any collective: each rank validates on its own, from its own offset into the held-out batches."""
import json
import os
import sys

sys.path.insert(0, ".")
os.environ.setdefault("VLA_DIST_BACKEND", "gloo")
os.environ["LOCAL_RANK"] = "0"                  # both ranks share the one GPU (gloo needs no device per rank)

from vla_adapter_amd import engine as E, finetune as F, synthetic as S  # noqa: E402


def batches(n, seed0, L):
    cfg, pad = E.tiny_config(), min(S.PAD_ID, E.tiny_config().llm.vocab - 1)
    return [F.pad_to(S.make_batch(cfg, 4, "cuda:0", seed=seed0 + i, P=32, ragged=True), L, pad) for i in range(n)]


def main(out_dir: str, L: int):
    rank = int(os.environ["RANK"])
    train, val = batches(3, 700, L), batches(3, 720, L)
    base = ["--tiny", "true", "--batch_size", "4", "--max_steps", "4", "--learning_rate", "1e-3", "--wandb_log_freq", "1", "--phase", "Training",
            "--use_proprio", "True", "--use_fz", "True", "--max_seq_len", str(L), "--run_id_override", "r"]
    a = F.finetune(F.parse_args(base + ["--save_freq", "2", "--run_root_dir", os.path.join(out_dir, "val"), "--use_val_set", "True", "--val_freq", "2"]),
                   batches=train, val_batches=val)
    b = F.finetune(F.parse_args(base + ["--save_freq", "1000", "--run_root_dir", os.path.join(out_dir, "plain")]), batches=train)
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(log=a["log"], val_log=a["val_log"], plain_log=b["log"], world=a["world"]), f)
    print(f"validation-two-ranks-ok rank {rank}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
