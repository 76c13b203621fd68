"""Two-rank run of finetune() with --val_episode_fraction on ONE GPU (collectives through gloo), for tests/test_heldout_gpu.py:
launched with torch.distributed.run --nproc-per-node 2 and the finetune() arguments behind the output directory.  Every rank writes
its val_log and the run's held-out record to <out>/rank<r>.json.  The ranks share the sweep batch by batch and merge their sums in one
all-reduce, so both must report the same entry."""
import json
import os
import sys

sys.path.insert(0, ".")
os.environ.setdefault("VLA_DIST_BACKEND", "gloo")
os.environ["LOCAL_RANK"] = "0"                  # both ranks share the one GPU (gloo needs no device per rank)

from vla_adapter_amd import finetune as F  # noqa: E402


def main(out_dir: str, argv):
    rank = int(os.environ["RANK"])
    out = F.finetune(F.parse_args(list(argv) + ["--run_root_dir", os.path.join(out_dir, f"run{rank}")]))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(val_log=out["val_log"], heldout=out["heldout"], world=out["world"]), f)
    print(f"heldout-two-ranks-ok rank {rank}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
