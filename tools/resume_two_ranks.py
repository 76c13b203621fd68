"""Two-rank run of finetune() on ONE GPU (collectives through gloo), for tests/test_resume_state_gpu.py: launched with
torch.distributed.run --nproc-per-node 2 and the finetune() arguments behind the output directory.  Rank 0 writes the checkpoints and
their train_state files under <out>/run0; every rank writes its log to <out>/rank<r>.json and its flat data / m / v buffers as they stand
behind the last step to <out>/rank<r>_flat.pt.  A resumed launch passes --resum_vla_path of an earlier launch's run0: both ranks read
the one state file rank 0 wrote."""
import json
import os
import sys

sys.path.insert(0, ".")
os.environ.setdefault("VLA_DIST_BACKEND", "gloo")
os.environ["LOCAL_RANK"] = "0"                  # both ranks share the one GPU (gloo needs no device per rank)

import torch  # noqa: E402

from vla_adapter_amd import finetune as F  # noqa: E402
from vla_adapter_amd import train_state as TS  # noqa: E402


def main(out_dir: str, argv):
    rank = int(os.environ["RANK"])
    flat = {}

    def grab(eng, trainer):
        for name, P in (trainer or eng)._state_buffers():
            for part in TS.PARTS:
                flat[f"{name}.{part}"] = getattr(P, part).detach().cpu().clone()
    out = F.finetune(F.parse_args(list(argv) + ["--run_root_dir", os.path.join(out_dir, f"run{rank}")]), on_finish=grab)
    torch.save(flat, os.path.join(out_dir, f"rank{rank}_flat.pt"))
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(log=out["log"], world=out["world"], final_step=out["final_step"]), f)
    print(f"resume-two-ranks-ok rank {rank}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
