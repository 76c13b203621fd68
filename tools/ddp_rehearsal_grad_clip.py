"""Functional rehearsal of --max_grad_norm under data parallelism on ONE GPU (gloo: RCCL refuses two ranks per device), launched
with torch.distributed.run --nproc-per-node 2.  VLA_TRAINER=full|lora|adapter, VLA_CAPTURED=1 for the segment-graph replay.
Every rank takes the norm of the same averaged gradients, each range behind its own collectives, so no collective is added:
the ranks must report the same grad_norm bit for bit on every step, clip (coefficient below 1), and end with identical parameters.
The norm must also be the fp64 norm of the exchanged gradient buffers scaled by 1 / world."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, ".")
os.environ.setdefault("VLA_DIST_BACKEND", "gloo")
from vla_adapter_amd import ddp, engine as E, synthetic as S  # noqa: E402
from vla_adapter_amd.trainers import FullFinetune, LoRAFinetune  # noqa: E402


def log(*a):
    sys.stdout.write(f"[rank {os.environ.get('RANK')}] " + " ".join(str(x) for x in a) + "\n")
    sys.stdout.flush()


rank, local, world = ddp.init_process_group_from_env()
torch.cuda.set_device(0)
dev, mode, captured = "cuda:0", os.environ.get("VLA_TRAINER", "full"), bool(int(os.environ.get("VLA_CAPTURED", "0")))
cfg = E.tiny_fused_config() if mode != "adapter" else E.tiny_config()
eng = E.VLAEngine(cfg, S.make_weights(cfg, dev, seed=3, std=0.05), dev)
tr = None if mode == "adapter" else FullFinetune(eng) if mode == "full" else LoRAFinetune(eng, rank=8, seed=5)
if mode == "lora":               # B = 0 at init: give both halves of every pair a gradient from step 1
    gen = torch.Generator(device=dev).manual_seed(9)
    for l in tr.L.values():
        for p, _ in l.projs:
            Bv = tr.P.view(f"{l.name}.{p}.lora_B")
            Bv[:l.n_real, :l.r] = (torch.randn(min(l.n_real, Bv.shape[0]), l.r, generator=gen, device=dev) * 0.02).to(torch.bfloat16)
    tr.refresh()
eng.reducer = ddp.FlatGradReducer(bucket_bytes=1 << 16, algo=os.environ.get("VLA_DDP_ALGO", "allreduce"))
model = tr or eng
model.set_max_grad_norm(0.005)
batch = S.make_batch(cfg, 2, dev, seed=100 + rank, P=24)
if captured:
    model.capture(batch, None)
lr, norms = 1e-3, []
for it in range(3):
    model.train_step_graphed(lr) if captured else model.train_step(batch, lr)
    eng.flush()                  # (the captured adapter step leaves its update pending)
    torch.cuda.synchronize()
    flats = [eng.head.P.grad] if tr is None else [tr.P.grad[lo:hi] for lo, hi in tr._adam_ranges()] + [eng.head.P.grad]
    want = (sum(((g.float() / world).bfloat16().double().square().sum()) for g in flats)).sqrt().item()
    got, coef = model.grad_norm.item(), model.clip_coef.item()
    log(f"step {it}: grad_norm {got!r} fp64 norm of the averaged gradients {want!r} coef {coef!r}")
    assert abs(got - want) / want <= 1e-5 and 0.0 < coef < 1.0
    norms.append(model.grad_norm.clone())
mine = torch.stack(norms).view(torch.int32)
every = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(every, mine)
assert all(torch.equal(e, mine) for e in every), f"the ranks report different norms: {[e.view(torch.float32).tolist() for e in every]}"
for name, buf in [("head", eng.head.P.data)] + ([("vlm", tr.P.data)] if tr is not None else []):
    p = buf.float()
    ref = p.clone()
    dist.all_reduce(ref)
    err = (p - ref / world).abs().max().item()
    log(f"max |{name} param - mean over ranks| =", err)
    assert err == 0.0, "ranks diverged"
dist.barrier()
dist.destroy_process_group()
log("grad-clip-ranks-in-sync-ok")
