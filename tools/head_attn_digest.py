#!/usr/bin/env python3
"""SHA-256 of what the action-head attention kernels write - (out, probs) of the forward in both softmax modes, the seven gradients
and dgate of the backward with and without the RoPE tables - for comparing two builds of the native library bit for bit.  Run it once
per library, each in a fresh process, in ONE job on one machine, and diff the two outputs:

    python tools/head_attn_digest.py > branch.txt
    VLA_NATIVE_LIB=/path/to/parent/libvla_native.so python tools/head_attn_digest.py > parent.txt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from epilogue_digest import DEV, gen, sha  # noqa: E402
from vla_adapter_amd import ops  # noqa: E402

H = 8
SHAPES = [  # B, T, Ka, Kt, D: T > 16, a ragged last key tile, nineteen key tiles, head dims 16 ... 128; last: the step's shape
    (3, 8, 65, 256, 896), (2, 8, 65, 512, 896), (2, 8, 65, 40, 512), (2, 20, 65, 100, 1024), (5, 8, 65, 16, 128), (1, 32, 33, 7, 256),
    (32, 8, 65, 256, 896)]


def main():
    print("# library:", os.environ.get("VLA_NATIVE_LIB", "(the tree's own)"), flush=True)
    for B, T, Ka, Kt, D in SHAPES:
        tag = f"B{B}_T{T}_Ka{Ka}_Kt{Kt}_D{D}"
        x3, a2, t2 = gen(B, T, 3 * D, seed=60, scale=0.3), gen(B, Ka, 2 * D, seed=61, scale=0.3), gen(B, Kt, 2 * D, seed=62, scale=0.3)
        gate, dout = torch.tensor([0.7]).to(x3.dtype).to(DEV), gen(B, T, D, seed=63)
        args = (x3[:, :, :D], x3[:, :, D:2 * D], x3[:, :, 2 * D:], a2[:, :, :D], a2[:, :, D:], t2[:, :, :D], t2[:, :, D:])
        fwd = {}
        for mode in ("flash", "ref_softmax"):         # (the slab beyond the LSE slots is not written: hashed as the zeros it starts as)
            probs = torch.zeros(B, H, T, T + Ka + Kt, device=DEV)
            fwd[mode] = ops.head_attn_fwd(*args, gate, H, ref_softmax=(mode == "ref_softmax"), probs=probs)
            torch.cuda.synchronize()
            print(f"{tag}/fwd_{mode}", sha(*fwd[mode]), flush=True)
        out, probs = fwd["flash"]
        for rope in (None, ops.rope_inter_tables(max(T, Ka, Kt), D // H, DEV)):
            g3, ga, gt, dg = torch.zeros_like(x3), torch.zeros_like(a2), torch.zeros_like(t2), torch.zeros(1, device=DEV)
            ops.head_attn_bwd(dout, out, *args, gate, probs, dg, g3[:, :, :D], g3[:, :, D:2 * D], g3[:, :, 2 * D:], ga[:, :, :D], ga[:, :, D:],
                              gt[:, :, :D], gt[:, :, D:], H, rope=rope)
            torch.cuda.synchronize()
            name = f"{tag}/bwd_{'rope' if rope else 'plain'}"
            print(f"{name}/dq", sha(g3[:, :, :D]), flush=True)
            print(f"{name}/dk_dv", sha(g3[:, :, D:], ga, gt), flush=True)
            print(f"{name}/dgate", sha(dg), flush=True)


if __name__ == "__main__":
    main()
