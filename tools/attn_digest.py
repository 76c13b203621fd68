#!/usr/bin/env python3
"""SHA-256 of what the flash attention kernels (csrc/attention.hip) write - o and lse of the forward without and with the latency hint
(head dims 64 and 72: the key-split kernel where it accepts the shape), dq, dk, dv and delta of the backward plain, through the fused
inverse RoPE and as the live-row backward (row0 > 0) - for comparing two builds of the native library bit for bit.  Run it once per
library, each in a fresh process, in ONE job on one machine, and diff the two outputs:

    python tools/attn_digest.py > branch.txt
    VLA_NATIVE_LIB=/path/to/parent/libvla_native.so python tools/attn_digest.py > parent.txt

A combination the library refuses prints the refusal instead of a digest (the same line for both builds).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench_attn import STEP_SHAPES  # noqa: E402
from epilogue_digest import DEV, gen, sha  # noqa: E402
from vla_adapter_amd import ops  # noqa: E402

MASKS = {
    "none": lambda B, S: None,
    "trailing": lambda B, S: (torch.arange(S)[None].expand(B, S) < max(S - 9, 1)).contiguous(),
    "isolated": lambda B, S: (torch.arange(S) != min(31, S - 1))[None].expand(B, S).contiguous(),        # one key out, alone in its tile
    # sample 0: the second half of its keys masked; the last sample (B > 1): every key masked
    "half": lambda B, S: torch.stack([torch.arange(S) < (S + 1) // 2] + [torch.ones(S, dtype=torch.bool)] * (B - 2)
                                     + [torch.zeros(S, dtype=torch.bool)] * (B > 1)),
}
# B, S, Hq, Hkv, dh, causal, mask: every instantiation (dh 64, 72, 112 forward only, 128), GQA groups 1, 2, 3, 7 and 8 (dK/dV: 1, 2
# and 4 key tiles per workgroup, 3 to 8 waves), causal and not, every mask, S below / at / off the 32-key tile and the 128-query block
SHAPES = [
    (1, 1, 2, 1, 64, True, "none"), (2, 33, 2, 2, 64, False, "half"), (2, 77, 4, 2, 64, True, "trailing"), (1, 70, 6, 2, 64, True, "isolated"),
    (1, 129, 14, 2, 64, True, "trailing"), (1, 40, 8, 1, 64, False, "isolated"), (2, 261, 2, 2, 64, False, "none"), (1, 352, 14, 2, 64, True, "half"),
    (2, 65, 4, 4, 72, True, "half"), (2, 65, 4, 2, 72, True, "trailing"), (1, 127, 7, 7, 72, False, "isolated"), (2, 100, 2, 2, 72, False, "none"),
    (1, 256, 16, 16, 72, False, "trailing"), (2, 32, 7, 1, 112, False, "isolated"), (1, 127, 7, 7, 112, True, "trailing"),
    (2, 100, 4, 2, 112, False, "half"), (1, 33, 2, 2, 128, True, "none"), (2, 32, 7, 1, 128, False, "isolated"), (1, 161, 12, 2, 128, True, "trailing"),
    (2, 77, 4, 2, 128, True, "half"), (2, 369, 2, 1, 128, False, "none"),
] + [(B, S, Hq, Hkv, dh, causal, "none") for _, B, S, Hq, Hkv, dh, causal in STEP_SHAPES]


def emit(name, fn):
    try:
        outs = fn()
        torch.cuda.synchronize()
        for part, ts in outs:
            print(f"{name}/{part}", sha(*ts), flush=True)
    except Exception as e:  # a refusal of the host-side checks: the same for both builds
        print(name, "REFUSED", str(e).splitlines()[0][:100], flush=True)


def main():
    print("# library:", os.environ.get("VLA_NATIVE_LIB", "(the tree's own)"), flush=True)
    for B, S, Hq, Hkv, dh, causal, mask in SHAPES:
        tag = f"B{B}_S{S}_H{Hq}:{Hkv}_dh{dh}_{'causal' if causal else 'full'}_{mask}"
        W = (Hq + 2 * Hkv) * dh
        qkv, dout = gen(B, S, W, seed=70, scale=0.5), gen(B, S, Hq * dh, seed=71)
        cut = lambda t, r0=0: (t[:, r0:, :Hq * dh], t[:, r0:, Hq * dh:(Hq + Hkv) * dh], t[:, r0:, (Hq + Hkv) * dh:])
        q, k, v = cut(qkv)
        km = MASKS[mask](B, S)
        kmd = km.to(torch.uint8).to(DEV) if km is not None else None

        def fwd(hint):
            o, lse = torch.zeros(B, S, Hq * dh, dtype=qkv.dtype, device=DEV), torch.zeros(B, Hq, S, device=DEV)
            if hint:
                with ops.latency_hint():
                    ops.attn_fwd(q, k, v, Hq, Hkv, dh, causal, kmd, want_lse=True, out=o, lse=lse)
            else:
                ops.attn_fwd(q, k, v, Hq, Hkv, dh, causal, kmd, want_lse=True, out=o, lse=lse)
            return o, lse

        o, lse = fwd(False)
        emit(f"{tag}/fwd", lambda: [("o", (o,)), ("lse", (lse,))])
        if dh in (64, 72):
            emit(f"{tag}/fwd_hint", lambda: [(n, (t,)) for n, t in zip(("o", "lse"), fwd(True))])
        if dh == 112:
            continue
        row0 = (S // 2) // 32 * 32
        for kind in ("plain", "rope", "row0"):
            if kind == "row0" and not (causal and row0 > 0):
                continue

            def bwd(kind=kind):
                r0 = row0 if kind == "row0" else 0
                g = torch.zeros(B, S - r0, W, dtype=qkv.dtype, device=DEV)
                delta = torch.zeros(B, Hq, S - r0, device=DEV)
                rope = ops.rope_half_tables(S, dh, 1e6, DEV) if kind == "rope" or (kind == "row0" and dh != 72) else None
                dq, dk, dv = cut(g)
                ops.attn_bwd(dout[:, r0:], cut(qkv, r0)[0], k, v, o[:, r0:], lse, Hq, Hkv, dh, causal, kmd, dq=dq, dk=dk, dv=dv, rope=rope,
                             row0=r0, delta=delta)
                return [("dq", (dq,)), ("dk", (dk,)), ("dv", (dv,)), ("delta", (delta,))]
            emit(f"{tag}/bwd_{kind}", bwd)


if __name__ == "__main__":
    main()
