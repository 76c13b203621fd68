#!/usr/bin/env python3
"""SHA-256 of the output of every GEMM kernel id under every epilogue it accepts, for comparing two builds of the native library
bit for bit.  Run it once per library, each in a fresh process, in ONE job on one machine, and diff the two outputs:

    python tools/epilogue_digest.py > branch.txt
    VLA_NATIVE_LIB=/path/to/parent/libvla_native.so python tools/epilogue_digest.py > parent.txt

A combination the library refuses prints the refusal instead of a digest (the same line for both builds).
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vla_adapter_amd import ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16


def gen(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is not None:
            h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:24]


def emit(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        print(name, sha(*(out if isinstance(out, tuple) else (out,))), flush=True)
    except Exception as e:  # a refusal of the host-side checks: the same for both builds
        print(name, "REFUSED", str(e).splitlines()[0][:100], flush=True)


def nt_epilogues(M, N, K, seed):
    """name -> callable for every epilogue of vla_gemm_bf16_nt on an [M, K] x [N, K] product."""
    a, w, bias, res = gen(M, K, seed=seed), gen(N, K, seed=seed + 1, scale=0.1), gen(N, seed=seed + 2), gen(M, N, seed=seed + 3)
    S = 50 if M % 50 == 0 else 32
    cos1, sin1 = ops.rope_half_tables(S, 64, 1e6, DEV)
    cos2, sin2 = ops.rope_inter_tables(S + 3, 16, DEV)
    big = gen(2 * M, N, seed=seed + 4)
    a2, b2 = gen(M, 64, seed=seed + 5), gen(N, 64, seed=seed + 6, scale=0.1)
    aq, asc = ops.quant_fp8_rows(a)
    wq, wsc = ops.quant_fp8_rows(w)
    g = M // 2
    cases = {
        "plain": lambda: ops.gemm_nt(a, w),
        "alpha": lambda: ops.gemm_nt(a, w, alpha=0.37),
        "bias": lambda: ops.gemm_nt(a, w, bias=bias),
        "bias_post": lambda: ops.gemm_nt(a, w, bias=bias, bias_post_round=True),
        "gelu": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_GELU),
        "relu": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_RELU),
        "gelu_tanh": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_GELU_TANH),
        "residual": lambda: ops.gemm_nt(a, w, bias=bias, residual=res),
        "gelu_residual": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_GELU, residual=res),
        "res_mod": lambda: ops.gemm_nt(a, w, residual=res[:S], res_mod=S),
        "r_group": lambda: ops.gemm_nt(a, w, residual=big[g // 2:], r_group=(g, 2 * g * N)),
        "c_group": lambda: (lambda o: (ops.gemm_nt(a, w, out=o[:M], c_group=(g, (g + 8) * N)), o)[1])(torch.zeros(M + 16, N, dtype=BF, device=DEV)),
        "c_live": lambda: ops.gemm_nt(a, w, bias=bias, out=torch.full((M, N), 7.0, dtype=BF, device=DEV), c_live=(S, S // 3)),
        "rope_half": lambda: ops.gemm_nt(a, w, bias=bias, rope=(1, cos1, sin1, S, 64, N // 2)),
        "rope_inter": lambda: ops.gemm_nt(a, w, bias=bias, rope=(2, cos2, sin2, S, 16, N // 2)),
        "rope_inter_post": lambda: ops.gemm_nt(a, w, bias=bias, bias_post_round=True, rope=(2, cos2, sin2, S, 16, N // 2)),
        "swiglu": lambda: ops.gemm_nt(a, w, act=ops.ACT_SWIGLU),
        "swiglu_bias_live": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_SWIGLU, out=torch.full((M, N), 3.0, dtype=BF, device=DEV),
                                                c_live=(S * 2, S)),
        "ext": lambda: ops.gemm_nt(a, w, bias=bias, residual=res, ext=(a2, b2)),
        "ext_swiglu": lambda: ops.gemm_nt(a, w, act=ops.ACT_SWIGLU, ext=(a2, b2)),
        "fp8": lambda: ops.gemm_nt(aq, wq, bias=bias, residual=res, fp8=(asc, wsc)),
        "fp8_swiglu": lambda: ops.gemm_nt(aq, wq, act=ops.ACT_SWIGLU, fp8=(asc, wsc)),
        "fp8_ext": lambda: ops.gemm_nt(aq, wq, bias=bias, fp8=(asc, wsc), ext=(a2, b2)),
        "split_k": lambda: ops.gemm_nt(a, w, bias=bias, act=ops.ACT_GELU, residual=res, split_k=2),
        "split_k_plain": lambda: ops.gemm_nt(a, w, split_k=2),
    }
    return cases


def main():
    torch.manual_seed(0)
    print("# library:", os.environ.get("VLA_NATIVE_LIB", "(the tree's own)"), flush=True)
    # (label, environment, latency hint, M, N, K): the shapes of the cross-kernel bit-identity tests - every kernel id is hit
    sweeps = [
        ("skinny_tall", {}, False, 4000, 64, 1024),
        ("skinny_short", {}, False, 96, 512, 1024),
        ("nt128x128", {"VLA_GEMM_TILE": "2"}, False, 300, 384, 512),
        ("nt128x128_ragged", {"VLA_GEMM_TILE": "2"}, False, 300, 392, 512),
        ("nt128x64", {"VLA_GEMM_TILE": "3"}, False, 300, 192, 512),
        ("nt256", {"VLA_GEMM_TILE": "6"}, False, 600, 768, 512),
        ("nt256_ragged", {"VLA_GEMM_TILE": "6"}, False, 500, 904, 512),
        ("hint_deep_ring", {"VLA_NO_SKINNY": "1"}, True, 300, 512, 1024),
        ("hint_small", {"VLA_NO_SKINNY": "1"}, True, 64, 896, 1024),
        ("auto_large", {}, False, 2048, 1792, 896),
    ]
    for label, env, hint, M, N, K in sweeps:
        for k in ("VLA_GEMM_TILE", "VLA_NO_SKINNY"):
            os.environ.pop(k, None)
        os.environ.update(env)
        for name, fn in nt_epilogues(M, N, K, seed=1000 + 7 * M + N).items():
            if hint:
                def run(fn=fn):
                    with ops.latency_hint():
                        return fn()
                emit(f"{label}/{name}", run)
            else:
                emit(f"{label}/{name}", fn)
    for k in ("VLA_GEMM_TILE", "VLA_NO_SKINNY"):
        os.environ.pop(k, None)
    # SwiGLU backward fused into the dH product (128-row and 256-row kernels), with a row-group window and a K extension
    for label, tile, M, D, I in (("swiglu_bwd128", "2", 300, 256, 192), ("swiglu_bwd256", "6", 600, 256, 512)):
        os.environ["VLA_GEMM_TILE"] = tile
        d, wt, gu = gen(M, D, seed=50), gen(I, D, seed=51, scale=0.1), gen(M, 2 * I, seed=52)
        gbig = gen(2 * M, 2 * I, seed=53)
        emit(f"{label}/plain", lambda: ops.gemm_swiglu_bwd(d, wt, gu))
        emit(f"{label}/gu_group", lambda: ops.gemm_swiglu_bwd(d, wt, gbig[M // 4:], gu_group=(M // 2, M * 2 * I)))
        emit(f"{label}/ext", lambda: ops.gemm_swiglu_bwd(d, wt, gu, ext=(gen(M, 64, seed=54), gen(I, 64, seed=55, scale=0.1))))
    os.environ.pop("VLA_GEMM_TILE", None)
    # TN (weight-gradient) products: 128 and 256 tiles, accumulate, contraction split
    for tile in ("128", "256"):
        os.environ["VLA_TN_TILE"] = tile
        a, b = gen(1100, 256, seed=60), gen(1100, 384, seed=61)
        c0 = gen(256, 384, seed=62)
        emit(f"tn{tile}/plain", lambda: ops.gemm_tn(a, b, alpha=0.5))
        emit(f"tn{tile}/accumulate", lambda: ops.gemm_tn(a, b, out=c0.clone(), accumulate=True))
        emit(f"tn{tile}/split", lambda: ops.gemm_tn(a, b, split=4))
        emit(f"tn{tile}/split_accumulate", lambda: ops.gemm_tn(a, b, out=c0.clone(), accumulate=True, split=4))
    os.environ.pop("VLA_TN_TILE", None)
    gu, dh = gen(333, 2 * 192, seed=70), gen(333, 192, seed=71)
    emit("swiglu_fwd", lambda: ops.swiglu_fwd(gu))
    emit("swiglu_bwd", lambda: ops.swiglu_bwd(dh, gu))


if __name__ == "__main__":
    main()
