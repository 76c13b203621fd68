"""Per-kernel parity: every C-ABI op (called through ctypes) against the CPU oracle on the same seeded inputs.

Tolerances (written per test): outputs are bf16, so one rounding flip is 2^-8 relative; we require
  rel-L2(native, oracle) <= 2e-3   and   max|diff| <= 2^-6 * max|ref|   for single ops with fp32 accumulation,
bit-exact for integer/index work and for AdamW (same op-by-op bf16 rounding as torch).
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vla_oracle as O  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vla_adapter_amd import ops as _ops
    return _ops


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def f(x):
    return x.detach().float().cpu()


def check(native, ref, rel=2e-3, mx=2 ** -6, name=""):
    a, b = f(native), ref.float()
    assert a.shape == b.shape, f"{name}: shape {a.shape} vs {b.shape}"
    assert torch.isfinite(a).all(), f"{name}: non-finite output"
    den = b.norm().item() + 1e-12
    r = (a - b).norm().item() / den
    m = (a - b).abs().max().item()
    assert r <= rel and m <= mx * (b.abs().max().item() + 1e-12) + 1e-6, f"{name}: rel-L2 {r:.3e} (<= {rel}), max|d| {m:.3e}"
    return r


# ------------------------------------------------------------------ layout probes
def test_probe_layouts(ops):
    import ctypes as C
    lib = ops.N.load()
    lib.vla_probe_layouts.argtypes = [C.c_void_p] * 4
    tr = torch.zeros(64 * 4, dtype=torch.int16, device=DEV)
    m32 = torch.zeros(64 * 16, dtype=torch.float32, device=DEV)
    m16 = torch.zeros(64 * 4, dtype=torch.float32, device=DEV)
    rc = lib.vla_probe_layouts(None, C.c_void_p(tr.data_ptr()), C.c_void_p(m32.data_ptr()), C.c_void_p(m16.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    tr = tr.cpu().view(64, 4).numpy()
    for lane in range(64):
        g, i = lane >> 4, lane & 15
        # lane i of group g receives column 16g+i of rows 0..3
        exp = [r * 256 + 16 * g + i for r in range(4)]
        assert tr[lane].tolist() == exp, f"ds_read_b64_tr_b16 lane {lane}: got {tr[lane].tolist()} want {exp}"
    m32 = m32.cpu().view(64, 16).numpy()
    for lane in range(64):
        col, h = lane & 31, lane >> 5
        for reg in range(16):
            row = (reg & 3) + 8 * (reg >> 2) + 4 * h
            exp = (8 * row + (col & 7)) if row < 16 else 0.0     # C = I[32x16] . B
            assert m32[lane, reg] == exp, f"mfma32 lane {lane} reg {reg}: {m32[lane, reg]} want {exp}"
    m16 = m16.cpu().view(64, 4).numpy()
    for lane in range(64):
        col, gq = lane & 15, lane >> 4
        for reg in range(4):
            row = 4 * gq + reg
            assert m16[lane, reg] == 8 * row + (col & 7), f"mfma16 lane {lane} reg {reg}"


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 128), (300, 200, 192), (1000, 896, 896), (64, 7, 128),
                                   (2080, 896, 896)])
def test_gemm_plain_bias(ops, M, N, K):
    a, b, bias = gen(M, K, seed=1), gen(N, K, seed=2, scale=0.05), gen(N, seed=3)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), bias=bias.to(DEV))
    check(out, O.linear(a.float(), b.float(), bias.float(), emu=True), name=f"gemm {M}x{N}x{K}")


@pytest.mark.parametrize("tile", [2, 3, 6])
@pytest.mark.parametrize("M,N,K", [(300, 200, 192), (1000, 896, 896), (512, 384, 64), (2080, 1792, 896), (64, 7, 128)])
def test_gemm_every_tile_config(ops, tile, M, N, K, monkeypatch):
    """The three tile geometries (128x128 8 waves, 128x64 4 waves, 256x256 two-phase) must agree with the oracle on ragged
    edges, K=64 (shorter than the pipeline depth) and long K; VLA_GEMM_TILE forces the choice."""
    monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    a, b, bias, r = gen(M, K, seed=1), gen(N, K, seed=2, scale=0.05), gen(N, seed=3), gen(M, N, seed=4)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), bias=bias.to(DEV), residual=r.to(DEV), act=2)
    y = torch.relu(O.linear(a.float(), b.float(), bias.float(), emu=True))
    check(out, O.rnd(y + r.float(), True), name=f"gemm tile{tile} {M}x{N}x{K}")


@pytest.mark.parametrize("tile", [2, 3, 6])
def test_gemm_swiglu_tile_configs(ops, tile, monkeypatch):
    monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    M, I, K = 330, 320, 256
    x, wg, wu = gen(M, K, seed=12), gen(I, K, seed=13, scale=0.1), gen(I, K, seed=14, scale=0.1)
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K)
    pre, h = ops.gemm_nt(x.to(DEV), w.to(DEV), act=ops.ACT_SWIGLU)
    g, u = O.linear(x.float(), wg.float(), None, True), O.linear(x.float(), wu.float(), None, True)
    check(h, O.rnd(O.rnd(g * torch.sigmoid(g), True) * u, True), name="swiglu h")
    check(pre, torch.stack([g.view(M, I // 16, 16), u.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I), name="swiglu pre")


@pytest.mark.parametrize("act,oact", [(1, "gelu"), (2, "relu"), (3, "gelu_tanh")])
def test_gemm_act_residual(ops, act, oact):
    M, N, K = 520, 256, 256
    a, b, bias, r = gen(M, K, seed=4), gen(N, K, seed=5, scale=0.08), gen(N, seed=6), gen(M, N, seed=7)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), bias=bias.to(DEV), residual=r.to(DEV), act=act)
    y = O.linear(a.float(), b.float(), bias.float(), emu=True)
    y = {"gelu": lambda t: O.gelu(t, True), "relu": lambda t: torch.relu(t), "gelu_tanh": lambda t: O.gelu(t, True, True)}[oact](y)
    check(out, O.rnd(y + r.float(), True), name=f"gemm act {oact}")


def test_gemm_res_mod_and_batched(ops):
    nb, M, N, K = 3, 256, 128, 128
    a, b, pos = gen(nb, M, K, seed=8), gen(N, K, seed=9, scale=0.1), gen(M, N, seed=10)
    # batched A with a shared B and a shared (row-broadcast) residual: the patch-embed + pos_embed pattern
    out = ops.gemm_nt(a.to(DEV).view(nb * M, K), b.to(DEV), residual=pos.to(DEV), res_mod=M)
    ref = O.rnd(O.linear(a.float(), b.float(), None, True) + pos.float(), True).view(nb * M, N)
    check(out, ref, name="gemm res_mod")
    # true batched: per-batch B, output written into a strided window of a larger buffer
    bb = gen(nb, N, K, seed=11, scale=0.1)
    big = torch.zeros(nb, M + 5, N, dtype=BF, device=DEV)
    ops.gemm_nt(a.to(DEV), bb.to(DEV), out=big[:, 1:M + 1])
    ref = torch.stack([O.linear(a[i].float(), bb[i].float(), None, True) for i in range(nb)])
    check(big[:, 1:M + 1], ref, name="gemm batched/strided")
    assert (f(big[:, 0]) == 0).all() and (f(big[:, M + 1:]) == 0).all(), "wrote outside the window"


def test_gemm_swiglu(ops):
    M, I, K = 200, 192, 128
    x, wg, wu = gen(M, K, seed=12), gen(I, K, seed=13, scale=0.1), gen(I, K, seed=14, scale=0.1)
    # interleave rows in groups of 16: [g0..15, u0..15, g16..31, u16..31, ...]
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K)
    pre, h = ops.gemm_nt(x.to(DEV), w.to(DEV), act=ops.ACT_SWIGLU)
    g, u = O.linear(x.float(), wg.float(), None, True), O.linear(x.float(), wu.float(), None, True)
    href = O.rnd(O.rnd(g * torch.sigmoid(g), True) * u, True)
    check(h, href, name="swiglu h")
    pre_ref = torch.stack([g.view(M, I // 16, 16), u.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I)
    check(pre, pre_ref, name="swiglu pre")
    # backward of the elementwise part
    dh = gen(M, I, seed=15)
    dgu = ops.swiglu_bwd(dh.to(DEV), pre)
    gg, uu = f(pre).view(M, I // 16, 2, 16)[:, :, 0].reshape(M, I).requires_grad_(True), f(pre).view(M, I // 16, 2, 16)[:, :, 1].reshape(M, I).requires_grad_(True)
    ((gg * torch.sigmoid(gg)) * uu * dh.float()).sum().backward()
    ref = torch.stack([gg.grad.view(M, I // 16, 16), uu.grad.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I)
    check(dgu, ref, rel=4e-3, name="swiglu bwd")


def test_gemm_rejects_bad_shapes(ops):
    a, b = gen(64, 100).to(DEV), gen(64, 100).to(DEV)       # K % 64 != 0
    with pytest.raises(ops.N.NativeError):
        ops.gemm_nt(a, b)


def test_transpose(ops):
    x = gen(3, 130, 70, seed=16)
    t = ops.transpose(x.to(DEV), ld_out=192)
    assert t.shape == (3, 70, 192)
    assert torch.equal(f(t[:, :, :130]), x.float().transpose(1, 2)) and (f(t[:, :, 130:]) == 0).all()


# ------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,cols,eps", [(37, 1152, 1e-6), (256, 896, 1e-5), (16, 6272, 1e-5), (5, 64, 1e-5),
                                           (9, 10752, 1e-5)])    # 7 x 1536: the 1.5B head's first LayerNorm
def test_layernorm(ops, rows, cols, eps):
    x, w, b, dy = gen(rows, cols, seed=20), (1 + 0.1 * gen(cols, seed=21).float()).to(BF), gen(cols, seed=22, scale=0.1), gen(rows, cols, seed=23)
    y, stats = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), eps, want_stats=True)
    check(y, O.layer_norm(x.float(), w.float(), b.float(), eps, True), name="layernorm fwd")
    xr, wr, br = x.float().requires_grad_(True), w.float().requires_grad_(True), b.float().requires_grad_(True)
    (O.layer_norm(xr, wr, br, eps) * dy.float()).sum().backward()
    dw = torch.zeros(cols, device=DEV)
    db = torch.zeros(cols, device=DEV)
    dx = ops.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), stats, dw, db)
    check(dx, xr.grad, rel=4e-3, name="layernorm dx")
    check(dw, wr.grad, rel=1e-3, mx=1e-2, name="layernorm dw")
    check(db, br.grad, rel=1e-3, mx=1e-2, name="layernorm db")


@pytest.mark.parametrize("rows,cols", [(100, 896), (7, 256), (33, 1536)])
def test_rmsnorm(ops, rows, cols):
    x, w, dy, dres = gen(rows, cols, seed=24), (1 + 0.1 * gen(cols, seed=25).float()).to(BF), gen(rows, cols, seed=26), gen(rows, cols, seed=27)
    y, rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), 1e-6, want_rstd=True)
    check(y, O.rms_norm(x.float(), w.float(), 1e-6, True), name="rmsnorm fwd")
    xr = x.float().requires_grad_(True)
    (O.rms_norm(xr, w.float(), 1e-6) * dy.float()).sum().backward()
    dx = ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), rstd, dres.to(DEV))
    check(dx, xr.grad + dres.float(), rel=4e-3, name="rmsnorm bwd")


# ------------------------------------------------------------------ RoPE
def test_rope_half(ops):
    B, S, H, KV, dh = 2, 40, 4, 2, 64
    qkv = gen(B * S, (H + 2 * KV) * dh, seed=30)
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    buf = qkv.to(DEV).clone()
    ops.rope_half_(buf[:, :H * dh], cos, sin, S, H, dh)
    ops.rope_half_(buf[:, H * dh:(H + KV) * dh], cos, sin, S, KV, dh)
    c, s = O.rope_half_tables(S, dh, 1e6, True)
    q = qkv.float()[:, :H * dh].view(B, S, H, dh).transpose(1, 2)
    k = qkv.float()[:, H * dh:(H + KV) * dh].view(B, S, KV, dh).transpose(1, 2)
    check(buf[:, :H * dh], O.rope_half(q, c, s, True).transpose(1, 2).reshape(B * S, H * dh), rel=1e-3, name="rope q")
    check(buf[:, H * dh:(H + KV) * dh], O.rope_half(k, c, s, True).transpose(1, 2).reshape(B * S, KV * dh), rel=1e-3, name="rope k")
    assert torch.equal(f(buf[:, (H + KV) * dh:]), qkv.float()[:, (H + KV) * dh:]), "v columns must be untouched"
    # backward = inverse rotation: rope(-theta)(rope(theta)(x)) ~ x
    ops.rope_half_(buf[:, :H * dh], cos, sin, S, H, dh, sign=-1)
    check(buf[:, :H * dh], qkv.float()[:, :H * dh], rel=1.5e-2, mx=5e-2, name="rope inverse")


def test_rope_interleaved(ops):
    B, T, H, dh = 3, 21, 8, 112
    x = gen(B * T, H * dh, seed=31)
    cos, sin = ops.rope_inter_tables(T, dh, DEV)
    buf = x.to(DEV).clone()
    ops.rope_inter_(buf, cos, sin, T, H, dh, 0)
    c, s = O.head_rope_tables(T, dh, True)
    xr = x.float().view(B, T, H, dh).transpose(1, 2)
    check(buf, O.head_rope(xr, c, s, True).transpose(1, 2).reshape(B * T, H * dh), rel=1e-3, name="head rope fwd")
    # backward = transpose of the (non-orthogonal) linear map
    dy = gen(B * T, H * dh, seed=32)
    xg = x.float().view(B, T, H, dh).transpose(1, 2).clone().requires_grad_(True)
    (O.head_rope(xg, c, s) * dy.float().view(B, T, H, dh).transpose(1, 2)).sum().backward()
    g = dy.to(DEV).clone()
    ops.rope_inter_(g, cos, sin, T, H, dh, 1)
    check(g, xg.grad.transpose(1, 2).reshape(B * T, H * dh), rel=3e-3, name="head rope bwd")


# ------------------------------------------------------------------ attention
def _attn_inputs(B, S, Hq, Hkv, dh, seed):
    W = (Hq + 2 * Hkv) * dh
    qkv = gen(B, S, W, seed=seed)
    return qkv, qkv[:, :, :Hq * dh], qkv[:, :, Hq * dh:(Hq + Hkv) * dh], qkv[:, :, (Hq + Hkv) * dh:]


@pytest.mark.parametrize("B,S,Hq,Hkv,dh,causal,masked", [
    (2, 128, 2, 2, 64, False, False), (2, 77, 4, 2, 64, True, True), (1, 352, 14, 2, 64, True, True),
    (2, 256, 2, 2, 72, False, False), (2, 100, 2, 1, 112, False, True), (1, 70, 2, 2, 128, True, False),
    (2, 261, 4, 4, 64, False, False)])
def test_attention_fwd(ops, B, S, Hq, Hkv, dh, causal, masked):
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 40)
    km = torch.ones(B, S, dtype=torch.bool)
    if masked:
        km[0, S - 9:] = False
        if B > 1:
            km[1, S // 2:] = False
    d = qkv.to(DEV)
    W = d.shape[-1]
    o, lse = ops.attn_fwd(d[:, :, :Hq * dh], d[:, :, Hq * dh:(Hq + Hkv) * dh], d[:, :, (Hq + Hkv) * dh:], Hq, Hkv, dh,
                          causal, km.to(torch.uint8).to(DEV) if masked else None, want_lse=True)
    hd = lambda t, h: t.float().reshape(B, S, h, dh).transpose(1, 2)
    ref = O.attention(hd(q, Hq), hd(k, Hkv), hd(v, Hkv), causal, km if masked else None, None, True)
    check(o, ref.transpose(1, 2).reshape(B, S, Hq * dh), rel=6e-3, mx=3e-2, name=f"attn fwd dh{dh}")
    # log-sum-exp against fp32
    kk, vv = hd(k, Hkv).repeat_interleave(Hq // Hkv, 1), None
    s = (hd(q, Hq) @ kk.transpose(-1, -2)) * dh ** -0.5
    allow = (torch.tril(torch.ones(S, S, dtype=torch.bool)) if causal else torch.ones(S, S, dtype=torch.bool))[None, None] & km[:, None, None, :]
    check(lse, torch.logsumexp(s.masked_fill(~allow, float("-inf")), -1), rel=1e-4, mx=1e-3, name="lse")


@pytest.mark.parametrize("B,S,Hq,Hkv,dh,causal,masked", [(1, 369, 14, 2, 64, True, True), (1, 369, 14, 2, 64, True, False), (1, 256, 16, 16, 72, False, False),
                                                         (1, 40, 4, 2, 64, True, False), (2, 100, 2, 2, 64, False, True), (1, 33, 2, 1, 72, True, True),
                                                         (1, 625, 14, 2, 64, True, True)])
def test_attention_fwd_keys_split_over_the_waves(ops, B, S, Hq, Hkv, dh, causal, masked):
    """attn_fwd_split_kernel (round 4, the batch-1 pass under the latency hint): 32-query workgroups whose four waves take every fourth key
    tile, partial (max, sum, O) merged in LDS.  Against the oracle's attention and fp32 log-sum-exp (the criteria of test_attention_fwd),
    and against the one-wave-per-query-tile kernel: the same masks, scale and P rounding, another association of the partial sums."""
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 44)
    km = torch.ones(B, S, dtype=torch.bool)
    if masked:
        km[0, S - 9:] = False
        km[0, 5] = False
        if B > 1:
            km[1, S // 2:] = False
    d = qkv.to(DEV)
    a, b = Hq * dh, (Hq + Hkv) * dh
    kmd = km.to(torch.uint8).to(DEV) if masked else None
    ref_o, ref_lse = ops.attn_fwd(d[:, :, :a], d[:, :, a:b], d[:, :, b:], Hq, Hkv, dh, causal, kmd, want_lse=True)
    with ops.latency_hint():
        o, lse = ops.attn_fwd(d[:, :, :a], d[:, :, a:b], d[:, :, b:], Hq, Hkv, dh, causal, kmd, want_lse=True)
    hd = lambda t, h: t.float().reshape(B, S, h, dh).transpose(1, 2)
    ref = O.attention(hd(q, Hq), hd(k, Hkv), hd(v, Hkv), causal, km if masked else None, None, True)
    valid = torch.ones(B, S, dtype=torch.bool)
    if causal and masked:            # a query whose every visible key is masked has no defined output
        for bb in range(B):
            for i in range(S):
                valid[bb, i] = bool(km[bb, :i + 1].any())
    check(o.float().cpu()[valid], ref.transpose(1, 2).reshape(B, S, Hq * dh)[valid], rel=6e-3, mx=3e-2, name=f"split-key attn fwd dh{dh}")
    dd = (o.float() - ref_o.float()).abs().cpu()[valid]
    # (about a third of the outputs move by one bf16 ulp: the two kernels round the same fp32 sums taken in another order)
    assert dd.max().item() <= 2 ** -6 * ref_o.float().abs().max().item() and (dd > 0).float().mean().item() < 0.5, (dd.max().item(), (dd > 0).float().mean().item())
    vm = valid[:, None, :].expand(B, Hq, S)
    assert torch.allclose(lse.cpu()[vm], ref_lse.cpu()[vm], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("B,S,Hq,Hkv,dh,causal,masked", [(2, 96, 2, 2, 64, False, False), (2, 77, 4, 2, 64, True, True),
                                                       (1, 352, 14, 2, 64, True, True), (1, 100, 2, 2, 72, False, False),
                                                       (1, 352, 12, 2, 128, True, True),      # Qwen2.5-1.5B head geometry
                                                       (2, 65, 4, 2, 72, True, True),         # dh 72 with a GQA group: pad columns in the group sum
                                                       (1, 33, 2, 2, 128, True, False)])      # dh 128, group 1: four key tiles' K / V LDS images
def test_attention_bwd(ops, B, S, Hq, Hkv, dh, causal, masked):
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 41)
    dout = gen(B, S, Hq * dh, seed=42)
    km = torch.ones(B, S, dtype=torch.bool)
    if masked:
        km[0, S - 9:] = False
    d = qkv.to(DEV)
    qd, kd, vd = d[:, :, :Hq * dh], d[:, :, Hq * dh:(Hq + Hkv) * dh], d[:, :, (Hq + Hkv) * dh:]
    kmd = km.to(torch.uint8).to(DEV) if masked else None
    o, lse = ops.attn_fwd(qd, kd, vd, Hq, Hkv, dh, causal, kmd, want_lse=True)
    dqkv = torch.zeros_like(d)
    ops.attn_bwd(dout.to(DEV), qd, kd, vd, o, lse, Hq, Hkv, dh, causal, kmd,
                 dq=dqkv[:, :, :Hq * dh], dk=dqkv[:, :, Hq * dh:(Hq + Hkv) * dh], dv=dqkv[:, :, (Hq + Hkv) * dh:])
    hd = lambda t, h: t.float().reshape(B, S, h, dh).transpose(1, 2)
    qr, kr, vr = (hd(t, h).clone().requires_grad_(True) for t, h in ((q, Hq), (k, Hkv), (v, Hkv)))
    ref = O.attention(qr, kr, vr, causal, km if masked else None)
    (ref * hd(dout, Hq)).sum().backward()
    un = lambda t, h: t.transpose(1, 2).reshape(B, S, h * dh)
    check(dqkv[:, :, :Hq * dh], un(qr.grad, Hq), rel=1e-2, mx=5e-2, name="dq")
    check(dqkv[:, :, Hq * dh:(Hq + Hkv) * dh], un(kr.grad, Hkv), rel=1e-2, mx=5e-2, name="dk")
    check(dqkv[:, :, (Hq + Hkv) * dh:], un(vr.grad, Hkv), rel=1e-2, mx=5e-2, name="dv")


# ------------------------------------------------------------------ action-head attention
@pytest.mark.parametrize("B,Ka,Kt,D", [(2, 65, 256, 896), (3, 65, 24, 64), (1, 65, 512, 896), (2, 65, 40, 512), (5, 65, 16, 128),
                                       (3, 65, 16, 256), (2, 65, 100, 1024), (2, 65, 512, 1536), (1, 65, 40, 1536)])     # D 1536: head dim 192 (Qwen2.5-1.5B, MFMA since round 4)
def test_head_attention(ops, B, Ka, Kt, D):
    H, T = 8, 8
    dh = D // H
    sc = 0.3 if D > 64 else 1.0
    x3 = gen(B, T, 3 * D, seed=50, scale=sc)          # fused q | k_self | v_self
    a2 = gen(B, Ka, 2 * D, seed=51, scale=sc)
    t2 = gen(B, Kt, 2 * D, seed=52, scale=sc)
    gate = torch.tensor([0.7]).to(BF)
    dx3, da2, dt2 = x3.to(DEV), a2.to(DEV), t2.to(DEV)
    args = (dx3[:, :, :D], dx3[:, :, D:2 * D], dx3[:, :, 2 * D:], da2[:, :, :D], da2[:, :, D:], dt2[:, :, :D], dt2[:, :, D:])
    out, probs = ops.head_attn_fwd(*args, gate.to(DEV), H)
    hd = lambda t, L: t.float().reshape(B, L, H, dh).transpose(1, 2)
    leaf = lambda t, L: hd(t, L).clone().requires_grad_(True)
    q, ks, vs = leaf(x3[:, :, :D], T), leaf(x3[:, :, D:2 * D], T), leaf(x3[:, :, 2 * D:], T)
    ka, va, kt, vt = leaf(a2[:, :, :D], Ka), leaf(a2[:, :, D:], Ka), leaf(t2[:, :, :D], Kt), leaf(t2[:, :, D:], Kt)
    g = gate.float().clone().requires_grad_(True)
    ref = O.head_attention_core(q, [(ks, vs), (ka, va), (kt, vt)], torch.tanh(g), True)
    check(out, ref.transpose(1, 2).reshape(B, T, D), rel=6e-3, mx=3e-2, name="head attn fwd")
    # backward vs fp32 autograd of the same math
    dout = gen(B, T, D, seed=53)
    ref32 = O.head_attention_core(q, [(ks, vs), (ka, va), (kt, vt)], torch.tanh(g), False)
    (ref32 * hd(dout, T)).sum().backward()
    g3, ga, gt = torch.zeros_like(dx3), torch.zeros_like(da2), torch.zeros_like(dt2)
    dgate = torch.zeros(1, device=DEV)
    ops.head_attn_bwd(dout.to(DEV), out, *args, gate.to(DEV), probs, dgate, g3[:, :, :D], g3[:, :, D:2 * D], g3[:, :, 2 * D:],
                      ga[:, :, :D], ga[:, :, D:], gt[:, :, :D], gt[:, :, D:], H)
    un = lambda t, L: t.transpose(1, 2).reshape(B, L, D)
    check(g3[:, :, :D], un(q.grad, T), rel=1.5e-2, mx=6e-2, name="head dq")
    check(g3[:, :, D:2 * D], un(ks.grad, T), rel=1.5e-2, mx=6e-2, name="head dk_self")
    check(g3[:, :, 2 * D:], un(vs.grad, T), rel=1.5e-2, mx=6e-2, name="head dv_self")
    check(ga[:, :, :D], un(ka.grad, Ka), rel=1.5e-2, mx=6e-2, name="head dk_adp")
    check(ga[:, :, D:], un(va.grad, Ka), rel=1.5e-2, mx=6e-2, name="head dv_adp")
    check(gt[:, :, :D], un(kt.grad, Kt), rel=1.5e-2, mx=6e-2, name="head dk_task")
    check(gt[:, :, D:], un(vt.grad, Kt), rel=1.5e-2, mx=6e-2, name="head dv_task")
    assert abs(dgate.item() - g.grad.item()) <= 3e-2 * abs(g.grad.item()) + 1e-3, f"dgate {dgate.item()} vs {g.grad.item()}"


# ------------------------------------------------------------------ glue (integer / index work is bit-exact)
def test_action_mask_and_splice(ops):
    z = np.load(os.path.join(G, "masks.npz"))
    labels = torch.from_numpy(z["labels"])
    B, L = labels.shape
    for shift in (0, 1):
        qidx, pos, cnt = ops.action_mask(labels.to(DEV), shift)
        m = O.all_actions_mask(labels[:, shift:])
        assert torch.equal(qidx.cpu() >= 0, m), "mask mismatch vs train_utils golden"
        assert cnt.cpu().tolist() == [64] * B
        for b in range(B):
            idx = torch.where(m[b])[0]
            assert pos[b].cpu().tolist() == idx.tolist()
            assert qidx[b].cpu()[idx].tolist() == list(range(64))
    # adversarial rows: fewer than 64 hits -> count reported, pos padded with -1
    adv = torch.from_numpy(z["labels_adv"])
    qa, pa, ca = ops.action_mask(adv.to(DEV), 0)
    ma = O.all_actions_mask(adv)
    assert torch.equal(qa.cpu() >= 0, ma) and ca.cpu().tolist() == ma.sum(1).tolist()
    # splice
    D, Np, V = 64, 16, 151936
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[labels > O.ACTION_TOKEN_BEGIN_IDX] = labels[labels > O.ACTION_TOKEN_BEGIN_IDX]
    am = ids != 151643
    am[1, -7:] = False
    table = gen(V, D, seed=60)
    aq, patches = gen(64, D, seed=61), gen(B, Np, D, seed=62)
    out = torch.zeros(B, L + Np, D, dtype=BF, device=DEV)
    out[:, 1:Np + 1] = patches.to(DEV)
    mm = torch.zeros(B, L + Np, dtype=torch.uint8, device=DEV)
    qidx, pos, cnt = ops.action_mask(labels.to(DEV), 0)
    ops.embed_splice(ids.to(DEV), am.to(torch.uint8).to(DEV), qidx, table.to(DEV), aq.to(DEV), out, mm, Np)
    ref, refm = O.embed_splice(ids, labels, am, table.float(), aq.float(), patches.float())
    assert torch.equal(f(out), ref), "embed_splice must be bit-exact"
    assert torch.equal(mm.cpu().bool(), refm)
    # backward of the splice into action_queries: sum over the batch of the rows at the masked positions
    dx = gen(B, L + Np, D, seed=63)
    dq = ops.action_query_grad(dx.to(DEV), pos, Np)
    mr = O.all_actions_mask(labels)
    ref = torch.stack([torch.stack([dx[b].float()[(Np + j) if j > 0 else 0] for j in torch.where(mr[b])[0].tolist()]) for b in range(B)]).sum(0)
    check(dq, ref, rel=1e-5, mx=1e-5, name="action_query_grad")


def test_gather_scatter_im2col_misc(ops):
    src = gen(50, 128, seed=70)
    idx = torch.tensor([3, -1, 49, 0, 7], dtype=torch.int32)
    out = torch.empty(5, 128, dtype=BF, device=DEV)
    ops.gather_rows(src.to(DEV), idx.to(DEV), out)
    ref = torch.stack([src[i].float() if i >= 0 else torch.zeros(128) for i in idx.tolist()])
    assert torch.equal(f(out), ref)
    acc = gen(50, 128, seed=71)
    accd = acc.to(DEV).clone()
    ops.scatter_add_rows(out, idx.to(DEV), accd)
    ref2 = acc.float().clone()
    for r, i in enumerate(idx.tolist()):
        if i >= 0:
            ref2[i] = O.rnd(ref2[i] + ref[r], True)
    assert torch.equal(f(accd), ref2)
    # im2col (bf16 and f32 pixels), second backbone's channel window
    px = torch.randn(2, 6, 28, 42, generator=torch.Generator().manual_seed(72))
    for t in (px, px.to(BF)):
        cols = ops.im2col_patch(t.to(DEV).contiguous(), 3, 14, 640)
        ref = O.rnd(O.im2col(t.float()[:, 3:6], 14), True).reshape(-1, 588)
        assert torch.equal(f(cols[:, :588]), ref) and (f(cols[:, 588:]) == 0).all()
    a, b = gen(1000, 64, seed=73), gen(1000, 64, seed=74)
    assert torch.equal(f(ops.add_(a.to(DEV).clone(), b.to(DEV))), O.rnd(a.float() + b.float(), True))
    check(ops.gelu_fwd(a.to(DEV)), O.gelu(a.float(), True), name="gelu")
    xr = a.float().requires_grad_(True)
    (torch.nn.functional.gelu(xr) * b.float()).sum().backward()
    check(ops.gelu_bwd(b.to(DEV), a.to(DEV)), xr.grad, rel=3e-3, name="gelu bwd")
    y = torch.relu(a.float())
    assert torch.equal(f(ops.relu_bwd(b.to(DEV), y.to(BF).to(DEV))), torch.where(y > 0, b.float(), torch.zeros(())))
    cs = torch.zeros(64, device=DEV)
    ops.colsum_(a.to(DEV), cs)
    check(cs, a.float().sum(0), rel=1e-5, mx=1e-5, name="colsum")
    x3 = gen(3, 700, 520, seed=75)
    cs3 = torch.zeros(3, 520, device=DEV)
    ops.colsum_(x3.to(DEV), cs3)
    check(cs3, x3.float().sum(1), rel=1e-5, mx=1e-5, name="colsum batched/vectorised")
    x7 = gen(100, 7, seed=76)
    cs7 = torch.zeros(7, device=DEV)
    ops.colsum_(x7.to(DEV), cs7)
    check(cs7, x7.float().sum(0), rel=1e-5, mx=1e-5, name="colsum odd cols")


def test_l1_loss(ops):
    pred, tgt = gen(4, 8, 7, seed=80), gen(4, 8, 7, seed=81)
    loss3, dpred = ops.l1_loss(pred.to(DEV), tgt.to(DEV))
    m = O.l1_metrics(pred.float(), tgt.float())
    ref = torch.stack([m["loss_value"], m["curr_action_l1_loss"], m["next_actions_l1_loss"]])
    check(loss3, ref, rel=1e-5, mx=1e-5, name="l1 loss")
    pr = pred.float().requires_grad_(True)
    O.l1_loss(pr, tgt.float()).backward()
    check(dpred, O.rnd(pr.grad, True), rel=1e-6, mx=1e-6, name="l1 grad")


def test_adamw_bit_exact_vs_torch_golden(ops):
    """Same fixture that pins the oracle (torch.optim.AdamW on bf16 tensors, generated by tools/make_golden.py)."""
    z = np.load(os.path.join(G, "adamw_bf16.npz"))
    lr, b1, b2, eps, wd = z["hyper"].tolist()
    p = torch.from_numpy(z["p0"]).to(BF).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(3):
        g = torch.from_numpy(z["grads"][step]).to(BF).to(DEV)
        ops.adamw_(p, g, m, v, step + 1, lr, b1, b2, eps, wd)
        assert torch.equal(f(p), torch.from_numpy(z["ps"][step])), f"AdamW params differ from torch at step {step}"
    assert torch.equal(f(m), torch.from_numpy(z["m"])) and torch.equal(f(v), torch.from_numpy(z["v"]))


# ------------------------------------------------------------------ fused rotary embeddings
@pytest.mark.parametrize("dh,H,KV,B,S,K", [(64, 4, 2, 2, 40, 128), (128, 3, 1, 3, 50, 192), (128, 12, 2, 2, 137, 1536)])
def test_gemm_fused_rope_half(ops, dh, H, KV, B, S, K, monkeypatch):
    """QKV projection with the HF rotate_half RoPE applied in the GEMM epilogue == Linear then apply_rotary_pos_emb; head dim 64
    (Qwen2.5-0.5B) and 128 (Qwen2.5-1.5B: one head per 128-column tile, round 4), the latter also bit-identical to the projection
    followed by the stand-alone vla_rope_half pass it replaces, and routed off the 256-row kernel even when that is forced."""
    N = (H + 2 * KV) * dh
    x, w, bias = gen(B * S, K, seed=90), gen(N, K, seed=91, scale=0.1), gen(N, seed=92)
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    out = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), rope=(1, cos, sin, S, dh, (H + KV) * dh))
    y = O.linear(x.float(), w.float(), bias.float(), True)
    c, s = O.rope_half_tables(S, dh, 1e6, True)
    q = O.rope_half(y[:, :H * dh].view(B, S, H, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(B * S, H * dh)
    k = O.rope_half(y[:, H * dh:(H + KV) * dh].view(B, S, KV, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(B * S, KV * dh)
    check(out, torch.cat([q, k, y[:, (H + KV) * dh:]], 1), name=f"gemm + rope_half dh {dh}")
    if dh == 128:
        plain = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV))
        ops.rope_half_(plain[:, :H * dh], cos, sin, S, H, dh)
        ops.rope_half_(plain[:, H * dh:(H + KV) * dh], cos, sin, S, KV, dh)
        assert torch.equal(out, plain), "fused epilogue vs projection + stand-alone RoPE pass"
        monkeypatch.setenv("VLA_GEMM_TILE", "6")
        assert torch.equal(ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), rope=(1, cos, sin, S, dh, (H + KV) * dh)), out)


@pytest.mark.parametrize("tile", [2, 3])
def test_gemm_fused_rope_interleaved(ops, tile, monkeypatch):
    monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    B, T, H, dh, K = 3, 21, 8, 16, 128
    D = H * dh
    x, w, bias = gen(B * T, K, seed=93), gen(2 * D, K, seed=94, scale=0.1), gen(2 * D, seed=95)
    cos, sin = ops.rope_inter_tables(T + 5, dh, DEV)
    out = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), rope=(2, cos, sin, T, dh, D))       # K half only
    y = O.linear(x.float(), w.float(), bias.float(), True)
    c, s = O.head_rope_tables(T, dh, True)
    k = O.head_rope(y[:, :D].view(B, T, H, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(B * T, D)
    check(out, torch.cat([k, y[:, D:]], 1), name="gemm + interleaved rope")


@pytest.mark.parametrize("B,S,Hq,Hkv,dh", [(2, 77, 4, 2, 64), (2, 77, 4, 2, 128), (1, 600, 12, 2, 128),   # dh 128: Qwen2.5-1.5B geometry (round 4)
                                           (1, 40, 2, 2, 64), (1, 33, 2, 2, 128)])                       # one query head per kv head: dK rotated in registers
def test_attention_bwd_fused_inverse_rope(ops, B, S, Hq, Hkv, dh):
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 96)
    dout = gen(B, S, Hq * dh, seed=97)
    d = qkv.to(DEV)
    qd, kd, vd = d[:, :, :Hq * dh], d[:, :, Hq * dh:(Hq + Hkv) * dh], d[:, :, (Hq + Hkv) * dh:]
    o, lse = ops.attn_fwd(qd, kd, vd, Hq, Hkv, dh, True, None, want_lse=True)
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    g0, g1 = torch.zeros_like(d), torch.zeros_like(d)
    sl = lambda t: (t[:, :, :Hq * dh], t[:, :, Hq * dh:(Hq + Hkv) * dh], t[:, :, (Hq + Hkv) * dh:])
    ops.attn_bwd(dout.to(DEV), qd, kd, vd, o, lse, Hq, Hkv, dh, True, None, dq=sl(g0)[0], dk=sl(g0)[1], dv=sl(g0)[2])
    ops.attn_bwd(dout.to(DEV), qd, kd, vd, o, lse, Hq, Hkv, dh, True, None, dq=sl(g1)[0], dk=sl(g1)[1], dv=sl(g1)[2], rope=(cos, sin))
    # reference: exact fp32 inverse rotation of the un-fused gradients
    c, s = O.rope_half_tables(S, dh, 1e6, True)
    def inv(t, h):
        x = f(t).view(B, S, h, dh).transpose(1, 2)
        hh = dh // 2
        rot = torch.cat([x[..., hh:], -x[..., :hh]], -1)
        return (x * c + rot * s).transpose(1, 2).reshape(B, S, h * dh)
    check(sl(g1)[0], inv(sl(g0)[0], Hq), rel=6e-3, mx=3e-2, name="dq through inverse rope")
    check(sl(g1)[1], inv(sl(g0)[1], Hkv), rel=6e-3, mx=3e-2, name="dk through inverse rope")
    assert torch.equal(f(sl(g1)[2]), f(sl(g0)[2]))


@pytest.mark.parametrize("D,T,Kt", [pytest.param(896, 8, 40, id="896"), pytest.param(64, 8, 40, id="64"),
                                    pytest.param(1024, 20, 40, id="1024-T20"), pytest.param(256, 32, 7, id="256-T32-Kt7")])
def test_head_attention_bwd_fused_rope_transpose(ops, D, T, Kt):
    """MFMA path (dh 112) and VALU fallback (dh 8): dq / dk returned through the transpose of the head's RoPE map; on the MFMA path
    also where the query contraction takes its second k-step (T > 16) and with a ragged last key tile (Kt = 7)."""
    B, Ka, H = 2, 65, 8
    dh = D // H
    x3, a2, t2 = gen(B, T, 3 * D, seed=50, scale=0.3), gen(B, Ka, 2 * D, seed=51, scale=0.3), gen(B, Kt, 2 * D, seed=52, scale=0.3)
    gate, dout = torch.tensor([0.7]).to(BF).to(DEV), gen(B, T, D, seed=53).to(DEV)
    dx3, da2, dt2 = x3.to(DEV), a2.to(DEV), t2.to(DEV)
    args = (dx3[:, :, :D], dx3[:, :, D:2 * D], dx3[:, :, 2 * D:], da2[:, :, :D], da2[:, :, D:], dt2[:, :, :D], dt2[:, :, D:])
    out, probs = ops.head_attn_fwd(*args, gate, H)
    tabs = ops.rope_inter_tables(max(T, Ka, Kt), dh, DEV)
    res = []
    for rope in (None, tabs):
        g3, ga, gt = torch.zeros_like(dx3), torch.zeros_like(da2), torch.zeros_like(dt2)
        dg = torch.zeros(1, device=DEV)
        ops.head_attn_bwd(dout, out, *args, gate, probs, dg, g3[:, :, :D], g3[:, :, D:2 * D], g3[:, :, 2 * D:], ga[:, :, :D], ga[:, :, D:],
                          gt[:, :, :D], gt[:, :, D:], H, rope=rope)
        res.append((g3, ga, gt))
    (g3, ga, gt), (r3, ra, rt) = res
    for unf, fus, L in ((g3[:, :, :D], r3[:, :, :D], T), (g3[:, :, D:2 * D], r3[:, :, D:2 * D], T), (ga[:, :, :D], ra[:, :, :D], Ka), (gt[:, :, :D], rt[:, :, :D], Kt)):
        ref = unf.clone().contiguous().view(B * L, D)
        ops.rope_inter_(ref, tabs[0], tabs[1], L, H, dh, 1)          # stand-alone transpose kernel on the un-fused gradient
        check(fus.reshape(B * L, D), f(ref), rel=8e-3, mx=3e-2, name=f"fused rope transpose L={L}")
    assert torch.equal(f(r3[:, :, 2 * D:]), f(g3[:, :, 2 * D:])) and torch.equal(f(ra[:, :, D:]), f(ga[:, :, D:]))


def test_head_attention_bwd_requires_workspace(ops):
    """vla_head_attn_bwd at an MFMA width without its workspace (NULL, or one float short) is refused on the host, before any launch:
    the error names the float count and no gradient byte is written; with exactly that many floats the call is ops.head_attn_bwd's."""
    import ctypes
    B, T, Ka, Kt, H, D = 1, 8, 31, 33, 8, 128
    need = B * H * ((T + Ka + Kt + 31) // 32) * (T * (D // H) + 1)
    x3, a2, t2 = gen(B, T, 3 * D, seed=70, scale=0.3).to(DEV), gen(B, Ka, 2 * D, seed=71, scale=0.3).to(DEV), gen(B, Kt, 2 * D, seed=72, scale=0.3).to(DEV)
    gate, dout = torch.tensor([0.7]).to(BF).to(DEV), gen(B, T, D, seed=73).to(DEV)
    args = (x3[:, :, :D], x3[:, :, D:2 * D], x3[:, :, 2 * D:], a2[:, :, :D], a2[:, :, D:], t2[:, :, :D], t2[:, :, D:])
    out, probs = ops.head_attn_fwd(*args, gate, H)
    views = lambda g3, ga, gt: (g3[:, :, :D], g3[:, :, D:2 * D], g3[:, :, 2 * D:], ga[:, :, :D], ga[:, :, D:], gt[:, :, :D], gt[:, :, D:])
    want = [torch.zeros_like(t) for t in (x3, a2, t2)] + [torch.zeros(1, device=DEV)]
    ops.head_attn_bwd(dout, out, *args, gate, probs, want[3], *views(*want[:3]), H)

    got = [torch.full_like(t, 3.0) for t in (x3, a2, t2)] + [torch.full((1,), 3.0, device=DEV)]      # the sentinel
    ws = torch.empty(need, device=DEV)
    d = ops.head_attn_desc(*args, gate, probs, out, H)
    d.dout, d.dgate = dout.data_ptr(), got[3].data_ptr()
    d.dq, d.dk_self, d.dv_self, d.dk_adp, d.dv_adp, d.dk_task, d.dv_task = (t.data_ptr() for t in views(*got[:3]))

    def call(ptr, floats):
        d.ws, d.ws_floats = ptr, floats
        ops.N.check(ops._lib().vla_head_attn_bwd(ops._st(), ctypes.byref(d)), "head_attn_bwd")
    for ptr, floats in ((0, need), (ws.data_ptr(), need - 1)):
        with pytest.raises(ops.N.NativeError, match=rf"\b{need} floats"):
            call(ptr, floats)
        torch.cuda.synchronize()
        assert all(bool((t == 3.0).all()) for t in got), "a refused call wrote to a gradient buffer"
    for t in got:
        t.zero_()
    call(ws.data_ptr(), need)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_gemm_fused_swiglu_backward(ops):
    """dGU from the fused epilogue == stand-alone swiglu_bwd(dH = d @ W_down)."""
    M, D, I = 330, 128, 192
    x, wg, wu = gen(M, D, seed=12), gen(I, D, seed=13, scale=0.1), gen(I, D, seed=14, scale=0.1)
    w = torch.stack([wg.view(I // 16, 16, D), wu.view(I // 16, 16, D)], dim=1).reshape(2 * I, D)
    gu, _ = ops.gemm_nt(x.to(DEV), w.to(DEV), act=ops.ACT_SWIGLU)
    d, wdT = gen(M, D, seed=15), gen(I, D, seed=16, scale=0.1)          # wdT = W_down^T [I, D]
    fused = ops.gemm_swiglu_bwd(d.to(DEV), wdT.to(DEV), gu)
    dh = ops.gemm_nt(d.to(DEV), wdT.to(DEV))
    ref = ops.swiglu_bwd(dh, gu)
    check(fused, f(ref), rel=3e-3, name="fused swiglu bwd vs two-pass")
    # and against autograd of the oracle math
    G = f(gu).view(M, I // 16, 2, 16)
    gg, uu = G[:, :, 0].reshape(M, I).requires_grad_(True), G[:, :, 1].reshape(M, I).requires_grad_(True)
    dhr = O.linear(d.float(), wdT.float(), None, True)
    ((gg * torch.sigmoid(gg)) * uu * dhr).sum().backward()
    refa = torch.stack([gg.grad.view(M, I // 16, 16), uu.grad.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I)
    check(fused, refa, rel=5e-3, name="fused swiglu bwd vs autograd")


# ------------------------------------------------------------------------------------------------ live-row windows
# Row-window forms used by the live-row LLM backward (engine.LLM.backward): each must reproduce, bit for bit, the rows
# >= row0 of the full-sequence op (same instructions in the same order per row).
@pytest.mark.parametrize("B,S,Hq,Hkv,dh,row0,masked,rope", [(2, 96, 4, 2, 64, 32, False, True), (2, 352, 14, 2, 64, 288, True, True),
                                                            (1, 120, 4, 2, 64, 64, True, False), (2, 100, 2, 2, 72, 32, False, False),
                                                            (2, 352, 12, 2, 128, 288, True, True)])
def test_attention_bwd_live_rows(ops, B, S, Hq, Hkv, dh, row0, masked, rope):
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 140)
    dout = gen(B, S, Hq * dh, seed=141).to(DEV)
    dout[:, :row0] = 0                      # dead rows carry no gradient: then full and windowed backward must agree
    km = torch.ones(B, S, dtype=torch.bool)
    if masked:
        km[0, S - 9:] = False
    d = qkv.to(DEV)
    a, b = Hq * dh, (Hq + Hkv) * dh
    qd, kd, vd = d[:, :, :a], d[:, :, a:b], d[:, :, b:]
    kmd = km.to(torch.uint8).to(DEV) if masked else None
    o, lse = ops.attn_fwd(qd, kd, vd, Hq, Hkv, dh, True, kmd, want_lse=True)
    rp = ops.rope_half_tables(S, dh, 1e6, DEV) if rope else None
    full = torch.zeros_like(d)
    ops.attn_bwd(dout, qd, kd, vd, o, lse, Hq, Hkv, dh, True, kmd, dq=full[:, :, :a], dk=full[:, :, a:b], dv=full[:, :, b:], rope=rp)
    R = S - row0
    win = torch.zeros(B, R, d.shape[-1], dtype=BF, device=DEV)
    ops.attn_bwd(dout[:, row0:].contiguous(), qd[:, row0:], kd, vd, o[:, row0:], lse, Hq, Hkv, dh, True, kmd,
                 dq=win[:, :, :a], dk=win[:, :, a:b], dv=win[:, :, b:], rope=rp, row0=row0)
    assert torch.equal(win[:, :, :a], full[:, row0:, :a]), "dq rows >= row0"
    assert torch.equal(win[:, :, a:b], full[:, row0:, a:b]), "dk rows >= row0"
    assert torch.equal(win[:, :, b:], full[:, row0:, b:]), "dv rows >= row0"


def test_rmsnorm_bwd_row_window(ops):
    B, S, D, r0 = 3, 40, 256, 8
    x, w = gen(B * S, D, seed=150), (1 + 0.1 * gen(D, seed=151).float()).to(BF)
    dy, dres = gen(B * S, D, seed=152), gen(B * S, D, seed=153)
    _, rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), 1e-6, want_rstd=True)
    full = ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), rstd, dres.to(DEV))
    cut = lambda t: t.view(B, S, D)[:, r0:].contiguous().view(-1, D).to(DEV)
    win = ops.rmsnorm_bwd(cut(dy), x.to(DEV), w.to(DEV), rstd, cut(dres), x_rows=(S - r0, S, r0))
    assert torch.equal(win.view(B, S - r0, D), full.view(B, S, D)[:, r0:])


def test_gemm_row_group_residual_and_swiglu_bwd_window(ops):
    B, S, r0, D, I = 3, 50, 18, 128, 192
    R = S - r0
    # residual read through a row window
    a, w, res = gen(B * R, D, seed=160), gen(D, D, seed=161, scale=0.1), gen(B * S, D, seed=162)
    resd = res.to(DEV)
    out = ops.gemm_nt(a.to(DEV), w.to(DEV), residual=resd[r0:], r_group=(R, S * D))
    ref = ops.gemm_nt(a.to(DEV), w.to(DEV), residual=resd.view(B, S, D)[:, r0:].contiguous().view(B * R, D))
    assert torch.equal(out, ref)
    # SwiGLU backward epilogue reading the forward's pre-activations through a row window
    gu, dd, wdT = gen(B * S, 2 * I, seed=163).to(DEV), gen(B * R, D, seed=164).to(DEV), gen(I, D, seed=165, scale=0.1).to(DEV)
    win = ops.gemm_swiglu_bwd(dd, wdT, gu[r0:], gu_group=(R, S * 2 * I))
    ref = ops.gemm_swiglu_bwd(dd, wdT, gu.view(B, S, 2 * I)[:, r0:].contiguous().view(B * R, 2 * I))
    assert torch.equal(win, ref)


def test_action_query_grad_row_window(ops):
    B, P, Np, D, r0 = 3, 40, 16, 64, 32
    L = P + 64
    labels = torch.full((B, L), -100, dtype=torch.int64)
    labels[:, P - 1:] = 151400
    labels[:, P - 1] = 77
    _, pos, _ = ops.action_mask(labels.to(DEV), 0)
    dx = gen(B, L + Np, D, seed=170).to(DEV)
    full = ops.action_query_grad(dx, pos, Np)
    win = ops.action_query_grad(dx[:, r0:].contiguous(), pos, Np, r0)
    assert torch.equal(full, win)


def test_gemm_live_row_store_and_bias_paths(ops):
    """c_live: rows m with m % period < first are left untouched, the others equal the plain GEMM; bias vector/scalar
    fetch paths (8-B aligned slice vs odd offset) agree."""
    B, S, r0, D, N = 3, 40, 24, 128, 200
    a, w = gen(B * S, D, seed=180), gen(N, D, seed=181, scale=0.1)
    bias_buf = gen(N + 1, seed=182).to(DEV)
    ref = ops.gemm_nt(a.to(DEV), w.to(DEV), bias=bias_buf[:N].contiguous())
    ref_odd = ops.gemm_nt(a.to(DEV), w.to(DEV), bias=bias_buf[1:])            # 2-B aligned only: scalar fetch path
    chk = ops.gemm_nt(a.to(DEV), w.to(DEV), bias=bias_buf[1:].contiguous().clone())
    assert torch.equal(ref_odd, chk)
    out = torch.full((B * S, N), 7.0, dtype=BF, device=DEV)
    ops.gemm_nt(a.to(DEV), w.to(DEV), bias=bias_buf[:N].contiguous(), out=out, c_live=(S, r0))
    o3, r3 = out.view(B, S, N), ref.view(B, S, N)
    assert torch.equal(o3[:, r0:], r3[:, r0:]) and bool((o3[:, :r0] == 7.0).all())


@pytest.mark.parametrize("M,N,K,act,res", [(261, 1024, 4096, 0, True), (625, 896, 4864, 0, True), (512, 1152, 4352, 1, False), (256, 896, 2688, 2, True),
                                            (2048, 896, 9728, 0, False), (3000, 896, 4864, 0, True)])
def test_gemm_split_k_matches_single_pass(ops, M, N, K, act, res, monkeypatch):
    """Few-tile long-K problems run split-K (slices meet in an fp32 workspace, epilogue in a second kernel): same result as
    the single-pass kernel up to the fp32 summation order."""
    a, w, bias, r = gen(M, K, seed=190), gen(N, K, seed=191, scale=0.05), gen(N, seed=192), gen(M, N, seed=193)
    kw = dict(bias=bias.to(DEV), act=act, residual=r.to(DEV) if res else None)
    out = torch.empty(M, N, dtype=BF, device=DEV)
    ops.gemm_nt(a.to(DEV), w.to(DEV), out=out, **kw)
    from vla_adapter_amd.scratch import ARENA
    assert (torch.cuda.current_stream().cuda_stream, str(out.device)) in ARENA.buffers, "the split-K path must have run"
    monkeypatch.setenv("VLA_NO_SPLITK", "1")
    ref = torch.empty(M, N, dtype=BF, device=DEV)
    ops.gemm_nt(a.to(DEV), w.to(DEV), out=ref, **kw)
    check(out, f(ref), rel=2e-3, name="split-K vs single pass")
    y = O.linear(a.float(), w.float(), bias.float(), emu=True)
    y = {0: y, 1: O.rnd(O.gelu(y), True), 2: torch.relu(y)}[act]
    check(out, O.rnd(y + r.float(), True) if res else y, name="split-K vs oracle")
    for sk in (2, 4, 8, 3, 7, 11, 16):          # forced factors agree with the automatic choice; those that do not divide K / 64 run uneven slices (round 4)
        forced = torch.empty(M, N, dtype=BF, device=DEV)
        ops.gemm_nt(a.to(DEV), w.to(DEV), out=forced, split_k=sk, **kw)
        check(forced, f(ref), rel=2e-3, name=f"split-K {sk} vs single pass")
    if M <= 640:                                 # the batch-1 pass's choice (latency hint): one 64 x 128 workgroup per CU, slices need not divide K
        with ops.latency_hint():
            hinted = torch.empty(M, N, dtype=BF, device=DEV)
            ops.gemm_nt(a.to(DEV), w.to(DEV), out=hinted, **kw)
        check(hinted, f(ref), rel=2e-3, name="split-K under the latency hint vs single pass")
    off = torch.empty(M, N, dtype=BF, device=DEV)
    monkeypatch.delenv("VLA_NO_SPLITK")
    ops.gemm_nt(a.to(DEV), w.to(DEV), out=off, split_k=0, **kw)
    assert torch.equal(off, ref), "split_k=0 is the single-pass kernel"


def test_gemm_random_shapes_and_epilogues(ops):
    """Seeded sweep over ragged M / N (not multiples of the tile, N odd included), short and long K, every plain epilogue
    combination - result vs the oracle (edge handling: clamped loads, masked stores, scalar bias / store fallbacks)."""
    rng = torch.Generator().manual_seed(1234)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for case in range(16):
        M, N, K = ri(1, 700), ri(1, 600), 64 * ri(1, 40)
        act = [0, 1, 2, 3][ri(0, 3)]
        use_bias, use_res = bool(ri(0, 1)), bool(ri(0, 1))
        a, w = gen(M, K, seed=300 + case), gen(N, K, seed=400 + case, scale=0.05)
        bias, r = gen(N, seed=500 + case), gen(M, N, seed=600 + case)
        out = ops.gemm_nt(a.to(DEV), w.to(DEV), bias=bias.to(DEV) if use_bias else None, act=act,
                          residual=r.to(DEV) if use_res else None)
        y = O.linear(a.float(), w.float(), bias.float() if use_bias else None, emu=True)
        y = {0: y, 1: O.rnd(O.gelu(y), True), 2: torch.relu(y), 3: O.rnd(O.gelu(y, tanh=True), True)}[act]
        ref = O.rnd(y + r.float(), True) if use_res else y
        check(out, ref, name=f"gemm case {case}: {M}x{N}x{K} act{act} bias{use_bias} res{use_res}")


def test_attention_random_shapes(ops):
    """Seeded sweep over ragged sequence lengths, GQA ratios, masks and live-row windows (forward + backward)."""
    rng = torch.Generator().manual_seed(4321)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for case in range(8):
        B, Hkv, grp, S = ri(1, 3), ri(1, 2), [1, 2, 7][ri(0, 2)], ri(33, 300)
        Hq, dh, causal, masked = Hkv * grp, 64, bool(ri(0, 1)), bool(ri(0, 1))
        qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 700 + case)
        km = torch.ones(B, S, dtype=torch.bool)
        if masked:
            km[0, S - ri(1, 20):] = False
        d = qkv.to(DEV)
        a, b = Hq * dh, (Hq + Hkv) * dh
        kmd = km.to(torch.uint8).to(DEV) if masked else None
        o, lse = ops.attn_fwd(d[:, :, :a], d[:, :, a:b], d[:, :, b:], Hq, Hkv, dh, causal, kmd, want_lse=True)
        hd = lambda t, h: t.float().reshape(B, S, h, dh).transpose(1, 2)
        qr, kr, vr = (hd(t, h).clone().requires_grad_(True) for t, h in ((q, Hq), (k, Hkv), (v, Hkv)))
        ref = O.attention(qr, kr, vr, causal, km if masked else None)
        check(o, ref.detach().transpose(1, 2).reshape(B, S, Hq * dh), rel=6e-3, mx=3e-2, name=f"attn fwd case {case}")
        dout = gen(B, S, Hq * dh, seed=800 + case)
        g = torch.zeros_like(d)
        ops.attn_bwd(dout.to(DEV), d[:, :, :a], d[:, :, a:b], d[:, :, b:], o, lse, Hq, Hkv, dh, causal, kmd,
                     dq=g[:, :, :a], dk=g[:, :, a:b], dv=g[:, :, b:])
        (ref * hd(dout, Hq)).sum().backward()
        un = lambda t, h: t.transpose(1, 2).reshape(B, S, h * dh)
        for name, got, want in (("dq", g[:, :, :a], un(qr.grad, Hq)), ("dk", g[:, :, a:b], un(kr.grad, Hkv)), ("dv", g[:, :, b:], un(vr.grad, Hkv))):
            check(got, want, rel=1.2e-2, mx=6e-2, name=f"attn {name} case {case} B{B} S{S} Hq{Hq} Hkv{Hkv} causal{causal} masked{masked}")
        if causal and S > 64:
            r0 = 32 * ri(1, (S - 1) // 32)
            dl = dout.to(DEV).clone()
            dl[:, :r0] = 0
            full, win = torch.zeros_like(d), torch.zeros(B, S - r0, d.shape[-1], dtype=BF, device=DEV)
            ops.attn_bwd(dl, d[:, :, :a], d[:, :, a:b], d[:, :, b:], o, lse, Hq, Hkv, dh, True, kmd, dq=full[:, :, :a], dk=full[:, :, a:b], dv=full[:, :, b:])
            ops.attn_bwd(dl[:, r0:].contiguous(), d[:, r0:, :a], d[:, :, a:b], d[:, :, b:], o[:, r0:], lse, Hq, Hkv, dh, True, kmd,
                         dq=win[:, :, :a], dk=win[:, :, a:b], dv=win[:, :, b:], row0=r0)
            assert torch.equal(win, full[:, r0:]), f"live-row window case {case} S{S} r0{r0}"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("masked_keys", [[31], [3], [28, 29, 30, 31], [3, 4, 5, 6], [0], [27], [5, 40, 63], list(range(30, 40))])
def test_attention_fwd_sparse_key_masks(ops, causal, masked_keys):
    """Key-padding masks that leave key rows 27 / 31 of a 32-key tile visible while the tile takes the masking path: an
    earlier formulation of that path returned wrong weights for exactly those rows (accumulator register 15) - trailing
    masks of >= 5 keys, the only kind the other tests used, hid it."""
    B, S, Hq, Hkv, dh = 2, 72, 4, 2, 64
    qkv, q, k, v = _attn_inputs(B, S, Hq, Hkv, dh, 900)
    km = torch.ones(B, S, dtype=torch.bool)
    km[0, masked_keys] = False
    d = qkv.to(DEV)
    a, b = Hq * dh, (Hq + Hkv) * dh
    o, lse = ops.attn_fwd(d[:, :, :a], d[:, :, a:b], d[:, :, b:], Hq, Hkv, dh, causal, km.to(torch.uint8).to(DEV), want_lse=True)
    hd = lambda t, h: t.float().reshape(B, S, h, dh).transpose(1, 2)
    qr, kr, vr = (hd(t, h).clone().requires_grad_(True) for t, h in ((q, Hq), (k, Hkv), (v, Hkv)))
    ref = O.attention(qr, kr, vr, causal, km)
    valid = torch.ones(B, S, dtype=torch.bool)
    if causal:                      # a query whose every visible key is masked has no defined output (all -inf row)
        for bb in range(B):
            for i in range(S):
                valid[bb, i] = bool(km[bb, :i + 1].any())
    got = o.float().cpu()[valid]
    want = ref.detach().transpose(1, 2).reshape(B, S, Hq * dh)[valid]
    check(got, want, rel=6e-3, mx=3e-2, name=f"attn fwd sparse mask {masked_keys} causal={causal}")
    dout = gen(B, S, Hq * dh, seed=901)
    dout[~valid] = 0
    g = torch.zeros_like(d)
    ops.attn_bwd(dout.to(DEV), d[:, :, :a], d[:, :, a:b], d[:, :, b:], o, lse, Hq, Hkv, dh, causal, km.to(torch.uint8).to(DEV),
                 dq=g[:, :, :a], dk=g[:, :, a:b], dv=g[:, :, b:])
    if bool(valid.all()):
        (ref * hd(dout, Hq)).sum().backward()
        un = lambda t, h: t.transpose(1, 2).reshape(B, S, h * dh)
        check(g[:, :, :a], un(qr.grad, Hq), rel=1.2e-2, mx=6e-2, name="dq sparse mask")
        check(g[:, :, a:b], un(kr.grad, Hkv), rel=1.2e-2, mx=6e-2, name="dk sparse mask")
        check(g[:, :, b:], un(vr.grad, Hkv), rel=1.2e-2, mx=6e-2, name="dv sparse mask")


def test_head_attention_random_shapes(ops):
    """Seeded sweep over (T, Ka, Kt, dh) of the action-head attention, ragged segment lengths included (segments that do
    not end on a 32-key tile boundary; Kt smaller than a tile)."""
    rng = torch.Generator().manual_seed(2468)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for case in range(8):
        B, T, Ka, Kt, H = ri(1, 3), [8, 5, 25, 8][ri(0, 3)], ri(2, 70), ri(3, 300), [8, 4][ri(0, 1)]
        dh = [16, 32, 64, 112][ri(0, 3)]
        if case == 0:
            B, T, Ka, Kt, H, dh = 2, 8, 65, 256, 8, 112          # the production shape
        tag = f"case {case}: B{B} T{T} Ka{Ka} Kt{Kt} H{H} dh{dh}"
        D = H * dh
        xs, xa, xt = gen(B, T, 3 * D, seed=1000 + case, scale=0.5), gen(B, Ka, 2 * D, seed=1100 + case, scale=0.5), gen(B, Kt, 2 * D, seed=1200 + case, scale=0.5)
        gate = torch.tensor([0.3] + [0] * 7).to(BF)
        args = [t.to(DEV) for t in (xs[:, :, :D], xs[:, :, D:2 * D], xs[:, :, 2 * D:], xa[:, :, :D], xa[:, :, D:], xt[:, :, :D], xt[:, :, D:])]
        hd = lambda t, n: t.float().reshape(B, n, H, dh).transpose(1, 2)
        leaves = [hd(xs[:, :, :D], T), hd(xs[:, :, D:2 * D], T), hd(xs[:, :, 2 * D:], T), hd(xa[:, :, :D], Ka), hd(xa[:, :, D:], Ka),
                  hd(xt[:, :, :D], Kt), hd(xt[:, :, D:], Kt)]
        leaves = [l.clone().requires_grad_(True) for l in leaves]
        gr = gate[:1].float().clone().requires_grad_(True)
        out, probs = ops.head_attn_fwd(*args, gate.to(DEV), H)
        ref32 = O.head_attention_core(leaves[0], [(leaves[1], leaves[2]), (leaves[3], leaves[4]), (leaves[5], leaves[6])], torch.tanh(gr), False)
        check(out, ref32.detach().transpose(1, 2).reshape(B, T, D), rel=8e-3, mx=4e-2, name="head fwd " + tag)
        dout = gen(B, T, D, seed=1300 + case)
        (ref32 * hd(dout, T)).sum().backward()
        dgate = torch.zeros(1, dtype=torch.float32, device=DEV)
        g3, ga, gt = torch.zeros_like(args[0].new_empty(B, T, 3 * D)), torch.zeros(B, Ka, 2 * D, dtype=BF, device=DEV), torch.zeros(B, Kt, 2 * D, dtype=BF, device=DEV)
        d3, da, dt = xs.to(DEV), xa.to(DEV), xt.to(DEV)
        a2 = (d3[:, :, :D], d3[:, :, D:2 * D], d3[:, :, 2 * D:], da[:, :, :D], da[:, :, D:], dt[:, :, :D], dt[:, :, D:])
        out2, probs2 = ops.head_attn_fwd(*a2, gate.to(DEV), H)
        ops.head_attn_bwd(dout.to(DEV), out2, *a2, gate.to(DEV), probs2, dgate, g3[:, :, :D], g3[:, :, D:2 * D], g3[:, :, 2 * D:],
                          ga[:, :, :D], ga[:, :, D:], gt[:, :, :D], gt[:, :, D:], H)
        un = lambda t, n: t.transpose(1, 2).reshape(B, n, D)
        for name, got, want in (("dq", g3[:, :, :D], un(leaves[0].grad, T)), ("dks", g3[:, :, D:2 * D], un(leaves[1].grad, T)),
                                ("dvs", g3[:, :, 2 * D:], un(leaves[2].grad, T)), ("dka", ga[:, :, :D], un(leaves[3].grad, Ka)),
                                ("dva", ga[:, :, D:], un(leaves[4].grad, Ka)), ("dkt", gt[:, :, :D], un(leaves[5].grad, Kt)),
                                ("dvt", gt[:, :, D:], un(leaves[6].grad, Kt))):
            check(got, want, rel=2e-2, mx=8e-2, name=f"head {name} " + tag)
        # the gate gradient is ONE scalar summed over every (sample, head, query, task key) with cancellation: looser bound
        assert abs(dgate.item() - gr.grad.item()) <= 1e-1 * abs(gr.grad.item()) + 2e-3, (tag, dgate.item(), gr.grad.item())


def test_norms_transpose_colsum_random_shapes(ops):
    """Seeded sweep over row counts / widths of the HBM-bound kernels (every chunk-count instantiation of the norm kernels:
    cols 8 .. 8192, rows not multiples of the 4 rows a block handles), transposes with padding, batched column sums."""
    rng = torch.Generator().manual_seed(1357)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for case in range(10):
        rows, cols = ri(1, 300), 8 * ri(1, 1024)
        if case < 6:
            cols = [8, 64, 520, 1032, 2056, 4104][case]            # one per NCH instantiation boundary (512-wide chunks + 8)
        x, w, b, dy = gen(rows, cols, seed=1400 + case), (1 + 0.1 * gen(cols, seed=1500 + case).float()).to(BF), gen(cols, seed=1600 + case, scale=0.1), gen(rows, cols, seed=1700 + case)
        y, stats = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), 1e-5, want_stats=True)
        check(y, O.layer_norm(x.float(), w.float(), b.float(), 1e-5, True), name=f"layernorm fwd {rows}x{cols}")
        xr, wr, br = x.float().requires_grad_(True), w.float().requires_grad_(True), b.float().requires_grad_(True)
        (O.layer_norm(xr, wr, br, 1e-5) * dy.float()).sum().backward()
        dw, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        dx = ops.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), stats, dw, db)
        check(dx, xr.grad, rel=5e-3, name=f"layernorm dx {rows}x{cols}")
        check(dw, wr.grad, rel=2e-3, mx=1e-2, name=f"layernorm dw {rows}x{cols}")
        check(db, br.grad, rel=2e-3, mx=1e-2, name=f"layernorm db {rows}x{cols}")
        yr, rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), 1e-6, want_rstd=True)
        check(yr, O.rms_norm(x.float(), w.float(), 1e-6, True), name=f"rmsnorm fwd {rows}x{cols}")
        xr2 = x.float().requires_grad_(True)
        (O.rms_norm(xr2, w.float(), 1e-6) * dy.float()).sum().backward()
        check(ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), rstd), xr2.grad, rel=5e-3, name=f"rmsnorm bwd {rows}x{cols}")
    for case in range(6):
        nb, R, Cc = ri(1, 4), ri(1, 200), 8 * ri(1, 40)
        ld = (R + 63) // 64 * 64
        x = gen(nb, R, Cc, seed=1800 + case)
        t = ops.transpose(x.to(DEV), ld_out=ld)
        assert torch.equal(f(t[:, :, :R]), x.float().transpose(1, 2)) and bool((f(t[:, :, R:]) == 0).all()), (nb, R, Cc)
        cs = torch.zeros(nb, Cc, device=DEV)
        ops.colsum_(x.to(DEV), cs)
        check(cs, x.float().sum(1), rel=1e-5, mx=1e-5, name=f"colsum {nb}x{R}x{Cc}")


@pytest.mark.parametrize("rows,cols,off", [(300, 904, 0), (3001, 1160, 0), (300, 904, 1), (3001, 136, 1)])
def test_weight_gradient_sums_in_a_fixed_order(ops, rows, cols, off):
    """LayerNorm dw / db, RMSNorm dw, bias column sums and the LayerScale gradient against a float64 sum, and bit-identical when
    repeated: short and tall (thousands of rows) inputs; off = 1 element makes the
    operands unaligned (the one-thread-per-column form)."""
    x, dy = gen(rows, cols, seed=3100 + rows), gen(rows, cols, seed=3200 + rows)
    w, b = (1 + 0.1 * gen(cols, seed=3300).float()).to(BF).to(DEV), gen(cols, seed=3400, scale=0.1).to(DEV)
    _, stats = ops.layernorm_fwd(x.to(DEV), w, b, 1e-5, want_stats=True)
    _, rstd = ops.rmsnorm_fwd(x.to(DEV), w, 1e-6, want_rstd=True)

    def shifted(t):                        # the same values at an element offset of `off`
        buf = torch.zeros(t.numel() + 8, dtype=BF, device=DEV)
        buf[off:off + t.numel()] = t.reshape(-1).to(DEV)
        return buf[off:off + t.numel()].view(t.shape)

    xs, dys = shifted(x), shifted(dy)

    def sums():
        dw, db, rw, cs = (torch.zeros(cols, device=DEV) for _ in range(4))
        ops.layernorm_bwd(dys, xs, w, stats, dw, db, want_dx=False)
        ops.N.check(ops._lib().vla_rmsnorm_dw(ops._st(), ops._p(dys), ops._p(xs), ops._p(rstd), ops._p(rw), rows, cols), "rmsnorm_dw")
        ops.colsum_(dys, cs)
        return dw, db, rw, cs

    first, again = sums(), sums()
    for a, c in zip(first, again):
        assert torch.equal(a, c), "sums must not depend on launch timing"
    d64, x64, st = dy.double(), x.double(), f(stats).double().view(rows, 2)
    xh = (x64 - st[:, :1]) * st[:, 1:]
    xr = (x.float() * f(rstd)[:, None]).to(BF).double()
    for got, want, name in ((first[0], (d64 * xh).sum(0), "layernorm dw"), (first[1], d64.sum(0), "layernorm db"),
                            (first[2], (d64 * xr).sum(0), "rmsnorm dw"), (first[3], d64.sum(0), "colsum")):
        check(got, want, rel=1e-5, mx=1e-4, name=f"{name} {rows}x{cols}+{off}")
    if off == 0:                           # LayerScale requires aligned operands
        a_, ls = gen(rows, cols, seed=3500 + rows), (0.5 + 0.1 * gen(cols, seed=3600).float()).to(BF).to(DEV)
        dls1, dls2 = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        da = ops.layerscale_bwd(dy.to(DEV), a_.to(DEV), ls, dls1)
        ops.layerscale_bwd(dy.to(DEV), a_.to(DEV), ls, dls2)
        assert torch.equal(dls1, dls2)
        check(dls1, (d64 * a_.double()).sum(0), rel=1e-5, mx=1e-4, name=f"layerscale dls {rows}x{cols}")
        check(da, dy.float() * f(ls), name=f"layerscale da {rows}x{cols}")


def test_glue_and_optimizer_random_sweep(ops):
    """Seeded sweep over the integer / index kernels (bit-exact), the fused epilogue GEMMs and AdamW:
    random label layouts for the action masks and the splice, random (B, S, heads) for the RoPE-in-GEMM epilogues,
    random (M, I) for SwiGLU forward and its fused backward, AdamW on odd lengths over several steps."""
    rng = torch.Generator().manual_seed(97531)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    # --- masks + splice + action-query gradient
    for case in range(6):
        B, P, extra, Np, D, V = ri(1, 5), ri(1, 40), ri(0, 9), 8 * ri(1, 6), 64 * ri(1, 3), 151936
        L = P + 64 + extra
        labels = torch.full((B, L), -100, dtype=torch.int64)
        ids = torch.randint(0, 151000, (B, L), generator=rng)
        for b in range(B):
            p = ri(1, P)
            labels[b, p - 1] = ri(0, 151000)                              # last prompt id: below ACTION_TOKEN_BEGIN_IDX
            labels[b, p:p + 64] = torch.randint(151387, 151643, (64,), generator=rng)
            ids[b, p:p + 64] = labels[b, p:p + 64]
            ids[b, p + 64:] = 151643                                       # right padding
        for shift in (0, 1):
            qidx, pos, cnt = ops.action_mask(labels.to(DEV), shift)
            m = O.all_actions_mask(labels[:, shift:])
            assert torch.equal(qidx.cpu() >= 0, m) and cnt.cpu().tolist() == [64] * B, (case, shift)
        am = ids != 151643
        table, aq, patches = gen(V, D, seed=2000 + case), gen(64, D, seed=2100 + case), gen(B, Np, D, seed=2200 + case)
        out = torch.zeros(B, L + Np, D, dtype=BF, device=DEV)
        out[:, 1:Np + 1] = patches.to(DEV)
        mm = torch.zeros(B, L + Np, dtype=torch.uint8, device=DEV)
        qidx, pos, cnt = ops.action_mask(labels.to(DEV), 0)
        ops.embed_splice(ids.to(DEV), am.to(torch.uint8).to(DEV), qidx, table.to(DEV), aq.to(DEV), out, mm, Np)
        ref, refm = O.embed_splice(ids, labels, am, table.float(), aq.float(), patches.float())
        assert torch.equal(f(out), ref) and torch.equal(mm.cpu().bool(), refm), f"splice case {case}"
    # --- RoPE epilogues
    for case in range(4):
        B, S, H, KV, K = ri(1, 3), ri(3, 90), 2 * ri(1, 4), ri(1, 2), 64 * ri(1, 4)
        dh = 64
        N = (H + 2 * KV) * dh
        x, w, bias = gen(B * S, K, seed=2300 + case), gen(N, K, seed=2400 + case, scale=0.1), gen(N, seed=2500 + case)
        cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
        out = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), rope=(1, cos, sin, S, dh, (H + KV) * dh))
        y = O.linear(x.float(), w.float(), bias.float(), True)
        c, s = O.rope_half_tables(S, dh, 1e6, True)
        q = O.rope_half(y[:, :H * dh].view(B, S, H, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(B * S, H * dh)
        k = O.rope_half(y[:, H * dh:(H + KV) * dh].view(B, S, KV, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(B * S, KV * dh)
        check(out, torch.cat([q, k, y[:, (H + KV) * dh:]], 1), name=f"gemm + rope_half B{B} S{S} H{H} KV{KV} K{K}")
        T, Hh, dhh = ri(2, 40), 8, [16, 32, 112][ri(0, 2)]
        Dd = Hh * dhh
        x2, w2, b2 = gen(B * T, K, seed=2600 + case), gen(2 * Dd, K, seed=2700 + case, scale=0.1), gen(2 * Dd, seed=2800 + case)
        c2, s2 = ops.rope_inter_tables(T + 3, dhh, DEV)
        out2 = ops.gemm_nt(x2.to(DEV), w2.to(DEV), bias=b2.to(DEV), rope=(2, c2, s2, T, dhh, Dd))
        y2 = O.linear(x2.float(), w2.float(), b2.float(), True)
        cc, ss = O.head_rope_tables(T, dhh, True)
        k2 = O.head_rope(y2[:, :Dd].view(B, T, Hh, dhh).transpose(1, 2), cc, ss, True).transpose(1, 2).reshape(B * T, Dd)
        check(out2, torch.cat([k2, y2[:, Dd:]], 1), name=f"gemm + interleaved rope B{B} T{T} dh{dhh}")
    # --- SwiGLU forward + fused backward
    for case in range(4):
        M, Dd, I = ri(1, 500), 64 * ri(1, 4), 64 * ri(1, 6)
        x, wg, wu = gen(M, Dd, seed=2900 + case), gen(I, Dd, seed=3000 + case, scale=0.1), gen(I, Dd, seed=3100 + case, scale=0.1)
        w = torch.stack([wg.view(I // 16, 16, Dd), wu.view(I // 16, 16, Dd)], dim=1).reshape(2 * I, Dd)
        pre, h = ops.gemm_nt(x.to(DEV), w.to(DEV), act=ops.ACT_SWIGLU)
        g_, u_ = O.linear(x.float(), wg.float(), None, True), O.linear(x.float(), wu.float(), None, True)
        check(h, O.rnd(O.rnd(g_ * torch.sigmoid(g_), True) * u_, True), name=f"swiglu h {M}x{I}x{Dd}")
        d, wdT = gen(M, Dd, seed=3200 + case), gen(I, Dd, seed=3300 + case, scale=0.1)
        fused = ops.gemm_swiglu_bwd(d.to(DEV), wdT.to(DEV), pre)
        check(fused, f(ops.swiglu_bwd(ops.gemm_nt(d.to(DEV), wdT.to(DEV)), pre)), rel=3e-3, name=f"fused swiglu bwd {M}x{I}x{Dd}")
    # --- AdamW, odd lengths, several steps, bit-exact against the oracle's torch-emulating restatement
    for case in range(3):
        n = 8 * ri(1, 5000)
        p0, m0, v0 = gen(n, seed=3400 + case, scale=0.05), torch.zeros(n), torch.zeros(n)
        p, m, v = p0.to(DEV).clone(), torch.zeros(n, dtype=BF, device=DEV), torch.zeros(n, dtype=BF, device=DEV)
        pr, mr, vr = p0.float(), m0, v0
        for step in range(1, 4):
            gg = gen(n, seed=3500 + 10 * case + step, scale=0.01)
            ops.adamw_(p, gg.to(DEV), m, v, step, 3e-4, 0.9, 0.999, 1e-8, 0.01)
            pr, mr, vr = O.adamw_step(pr, gg.float(), mr, vr, step, 3e-4, emu=True)
            assert torch.equal(f(p), pr) and torch.equal(f(m), mr) and torch.equal(f(v), vr), f"adamw n={n} step {step}"


# ------------------------------------------------------------------------------------------------ 256 x 256 8-phase kernel
# gemm256.hip accumulates every output element over K in the same order, with the same MFMA, as the 128-row kernels (K-tiles of
# 64 in ascending order, two 32-deep k-steps each), and its epilogue rounds at the same points: results must be BIT-IDENTICAL
# to the 128 x 128 kernel on every shape and epilogue - a far sharper check of the staggered pipeline (stale or early LDS
# reads, half-tile mix-ups, edge clamps) than any tolerance against the oracle.
def _both_tiles(monkeypatch, fn):
    monkeypatch.setenv("VLA_GEMM_TILE", "2")
    ref = fn()
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    out = fn()
    monkeypatch.setenv("VLA_GEMM_TILE", "0")
    return out, ref


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (256, 256, 128), (256, 256, 192), (512, 768, 320), (1300, 900, 896), (5632, 1152, 1152),
                                   (2048, 1000, 4864), (300, 77, 448), (11264, 1792, 896)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm256_bit_identical_to_128_tiles(ops, M, N, K, act, monkeypatch):
    a, b, bias, r = gen(M, K, seed=201).to(DEV), gen(N, K, seed=202, scale=0.05).to(DEV), gen(N, seed=203).to(DEV), gen(M, N, seed=204).to(DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(a, b, bias=bias, residual=r if act != 1 else None, act=act, split_k=0))
    assert torch.equal(out, ref), f"gemm256 {M}x{N}x{K} act {act}: {(out.float() - ref.float()).abs().max().item()}"
    if M * N * K <= 2 ** 31:
        y = O.linear(f(a), f(b), f(bias), emu=True)
        y = {0: y, 1: O.gelu(y, True), 2: torch.relu(y)}[act]
        check(out, O.rnd(y + f(r), True) if act != 1 else y, name=f"gemm256 vs oracle {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", [(2048, 1024, 64), (2048, 1024, 128), (2048, 1024, 192), (2048, 1024, 256), (4096, 2304, 896), (8192, 1152, 4352)])
def test_gemm256_race_screen(ops, M, N, K, monkeypatch):
    """The two-phase K loop is a sync structure of its own (segment-counted WAR / RAW distances, hand-counted vmcnt): screened by
    repetition - every tile of 25 launches, run while a second stream keeps the memory system busy (the LDS-DMA's landing time
    moves with the load), must equal the 128-row kernel's result bit for bit, with and without a residual; K = 64 ... 256 are the
    one- to four-K-tile prologue / tail cases of the counted waits."""
    a, b, bias, r = gen(M, K, seed=221).to(DEV), gen(N, K, seed=222, scale=0.05).to(DEV), gen(N, seed=223).to(DEV), gen(M, N, seed=224).to(DEV)
    junk, side = torch.empty(64 << 20, dtype=torch.uint8, device=DEV), torch.cuda.Stream()
    for res in (None, r):
        monkeypatch.setenv("VLA_GEMM_TILE", "2")
        ref = ops.gemm_nt(a, b, bias=bias, residual=res, split_k=0)
        monkeypatch.setenv("VLA_GEMM_TILE", "6")
        outs = []
        for i in range(25):
            with torch.cuda.stream(side):
                junk.add_(1)
            outs.append(ops.gemm_nt(a, b, bias=bias, residual=res, split_k=0))
        torch.cuda.synchronize()
        bad = [i for i, o in enumerate(outs) if not torch.equal(o, ref)]
        assert not bad, f"gemm256 {M}x{N}x{K} residual={res is not None}: launches {bad} differ from the 128-row kernel"
    monkeypatch.setenv("VLA_GEMM_TILE", "0")


@pytest.mark.parametrize("M,N,K,kind", [(8, 896, 896, "plain"), (8, 2688, 896, "rope2"), (369, 1152, 896, "rope1"), (256, 4304, 1152, "gelu"),
                                        (369, 896, 4864, "res"), (64, 896, 256, "plain"), (130, 200, 320, "res"), (369, 896, 4864, "split"),
                                        (256, 1152, 192, "plain"), (369, 9728, 896, "plain"), (1000, 2048, 512, "gelu"), (64, 896, 384, "res"),
                                        (100, 640, 448, "plain"), (369, 1152, 1152, "rope1")])
def test_gemm_deep_ring_bit_identical(ops, M, N, K, kind, monkeypatch):
    """Under vla_gemm_latency_hint launches of at most one workgroup per CU run on deeper operand rings (latency-bound batch-1 products,
    round 4): 64 x 128 tiles with six stages when those still fit one round, else 128 x 128 tiles with four (369 x 9728, 1000 x 2048) -
    same K order, same MFMA sequence: equal to the two-stage kernel bit for bit, repeated under memory load (the counted waits of a
    deeper ring are a synchronisation structure of their own; K = 192 ... 448: the three- to seven-K-tile prologue / tail cases, K = 192
    stays on two stages)."""
    a, b, bias, r = gen(M, K, seed=231).to(DEV), gen(N, K, seed=232, scale=0.05).to(DEV), gen(N, seed=233).to(DEV), gen(M, N, seed=234).to(DEV)
    kw = dict(bias=bias, split_k=0)
    if kind == "rope1":
        cos, sin = ops.rope_half_tables(M, 64, 1e6, DEV)
        kw["rope"] = (1, cos, sin, M, 64, 1024)
    elif kind == "rope2":
        T, dh = 8, 112
        rc, rs_ = ops.rope_inter_tables(T, dh, DEV)
        kw["rope"] = (2, rc, rs_, T, dh, 1792)
    elif kind == "gelu":
        kw["act"] = 1
    elif kind == "res":
        kw["residual"] = r
    elif kind == "split":
        kw.update(residual=r, split_k=4)
    assert ops._lib().vla_gemm_latency_hint(-1) == 0
    monkeypatch.setenv("VLA_NO_SMALL_ROWS", "1")      # (the hint's other routing - gemm_skinny.hip for <= 512 rows - has its own test below)
    ref = ops.gemm_nt(a, b, **kw)
    junk, side = torch.empty(64 << 20, dtype=torch.uint8, device=DEV), torch.cuda.Stream()
    outs = []
    with ops.latency_hint():
        assert ops._lib().vla_gemm_latency_hint(-1) == 1
        for i in range(12):
            with torch.cuda.stream(side):
                junk.add_(1)
            outs.append(ops.gemm_nt(a, b, **kw))
    assert ops._lib().vla_gemm_latency_hint(-1) == 0
    torch.cuda.synchronize()
    bad = [i for i, o in enumerate(outs) if not torch.equal(o, ref)]
    assert not bad, f"deep ring {M}x{N}x{K} {kind}: launches {bad} differ from the two-stage kernel"


@pytest.mark.parametrize("M,N,K,sk", [(4096, 64, 1152, 0), (5632, 192, 896, 0), (2048, 128, 1024, 0), (1500, 64, 256, 0), (1024, 192, 1792, 0),
                                      (5632, 128, 1536, 0), (1031, 64, 128, 0), (4096, 192, 1152, 0), (4096, 128, 896, 0),
                                      (4096, 64, 1920, None), (2048, 192, 2048, None)])
def test_gemm_skinny(ops, M, N, K, sk, monkeypatch):
    """gemm_skinny.hip (the LoRA t = 2 x A^T / dt = 2 dy B products, round 4): 32 rows x all N columns per workgroup, the contraction
    split over its four waves.  Against the oracle's Linear; against the 128-row tiles (another fp32 association: a tolerance); bit for
    bit against the 128-row tiles with split_k = 4 where their slices coincide (K % 256 == 0: the same four partial sums in the same
    order).  Ragged M, a strided output; sk = None: ops.gemm_nt's own choice (K = 2048 and more stays on the 128-row tiles with split-K)."""
    a, b = gen(M, K, seed=241).to(DEV), gen(N, K, seed=242, scale=0.05).to(DEV)
    big = torch.zeros(M, N + 64, dtype=BF, device=DEV)
    out = ops.gemm_nt(a, b, alpha=2.0, out=big[:, :N], split_k=sk)
    assert torch.equal(big[:, N:], torch.zeros_like(big[:, N:])), "wrote outside its columns"
    check(out, O.rnd(2.0 * (f(a) @ f(b).T), True), name=f"skinny {M}x{N}x{K} vs fp32")
    monkeypatch.setenv("VLA_NO_SKINNY", "1")
    ref = ops.gemm_nt(a, b, alpha=2.0, split_k=0)
    d = (out.float() - ref.float()).abs()
    assert (d > 0).float().mean().item() < 0.02 and d.max().item() <= 2 ** -7 * ref.float().abs().max().item(), "against the 128-row tiles"
    if K % 256 == 0 and sk == 0:
        ref4 = ops.gemm_nt(a, b, alpha=2.0, split_k=4, out=torch.empty(M, N, dtype=BF, device=DEV))
        assert torch.equal(out, ref4), f"skinny {M}x{N}x{K}: differs from split_k = 4 of the 128-row tiles"
    monkeypatch.delenv("VLA_NO_SKINNY")


@pytest.mark.parametrize("M,N,K,kind", [(256, 896, 896, "bias_relu"), (256, 2688, 896, "rope2"), (256, 896, 896, "res"), (8, 896, 896, "res"),
                                        (8, 2688, 896, "rope2"), (369, 896, 896, "res"), (256, 3456, 1152, "bias"), (256, 4352, 1152, "gelu"),
                                        (100, 1008, 640, "post"), (512, 1024, 1024, "res"), (200, 48, 512, "bias"), (64, 896, 1792, "gelu_res"),
                                        (369, 1152, 896, "rope1"), (48, 1152, 1024, "rope1")])
def test_gemm_small_rows(ops, M, N, K, kind, monkeypatch):
    """gemm_skinny.hip, shape class (b), under the latency hint: products of at most 512 rows (the batch-1 pass) on
    16 x 16 ... 64 x 96 output tiles with the contraction split over the workgroup's four waves, gemm.hip's epilogue at gemm.hip's rounding
    points.  Against the oracle's Linear; against the 128-row tiles (another fp32 association: rare one-ulp differences); bit for bit against
    the 128-row tiles with split_k = 4 where the four K slices coincide (K % 256 == 0, epilogues the split-K second pass has)."""
    a, b = gen(M, K, seed=251).to(DEV), gen(N, K, seed=252, scale=0.05).to(DEV)
    bias, r = gen(N, seed=253).to(DEV), gen(M, N, seed=254).to(DEV)
    kw = {}
    if kind in ("bias_relu", "bias", "gelu", "rope2", "rope1", "post", "res", "gelu_res"):
        kw["bias"] = bias
    if kind == "rope1":                              # Qwen2 q | k | v projection: rotate_half on the q and k columns (14 + 2 heads of 64), v untouched
        cos, sin = ops.rope_half_tables(M, 64, 1e6, DEV)
        kw["rope"] = (1, cos, sin, M, 64, 1024)
    if kind == "bias_relu":
        kw["act"] = 2
    if kind in ("gelu", "gelu_res"):
        kw["act"] = 1
    if kind in ("res", "gelu_res"):
        kw["residual"] = r
    if kind == "post":
        kw["bias_post_round"] = True
    if kind == "rope2":
        T, dh = 8, 112
        rc, rs_ = ops.rope_inter_tables(T, dh, DEV)
        kw["rope"] = (2, rc, rs_, T, dh, 1792)
    with ops.latency_hint():                       # (class (b) is the batch-1 pass's: only under vla_gemm_latency_hint)
        out = ops.gemm_nt(a, b, split_k=0, **kw)
    ref = ops.gemm_nt(a, b, split_k=0, **kw)
    d = (out.float() - ref.float()).abs()
    assert (d > 0).float().mean().item() < 0.02 and d.max().item() <= 2 ** -6 * ref.float().abs().max().item(), \
        f"{kind} {M}x{N}x{K}: {(d > 0).float().mean().item():.4f} of the elements differ, max {d.max().item():.3e}"
    if K % 256 == 0 and kind not in ("rope2", "rope1", "post"):
        ref4 = ops.gemm_nt(a, b, split_k=4, out=torch.empty(M, N, dtype=BF, device=DEV), **kw)
        assert torch.equal(out, ref4), f"{kind} {M}x{N}x{K}: differs from split_k = 4 of the 128-row tiles"
    if kind in ("bias", "res", "bias_relu"):
        y = O.linear(f(a), f(b), f(bias), emu=True)
        y = torch.relu(y) if kind == "bias_relu" else y
        check(out, O.rnd(y + f(r), True) if kind == "res" else y, name=f"small rows {kind} vs oracle")


def test_gemm256_swiglu_forward_and_backward_bit_identical(ops, monkeypatch):
    M, D, I = 1100, 896, 1216
    x, wg, wu = gen(M, D, seed=211), gen(I, D, seed=212, scale=0.05), gen(I, D, seed=213, scale=0.05)
    w = torch.stack([wg.view(I // 16, 16, D), wu.view(I // 16, 16, D)], dim=1).reshape(2 * I, D).to(DEV)
    xd = x.to(DEV)
    (pre, h), (pre_r, h_r) = _both_tiles(monkeypatch, lambda: ops.gemm_nt(xd, w, act=ops.ACT_SWIGLU))
    assert torch.equal(pre, pre_r) and torch.equal(h, h_r)
    # live-row store of the pre-activations (rows below the window untouched), no pre-activation output at all
    S, r0 = 100, 64
    o1 = torch.full((M, 2 * I), 3.0, dtype=BF, device=DEV)
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    _, h2 = ops.gemm_nt(xd, w, act=ops.ACT_SWIGLU, out=o1, c_live=(S, r0))
    _, h3 = ops.gemm_nt(xd, w, act=ops.ACT_SWIGLU, want_pre=False)
    rows = torch.arange(M, device=DEV) % S >= r0
    assert torch.equal(h2, h_r) and torch.equal(h3, h_r) and torch.equal(o1[rows], pre_r[rows]) and bool((o1[~rows] == 3.0).all())
    # fused SwiGLU backward, plain and through a row window of the pre-activations
    d, wdT = gen(M, D, seed=214).to(DEV), gen(I, D, seed=215, scale=0.05).to(DEV)
    fused, fused_r = _both_tiles(monkeypatch, lambda: ops.gemm_swiglu_bwd(d, wdT, pre_r))
    assert torch.equal(fused, fused_r)
    B, Sx, r0x = 11, 100, 36
    R = Sx - r0x
    dd = gen(B * R, D, seed=216).to(DEV)
    win, win_r = _both_tiles(monkeypatch, lambda: ops.gemm_swiglu_bwd(dd, wdT, pre_r[r0x:], gu_group=(R, Sx * 2 * I)))
    assert torch.equal(win, win_r)


def test_gemm256_row_groups_batched_and_res_mod(ops, monkeypatch):
    # A read through a row-group window, C written through one, residual broadcast by res_mod, batched with per-batch B / bias
    B, S, Kt, D, N = 6, 352, 256, 896, 1792
    hs = gen(B * S, D, seed=221).to(DEV)
    w, bias = gen(N, D, seed=222, scale=0.05).to(DEV), gen(N, seed=223).to(DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(hs[:B * Kt], w, bias=bias, a_group=(Kt, S * D)))
    assert torch.equal(out, ref)
    big1, big2 = torch.zeros(B * S, N, dtype=BF, device=DEV), torch.zeros(B * S, N, dtype=BF, device=DEV)
    a2 = gen(B * Kt, D, seed=224).to(DEV)
    monkeypatch.setenv("VLA_GEMM_TILE", "2")
    ops.gemm_nt(a2, w, out=big1[:B * Kt], c_group=(Kt, S * N))
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    ops.gemm_nt(a2, w, out=big2[:B * Kt], c_group=(Kt, S * N))
    assert torch.equal(big1, big2) and bool((big2.view(B, S, N)[:, Kt:] == 0).all())
    pos = gen(Kt, N, seed=225).to(DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(a2, w, bias=bias, residual=pos, res_mod=Kt))
    assert torch.equal(out, ref)
    nb, M2 = 3, 1024
    ab, bb, bias_b = gen(nb, M2, D, seed=226).to(DEV), gen(nb, N, D, seed=227, scale=0.05).to(DEV), gen(nb, N, seed=228).to(DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(ab, bb, bias=bias_b))
    assert torch.equal(out, ref)


def test_gemm256_repeatable_under_load(ops, monkeypatch):
    """Race screen: the same multi-round launch (more tiles than CUs, long K) repeated back to back on two streams at once
    must reproduce its first result bit for bit every time (an early LDS read shows up as rare differing tiles)."""
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    M, N, K = 8192, 4352, 1152
    a, b = gen(M, K, seed=231).to(DEV), gen(N, K, seed=232, scale=0.05).to(DEV)
    a2, b2 = gen(4096, 4864, seed=233).to(DEV), gen(896, 4864, seed=234, scale=0.05).to(DEV)
    first, first2 = ops.gemm_nt(a, b, act=1), ops.gemm_nt(a2, b2, split_k=0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs, outs2 = [], []
    for _ in range(12):
        outs.append(ops.gemm_nt(a, b, act=1))
        with torch.cuda.stream(side):
            outs2.append(ops.gemm_nt(a2, b2, split_k=0))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(o, first) for o in outs) and all(torch.equal(o, first2) for o in outs2)


def test_gemm256_persistent_step_shapes_repeatable_under_load(ops, monkeypatch):
    """Race screen of the persistent walk at the step's whole-batch shapes: gate/up with the SwiGLU epilogue and live-row stores
    (1672 tiles, 6.5 per workgroup: next tile's K-tile 0 lands in one K-tile buffer while the epilogue stages through the
    other) and the down projection with residual (176 tiles), repeated back to back while a second stream runs the ViT's fc1 -
    every repetition bit-identical to the first, and the first bit-identical to the 128-row kernel."""
    M, D, I, S, r0 = 11264, 896, 4864, 352, 288
    x, wgu, wd = gen(M, D, seed=281).to(DEV), gen(2 * I, D, seed=282, scale=0.05).to(DEV), gen(D, I, seed=283, scale=0.05).to(DEV)
    res = gen(M, D, seed=284).to(DEV)
    a2, b2 = gen(8192, 1152, seed=285).to(DEV), gen(4352, 1152, seed=286, scale=0.05).to(DEV)
    pre = torch.zeros(M, 2 * I, dtype=BF, device=DEV)
    monkeypatch.setenv("VLA_GEMM_TILE", "2")
    pre_r = torch.zeros(M, 2 * I, dtype=BF, device=DEV)
    _, h_r = ops.gemm_nt(x, wgu, act=ops.ACT_SWIGLU, out=pre_r, c_live=(S, r0))
    y_r = ops.gemm_nt(h_r, wd, residual=res)
    monkeypatch.setenv("VLA_GEMM_TILE", "0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    hs, ys, others = [], [], []
    for _ in range(8):
        _, h = ops.gemm_nt(x, wgu, act=ops.ACT_SWIGLU, out=pre, c_live=(S, r0))
        hs.append(h)
        ys.append(ops.gemm_nt(h, wd, residual=res))
        with torch.cuda.stream(side):
            others.append(ops.gemm_nt(a2, b2, act=1))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(h, h_r) for h in hs) and all(torch.equal(y, y_r) for y in ys) and torch.equal(pre, pre_r)
    assert all(torch.equal(o, others[0]) for o in others)


@pytest.mark.parametrize("grid", ["1", "3", "8", "37"])
def test_gemm256_persistent_walk_small_grids(ops, grid, monkeypatch):
    """The persistent walk proper: a forced grid of 1 / 3 / 8 / 37 workgroups makes each of them run many tiles back to back
    (next tile's K-tile 0 in flight under the epilogue, staging region alternating between the K-tile buffers, bias slice and
    sources re-derived per tile) - bit-identical to the 128-row kernel on ragged M / N, with residual, with an unaligned bias
    (element path), with K = 64 (one K-tile: no second buffer in flight), batched, SwiGLU with live-row stores."""
    monkeypatch.setenv("VLA_GEMM256_GRID", grid)
    for (M, N, K, act, res) in [(1300, 900, 320, 0, True), (1100, 1152, 64, 1, False), (777, 520, 448, 2, True), (2048, 896, 896, 0, False)]:
        a, b, bias, r = gen(M, K, seed=251).to(DEV), gen(N, K, seed=252, scale=0.05).to(DEV), gen(N + 1, seed=253).to(DEV), gen(M, N, seed=254).to(DEV)
        for bb in (bias[:N], bias[1:]):                       # 8-B aligned / odd-element offset: vector and element bias paths
            out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(a, b, bias=bb, residual=r if res else None, act=act, split_k=0))
            assert torch.equal(out, ref), f"grid {grid} {M}x{N}x{K} act {act}"
    nb, M2, D, N2 = 3, 600, 448, 700
    ab, wb, bias_b = gen(nb, M2, D, seed=255).to(DEV), gen(nb, N2, D, seed=256, scale=0.05).to(DEV), gen(nb, N2, seed=257).to(DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(ab, wb, bias=bias_b))
    assert torch.equal(out, ref)
    M, D, I, S, r0 = 1100, 448, 640, 100, 64
    x, w = gen(M, D, seed=258).to(DEV), gen(2 * I, D, seed=259, scale=0.05).to(DEV)
    o1, o2 = torch.full((M, 2 * I), 3.0, dtype=BF, device=DEV), torch.full((M, 2 * I), 3.0, dtype=BF, device=DEV)
    monkeypatch.setenv("VLA_GEMM_TILE", "2")
    _, h_r = ops.gemm_nt(x, w, act=ops.ACT_SWIGLU, out=o1, c_live=(S, r0))
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    _, h = ops.gemm_nt(x, w, act=ops.ACT_SWIGLU, out=o2, c_live=(S, r0))
    assert torch.equal(h, h_r) and torch.equal(o1, o2)
    d, wdT = gen(M, D, seed=260).to(DEV), gen(I, D, seed=261, scale=0.05).to(DEV)
    pre = gen(M, 2 * I, seed=262).to(DEV)
    fused, fused_r = _both_tiles(monkeypatch, lambda: ops.gemm_swiglu_bwd(d, wdT, pre))
    assert torch.equal(fused, fused_r)


@pytest.mark.parametrize("grid", [None, "5"])
def test_gemm256_fused_rope_half_bit_identical(ops, grid, monkeypatch):
    """The rotate_half RoPE epilogue of the 256-row kernel (the LLM's q|k|v projection: 14 + 2 rotated heads, v untouched) against
    the 128-row kernel's, bit for bit - at the step's shape, on a ragged one (last rows / partial column tile) and walked by a
    grid of five workgroups."""
    if grid:
        monkeypatch.setenv("VLA_GEMM256_GRID", grid)
    for B, S, H, KV, K in [(16, 352, 14, 2, 896), (3, 100, 6, 2, 320)]:
        dh = 64
        N = (H + 2 * KV) * dh
        x, w, bias = gen(B * S, K, seed=271).to(DEV), gen(N, K, seed=272, scale=0.05).to(DEV), gen(N, seed=273).to(DEV)
        cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
        out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(x, w, bias=bias, rope=(1, cos, sin, S, dh, (H + KV) * dh)))
        assert torch.equal(out, ref), f"gemm256 rope {B}x{S}: {(out.float() - ref.float()).abs().max().item()}"


@pytest.mark.parametrize("grid", [None, "5"])
def test_gemm256_fused_rope_interleaved_bit_identical(ops, grid, monkeypatch):
    """The interleaved RoPE epilogue of the 256-row kernel (the head's task-token K|V projection: K half rotated, V untouched; with
    the strided-input rounding order of the reference's CPU Linear, read through row groups) against the 128-row kernel's, bit for
    bit, and against the stand-alone pass on the plain projection - at the step's shape and on a ragged one."""
    if grid:
        monkeypatch.setenv("VLA_GEMM256_GRID", grid)
    for B, Kt, S, H, dh, K, post in [(32, 256, 352, 8, 112, 896, True), (3, 100, 130, 4, 48, 320, False)]:
        D = H * dh
        hs = gen(B * S, K, seed=281).to(DEV)
        w, bias = gen(2 * D, K, seed=282, scale=0.05).to(DEV), gen(2 * D, seed=283).to(DEV)
        cos, sin = ops.rope_inter_tables(Kt + 3, dh, DEV)
        run = lambda: ops.gemm_nt(hs[:B * Kt], w, bias=bias, a_group=(Kt, S * K), bias_post_round=post, rope=(2, cos, sin, Kt, dh, D))
        out, ref = _both_tiles(monkeypatch, run)
        assert torch.equal(out, ref), f"gemm256 interleaved rope {B}x{Kt}: {(out.float() - ref.float()).abs().max().item()}"
        plain = ops.gemm_nt(hs[:B * Kt], w, bias=bias, a_group=(Kt, S * K), bias_post_round=post)
        ops.rope_inter_(plain[:, :D], cos, sin, Kt, H, dh, 0)
        assert torch.equal(out, plain), f"fused vs stand-alone {B}x{Kt}: {(out.float() - plain.float()).abs().max().item()}"


def test_gemm_forced_tile_with_split_k(ops, monkeypatch):
    """Forced big tiles used to launch grid.z = batch instead of the K-slice count: every forced tile must agree
    with the automatic split-K result."""
    M, N, K = 512, 896, 4096
    a, w, bias = gen(M, K, seed=241).to(DEV), gen(N, K, seed=242, scale=0.05).to(DEV), gen(N, seed=243).to(DEV)
    ref = ops.gemm_nt(a, w, bias=bias, split_k=4)
    for tile in (2, 3, 6):
        monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
        out = ops.gemm_nt(a, w, bias=bias, split_k=4)
        check(out, f(ref), rel=2e-3, name=f"split-K 4 with forced tile {tile}")


# ------------------------------------------------------------------------------------------------ fp8 (OCP e4m3) weight path
# BASELINE configs[4] names an "fp8 MFMA weight path"; the reference has no fp8 code, so there is nothing to pin against:
# PARITY UNPINNED.  What is checked: the quantiser against torch's own e4m3 conversion of the same scaled values (bit-exact
# codes), and the GEMM against the fp32 product of the DEQUANTISED operands (the arithmetic the kernel claims to do).
def _q8_ref(x):
    amax = x.float().abs().amax(dim=1, keepdim=True)
    inv = torch.where(amax > 0, 448.0 / amax, torch.ones_like(amax))
    q = (x.float() * inv).to(torch.float8_e4m3fn)
    return q, torch.where(amax > 0, amax / 448.0, torch.ones_like(amax)).squeeze(1)


@pytest.mark.parametrize("rows,cols", [(37, 896), (256, 1152), (5, 64), (300, 4864)])
def test_quant_fp8_rows_matches_torch_e4m3(ops, rows, cols):
    x = gen(rows, cols, seed=301, scale=1.7)
    x[1] = 0                                                     # an all-zero row: scale 1, codes 0
    q, s = ops.quant_fp8_rows(x.to(DEV))
    qr, sr = _q8_ref(x)
    assert torch.equal(s.cpu(), sr), (s.cpu() - sr).abs().max()
    # Codes equal torch's round-to-nearest-even conversion - except where the scaled fp32 value sits within two of its ulps of a
    # rounding tie: v_cvt_pk_fp8_f32 resolves those as ties (to the even code; observed: 10.500000954 -> 10, torch -> 11).
    # There the kernel's code must be one of the two neighbours, and such elements must be rare.
    got, want = q.cpu().view(torch.float8_e4m3fn).float(), qr.float()
    diff = got != want
    assert diff.float().mean().item() < 2e-3, diff.sum()
    if diff.any():
        amax = x.float().abs().amax(dim=1, keepdim=True)
        v = (x.float() * torch.where(amax > 0, 448.0 / amax, torch.ones_like(amax)))[diff]
        tie = (got[diff] + want[diff]) / 2
        ulp = torch.ldexp(torch.ones_like(v), torch.floor(torch.log2(v.abs())).int() - 23)
        assert bool(((v - tie).abs() <= 2 * ulp).all()), (v - tie).abs().max()


@pytest.mark.parametrize("M,N,K,act,res", [(256, 256, 128, 0, False), (300, 200, 384, 0, True), (1000, 896, 896, 1, False), (2048, 1152, 4352, 0, True),
                                           (64, 24, 256, 2, False)])
def test_gemm_fp8_matches_dequantised_product(ops, M, N, K, act, res):
    x, w, bias, r = gen(M, K, seed=311), gen(N, K, seed=312, scale=0.05), gen(N, seed=313), gen(M, N, seed=314)
    qa, sa = ops.quant_fp8_rows(x.to(DEV))
    qb, sb = ops.quant_fp8_rows(w.to(DEV))
    out = ops.gemm_nt(qa, qb, bias=bias.to(DEV), residual=r.to(DEV) if res else None, act=act, fp8=(sa, sb))
    A = qa.cpu().view(torch.float8_e4m3fn).float() * sa.cpu()[:, None]
    B = qb.cpu().view(torch.float8_e4m3fn).float() * sb.cpu()[:, None]
    y = O.rnd(A @ B.t() + bias.float(), True)
    y = {0: y, 1: O.gelu(y, True), 2: torch.relu(y)}[act]
    check(out, O.rnd(y + r.float(), True) if res else y, name=f"fp8 gemm {M}x{N}x{K}")
    # and the quantisation error itself stays what e4m3 with per-row scales gives (~3 % of the product's norm)
    exact = x.float() @ w.float().t()
    assert ((A @ B.t() - exact).norm() / exact.norm()).item() < 0.06


def test_gemm_fp8_swiglu_and_rope_epilogues(ops):
    M, D, I = 600, 512, 640
    x, w = gen(M, D, seed=321), gen(2 * I, D, seed=322, scale=0.05)
    qa, sa = ops.quant_fp8_rows(x.to(DEV))
    qb, sb = ops.quant_fp8_rows(w.to(DEV))
    pre, h = ops.gemm_nt(qa, qb, act=ops.ACT_SWIGLU, fp8=(sa, sb))
    A = qa.cpu().view(torch.float8_e4m3fn).float() * sa.cpu()[:, None]
    B = qb.cpu().view(torch.float8_e4m3fn).float() * sb.cpu()[:, None]
    y = O.rnd(A @ B.t(), True)
    check(pre, y, name="fp8 swiglu pre-activations")
    g, u = y.view(M, I // 16, 2, 16)[:, :, 0].reshape(M, I), y.view(M, I // 16, 2, 16)[:, :, 1].reshape(M, I)
    check(h, O.rnd(O.rnd(g * torch.sigmoid(g), True) * u, True), rel=6e-3, name="fp8 swiglu h")
    Bq, S, H, KV, dh, K = 2, 40, 4, 2, 64, 256
    N = (H + 2 * KV) * dh
    x2, w2, bias = gen(Bq * S, K, seed=323), gen(N, K, seed=324, scale=0.1), gen(N, seed=325)
    qa, sa = ops.quant_fp8_rows(x2.to(DEV))
    qb, sb = ops.quant_fp8_rows(w2.to(DEV))
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    out = ops.gemm_nt(qa, qb, bias=bias.to(DEV), rope=(1, cos, sin, S, dh, (H + KV) * dh), fp8=(sa, sb))
    A = qa.cpu().view(torch.float8_e4m3fn).float() * sa.cpu()[:, None]
    B = qb.cpu().view(torch.float8_e4m3fn).float() * sb.cpu()[:, None]
    y = O.rnd(A @ B.t() + bias.float(), True)
    c, s = O.rope_half_tables(S, dh, 1e6, True)
    q = O.rope_half(y[:, :H * dh].view(Bq, S, H, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(Bq * S, H * dh)
    k = O.rope_half(y[:, H * dh:(H + KV) * dh].view(Bq, S, KV, dh).transpose(1, 2), c, s, True).transpose(1, 2).reshape(Bq * S, KV * dh)
    check(out, torch.cat([q, k, y[:, (H + KV) * dh:]], 1), name="fp8 gemm + rope_half")


def test_norms_with_fused_fp8_output_match_norm_then_quantise(ops):
    """rmsnorm_fwd_q8 / layernorm_fwd_q8 == the plain norm followed by quant_fp8_rows, bit for bit (codes, scales, and the
    optional bf16 output / statistics)."""
    rows, cols = 77, 896
    x, w, b = gen(rows, cols, seed=331).to(DEV), (1 + 0.1 * gen(cols, seed=332).float()).to(BF).to(DEV), gen(cols, seed=333, scale=0.1).to(DEV)
    y, rstd = ops.rmsnorm_fwd(x, w, 1e-6, want_rstd=True)
    q_ref, s_ref = ops.quant_fp8_rows(y)
    q, s = torch.empty(rows, cols, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.float32, device=DEV)
    y2, r2 = torch.empty_like(y), torch.empty_like(rstd)
    ops.rmsnorm_fwd_q8(x, w, 1e-6, q, s, rstd=r2, y=y2)
    assert torch.equal(q, q_ref) and torch.equal(s, s_ref) and torch.equal(y2, y) and torch.equal(r2, rstd)
    q3, s3 = torch.empty_like(q), torch.empty_like(s)
    ops.rmsnorm_fwd_q8(x, w, 1e-6, q3, s3)                        # no bf16 output at all
    assert torch.equal(q3, q_ref) and torch.equal(s3, s_ref)
    cols = 1152
    x, w, b = gen(rows, cols, seed=334).to(DEV), (1 + 0.1 * gen(cols, seed=335).float()).to(BF).to(DEV), gen(cols, seed=336, scale=0.1).to(DEV)
    y = ops.layernorm_fwd(x, w, b, 1e-6)
    q_ref, s_ref = ops.quant_fp8_rows(y)
    q, s = torch.empty(rows, cols, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.float32, device=DEV)
    y2 = torch.empty_like(y)
    ops.layernorm_fwd_q8(x, w, b, 1e-6, q, s, y=y2)
    assert torch.equal(q, q_ref) and torch.equal(s, s_ref) and torch.equal(y2, y)


@pytest.mark.parametrize("grid", [None, "3"])
def test_gemm256_fp8_bit_identical_to_128_row_fp8(ops, grid, monkeypatch):
    """The fp8 form of the 256-row persistent kernel against the fp8 form of the 128-row kernel (same K order, one 128-deep MFMA
    per K-tile in both): bit-identical on plain / GELU / residual / SwiGLU / rotate_half epilogues, ragged shapes, small grids."""
    if grid:
        monkeypatch.setenv("VLA_GEMM256_GRID", grid)
    for (M, N, K, act, res) in [(1300, 900, 384, 0, True), (1100, 1152, 128, 1, False), (777, 520, 512, 2, True), (2048, 896, 896, 0, False)]:
        x, w, bias, r = gen(M, K, seed=341), gen(N, K, seed=342, scale=0.05), gen(N, seed=343).to(DEV), gen(M, N, seed=344).to(DEV)
        qa, sa = ops.quant_fp8_rows(x.to(DEV))
        qb, sb = ops.quant_fp8_rows(w.to(DEV))
        out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(qa, qb, bias=bias, residual=r if res else None, act=act, fp8=(sa, sb)))
        assert torch.equal(out, ref), f"fp8 gemm256 {M}x{N}x{K} act {act}: {(out.float() - ref.float()).abs().max().item()}"
    M, D, I = 1100, 512, 640
    qa, sa = ops.quant_fp8_rows(gen(M, D, seed=345).to(DEV))
    qb, sb = ops.quant_fp8_rows(gen(2 * I, D, seed=346, scale=0.05).to(DEV))
    (pre, h), (pre_r, h_r) = _both_tiles(monkeypatch, lambda: ops.gemm_nt(qa, qb, act=ops.ACT_SWIGLU, fp8=(sa, sb)))
    assert torch.equal(pre, pre_r) and torch.equal(h, h_r)
    B, S, H, KV, dh, K = 4, 352, 14, 2, 64, 896
    N = (H + 2 * KV) * dh
    qa, sa = ops.quant_fp8_rows(gen(B * S, K, seed=347).to(DEV))
    qb, sb = ops.quant_fp8_rows(gen(N, K, seed=348, scale=0.05).to(DEV))
    bias = gen(N, seed=349).to(DEV)
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    out, ref = _both_tiles(monkeypatch, lambda: ops.gemm_nt(qa, qb, bias=bias, rope=(1, cos, sin, S, dh, (H + KV) * dh), fp8=(sa, sb)))
    assert torch.equal(out, ref)
