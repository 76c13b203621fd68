"""Every kernel element by element against a float64 truth (tests/accuracy.py): the GEMM family through each of its kernels, the
norms, attention, the elementwise kernels at the ends of their argument range, the token cross-entropy - and the kernels the step
reaches only end to end (embedding gradient, dropout backward, head index preparation), bit-exact against a short restatement.

The truth is the op in float64 from the exact bf16 inputs, rounded to bf16 only at the op's declared rounding points (the emu
oracle's, e.g. the GEMM epilogue rounds the linear output before an activation); assert_contract holds outputs to 1 ulp of it
(2 where the contract chains two roundings), assert_row_budget holds every row of the kernels whose internal rounding points
differ legitimately from the oracle's to a multiple of the oracle's own error on that row."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import vla_oracle as O
from tests import accuracy as A

pytestmark = pytest.mark.gpu

DEV, BF, F64 = "cuda", torch.bfloat16, torch.float64
U = A.U32

# (the activation floors - the documented approximations of csrc/common.h - are accuracy.act_floor)
EXP_C, FTZ = A.EXP_C, A.FTZ
# e4m3 GEMM: accumulation floor constant in place of accuracy.ACC_C (test_gemm_nt_fp8).  Measured on the MI355X: the worst output
# error beyond half an ulp is 0.51 x the ACC_C floor at 1000 x 896 x 896 (0.43 x with unit scales, i.e. in the MFMA sums themselves,
# where the bf16 kernels stay below 0.25 x), and at 4096^3 one output in 2.8e5 exceeds the ACC_C floor; none exceeds FP8_ACC_C.
FP8_ACC_C = 4 * A.ACC_C


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vla_adapter_amd import ops as _ops
    return _ops


def gen(*shape, seed=0, scale=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + mean).to(BF)


def d64(t):
    return t.detach().cpu().to(F64)


def cpu(t):
    return t.detach().cpu()


# ------------------------------------------------------------------ float64 epilogue truths
def gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))            # 0.5 x (1 + erf(x / sqrt 2)) without the cancellation of the tail


def gelu_tanh64(x):
    return x * torch.sigmoid(A.gelu_tanh_arg(x))                # 0.5 x (1 + tanh u), likewise


def silu64(x):
    return x * torch.sigmoid(x)


act_floor = A.act_floor


ACTS = {"none": (0, lambda x: x), "gelu": (1, gelu64), "relu": (2, torch.relu), "gelu_tanh": (3, gelu_tanh64)}


def epilogue_truth(acc, floor, *, bias=None, act="none", res=None, alpha=1.0, post=False):
    """(truth64, floor, max_ulp) of C = [res +] bf16(act(bf16(alpha acc + bias))) as the GEMM epilogue declares it."""
    return _epilogue(acc, floor, bias, act, res, alpha, post)[:3]


def _epilogue(acc, floor, bias, act, res, alpha, post):
    """... and the elements the fraction criterion counts: all but those where an activation's documented floor reaches the
    rounding step (the erf tail)."""
    v, fl, chained, where = alpha * acc, abs(alpha) * floor, 0, None
    if post:                                          # bf16(bf16(alpha acc) + bias)
        v, fl = A.round_point(v, fl)
        chained += 1
    if bias is not None:
        v = v + d64(bias)
    if act in ("gelu", "gelu_tanh"):
        x, fl = A.round_point(v, fl)
        y = ACTS[act][1](x)
        where = act_floor(act, x, y) < A.ulp_at(y) / 4
        v, fl, chained = y, 1.2 * fl + act_floor(act, x, y), chained + 1
    elif act == "relu":
        v = torch.relu(v)
    if res is not None:
        v, fl = A.round_point(v, fl)
        v, chained = v + d64(res), chained + 1
    return v, fl, 1 + min(chained, 1), where


# ------------------------------------------------------------------ a. NT GEMM
def _gemm(ops, M, N, K, seed, kind="bias", tile=None, hint=False, split_k=None, alpha=1.0, monkeypatch=None):
    a, b = gen(M, K, seed=seed), gen(N, K, seed=seed + 1, scale=0.05)
    bias, r = gen(N, seed=seed + 2), gen(M, N, seed=seed + 3)
    kw = dict(split_k=split_k, alpha=alpha)
    tk = dict(alpha=alpha)
    if kind in ("bias", "res", "relu", "gelu", "gelu_tanh", "gelu_res", "post"):
        kw["bias"], tk["bias"] = bias.to(DEV), bias
    if kind in ("res", "gelu_res", "plain_res"):
        kw["residual"], tk["res"] = r.to(DEV), r
    if kind in ("relu", "gelu", "gelu_tanh", "gelu_res"):
        name = "gelu" if kind == "gelu_res" else kind
        kw["act"], tk["act"] = ACTS[name][0], name
    if kind == "post":
        kw["bias_post_round"], tk["post"] = True, True
    if tile is not None:
        monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    if hint:
        with ops.latency_hint():
            out = ops.gemm_nt(a.to(DEV), b.to(DEV), **kw)
    else:
        out = ops.gemm_nt(a.to(DEV), b.to(DEV), **kw)
    t, fl, mu, fw = _epilogue(d64(a) @ d64(b).t(), A.acc_floor(a, b), tk.get("bias"), tk.get("act", "none"), tk.get("res"), alpha,
                              tk.get("post", False))
    A.assert_contract(out, t, acc_floor=fl, max_ulp=mu, name=f"gemm {kind} {M}x{N}x{K} tile {tile} hint {hint} split {split_k}",
                      frac_where=fw)


EDGES = [(63, 64, 64), (64, 65, 128), (65, 63, 192), (127, 128, 896), (128, 129, 128), (129, 127, 192), (255, 256, 896),
         (256, 257, 192), (257, 255, 128), (300, 200, 192), (1000, 896, 896)]


@pytest.mark.parametrize("M,N,K", EDGES)
def test_gemm_nt_tile_edges_automatic(ops, M, N, K):
    _gemm(ops, M, N, K, 1000 + M, "res")


@pytest.mark.parametrize("tile", [2, 3, 6])
@pytest.mark.parametrize("M,N,K", [(63, 64, 64), (129, 128, 192), (255, 256, 896), (257, 384, 128), (520, 512, 4864), (300, 200, 192)])
@pytest.mark.parametrize("kind", ["bias", "res"])
def test_gemm_nt_every_tile(ops, monkeypatch, tile, M, N, K, kind):
    _gemm(ops, M, N, K, 1100 + M + N, kind, tile=tile, monkeypatch=monkeypatch)


@pytest.mark.parametrize("kind", ["plain", "bias", "res", "plain_res", "relu", "gelu", "gelu_tanh", "gelu_res", "post"])
@pytest.mark.parametrize("tile", [None, 2, 6])
def test_gemm_nt_epilogues(ops, monkeypatch, kind, tile):
    _gemm(ops, 520, 256, 256, 1200, kind, tile=tile, monkeypatch=monkeypatch)


def test_gemm_nt_alpha(ops):
    _gemm(ops, 300, 256, 896, 1250, "bias", alpha=0.125)


@pytest.mark.parametrize("M,N,K", [(1, 896, 896), (8, 896, 4864), (63, 1152, 4352), (65, 256, 8960), (256, 1152, 4352), (511, 896, 896)])
@pytest.mark.parametrize("kind", ["plain", "bias", "res", "gelu"])
def test_gemm_nt_latency_hint(ops, M, N, K, kind):
    """The batch-1 pass's kernels: tall-skinny, the <= 512-row kernel, the deep ring, hint-sized split-K."""
    _gemm(ops, M, N, K, 1300 + M, kind, hint=True)


@pytest.mark.parametrize("M,N,K,sk", [(128, 256, 4864, None), (256, 128, 8960, None), (128, 256, 4864, 4), (200, 128, 8192, 8),
                                      (128, 256, 4864, 0), (300, 200, 2048, 2)])
@pytest.mark.parametrize("kind", ["plain", "bias", "res", "relu"])
def test_gemm_nt_split_k(ops, M, N, K, sk, kind):
    _gemm(ops, M, N, K, 1400 + K, kind, split_k=sk)


def test_gemm_nt_res_mod_and_batched(ops):
    nb, M, N, K = 3, 129, 128, 192
    a, b, pos = gen(nb, M, K, seed=1500), gen(N, K, seed=1501, scale=0.1), gen(M, N, seed=1502)
    out = ops.gemm_nt(a.to(DEV).view(nb * M, K), b.to(DEV), residual=pos.to(DEV), res_mod=M)
    acc = (d64(a) @ d64(b).t()).view(nb * M, N)
    t, fl, mu = epilogue_truth(acc, A.acc_floor(a.view(nb * M, K), b), res=pos.repeat(nb, 1))
    A.assert_contract(out, t, acc_floor=fl, max_ulp=mu, name="res_mod")
    bb = gen(nb, N, K, seed=1503, scale=0.1)
    out = ops.gemm_nt(a.to(DEV), bb.to(DEV))
    t = d64(a) @ d64(bb).transpose(1, 2)
    fl = torch.stack([A.acc_floor(a[i], bb[i]) for i in range(nb)])
    A.assert_contract(out, t, acc_floor=fl, name="batched")


@pytest.mark.parametrize("tile", [None, 2, 3, 6])
def test_gemm_nt_swiglu(ops, monkeypatch, tile):
    if tile is not None:
        monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    M, I, K = 330, 320, 256
    x, wg, wu = gen(M, K, seed=1600), gen(I, K, seed=1601, scale=0.1), gen(I, K, seed=1602, scale=0.1)
    bg, bu = gen(I, seed=1603), gen(I, seed=1604)
    w = torch.stack([wg.view(I // 16, 16, K), wu.view(I // 16, 16, K)], dim=1).reshape(2 * I, K)
    bias = torch.stack([bg.view(I // 16, 16), bu.view(I // 16, 16)], dim=1).reshape(2 * I)
    pre, h = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), act=ops.ACT_SWIGLU)
    g, flg = A.round_point(d64(x) @ d64(wg).t() + d64(bg), A.acc_floor(x, wg))
    u, flu = A.round_point(d64(x) @ d64(wu).t() + d64(bu), A.acc_floor(x, wu))
    tpre = torch.stack([g.view(M, I // 16, 16), u.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I)
    A.assert_contract(pre, tpre, acc_floor=torch.stack([flg.view(M, I // 16, 16), flu.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I),
                      name="swiglu pre")
    s = silu64(g)
    s, fls = A.round_point(s, 1.1 * flg + act_floor("silu", g, s))
    A.assert_contract(h, s * u, acc_floor=fls * u.abs() + s.abs() * flu, max_ulp=2, name="swiglu h")


@pytest.mark.parametrize("mode", [1, 2])
def test_gemm_nt_fused_rope(ops, mode):
    if mode == 1:                     # Qwen2 q | k | v: rotate_half on the q and k heads of 64
        S, dh, H, KV, K = 130, 64, 4, 2, 256
        ncols, N = (H + KV) * dh, (H + 2 * KV) * dh
        cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
        M, T = S, S
    else:                             # action head: interleaved pairs on the first D columns
        T, dh, D, K = 8, 112, 896, 256
        cos, sin = ops.rope_inter_tables(T, dh, DEV)
        ncols, N, M = D, 2 * D, 4 * T
    x, w, bias = gen(M, K, seed=1700 + mode), gen(N, K, seed=1702, scale=0.05), gen(N, seed=1703)
    out = ops.gemm_nt(x.to(DEV), w.to(DEV), bias=bias.to(DEV), rope=(mode, cos, sin, T, dh, ncols))
    y, fl = A.round_point(d64(x) @ d64(w).t() + d64(bias), A.acc_floor(x, w))
    c, s = d64(cos), d64(sin)
    pos = torch.arange(M) % T
    yr = y[:, :ncols].reshape(M, -1, dh)
    flr = fl[:, :ncols].reshape(M, -1, dh)
    if mode == 1:
        h = dh // 2
        cc, ss = torch.cat([c, c], -1)[pos][:, None], torch.cat([s, s], -1)[pos][:, None]
        rot = torch.cat([-yr[..., h:], yr[..., :h]], -1)
        frot = torch.cat([flr[..., h:], flr[..., :h]], -1)
    else:
        cc, ss = c[pos][:, None], s[pos][:, None]
        rot = torch.stack([-yr[..., 1::2], yr[..., 0::2]], -1).reshape(yr.shape)
        frot = torch.stack([flr[..., 1::2], flr[..., 0::2]], -1).reshape(yr.shape)
    p1, f1 = A.round_point(yr * cc, flr * cc.abs())
    p2, f2 = A.round_point(rot * ss, frot * ss.abs())
    t = y.clone()
    t[:, :ncols] = (p1 + p2).reshape(M, ncols)
    ft = fl.clone() * 0
    ft[:, :ncols] = (f1 + f2).reshape(M, ncols)
    A.assert_contract(out, t, acc_floor=ft, max_ulp=2, name=f"rope {mode}")


@pytest.mark.parametrize("M,N,K,K2", [(300, 256, 896, 64), (1000, 896, 896, 128), (65, 200, 192, 64)])
def test_gemm_nt_k_extension(ops, M, N, K, K2):
    a, b, a2, b2 = gen(M, K, seed=1800), gen(N, K, seed=1801, scale=0.05), gen(M, K2, seed=1802, scale=0.2), gen(N, K2, seed=1803, scale=0.2)
    bias = gen(N, seed=1804)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), bias=bias.to(DEV), ext=(a2.to(DEV), b2.to(DEV)))
    acc = d64(a) @ d64(b).t() + d64(a2) @ d64(b2).t()
    t, fl, mu = epilogue_truth(acc, A.acc_floor(torch.cat([a, a2], 1), torch.cat([b, b2], 1)), bias=bias)
    A.assert_contract(out, t, acc_floor=fl, max_ulp=mu, name="K extension")


@pytest.mark.parametrize("tile", [None, 6])
@pytest.mark.parametrize("M,N,K,K2", [(300, 256, 896, 0), (1000, 896, 896, 0), (4096, 4096, 4096, 0), (300, 256, 896, 64)])
def test_gemm_nt_fp8(ops, monkeypatch, tile, M, N, K, K2):
    """e4m3 operands: the truth is the product of the dequantised operands (exact products), so the same contract applies; the two
    per-row scales add two fp32 roundings (4 u |acc| in the floor).  The accumulation floor is FP8_ACC_C, not ACC_C: the e4m3 MFMA's
    sums carry more error than the bf16 one's (measured: 0.51 x the ACC_C floor at K = 896, and one output in 2.8e5 over it at
    K = 4096; the bf16 kernels stay below 0.25 x)."""
    if tile is not None:
        monkeypatch.setenv("VLA_GEMM_TILE", str(tile))
    a, b, bias, r = gen(M, K, seed=1900), gen(N, K, seed=1901, scale=0.05), gen(N, seed=1902), gen(M, N, seed=1903)
    qa, sa = ops.quant_fp8_rows(a.to(DEV))
    qb, sb = ops.quant_fp8_rows(b.to(DEV))
    kw = dict(bias=bias.to(DEV), residual=r.to(DEV), fp8=(sa, sb))
    rows = torch.arange(0, M, 61) if M * N > 4e6 else torch.arange(M)       # the big square's truth on a row sample (CPU time)
    deq = lambda q, s: cpu(q).view(torch.float8_e4m3fn).to(F64) * d64(s)[:, None]
    da, db = deq(qa, sa)[rows], deq(qb, sb)
    acc = da @ db.t()
    fl = A.acc_floor(da, db, FP8_ACC_C) + 4 * U * acc.abs()
    if K2:
        a2, b2 = gen(M, K2, seed=1904, scale=0.2), gen(N, K2, seed=1905, scale=0.2)
        kw["ext"] = (a2.to(DEV), b2.to(DEV))
        acc = acc + d64(a2[rows]) @ d64(b2).t()
        fl = fl + A.acc_floor(a2[rows], b2)
    out = ops.gemm_nt(qa, qb, **kw)
    t, fl, mu = epilogue_truth(acc, fl, bias=bias, res=r[rows])
    A.assert_contract(cpu(out)[rows], t, acc_floor=fl, max_ulp=mu, name=f"fp8 {M}x{N}x{K}+{K2}")


# ------------------------------------------------------------------ b. TN GEMM
@pytest.mark.parametrize("tn_tile", [None, "128", "256"])
@pytest.mark.parametrize("M,N1,N2", [(64, 128, 128), (1000, 256, 136), (4096, 128, 256), (333, 72, 200), (2000, 1152, 896)])
def test_gemm_tn(ops, monkeypatch, tn_tile, M, N1, N2):
    if tn_tile is not None:
        monkeypatch.setenv("VLA_TN_TILE", tn_tile)
    a, b = gen(M, N1, seed=2000), gen(M, N2, seed=2001, scale=0.1)
    out = ops.gemm_tn(a.to(DEV), b.to(DEV), alpha=0.5)
    fl = 0.5 * A.acc_floor(a.t(), b.t())
    t = 0.5 * d64(a).t() @ d64(b)
    A.assert_contract(out, t, acc_floor=fl, name=f"tn {M}x{N1}x{N2}")
    c0 = gen(N1, N2, seed=2002)
    acc = c0.to(DEV).clone()
    ops.gemm_tn(a.to(DEV), b.to(DEV), out=acc, accumulate=True)      # C = bf16(bf16(product) + C)
    p, flp = A.round_point(d64(a).t() @ d64(b), A.acc_floor(a.t(), b.t()))
    A.assert_contract(acc, p + d64(c0), acc_floor=flp, max_ulp=2, name="tn accumulate")


def test_gemm_tn_grouped(ops):
    probs, outs, truths = [], [], []
    for i, (M, N1, N2) in enumerate([(64, 128, 64), (200, 64, 256), (1000, 136, 72)]):
        a, b = gen(M, N1, seed=2100 + i), gen(M, N2, seed=2110 + i, scale=0.1)
        o = torch.empty(N1, N2, dtype=BF, device=DEV)
        probs.append(ops.tn_problem(a.to(DEV), b.to(DEV), o, alpha=2.0))
        outs.append(o)
        truths.append((2.0 * d64(a).t() @ d64(b), 2.0 * A.acc_floor(a.t(), b.t())))
    ops.gemm_tn_grouped(probs)
    for o, (t, fl) in zip(outs, truths):
        A.assert_contract(o, t, acc_floor=fl, name="tn grouped")


# ------------------------------------------------------------------ c. norms
def _norm_inputs(kind, rows, cols, seed):
    if kind == "normal":
        return gen(rows, cols, seed=seed)
    if kind == "mean50":
        return gen(rows, cols, seed=seed, mean=50.0)
    if kind == "outliers":
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))
        x[:, [3, cols // 2, cols - 1]] *= 300
        return x.to(BF)
    x = torch.full((rows, cols), 0.75)                     # near-zero variance: eps dominates
    x[:, ::7] += 2 ** -7
    x[rows // 2:] = 0.75                                   # and exactly constant rows
    return x.to(BF)


NORM_KINDS = ["normal", "mean50", "outliers", "flat"]


def _ln64(x, w, b, eps):
    """(y, x^, mean, rstd) in float64, the statistics two-pass."""
    x64 = d64(x)
    mu = x64.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x64 - mu) * rstd
    return xh * d64(w) + d64(b), xh, mu, rstd


def _rms64(x, eps):
    x64 = d64(x)
    return x64 / torch.sqrt((x64 * x64).mean(-1, keepdim=True) + eps)


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (67, 1152), (33, 896), (9, 1536)])
def test_layernorm_fwd(ops, kind, rows, cols):
    eps = 1e-6
    x, w, b = _norm_inputs(kind, rows, cols, 2200), gen(cols, seed=2201), gen(cols, seed=2202, scale=0.1)
    y, stats = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), eps, want_stats=True)
    t, xh, mu64, rstd64 = _ln64(x, w, b, eps)
    fl = A.norm_floor(xh, w, b, mu64, rstd64)
    A.assert_contract(y, t, acc_floor=fl, max_frac=A.NORM_MAX_FRAC, name=f"LN {kind} {rows}x{cols}")
    x64 = d64(x)
    mu = x64.mean(-1)
    rstd = 1 / torch.sqrt(((x64 - mu[:, None]) ** 2).mean(-1) + eps)
    st = cpu(stats).to(F64)
    assert ((st[:, 1] - rstd).abs() <= 1e-5 * rstd).all(), f"LN rstd {kind}"
    assert ((st[:, 0] - mu).abs() <= 1e-5 * (mu.abs() + 1)).all(), f"LN mean {kind}"
    q8, qs = torch.empty(rows, cols, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.float32, device=DEV)
    y2 = torch.empty_like(y)
    ops.layernorm_fwd_q8(x.to(DEV), w.to(DEV), b.to(DEV), eps, q8, qs, y=y2)
    assert torch.equal(y2, y), "the _q8 form's bf16 output is the plain forward's"


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (67, 896), (9, 1536)])
def test_rmsnorm_fwd(ops, kind, rows, cols):
    eps = 1e-6
    x, w = _norm_inputs(kind, rows, cols, 2300), gen(cols, seed=2301)
    y, rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), eps, want_rstd=True)
    n64 = _rms64(x, eps)
    n, fln = A.round_point(n64, rms_floor(n64))             # Qwen2RMSNorm: w * bf16(x rstd)
    A.assert_contract(y, n * d64(w), acc_floor=fln * d64(w).abs(), max_ulp=2, max_frac=A.NORM_MAX_FRAC, name=f"RMS {kind} {rows}x{cols}")
    x64 = d64(x)
    r64 = 1 / torch.sqrt((x64 * x64).mean(-1) + eps)
    assert ((cpu(rstd).to(F64) - r64).abs() <= 1e-5 * r64).all()
    q8, qs = torch.empty(rows, cols, dtype=torch.uint8, device=DEV), torch.empty(rows, dtype=torch.float32, device=DEV)
    y2 = torch.empty_like(y)
    ops.rmsnorm_fwd_q8(x.to(DEV), w.to(DEV), eps, q8, qs, y=y2)
    assert torch.equal(y2, y), "the _q8 form's bf16 output is the plain forward's"


def rms_floor(n64):
    """fp32 error of x rstd: NORM_C ulps, plus the fp32 mean of squares over the row (sqrt(cols) u32 relative)."""
    return (A.NORM_C + math.sqrt(n64.shape[-1])) * U * n64.abs()


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (67, 1152), (40, 896)])
def test_layernorm_bwd(ops, kind, rows, cols):
    eps = 1e-6
    x, w, b, dy = _norm_inputs(kind, rows, cols, 2400), gen(cols, seed=2401), gen(cols, seed=2402), gen(rows, cols, seed=2403)
    _, stats = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), eps, want_stats=True)
    dw = torch.zeros(cols, dtype=torch.float32, device=DEV)
    db = torch.zeros(cols, dtype=torch.float32, device=DEV)
    dx = ops.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), stats, dw=dw, db=db)

    def grads(dt):
        xs, ws, bs = (t.to(dt).requires_grad_() for t in (x, w, b))
        if dt == F64:
            y = F.layer_norm(xs, (cols,), ws, bs, eps)
        else:
            y = O.layer_norm(xs, ws, bs, eps, emu=True)
        y.backward(dy.to(dt))
        return xs.grad, ws.grad, bs.grad

    tx, tw, tb = grads(F64)
    ex, _, _ = grads(torch.float32)
    A.assert_row_budget(dx, ex.to(BF), tx, 1, A.NORM_FACTOR, A.NORM_FLOOR, name=f"LN dx {kind}")
    _, xh, mu64, rstd64 = _ln64(x, w, b, eps)
    exh = A.norm_floor(xh, torch.ones(cols), None, mu64, rstd64)     # fp32 error of x^ itself (the kernel's statistics)
    flw = 4 * math.sqrt(rows) * U * (d64(dy).abs() * xh.abs()).sum(0) + (d64(dy).abs() * exh).sum(0)
    assert ((cpu(dw).to(F64) - tw).abs() <= flw).all(), f"LN dw {kind}: {((cpu(dw).to(F64) - tw).abs() / flw).max():.2f} x the floor"
    flb = 4 * math.sqrt(rows) * U * d64(dy).abs().sum(0)
    assert ((cpu(db).to(F64) - tb).abs() <= flb).all(), f"LN db {kind}"


@pytest.mark.parametrize("kind", NORM_KINDS)
@pytest.mark.parametrize("rows,cols", [(5, 64), (67, 896), (9, 1536)])
def test_rmsnorm_bwd_and_dw(ops, kind, rows, cols):
    eps = 1e-6
    x, w, dy = _norm_inputs(kind, rows, cols, 2500), gen(cols, seed=2501), gen(rows, cols, seed=2502)
    _, rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), eps, want_rstd=True)
    dx = ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), rstd)
    dw = torch.zeros(cols, dtype=torch.float32, device=DEV)
    dyd, xd = dy.to(DEV), x.to(DEV)
    ops.N.check(ops._lib().vla_rmsnorm_dw(ops._st(), ops._p(dyd), ops._p(xd), ops._p(rstd), ops._p(dw), rows, cols), "rmsnorm_dw")

    def grads(dt, emu):
        xs, ws = x.to(dt).requires_grad_(), w.to(dt).requires_grad_()
        y = O.rms_norm(xs, ws, eps, emu=emu)
        y.backward(dy.to(dt))
        return xs.grad, ws.grad

    tx, _ = grads(F64, False)
    ex, _ = grads(torch.float32, True)
    A.assert_row_budget(dx, ex.to(BF), tx, 1, A.NORM_FACTOR, A.NORM_FLOOR, name=f"RMS dx {kind}")
    # dw[c] = sum_rows dy bf16(x rstd): the declared rounding point of the forward, fp32 sum over the rows
    n64 = _rms64(x, eps)
    n, fa = A.round_point(n64, rms_floor(n64))
    tw = (d64(dy) * n).sum(0)
    flw = 4 * math.sqrt(rows) * U * (d64(dy).abs() * n.abs()).sum(0) + (d64(dy).abs() * fa).sum(0)
    assert ((cpu(dw).to(F64) - tw).abs() <= flw + 1e-30).all(), f"rmsnorm dw {kind}: {((cpu(dw).to(F64) - tw).abs() / flw).max():.2f} x the floor"


# ------------------------------------------------------------------ d. attention
def attn_ref(q, k, v, allow, scale, emu):
    """O.attention with the kernel's definition of a row with no visible key (output 0); q [B,H,Sq,dh], allow [B,1,Sq,Sk]."""
    H, KV = q.shape[1], k.shape[1]
    k, v = k.repeat_interleave(H // KV, 1), v.repeat_interleave(H // KV, 1)
    s = (q @ k.transpose(-1, -2)) * scale
    live = allow.any(-1, keepdim=True)
    s = torch.where(allow, s, torch.full_like(s, float("-inf")))
    s = torch.where(live, s, torch.zeros_like(s))
    p = torch.softmax(s, -1) * live
    return O.rnd(O.rnd(p, emu) @ v, emu)


def _allow(B, S, causal, km):
    a = torch.ones(S, S, dtype=torch.bool)
    if causal:
        a = torch.tril(a)
    return a[None, None] & km[:, None, None, :]


def _attn_case(B, S, Hq, Hkv, dh, seed, value):
    """q, k, v as [B, S, heads*dh] bf16.  value: 'normal', 'peaked' (each row's top logit leads the next by 20-40), or
    'sink@j' (key j favoured strongly by every query)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, Hq, dh, generator=g)
    k = torch.randn(B, S, Hkv, dh, generator=g)
    v = torch.randn(B, S, Hkv, dh, generator=g)
    if value == "peaked":
        grp = Hq // Hkv
        tgt = (torch.rand(B, S, generator=g) * (torch.arange(S) + 1)).long()      # a visible key under causal masking
        kk = k.repeat_interleave(grp, 2)
        alpha = 30.0 / (dh ** 0.5 - 3.0)          # target logit alpha sqrt(dh), the others ~ alpha N(0, 1)
        q = alpha * kk[torch.arange(B)[:, None], tgt] + 0.1 * q
    elif value.startswith("sink@"):
        j = int(value[5:])
        u = torch.randn(dh, generator=g)
        q = 0.5 * q + u
        k[:, j] = 3.0 * u
    return q.reshape(B, S, Hq * dh).to(BF), k.reshape(B, S, Hkv * dh).to(BF), v.reshape(B, S, Hkv * dh).to(BF)


MASKS = {
    "none": lambda B, S: None,
    "trailing": lambda B, S: torch.arange(S)[None].expand(B, S) < max(S - 9, 1),
    "leading": lambda B, S: torch.arange(S)[None].expand(B, S) >= min(5, S - 1),
    "isolated": lambda B, S: ~((torch.arange(S)[None] == torch.tensor([31, 32, 63, 64])[:, None]).any(0))[None].expand(B, S),
    "row_dead": lambda B, S: torch.stack([torch.ones(S, dtype=torch.bool)] + [torch.zeros(S, dtype=torch.bool)] * (B - 1)),
}

ATTN_CASES = [  # B, S, Hq, Hkv, dh, causal, mask, value
    (1, 1, 2, 1, 64, True, "none", "normal"), (2, 2, 2, 2, 72, False, "none", "normal"), (1, 31, 14, 2, 64, True, "trailing", "normal"),
    (2, 32, 7, 1, 128, False, "isolated", "normal"), (1, 33, 4, 2, 128, True, "leading", "normal"), (2, 63, 2, 1, 64, False, "row_dead", "normal"),
    (1, 64, 14, 2, 64, True, "isolated", "peaked"), (2, 65, 4, 4, 72, True, "row_dead", "normal"), (1, 127, 7, 7, 72, False, "trailing", "peaked"),
    (1, 129, 14, 2, 64, True, "leading", "sink@0"), (1, 352, 14, 2, 64, True, "trailing", "normal"), (2, 369, 2, 1, 128, False, "none", "sink@368"),
    (1, 625, 14, 2, 64, True, "trailing", "sink@40"), (1, 129, 7, 1, 64, True, "isolated", "peaked"), (2, 100, 2, 2, 72, False, "leading", "sink@70"),
    (1, 70, 6, 2, 64, True, "trailing", "normal"), (1, 40, 8, 1, 64, False, "isolated", "normal"),      # GQA groups of 3 and 8 (the host's limit)
]


def _attn_fwd_check(ops, B, S, Hq, Hkv, dh, causal, mask, value, hint, seed=2600):
    q, k, v = _attn_case(B, S, Hq, Hkv, dh, seed, value)
    km = MASKS[mask](B, S)
    kmd = km.to(torch.uint8).to(DEV) if km is not None else None
    if hint:
        with ops.latency_hint():
            o, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), Hq, Hkv, dh, causal, kmd, want_lse=True)
    else:
        o, lse = ops.attn_fwd(q.to(DEV), k.to(DEV), v.to(DEV), Hq, Hkv, dh, causal, kmd, want_lse=True)
    km = km if km is not None else torch.ones(B, S, dtype=torch.bool)
    allow = _allow(B, S, causal, km)
    hd = lambda t, h, dt: t.to(dt).reshape(B, S, h, dh).transpose(1, 2)
    scale = dh ** -0.5
    t = attn_ref(hd(q, Hq, F64), hd(k, Hkv, F64), hd(v, Hkv, F64), allow, scale, False)
    e = attn_ref(hd(q, Hq, torch.float32), hd(k, Hkv, torch.float32), hd(v, Hkv, torch.float32), allow, scale, True)
    on = cpu(o).reshape(B, S, Hq, dh).transpose(1, 2)
    name = f"attn fwd {B}x{S} {Hq}/{Hkv} dh{dh} causal {causal} {mask} {value} hint {hint}"
    ratio = A.assert_row_budget(on, e.to(BF), t, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=name)
    dead = ~allow.any(-1)[:, 0]                                                   # [B, Sq]
    if dead.any():
        assert (on.transpose(1, 2)[dead] == 0).all(), f"{name}: a row without a visible key is not 0"
        assert torch.isneginf(cpu(lse).transpose(1, 2)[dead]).all(), f"{name}: lse of a row without a visible key is not -inf"
    s = (hd(q, Hq, F64) @ hd(k, Hkv, F64).repeat_interleave(Hq // Hkv, 1).transpose(-1, -2)) * scale
    tl = torch.logsumexp(s.masked_fill(~allow, float("-inf")), -1)
    ln = cpu(lse).to(F64)
    live = ~dead[:, None, :].expand_as(ln)
    err = ((ln - tl).abs() / tl.abs().clamp_min(1.0))[live]
    assert (err <= 1e-5).all(), f"{name}: lse {err.max():.2e} relative"
    return q, k, v, o, lse, km, allow, ratio


@pytest.mark.parametrize("hint", [False, True])
@pytest.mark.parametrize("B,S,Hq,Hkv,dh,causal,mask,value", ATTN_CASES + [(2, 32, 7, 1, 112, False, "isolated", "normal"),
                                                                          (1, 127, 7, 7, 112, False, "trailing", "peaked")])
def test_attention_fwd_rows(ops, B, S, Hq, Hkv, dh, causal, mask, value, hint):
    _attn_fwd_check(ops, B, S, Hq, Hkv, dh, causal, mask, value, hint)


def _attn_delta_floors(q, k, v, dout, allow, B, S, Hq, Hkv, dh):
    """Per-row absolute floors (dq [B, Hq, S], dk [B, Hkv, S]) of the bf16-O delta of the flash backward (accuracy.ATTN_DELTA_C)."""
    grp, scale = Hq // Hkv, dh ** -0.5
    hd = lambda t, h: t.to(F64).reshape(B, S, h, dh).transpose(1, 2)
    qq, kk, vv, do = hd(q, Hq), hd(k, Hkv).repeat_interleave(grp, 1), hd(v, Hkv).repeat_interleave(grp, 1), hd(dout, Hq)
    live = allow.any(-1, keepdim=True)
    s = torch.where(allow, (qq @ kk.transpose(-1, -2)) * scale, torch.full((), float("-inf"), dtype=F64))
    p = torch.softmax(torch.where(live, s, torch.zeros_like(s)), -1) * live
    g = do.norm(dim=-1) * (p @ vv).norm(dim=-1)                                   # |dO_i| |O_i|
    c = A.ATTN_DELTA_C * 2.0 ** -8 * scale
    fq = c * g * (p @ kk.norm(dim=-1, keepdim=True))[..., 0]
    fk = c * (p.transpose(-1, -2) @ (g * qq.norm(dim=-1))[..., None])[..., 0]
    return fq, fk.view(B, Hkv, grp, S).sum(2)


def _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, dt, emu):
    hd = lambda t, h: t.to(dt).reshape(B, S, h, dh).transpose(1, 2).clone().requires_grad_()
    qs, ks, vs = hd(q, Hq), hd(k, Hkv), hd(v, Hkv)
    attn_ref(qs, ks, vs, allow, dh ** -0.5, emu).backward(dout.to(dt).reshape(B, S, Hq, dh).transpose(1, 2))
    return qs.grad, ks.grad, vs.grad


@pytest.mark.parametrize("B,S,Hq,Hkv,dh,causal,mask,value", ATTN_CASES)
def test_attention_bwd_rows(ops, B, S, Hq, Hkv, dh, causal, mask, value):
    q, k, v, o, lse, km, allow, _ = _attn_fwd_check(ops, B, S, Hq, Hkv, dh, causal, mask, value, False, seed=2700)
    dout = gen(B, S, Hq * dh, seed=2701)
    kmd = km.to(torch.uint8).to(DEV) if mask != "none" else None
    dq, dk, dv = ops.attn_bwd(dout.to(DEV), q.to(DEV), k.to(DEV), v.to(DEV), o, lse, Hq, Hkv, dh, causal, kmd)
    tg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, F64, False)
    eg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, torch.float32, True)
    fq, fk = _attn_delta_floors(q, k, v, dout, allow, B, S, Hq, Hkv, dh)
    for nm, n, t, e, h, af in (("dq", dq, tg[0], eg[0], Hq, fq), ("dk", dk, tg[1], eg[1], Hkv, fk), ("dv", dv, tg[2], eg[2], Hkv, None)):
        nn = cpu(n).reshape(B, S, h, dh).transpose(1, 2)
        A.assert_row_budget(nn, e.to(BF), t, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=f"attn bwd {nm} {B}x{S} {mask} {value}", abs_floor=af)
    dead = ~allow.any(-1)[:, 0]
    if dead.any():
        assert (cpu(dq).reshape(B, S, Hq, dh)[dead] == 0).all(), "dq of a row without a visible key is not 0"
    keys_off = ~km
    if keys_off.any():
        assert (cpu(dk).reshape(B, S, Hkv, dh)[keys_off] == 0).all() and (cpu(dv).reshape(B, S, Hkv, dh)[keys_off] == 0).all(), "masked keys get gradient"


@pytest.mark.parametrize("S,row0,value", [(129, 32, "normal"), (352, 64, "peaked"), (369, 96, "sink@100")])
def test_attention_bwd_live_rows(ops, S, row0, value):
    B, Hq, Hkv, dh = 2, 14, 2, 64
    q, k, v, o, lse, km, allow, _ = _attn_fwd_check(ops, B, S, Hq, Hkv, dh, True, "none", value, False, seed=2800)
    dout = gen(B, S, Hq * dh, seed=2801)
    qd, od, dd = q.to(DEV)[:, row0:], o[:, row0:], dout.to(DEV)[:, row0:]
    dq, dk, dv = ops.attn_bwd(dd, qd, k.to(DEV), v.to(DEV), od, lse.contiguous(), Hq, Hkv, dh, True, None, row0=row0)
    tg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, F64, False)
    eg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, torch.float32, True)
    fq, fk = _attn_delta_floors(q, k, v, dout, allow, B, S, Hq, Hkv, dh)
    for nm, n, t, e, h, af in (("dq", dq, tg[0], eg[0], Hq, fq), ("dk", dk, tg[1], eg[1], Hkv, fk), ("dv", dv, tg[2], eg[2], Hkv, None)):
        nn = cpu(n).reshape(B, S - row0, h, dh).transpose(1, 2)
        A.assert_row_budget(nn, e[:, :, row0:].to(BF), t[:, :, row0:], 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=f"live-row {nm} S{S} row0 {row0}",
                            abs_floor=None if af is None else af[:, :, row0:])


@pytest.mark.parametrize("S,value", [(129, "normal"), (352, "peaked")])
def test_attention_bwd_fused_inverse_rope_rows(ops, S, value):
    B, Hq, Hkv, dh = 1, 14, 2, 64
    q, k, v, o, lse, km, allow, _ = _attn_fwd_check(ops, B, S, Hq, Hkv, dh, True, "none", value, False, seed=2900)
    dout = gen(B, S, Hq * dh, seed=2901)
    cos, sin = ops.rope_half_tables(S, dh, 1e6, DEV)
    dq, dk, dv = ops.attn_bwd(dout.to(DEV), q.to(DEV), k.to(DEV), v.to(DEV), o, lse, Hq, Hkv, dh, True, None, rope=(cos, sin))
    c, s = torch.cat([d64(cos)] * 2, -1), torch.cat([d64(sin)] * 2, -1)

    def inv(x):                       # transpose of rotate_half RoPE: x c + rot^T(x) s
        hh = dh // 2
        return x * c.to(x.dtype) + torch.cat([x[..., hh:], -x[..., :hh]], -1) * s.to(x.dtype)

    tg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, F64, False)
    eg = _attn_grads(q, k, v, dout, allow, B, S, Hq, Hkv, dh, torch.float32, True)
    fq, fk = _attn_delta_floors(q, k, v, dout, allow, B, S, Hq, Hkv, dh)     # (the rotation keeps a row's norm)
    for nm, n, t, e, h, af in (("dq", dq, inv(tg[0]), inv(eg[0]), Hq, fq), ("dk", dk, inv(tg[1]), inv(eg[1]), Hkv, fk)):
        nn = cpu(n).reshape(B, S, h, dh).transpose(1, 2)
        A.assert_row_budget(nn, e.to(BF), t, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=f"rope bwd {nm} S{S}", abs_floor=af)


# ------------------------------------------------------------------ e. head attention
def _st(x):
    """A declared bf16 rounding point inside an autograd graph: the rounded value, the gradient passed through (as the oracle's rnd)."""
    return x + (A.r64(x) - x).detach() if x.dtype == F64 else O.rnd(x, True)


def head_core(q, segs, tg, emu):
    """O.head_attention_core's math with the kernels' declared rounding points on the scores (rbf(q k), rbf(s tg) on the task
    segment, rbf(s / sqrt dh): csrc/head_attn_mfma.hip score_chain); emu=True adds the oracle's rounding of the weights and the
    output.  tg is the rounded tanh(gate) (a leaf: its gradient is taken to the gate by the caller)."""
    dh = q.shape[-1]
    sc = [_st(q @ k.transpose(-1, -2)) for k, _ in segs]
    sc[2] = _st(sc[2] * tg)
    w = torch.softmax(_st(torch.cat(sc, -1) / math.sqrt(dh)), -1)
    w = O.rnd(w, emu)
    return O.rnd(w @ torch.cat([v for _, v in segs], 2), emu)


def _gate_near_midpoint():
    """A bf16 gate whose tanh lies near a bf16 rounding midpoint: the kernels' rbf(tanh(gate)) then moves the task scores by ~2^-9,
    so a kernel that skips that rounding point is visible."""
    g = torch.arange(0.3, 1.0, 2 ** -8, dtype=F64).to(BF).unique()
    t = torch.tanh(g.to(F64))
    return g[((t - A.r64(t)).abs() / A.ulp_at(t)).argmax()]


def _head_inputs(B, T, Ka, Kt, H, dh, value, tg, seed):
    """[B, L, H, dh] float tensors.  value 'peaked': one adapter key and one task key aligned with every query, their (gated)
    scores ~30 and equal, so the weights split between the two segments and follow the task scores' gate factor."""
    g = torch.Generator().manual_seed(seed)
    sc = 0.3 if H * dh > 64 else 1.0
    r = lambda L: torch.randn(B, L, H, dh, generator=g) * sc
    q, ks, vs, ka, va, kt, vt = r(T), r(T), r(T), r(Ka), r(Ka), r(Kt), r(Kt)
    if value == "peaked":
        u = torch.randn(B, 1, H, dh, generator=g)
        q = u + 0.1 * q
        c = 30.0 / dh ** 0.5
        ka[:, Ka // 2] = c * u[:, 0]
        kt[:, Kt - 1] = c / tg * u[:, 0]
    return [t.to(BF) for t in (q, ks, vs, ka, va, kt, vt)]


HEAD_CASES = [  # B, T, Ka, Kt, D, value
    (2, 8, 31, 33, 64, "normal"), (3, 8, 32, 31, 256, "peaked"), (2, 8, 33, 32, 896, "normal"), (1, 8, 65, 33, 896, "peaked"),
    (2, 8, 65, 256, 1536, "normal"), (1, 8, 31, 40, 1536, "peaked"), (2, 8, 65, 512, 512, "normal"),
    # the MFMA kernels beyond the step's T = 8 (the VALU kernels refuse other T): the query contraction's second k-step (T > 16), a
    # ragged last key tile (Kt = 7), nineteen key tiles (Kt = 512: five workgroups per (sample, head), the last partly idle), head dim 16
    (2, 20, 65, 100, 1024, "normal"), (1, 32, 33, 7, 256, "normal"), (2, 8, 65, 512, 896, "normal"), (5, 8, 65, 16, 128, "normal")]


def _head_params():
    for m in ("mfma", "valu", "ref_softmax"):
        for i, c in enumerate(HEAD_CASES):
            if m == "valu" and (i >= 7 or c[4] > 896):     # (the VALU kernel: the first seven cases, head dims up to 112)
                continue
            B, T, Ka, Kt, D, value = c
            yield pytest.param(m, *c, id=f"{m}-{B}-{Ka}-{Kt}-{D}-{value}" if i < 7 else f"{m}-{B}-T{T}-{Ka}-{Kt}-{D}-{value}")


@pytest.mark.parametrize("mode,B,T,Ka,Kt,D,value", list(_head_params()))
def test_head_attention_rows(ops, monkeypatch, mode, B, T, Ka, Kt, D, value):
    """The action head's three-segment attention, forward and backward, per row against float64 (assert_row_budget, the attention
    family's constants) and the gate gradient against float64 under the same budget."""
    if mode == "valu":
        monkeypatch.setenv("VLA_HEAD_ATTN_VALU", "1")
    H = 8
    dh = D // H
    gate = _gate_near_midpoint().reshape(1)
    tgv = A.r64(torch.tanh(gate.to(F64)))
    ins = _head_inputs(B, T, Ka, Kt, H, dh, value, float(tgv), 4000 + D + Ka)
    dev = [t.reshape(t.shape[0], t.shape[1], D).to(DEV) for t in ins]
    out, probs = ops.head_attn_fwd(*dev, gate.to(DEV), H, ref_softmax=(mode == "ref_softmax"))
    dout = gen(B, T, D, seed=4001)
    grads = [torch.zeros_like(t) for t in dev]
    dgate = torch.zeros(1, device=DEV)
    ops.head_attn_bwd(dout.to(DEV), out, *dev, gate.to(DEV), probs, dgate, *grads, H)

    def run(dt, emu):
        leaves = [t.to(dt).transpose(1, 2).clone().requires_grad_() for t in ins]       # [B, H, L, dh]
        tg = tgv.to(dt).clone().requires_grad_()
        q, ks, vs, ka, va, kt, vt = leaves
        o = head_core(q, [(ks, vs), (ka, va), (kt, vt)], tg, emu)
        o.backward(dout.to(dt).reshape(B, T, H, dh).transpose(1, 2))
        dg = tg.grad * (1 - torch.tanh(gate.to(dt)) ** 2)          # d tanh / d gate at the unrounded tanh, as the kernels take it
        return o.detach(), [l.grad for l in leaves], dg

    to, tgr, tdg = run(F64, False)
    eo, egr, edg = run(torch.float32, True)
    name = f"head {mode} B{B} T{T} Ka{Ka} Kt{Kt} D{D} {value}"
    A.assert_row_budget(cpu(out).reshape(B, T, H, dh).transpose(1, 2), eo.to(BF), to, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=name + " out")
    # the flash backward's delta from the bf16 output (accuracy.ATTN_DELTA_C): per query / key row, as for the main attention
    qq = ins[0].to(F64).transpose(1, 2)
    keys = torch.cat([ins[1], ins[3], ins[5] * float(tgv)], 1).to(F64).transpose(1, 2)
    lg = torch.cat([_st(qq @ k.transpose(-1, -2)) for k in (ins[1].to(F64).transpose(1, 2), ins[3].to(F64).transpose(1, 2))]
                   + [_st(_st(qq @ ins[5].to(F64).transpose(1, 2).transpose(-1, -2)) * tgv)], -1)
    p = torch.softmax(_st(lg / math.sqrt(dh)), -1)
    gnorm = dout.to(F64).reshape(B, T, H, dh).transpose(1, 2).norm(dim=-1) * to.norm(dim=-1)
    c = A.ATTN_DELTA_C * 2.0 ** -8 / math.sqrt(dh)
    fq = c * gnorm * (p @ keys.norm(dim=-1, keepdim=True))[..., 0]
    fk = c * (p.transpose(-1, -2) @ (gnorm * qq.norm(dim=-1))[..., None])[..., 0]
    floors = [fq, fk[..., 0:T], None, fk[..., T:T + Ka], None, fk[..., T + Ka:], None]
    for nm, gn, t, e, af in zip(("dq", "dk_self", "dv_self", "dk_adp", "dv_adp", "dk_task", "dv_task"), grads, tgr, egr, floors):
        L = t.shape[2]
        A.assert_row_budget(cpu(gn).reshape(B, L, H, dh).transpose(1, 2), e.to(BF), t, 1, A.ATTN_FACTOR, A.ATTN_FLOOR,
                            name=f"{name} {nm}", abs_floor=af)
    A.assert_row_budget(cpu(dgate).to(F64), edg, tdg, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=f"{name} dgate")


# ------------------------------------------------------------------ f. elementwise kernels at argument extremes
def _extremes():
    sub = [2.0 ** -133, 2.0 ** -130, 3 * 2.0 ** -128]
    mags = [0.0] + sub + [1e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 12.0, 20.0, 50.0, 88.0, 89.0, 100.0, 1e4,
                          float(torch.finfo(BF).max)]
    vals = torch.tensor([s * m for m in mags for s in (1.0, -1.0)], dtype=torch.float32)
    fill = torch.linspace(-12, 12, 4096 - vals.numel())
    return torch.cat([vals, fill]).to(BF)


def test_gelu_extremes(ops):
    x = _extremes()
    y = ops.gelu_fwd(x.to(DEV))
    x64 = d64(x)
    t = gelu64(x64)
    fl = act_floor("gelu", x64, t)
    A.assert_contract(y, t, acc_floor=fl, max_frac=A.EW_MAX_FRAC, name="gelu", frac_where=fl < A.ulp_at(t) / 4)
    dy = gen(x.numel(), seed=3000)
    dx = ops.gelu_bwd(dy.to(DEV), x.to(DEV))
    dg = 0.5 * (1 + torch.erf(x64 / math.sqrt(2))) + x64 * torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
    td = d64(dy) * dg
    # 0.5 (1 + fast_erf) carries the A&S error absolutely; exp(-x^2 / 2) a x^2 u32 relative one
    fl = (A.GELU_ERF_ABS + EXP_C * U * dg.abs() * (1 + x64 * x64)) * d64(dy).abs() + FTZ
    A.assert_contract(dx, td, acc_floor=fl, max_frac=A.EW_MAX_FRAC, name="gelu bwd", frac_where=fl < A.ulp_at(td) / 4)


@pytest.mark.parametrize("act", ["gelu", "gelu_tanh", "relu"])
def test_gemm_activation_epilogue_extremes(ops, act):
    """The activation epilogue on pre-activations spanning the tails: A = identity rows, so acc = B row values exactly."""
    x = _extremes()
    x = x[torch.isfinite(x.float()) & (x.float().abs() < 1e30)]
    n = (x.numel() // 64) * 64
    vals = x[:n].view(-1, 64)                                   # [N, 64]: column c of output row r is vals[c, r]
    M = 64
    a = torch.eye(M).to(BF)
    out = ops.gemm_nt(a.to(DEV), vals.contiguous().to(DEV), act=ACTS[act][0])
    t, fl, mu, fw = _epilogue(d64(vals).t().contiguous(), torch.zeros(M, vals.shape[0], dtype=F64), None, act, None, 1.0, False)
    A.assert_contract(out, t, acc_floor=fl, max_ulp=mu, name=f"gemm {act} epilogue extremes", frac_where=fw)


def test_swiglu_and_relu_bwd_extremes(ops):
    x = _extremes()
    x = torch.where(x.float().abs() > 1e30, torch.zeros(()), x.float()).to(BF)     # (bf16 max * u overflows in the truth as well)
    M, I = 4, 1024
    g = x[:M * I].view(M, I)
    u = gen(M, I, seed=3100)
    gu = torch.stack([g.view(M, I // 16, 16), u.view(M, I // 16, 16)], dim=2).reshape(M, 2 * I)
    h = ops.swiglu_fwd(gu.to(DEV))
    g64, u64 = d64(g), d64(u)
    s = silu64(g64)
    sr, fls = A.round_point(s, act_floor("silu", g64, s))
    A.assert_contract(h, sr * u64, acc_floor=fls * u64.abs(), max_ulp=2, max_frac=A.EW_MAX_FRAC, name="swiglu fwd")
    dh = gen(M, I, seed=3101)
    dgu = cpu(ops.swiglu_bwd(dh.to(DEV), gu.to(DEV))).view(M, I // 16, 2, 16)
    sg = torch.sigmoid(g64)
    dg = d64(dh) * u64 * sg * (1 + g64 * (1 - sg))
    du = d64(dh) * g64 * sg
    # sg = rcp(1 + exp(-g)) is EXP_C u32 (1 + |g|) relative; 1 + g (1 - sg) cancels near g = -1.28 (|g| sg u32 absolute)
    flg = EXP_C * U * (d64(dh) * u64 * sg).abs() * (1 + g64.abs()) ** 2 + FTZ * (d64(dh) * u64).abs() * (1 + g64.abs())
    flu = EXP_C * U * (d64(dh) * g64 * sg).abs() * (1 + g64.abs()) + FTZ * (d64(dh) * g64).abs()
    A.assert_contract(dgu[:, :, 0].reshape(M, I), dg, acc_floor=flg, max_ulp=2, max_frac=A.EW_MAX_FRAC, name="swiglu bwd dg",
                      frac_where=flg < A.ulp_at(dg) / 4)
    A.assert_contract(dgu[:, :, 1].reshape(M, I), du, acc_floor=flu, max_ulp=2, max_frac=A.EW_MAX_FRAC, name="swiglu bwd du",
                      frac_where=flu < A.ulp_at(du) / 4)
    y = torch.relu(x.float()).to(BF)
    dy = gen(x.numel(), seed=3102)
    dx = ops.relu_bwd(dy.to(DEV), y.to(DEV))
    assert torch.equal(cpu(dx), torch.where(y.float() > 0, dy.float(), torch.zeros(())).to(BF)), "relu_bwd"


# ------------------------------------------------------------------ g. token cross-entropy
def _ce(ops, logits, labels, gscale=1.0):
    out2 = torch.zeros(2, dtype=torch.float32, device=DEV)
    rows, V = logits.shape
    L = ops._lib()
    ops.N.check(L.vla_token_ce(ops._st(), ops._p(logits), V, ops._p(labels), rows, V, ops._p(out2)), "token_ce")
    dl = torch.full_like(logits, float("nan"))
    ops.N.check(L.vla_token_ce_bwd(ops._st(), ops._p(logits), V, ops._p(labels), rows, V, ops._p(out2), gscale, ops._p(dl), V), "token_ce_bwd")
    return out2, dl


def _ce_logits(rows, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(rows, V, generator=g) * 160 - 80)                     # spread +-80
    x[1] = torch.randn(V, generator=g)
    x[1, 7] = 60.0                                                      # near one-hot
    x[2] = -80.0
    x[2, V - 1] = 80.0                                                  # the peak in the vector loop's tail
    return x.to(BF)


@pytest.mark.parametrize("V", [151936, 2056, 136])
def test_token_ce_rows(ops, V):
    rows = 6
    x = _ce_logits(rows, V, 3200 + V)
    labels = torch.tensor([3, 7, V - 1, -100, V - 2, 0], dtype=torch.int64)
    x64 = d64(x)
    ls = torch.log_softmax(x64, -1)
    valid = labels >= 0
    for r in range(rows):                                               # the per-row loss: one valid row per launch
        lab = torch.full((rows,), -100, dtype=torch.int64)
        lab[r] = labels[r]
        out2, _ = _ce(ops, x.to(DEV), lab.to(DEV))
        o = cpu(out2).to(F64)
        if valid[r]:
            t = -ls[r, labels[r]]
            assert o[1] == 1 and (o[0] - t).abs() <= 1e-5 * t.abs().clamp_min(1.0), f"CE row {r}: {o[0].item()} vs {t.item()}"
        else:
            assert (o == 0).all()
    gscale = 0.5
    out2, dl = _ce(ops, x.to(DEV), labels.to(DEV), gscale)
    cnt = int(valid.sum())
    assert cpu(out2)[1].item() == cnt
    oh = torch.zeros_like(x64)
    oh[valid, labels[valid]] = 1
    p = ls.exp()
    t = torch.where(valid[:, None], (p - oh) * gscale / cnt, torch.zeros_like(p))
    # exp(x - m) is EXP_C u32 (1 + |x - m|) relative, the row sum sqrt(V) u32; p - 1 at the label cancels (absolute u32 there)
    arg = (x64 - x64.max(-1, keepdim=True).values).abs()
    fl = (EXP_C * U * (p * (1 + arg + math.sqrt(V)) + oh) + FTZ) * gscale / cnt * valid[:, None]
    A.assert_contract(dl, t, acc_floor=fl, max_frac=A.EW_MAX_FRAC, name=f"CE bwd V {V}", frac_where=fl < A.ulp_at(t) / 4)
    assert (cpu(dl)[~valid] == 0).all(), "ignored rows get zero gradient"


def test_token_ce_every_row_ignored(ops):
    x = _ce_logits(4, 2056, 3300)
    out2, dl = _ce(ops, x.to(DEV), torch.full((4,), -100, dtype=torch.int64, device=DEV))
    assert (cpu(out2) == 0).all()
    assert (cpu(dl).float() == 0).all() and torch.isfinite(cpu(dl).float()).all()


# ------------------------------------------------------------------ 3. kernels reached only end to end
def test_embed_grad_direct(ops):
    """vla_embed_grad OVERWRITES the table row of every id that occurs (it does not add to it): the first position holding an id owns
    the row and writes the fp32 position-order sum of that id's dX rows, rounded once; rows of ids that do not occur are untouched."""
    B, L, Np, D, vocab = 3, 9, 4, 136, 50
    S = L + Np
    ids = torch.tensor([[5, 7, 5, 9, 60, -3, 11, 12, 5],
                        [7, 7, 13, 5, 14, 15, 9, 16, 0],
                        [17, 18, 19, 20, 21, 22, 23, 24, 25]], dtype=torch.int64)
    qidx = torch.full((B, L), -1, dtype=torch.int32)
    qidx[0, 7] = 0                      # id 12 occurs only in action-query slots
    qidx[1, 8] = 1
    qidx[2, 1:4] = torch.tensor([2, 3, 4], dtype=torch.int32)    # ids 18-20 likewise
    qidx[1, 2] = 5                      # id 13 too; and a repeated id (7) shares a sample
    dx = gen(B, S, D, seed=3400, scale=3.0)
    table = gen(vocab, D, seed=3401)
    gt = table.to(DEV).clone()
    dxd, idd, qd = dx.to(DEV), ids.to(DEV), qidx.to(DEV)
    ops.N.check(ops._lib().vla_embed_grad(ops._st(), ops._p(dxd), ops._p(idd), ops._p(qd), ops._p(gt), B, L, Np, D, vocab), "embed_grad")
    exp = table.clone()
    acc = {}
    for b in range(B):
        for j in range(L):
            if qidx[b, j] >= 0:
                continue
            i = int(ids[b, j])
            i = 0 if (i < 0 or i >= vocab) else i
            row = dx[b, 0 if j == 0 else Np + j].float()
            acc[i] = row.clone() if i not in acc else acc[i] + row      # fp32, position order
    for i, a in acc.items():
        exp[i] = a.to(BF)
    assert 12 not in acc and 13 not in acc and 18 not in acc and 0 in acc
    assert torch.equal(cpu(gt).view(torch.int16), exp.view(torch.int16)), "embed_grad differs from the fp32 position-order sum"


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_bwd_add_direct(ops, p):
    rows, cols, seed = 37, 136, 12345
    u, dx0 = gen(rows, cols, seed=3500), gen(rows, cols, seed=3501)
    step = torch.tensor([3], dtype=torch.int32, device=DEV)
    y = ops.dropout(u.to(DEV), torch.empty(rows, cols, dtype=BF, device=DEV), p, seed, step)
    keep = cpu(y).float() != 0
    assert 0.3 * p < 1 - keep.float().mean().item() < 2 * p + 0.05
    dx = dx0.to(DEV).clone()
    ops.dropout_bwd_add_(dx, u.to(DEV), p, seed, step)
    exp = (dx0.float() + cpu(y).float()).to(BF)                 # y = bf16(u / (1 - p)) on the kept positions
    assert torch.equal(cpu(dx).view(torch.int16), exp.view(torch.int16)), "dropout_bwd_add: mask or sum differs from dropout's"
    step2 = torch.tensor([4], dtype=torch.int32, device=DEV)
    y2 = ops.dropout(u.to(DEV), torch.empty(rows, cols, dtype=BF, device=DEV), p, seed, step2)
    assert not torch.equal(y2, y), "the step is part of the mask's key"


@pytest.mark.parametrize("row0", [0, 32, 64])
def test_head_index_prep_direct(ops, row0):
    B, S, Np = 3, 120, 20
    g = torch.Generator().manual_seed(3600 + row0)
    pos1 = torch.randint(0, S - Np, (B, 64), generator=g, dtype=torch.int32)
    pos1[1, 60:] = -1
    pos0 = torch.randint(0, S - Np, (B, 64), generator=g, dtype=torch.int32)
    cnt0 = torch.tensor([3, 0, 5], dtype=torch.int32)
    gather = torch.full((B * 65,), 7777, dtype=torch.int32, device=DEV)
    scatter = torch.full((B * 65,), 7777, dtype=torch.int32, device=DEV)
    guard = torch.full((1,), 5.0, dtype=torch.float32, device=DEV)
    ops.head_index_prep(pos1.to(DEV), pos0.to(DEV), cnt0.to(DEV), gather, scatter, guard, B, S, Np, row0)
    eg, es = torch.empty(B, 65, dtype=torch.int32), torch.empty(B, 65, dtype=torch.int32)
    for b in range(B):
        for k in range(64):
            p = int(pos1[b, k])
            eg[b, k] = b * S + Np + p
            loc = Np + p - row0
            es[b, k] = b * (S - row0) + loc if (loc >= 0 and p >= 0) else -1
        eg[b, 64], es[b, 64] = -2, -1
    assert torch.equal(cpu(gather).view(B, 65), eg) and torch.equal(cpu(scatter).view(B, 65), es)
    bad = any(row0 > 0 and ((int(pos0[b, 0]) + Np) if cnt0[b] > 0 else 0) < row0 for b in range(B))
    gv = cpu(guard).item()
    assert (math.isnan(gv) if bad else gv == 0.0), f"guard {gv}, expected {'NaN' if bad else 0}"
