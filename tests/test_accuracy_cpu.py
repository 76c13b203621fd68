"""The accuracy criteria of tests/accuracy.py, proven on the CPU: they accept the fp32 bf16-emulating oracle and reject
evaluations with one extra rounding, the wrong variance or one wrong row - faults that the aggregate check() of
test_kernels_gpu.py lets through (see the docstrings of the cases)."""
import pytest
import torch

from oracle import vla_oracle as O
from tests import accuracy as A

BF = torch.bfloat16
F64 = torch.float64


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def agg_rel(x, ref):
    x, ref = x.float(), ref.float()
    return ((x - ref).norm() / ref.norm()).item()


# ------------------------------------------------------------------ the bit tools
def test_ordinal_and_ulp_distance():
    x = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.0, -1.0], dtype=torch.float32).to(BF)
    assert A.ordinal(x).tolist()[:2] == [0, 0], "+0 and -0 are the same point"
    assert A.ulp_distance(x[2:3], x[0:1]).item() == 1, "the smallest subnormal is one ulp from zero"
    assert A.ulp_distance(x[3:4], x[2:3]).item() == 2
    one = torch.tensor([1.0]).to(BF)
    nxt = A.from_ordinal(A.ordinal(one) + 1)
    assert nxt.float().item() == 1.0 + 2 ** -7
    assert A.ulp_distance(torch.tensor([1.0]).to(BF), torch.tensor([-1.0]).to(BF)).item() == 2 * A.ordinal(one).item()


def test_rne_rounds_once():
    # float64 -> float32 -> bf16 rounds a value just above a bf16 midpoint down to the midpoint, then to even: wrong
    t = torch.tensor([1 + 2 ** -8 + 2 ** -30, 1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8 + 2 ** -30), 3.0e38, 1e-45], dtype=F64)
    assert A.rne(t).float().tolist() == [1 + 2 ** -7, 1.0, 1 + 2 ** -6, -(1 + 2 ** -7), A.rne(t[4:5]).float().item(), 0.0]
    assert t[:1].float().to(BF).float().item() == 1.0


def test_contract_rejects_non_finite():
    t = torch.ones(4, dtype=F64)
    for bad in (float("nan"), float("inf")):
        n = torch.ones(4).to(BF)
        n[2] = bad
        with pytest.raises(AssertionError, match="non-finite"):
            A.assert_contract(n, t, name="x")


# ------------------------------------------------------------------ GEMM: fp32 accumulate, round once after the bias
def _gemm_case(M, N, K):
    a, b, bias = gen(M, K, seed=1), gen(N, K, seed=2, scale=0.05), gen(N, seed=3)
    truth = a.to(F64) @ b.to(F64).t() + bias.to(F64)
    return a, b, bias, truth, A.acc_floor(a, b)


@pytest.mark.parametrize("M,N,K", [(300, 200, 192), (256, 384, 128), (64, 72, 8960)])
def test_contract_accepts_the_fp32_oracle(M, N, K):
    a, b, bias, truth, fl = _gemm_case(M, N, K)
    emu = O.linear(a.float(), b.float(), bias.float(), emu=True).to(BF)
    frac = A.assert_contract(emu, truth, acc_floor=fl, name=f"oracle {M}x{N}x{K}")
    assert frac < A.GEMM_MAX_FRAC / 10, "a correct fp32 evaluation flips far fewer outputs than the bound"


def test_acc_floor_bounds_an_fp32_sum_at_long_k():
    """The fp32 error floor holds the unrounded fp32 product at K = 8960 with margin, and it is not vacuous: it is far below one bf16
    ulp of most outputs, so only outputs that cancel towards zero use it."""
    a, b, bias, truth, fl = _gemm_case(64, 72, 8960)
    y32 = (a.float() @ b.float().t() + bias.float()).double()
    ratio = ((y32 - truth).abs() / fl).max().item()
    assert ratio < 0.25, f"fp32 error / floor = {ratio:.3f}"
    assert (fl < A.ulp_at(truth)).float().mean() > 0.75


def test_contract_rejects_bf16_split_k_partials():
    """Split-K partials rounded to bf16 before the reduction: rel-L2 1.9e-3 against the emu oracle - check() accepts it."""
    M, N, K = 300, 200, 192
    a, b, bias, truth, fl = _gemm_case(M, N, K)
    parts = [(a[:, z:z + 64].float() @ b[:, z:z + 64].float().t()).to(BF).float() for z in range(0, K, 64)]
    bad_out = (sum(parts) + bias.float()).to(BF)
    emu = O.linear(a.float(), b.float(), bias.float(), emu=True)
    assert agg_rel(bad_out, emu) <= 2e-3, "the aggregate criterion does not see it"
    _, frac, _ = A.contract_stats(bad_out, truth, fl)
    assert frac > 5 * A.GEMM_MAX_FRAC
    with pytest.raises(AssertionError):
        A.assert_contract(bad_out, truth, acc_floor=fl, name="bf16 split-K partials")


def test_contract_rejects_rounding_before_the_bias():
    M, N, K = 300, 200, 192
    a, b, bias, truth, fl = _gemm_case(M, N, K)
    bad_out = ((a.float() @ b.float().t()).to(BF).float() + bias.float()).to(BF)
    emu = O.linear(a.float(), b.float(), bias.float(), emu=True)
    assert agg_rel(bad_out, emu) <= 3e-3, "within a hair of the aggregate limit"
    _, frac, _ = A.contract_stats(bad_out, truth, fl)
    assert frac > 10 * A.GEMM_MAX_FRAC
    with pytest.raises(AssertionError):
        A.assert_contract(bad_out, truth, acc_floor=fl, name="rounded before bias")


# ------------------------------------------------------------------ attention backward: the row budget
ATTN_SHAPE = (1, 352, 14, 2, 64)


def _attn_grads(q, k, v, dout, causal, dtype, emu):
    q, k, v = (t.to(dtype).requires_grad_() for t in (q, k, v))
    o = O.attention(q, k, v, causal, emu=emu)
    o.backward(dout.to(dtype))
    return o.detach(), q.grad, k.grad, v.grad


def test_row_budget_accepts_oracle_and_rejects_one_wrong_dq_row():
    """dq with one query row 15 % off: rel-L2 5.1e-3 (limit 1e-2) and max 1.4e-2 (limit 5e-2) - test_attention_bwd accepts it."""
    B, S, H, KV, dh = ATTN_SHAPE
    q, k, v = gen(B, H, S, dh, seed=20), gen(B, KV, S, dh, seed=21), gen(B, KV, S, dh, seed=22)
    dout = gen(B, H, S, dh, seed=23)
    _, dq64, _, _ = _attn_grads(q, k, v, dout, True, F64, False)
    _, dqe, _, _ = _attn_grads(q, k, v, dout, True, torch.float32, True)
    emu = dqe.to(BF)
    A.assert_row_budget(emu, emu, dq64, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name="oracle dq")
    _, dq32, _, _ = _attn_grads(q, k, v, dout, True, torch.float32, False)
    A.assert_row_budget(dq32.to(BF), emu, dq64, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name="fp32 dq")   # another valid evaluation
    bad = emu.float().clone()
    bad[0, 5, 200] *= 1.15
    bad = bad.to(BF)
    r = agg_rel(bad, dqe)
    assert r <= 1e-2, f"the aggregate criterion does not see it ({r:.2e})"
    with pytest.raises(AssertionError, match="rows over budget"):
        A.assert_row_budget(bad, emu, dq64, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name="dq, one row 15 % off")


# ------------------------------------------------------------------ LayerNorm: biased variance, one rounding
def _ln_truth(x, w, b, eps):
    x64 = x.to(F64)
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xh = (x64 - mu) * rstd
    return xh * w.to(F64) + b.to(F64), xh, mu, rstd


@pytest.mark.parametrize("cols", [64, 1152])
def test_contract_rejects_unbiased_layernorm(cols):
    """LayerNorm with var / (cols - 1): 97 % (cols 64) and 9 % (cols 1152) of the outputs differ from RN(truth), ~1e-4 for the oracle."""
    rows, eps = 96, 1e-6
    x, w, b = gen(rows, cols, seed=30), gen(cols, seed=31), gen(cols, seed=32, scale=0.1)
    truth, xh, mu64, rstd64 = _ln_truth(x, w, b, eps)
    fl = A.norm_floor(xh, w, b, mu64, rstd64)
    emu = O.layer_norm(x.float(), w.float(), b.float(), eps, emu=True).to(BF)
    assert A.assert_contract(emu, truth, acc_floor=fl, max_frac=A.NORM_MAX_FRAC, name="oracle LN") < A.NORM_MAX_FRAC / 10
    xf = x.float()
    mu = xf.mean(-1, keepdim=True)
    var = ((xf - mu) ** 2).sum(-1, keepdim=True) / (cols - 1)
    bad = ((xf - mu) * torch.rsqrt(var + eps) * w.float() + b.float()).to(BF)
    _, frac, _ = A.contract_stats(bad, truth, fl)
    assert frac > 5 * A.NORM_MAX_FRAC
    with pytest.raises(AssertionError):
        A.assert_contract(bad, truth, acc_floor=fl, max_frac=A.NORM_MAX_FRAC, name="unbiased LN")


def test_row_budget_rejects_one_wrong_layernorm_row():
    """A LayerNorm output with one row 1 % off passes test_layernorm (rel-L2 1.6e-3, max 8.6e-3 against 2e-3 and 1.56e-2)."""
    x, w, b = gen(64, 1152, seed=30), gen(1152, seed=31), gen(1152, seed=32, scale=0.1)
    truth = _ln_truth(x, w, b, 1e-6)[0]
    emu = O.layer_norm(x.float(), w.float(), b.float(), 1e-6, emu=True).to(BF)
    bad = emu.float().clone()
    bad[63] *= 1.01
    with pytest.raises(AssertionError, match="rows over budget"):
        A.assert_row_budget(bad.to(BF), emu, truth, 1, A.NORM_FACTOR, A.NORM_FLOOR, name="LN, one row 1 % off")


# ------------------------------------------------------------------ activation tails: the floors follow y, not x
def _extremes():
    mags = [0.0, 2.0 ** -133, 1e-3, 0.5, 1.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 50.0, 88.0, 89.0, 1e4]
    x = torch.tensor([s * m for m in mags for s in (1.0, -1.0)], dtype=torch.float32)
    return torch.cat([x, torch.linspace(-12, 12, 4001)]).to(BF)


def _gelu_tanh_fp32(x, coef):
    """The kernel's formula (csrc/common.h gelu_tanh) evaluated in fp32."""
    x = x.float()
    k = 1.5957691216057308
    u2 = x * (x * x * (coef * k) + k)
    return x * torch.reciprocal(1.0 + torch.exp2(u2 * -1.4426950408889634))


def test_act_floor_accepts_gelu_tanh_and_rejects_a_wrong_coefficient():
    """gelu_tanh in fp32 with 0.044715 meets the contract; with 0.0447 (a relative error of ~1e-3 in u, growing with |x|^3 in the
    tail) it does not.  A floor absolute in x would let the whole negative tail through."""
    x = _extremes()
    x64 = x.to(F64)
    t = x64 * torch.sigmoid(A.gelu_tanh_arg(x64))               # 0.5 x (1 + tanh u) without the cancellation
    fl = A.act_floor("gelu_tanh", x64, t)
    fw = fl < A.ulp_at(t) / 4
    assert A.assert_contract(_gelu_tanh_fp32(x, 0.044715).to(BF), t, acc_floor=fl, max_frac=A.EW_MAX_FRAC, frac_where=fw,
                             name="gelu_tanh") == 0.0
    bad, _, worst = A.contract_stats(_gelu_tanh_fp32(x, 0.0447).to(BF), t, fl, 1, fw)
    assert bad.any() and worst > 1, "the wrong coefficient is visible per element"
    tail = (x64 < -3) & (t.abs() > 2.0 ** -100)                 # (below that the subnormal flush of rcp / exp is the floor)
    assert (fl[tail] < A.ulp_at(t[tail]) / 4).all(), "the floor stays below a quarter ulp in the negative tail"


def test_act_floor_accepts_silu_tail():
    x = _extremes()
    x64 = x.to(F64)
    t = x64 * torch.sigmoid(x64)
    xf = x.float()
    y = (xf * torch.reciprocal(1.0 + torch.exp(-xf))).to(BF)
    A.assert_contract(y, t, acc_floor=A.act_floor("silu", x64, t), max_frac=A.EW_MAX_FRAC, name="silu")
