"""Element-wise and row-wise accuracy criteria against a float64 truth (imported by the kernel tests; not a conftest).

The aggregate check() of test_kernels_gpu.py (rel-L2 <= 2e-3 against the bf16-emulating oracle) cannot tell "fp32 accumulate,
round once" from "one extra bf16 rounding somewhere" (one rounding alone is ~1.7e-3 rel-L2), and a wrong row hardly moves an
aggregate.  The two criteria here do:

* assert_contract: the op evaluated in float64 from the exact bf16 inputs, rounded to nearest even (RN) only at the op's declared
  bf16 rounding points and at the output, is the truth.  Every element must be within max_ulp of RN(truth) - or, where the output
  cancels towards zero, within an a-priori fp32 error floor of the truth - and at most max_frac of the elements may differ from
  RN(truth) at all.
* assert_row_budget: for kernels whose internal rounding points legitimately differ from the oracle's (flash-style P, the
  attention / head backward passes, the norm backward), every row's relative error against float64 must stay within
  factor x the bf16-emulating oracle's own error on that row, plus floor.

tests/test_accuracy_cpu.py shows on the CPU that these constants accept the fp32 oracle and reject faulty variants.
"""
import math

import torch

BF = torch.bfloat16
U32 = 2.0 ** -24                 # fp32 unit roundoff

# GEMM family: outputs differing from RN(truth).  A correct fp32 evaluation flips ~1e-4 of them (a result within its fp32 error
# of a bf16 rounding midpoint); rounding the accumulator before the bias flips 27-38 %, bf16 split-K partials ~30 %
# (test_accuracy_cpu.py measures all three).
GEMM_MAX_FRAC = 0.01
# fp32 accumulation over K terms: |err| <= ACC_C sqrt(K) u32 sum|a||b|.  A correct fp32 evaluation on the CPU was up to 31 ulp off
# RN(truth) at K = 8960 where the output cancels; the bound below covers it with margin (test_accuracy_cpu.py).
ACC_C = 4.0
# affine tail of a norm, (x - mean) rstd w + b in fp32: a few fp32 ulps of |x^ w| + |b|, plus the fp32 error of the mean carried
# into x - mean (sqrt(cols) u32 |mean| rstd |w|)
NORM_C = 8.0
# norm forward outputs differing from RN(truth): 0 % for the fp32 oracle; 97 % (cols 64) and 9 % (cols 1152) for a LayerNorm with
# the unbiased variance (test_accuracy_cpu.py)
NORM_MAX_FRAC = 0.01

# Row budgets (assert_row_budget): one factor per family.  The floor is one bf16 ulp (2^-8) of relative error: a row the emu oracle
# happens to get exact (one visible key, a constant row) may still be one rounding off in a valid kernel.
# attention forward / backward: the flash kernels round P (and dS) at other points than the oracle's softmax -> bf16 P -> P V.
ATTN_FACTOR = 2.0
ATTN_FLOOR = 2.0 ** -8
# norm backward dx: fp32 row sums in another order, one rounding at the output (the oracle's autograd rounds dx once too)
NORM_FACTOR = 2.0
NORM_FLOOR = 2.0 ** -8
# attention backward: the flash formulation forms delta_i = rowsum(dO_i * O_i) from the stored bf16 O, whose rounding is at most
# 2^-9 relative; dS_ij = P_ij (dP_ij - delta_i) then carries an absolute error up to P_ij 2^-9 |dO_i| |O_i|.  The per-row allowance
# is ATTN_DELTA_C x 2^-8 x that product (twice the bound): it is the whole gradient where the truth cancels, so on a peaked softmax
# (one key takes nearly all the weight, dq nearly 0) the dq rows are checked only to this absolute level, not relatively.
ATTN_DELTA_C = 2.0


# Activations: the documented approximations of csrc/common.h, the only deviations from RN(truth) a correct kernel may show.
# gelu_erf: Abramowitz-Stegun 7.1.26 erf, |abs err| <= 1.5e-7 -> |gelu err| <= 0.75e-7 |x|: 1-4 bf16 ulp for x <= -5, where
# |gelu| < 1.5e-6.
GELU_ERF_ABS = 1.0e-7
# gelu_tanh = x rcp(1 + exp2(-2u log2 e)) and silu = x rcp(1 + exp(-x)) do not cancel, so their error is relative to y: the
# argument a (2u, or x) carries a few u32 of relative rounding, which exp turns into a |a| u32 relative error of y; exp2, rcp and
# the products add ~1 ulp each.  |dy| <= EXP_C u32 |y| (1 + |a|).
EXP_C = 8.0
# v_rcp_f32 / v_exp_f32 flush fp32 subnormals: where the true sigmoid is below 2^-126 the kernel may return 0 (|y| < 2^-126 |x|).
FTZ = 2.0 ** -126
# elementwise family (activations, their gradients, the CE gradient): outputs differing from RN(truth), counted where the floor is
# below a quarter ulp.  An fp32 evaluation of the kernels' formulas flips none of the extremes inputs (test_accuracy_cpu.py); the
# gelu_tanh coefficient 0.0447 instead of 0.044715 fails the per-element bound there.
EW_MAX_FRAC = 0.01


def gelu_tanh_arg(x: torch.Tensor) -> torch.Tensor:
    """2u = sqrt(8 / pi) (x + 0.044715 x^3), the argument of gelu_tanh's sigmoid (float64)."""
    return math.sqrt(8.0 / math.pi) * (x + 0.044715 * x ** 3)


def act_floor(act: str, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """fp32 evaluation error of an activation at x (float64), y = act(x) (float64)."""
    if act == "gelu":
        return GELU_ERF_ABS * x.abs() + EXP_C * U32 * y.abs() + FTZ * x.abs()
    if act == "gelu_tanh":
        return EXP_C * U32 * y.abs() * (1 + gelu_tanh_arg(x).abs()) + FTZ * x.abs()
    if act == "silu":
        return EXP_C * U32 * y.abs() * (1 + x.abs()) + FTZ * x.abs()
    return torch.zeros_like(x)


# ------------------------------------------------------------------ bf16 bit tools
def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.detach().to(BF).cpu().contiguous().view(torch.int16).to(torch.int32)


def ordinal(x: torch.Tensor) -> torch.Tensor:
    """bf16 -> monotone integer: consecutive bf16 values differ by 1, +0 and -0 are both 0, the smallest subnormal is 1."""
    b = _bits(x)
    mag = b & 0x7FFF
    return torch.where(b < 0, -mag, mag)


def from_ordinal(o: torch.Tensor) -> torch.Tensor:
    bits = torch.where(o < 0, (-o) | 0x8000, o).to(torch.int32)
    bits = torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16)
    return bits.view(BF)


def ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|ordinal(a) - ordinal(b)| elementwise (int64).  NaN / Inf are not judged here: assert_contract rejects them first."""
    return (ordinal(a).to(torch.int64) - ordinal(b).to(torch.int64)).abs()


def rne(t: torch.Tensor) -> torch.Tensor:
    """float64 -> bf16, rounded to nearest even ONCE (float64 -> float32 -> bf16 rounds twice, and differs at bf16 midpoints)."""
    t = t.detach().to(torch.float64).cpu()
    o = ordinal(t.to(torch.float32).to(BF)).to(torch.int64)
    best, bd = o, (from_ordinal(o).to(torch.float64) - t).abs()
    for step in (-1, 1):
        c = o + step
        cd = (from_ordinal(c.clamp(-0x7F80, 0x7F80)).to(torch.float64) - t).abs()
        take = (cd < bd) | ((cd == bd) & (c % 2 == 0) & (c.abs() <= 0x7F80))
        best, bd = torch.where(take, c, best), torch.where(take, cd, bd)
    return from_ordinal(torch.where(torch.isfinite(t), best, o))


def ulp_at(t: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |t| (float64): the step from RN(|t|) to the next bf16 value up."""
    o = ordinal(rne(t.abs())).to(torch.int64)
    return (from_ordinal(o + 1).to(torch.float64) - from_ordinal(o).to(torch.float64)).abs()


def r64(t: torch.Tensor) -> torch.Tensor:
    """A declared bf16 rounding point inside a float64 truth: RN, back to float64."""
    return rne(t).to(torch.float64)


def round_point(t: torch.Tensor, floor: torch.Tensor):
    """A bf16 rounding point on a value known only to +-floor (fp32 evaluation error): (RN(t) in float64, floor after the point).
    Where t lies within floor of a rounding midpoint a correct kernel may round either way, so the floor after the point is the floor
    plus one ulp there; elsewhere the rounding absorbs the fp32 error and the floor is 0."""
    r = r64(t)
    mid_dist = (ulp_at(t) / 2 - (t - r).abs()).abs()
    return r, torch.where(mid_dist <= floor, floor + ulp_at(t), torch.zeros_like(t))


def acc_floor(a: torch.Tensor, b: torch.Tensor, c=ACC_C) -> torch.Tensor:
    """A priori error bound of an fp32-accumulated a @ b^T (float64 [M, N]): c sqrt(K) u32 (|a| @ |b|^T)."""
    a, b = a.detach().to(torch.float64).cpu(), b.detach().to(torch.float64).cpu()
    return c * math.sqrt(a.shape[-1]) * U32 * (a.abs() @ b.abs().transpose(-1, -2))


def norm_floor(xh: torch.Tensor, w: torch.Tensor, b, mean: torch.Tensor, rstd: torch.Tensor) -> torch.Tensor:
    """A priori fp32 error of a norm's affine tail x^ w + b (float64 x^ = (x - mean) rstd, mean / rstd [rows, 1] the float64
    statistics): NORM_C fp32 ulps of |x^ w| + |b|, plus the fp32 error of the mean (sqrt(cols) u32 |mean|) scaled by rstd |w|."""
    w64 = w.detach().to(torch.float64).cpu()
    fl = (xh * w64).abs() + math.sqrt(xh.shape[-1]) * mean.abs() * rstd * w64.abs()
    if b is not None:
        fl = fl + b.detach().to(torch.float64).cpu().abs()
    return NORM_C * U32 * fl


# ------------------------------------------------------------------ the criteria
def _finite(x: torch.Tensor, name: str):
    x = x.detach().float().cpu()
    bad = ~torch.isfinite(x)
    assert not bad.any(), f"{name}: {int(bad.sum())} non-finite outputs (first at {bad.nonzero()[0].tolist()})"


def contract_stats(native: torch.Tensor, truth64: torch.Tensor, floor=None, max_ulp: int = 1, frac_where=None):
    """(elements violating the contract, fraction differing from RN(truth), worst ulp distance outside the floor).
    frac_where: the elements the fraction counts (default all) - for approximations whose documented floor exceeds an ulp on part of
    the range, the elements where the floor is below the rounding step."""
    t = truth64.detach().to(torch.float64).cpu()
    n = native.detach().cpu()
    assert n.shape == t.shape, f"shape {tuple(n.shape)} vs {tuple(t.shape)}"
    d = ulp_distance(n, rne(t))
    ok = d <= max_ulp
    if floor is not None:
        fl = torch.as_tensor(floor, dtype=torch.float64).cpu().expand_as(t)
        ok = ok | ((n.to(torch.float64) - t).abs() <= fl + ulp_at(t))
    worst = int(d[~ok].max()) if (~ok).any() else int(d[ok].max()) if d.numel() else 0
    dd = d if frac_where is None else d[frac_where]
    return ~ok, (dd != 0).double().mean().item() if dd.numel() else 0.0, worst


def assert_contract(native: torch.Tensor, truth64: torch.Tensor, *, acc_floor=None, max_ulp: int = 1, max_frac: float = GEMM_MAX_FRAC,
                    name: str = "", frac_where=None):
    """native (bf16) against RN(truth64).  acc_floor: float64 tensor (broadcastable) of the op's a-priori fp32 error, or None."""
    _finite(native, name)
    bad, frac, worst = contract_stats(native, truth64, acc_floor, max_ulp, frac_where)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        n, t = native.detach().cpu()[tuple(i)].item(), truth64.detach().cpu()[tuple(i)].item()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements more than {max_ulp} ulp from RN(truth) outside the "
                             f"fp32 floor (worst {worst} ulp); first at {i}: native {n!r}, truth {t!r}")
    assert frac <= max_frac, f"{name}: {frac:.2%} of the elements differ from RN(truth) (<= {max_frac:.2%})"
    return frac


def row_errors(x: torch.Tensor, truth64: torch.Tensor, row_dims: int = 1, den_floor: float = 1e-30):
    """Relative L2 error of every row (the trailing row_dims dimensions form one row) against float64."""
    t = truth64.detach().to(torch.float64).cpu()
    x = x.detach().to(torch.float64).cpu()
    lead = t.shape[:t.dim() - row_dims]
    t, x = t.reshape(*lead, -1), x.reshape(*lead, -1)
    return (x - t).norm(dim=-1) / t.norm(dim=-1).clamp_min(den_floor)


def assert_row_budget(native, emu, truth64, row_dims: int, factor: float, floor: float, name: str = "", abs_floor=None):
    """Every row: rel-err(native) <= factor x rel-err(emu) + floor (both against float64).  abs_floor (per row, float64): an
    a-priori absolute error of the kernel's formulation, for rows whose truth cancels towards zero (divided by the row's norm here).
    Returns the worst ratio rel-err(native) / limit, which is <= 1 when it passes."""
    _finite(native, name)
    en, ee = row_errors(native, truth64, row_dims), row_errors(emu, truth64, row_dims)
    lim = factor * ee + floor
    if abs_floor is not None:
        t = truth64.detach().to(torch.float64).cpu()
        tn = t.reshape(*t.shape[:t.dim() - row_dims], -1).norm(dim=-1).clamp_min(1e-30)
        lim = lim + abs_floor / tn
    bad = en > lim
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} rows over budget; first row {i}: native {en[tuple(i)]:.3e}, "
                             f"emu {ee[tuple(i)]:.3e} (x{factor} + {floor})")
    return (en / lim).max().item() if en.numel() else 0.0
