"""Tensor-level wrappers over the C ABI: pointer/stride plumbing only (PyTorch owns memory and the stream).

Every function launches on ``torch.cuda.current_stream()`` and raises on failure.  Shapes are validated here
(host side) before any kernel is launched.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import native as N
from .native import ACT_GELU, ACT_GELU_TANH, ACT_NONE, ACT_RELU, ACT_SWIGLU, ACT_SWIGLU_BWD  # noqa: F401
from .scratch import ARENA

BF16 = torch.bfloat16


def _lib():
    return N.load()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk_bf16(*ts):
    for t in ts:
        if t is not None:
            assert t.is_cuda and t.dtype == BF16, f"expected CUDA bf16 tensor, got {t.device} {t.dtype}"


def gemm_nt(a: torch.Tensor, b: torch.Tensor, *, bias=None, residual=None, res_mod: int = 0, act: int = ACT_NONE,
            out: Optional[torch.Tensor] = None, out2: Optional[torch.Tensor] = None, alpha: float = 1.0,
            want_pre: bool = True, a_group=None, c_group=None, r_group=None, rope=None, c_live=None,
            split_k: Optional[int] = None, bias_post_round: bool = False, fp8=None, ext=None, query_256: bool = False,
            query_plan: bool = False):
    """C = epilogue(A @ B^T).  a: [M,K] or [batch,M,K] (row stride = a.stride(-2)); b: [N,K] or [batch,N,K].
    SwiGLU: returns (pre [.., N] or None, h [.., N/2]).  split_k: None = automatic, 0/1 = off, k = forced.
    fp8=(a_scale [M] f32, b_scale [N] f32): a and b are uint8 tensors of OCP e4m3 codes (quant_fp8_rows).
    ext=(a2 [M, K2], b2 [N, K2]) bf16: K extension, C = epilogue(A @ B^T + A2 @ B2^T) in one fp32 accumulator (LoRA branch); with fp8
    the base pair is e4m3 and dequantised before the extension adds to it.  query_256=True: no launch, returns whether this call
    would run on the 256-row kernel; query_plan=True: no launch, returns (kernel id, K slices) of this call (gemm_plan) - one query
    path, query_256 is its kernel id compared with KERNEL_NT_256.  Otherwise returns the output tensor (SwiGLU: the pair)."""
    if fp8 is not None:
        assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.dim() == 2 and split_k in (None, 0, 1)
        _chk_bf16(bias, residual, out, out2)
        split_k = 0
    else:
        _chk_bf16(a, b, bias, residual, out, out2)
    assert a.stride(-1) == 1 and b.stride(-1) == 1
    batched = a.dim() == 3
    if batched:
        nb, M, K = a.shape
        sA = a.stride(0)
        sB = b.stride(0) if b.dim() == 3 else 0
        Nn = b.shape[-2]
    else:
        nb, (M, K), sA, sB, Nn = 1, a.shape, 0, 0, b.shape[0]
    assert b.shape[-1] == K, f"K mismatch {a.shape} x {b.shape}"
    d = N.GemmDesc()
    d.A, d.B = a.data_ptr(), b.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldb, d.batch = M, Nn, K, a.stride(-2), b.stride(-2), nb
    d.sA, d.sB, d.act, d.alpha, d.res_mod = sA, sB, act, alpha, res_mod
    shape = (nb, M, Nn) if batched else (M, Nn)
    if act == ACT_SWIGLU:
        if out is None and want_pre:
            out = torch.empty(shape, device=a.device, dtype=BF16)
        hshape = shape[:-1] + (Nn // 2,)
        if out2 is None:
            out2 = torch.empty(hshape, device=a.device, dtype=BF16)
        assert out2.shape == hshape and out2.stride(-1) == 1
        d.C2, d.ldc2, d.sC2 = out2.data_ptr(), out2.stride(-2), (out2.stride(0) if batched else 0)
    elif out is None:
        out = torch.empty(shape, device=a.device, dtype=BF16)
    if out is not None:
        assert tuple(out.shape) == tuple(shape) and out.stride(-1) == 1, f"out shape {out.shape} != {shape}"
        d.C, d.ldc, d.sC = out.data_ptr(), out.stride(-2), (out.stride(0) if batched else 0)
    if bias is not None:
        assert bias.shape[-1] == Nn and bias.stride(-1) == 1
        d.bias = bias.data_ptr()
        d.sBias = bias.stride(0) if bias.dim() == 2 else 0
    if residual is not None:
        assert residual.stride(-1) == 1 and residual.shape[-1] == Nn
        assert res_mod > 0 or r_group is not None or tuple(residual.shape) == tuple(shape)
        d.R, d.ldr = residual.data_ptr(), residual.stride(-2)
        d.sR = residual.stride(0) if (batched and residual.dim() == 3) else 0
    if a_group is not None:      # (rows per group, stride between groups): a = first row-group view [g, K]
        d.a_group, d.a_group_stride = a_group
    if c_group is not None:
        d.c_group, d.c_group_stride = c_group
    if r_group is not None:
        d.r_group, d.r_group_stride = r_group
    if c_live is not None:       # (period, first live row): rows m of C with m % period < first are not stored
        d.c_live_mod, d.c_live_from = c_live
    if rope is not None:         # (mode, cos, sin, T, dh, ncols): fused rotary embedding on output columns [0, ncols)
        mode, cos_t, sin_t, T, dh, ncols = rope
        assert cos_t.dtype == torch.float32 and cos_t.is_contiguous() and sin_t.is_contiguous() and cos_t.shape[0] >= T
        assert cos_t.shape[1] == (dh // 2 if mode == 1 else dh)
        d.rope_mode, d.rope_T, d.rope_dh, d.rope_cols = mode, T, dh, ncols
        d.rope_cos, d.rope_sin = cos_t.data_ptr(), sin_t.data_ptr()
    if fp8 is not None:
        sa, sb = fp8
        assert sa.dtype == torch.float32 and sb.dtype == torch.float32 and sa.numel() == M and sb.numel() == Nn and sa.is_contiguous() and sb.is_contiguous()
        d.fp8, d.a_scale, d.b_scale = 1, sa.data_ptr(), sb.data_ptr()
    if ext is not None:
        a2, b2 = ext
        _chk_bf16(a2, b2)
        assert not batched and a2.dim() == 2 and b2.dim() == 2 and a2.shape[0] == M and b2.shape[0] == Nn and a2.shape[1] == b2.shape[1]
        assert a2.stride(1) == 1 and b2.stride(1) == 1 and a2.shape[1] % 64 == 0 and split_k in (None, 0, 1)
        d.A2, d.B2, d.K2, d.lda2, d.ldb2 = a2.data_ptr(), b2.data_ptr(), a2.shape[1], a2.stride(0), b2.stride(0)
        split_k = 0
    if bias_post_round:          # C = bf16(bf16(A.B^T) + bias): torch CPU Linear on a strided bf16 input (vla_native.h)
        assert bias is not None
        d.bias_post_round = 1
    if split_k is None and not batched and K >= 2048:    # (shorter contractions and batched products never split)
        split_k = _nt_plan(d)[1]
    if split_k and split_k > 1:
        d.split_k, d.ws = split_k, _scratch_f32(split_k * M * Nn, a.device).data_ptr()
    if query_plan or query_256:
        plan = _nt_plan(d)
        return plan if query_plan else plan[0] == N.KERNEL_NT_256
    N.check(_lib().vla_gemm_bf16_nt(_st(), C.byref(d)), "gemm_bf16_nt")
    if act == ACT_SWIGLU:
        return out, out2
    return out


def _nt_plan(d) -> Tuple[int, int]:
    """(kernel id, K slices) of vla_gemm_nt_plan for a descriptor: the library's routing, as the launch will run it."""
    split = C.c_int(0)
    kernel = _lib().vla_gemm_nt_plan(C.byref(d), -1, 0, C.byref(split))
    N.check(min(kernel, 0), "gemm_nt_plan")
    return kernel, split.value


def gemm_plan(a: torch.Tensor, b: torch.Tensor, **kw) -> Tuple[int, int]:
    """(kernel id N.KERNEL_NT_*, K slices) gemm_nt(a, b, **kw) would run with, under the calling thread's latency hint and the test
    overrides in force: the library's own routing (vla_gemm_nt_plan) on the descriptor gemm_nt builds.  Nothing is launched."""
    return gemm_nt(a, b, query_plan=True, **kw)


class latency_hint:
    """``with ops.latency_hint():`` - the products launched (or captured into a hipGraph) by this thread inside run on an otherwise idle
    chip and are latency-bound (batch-1 predict_action): vla_gemm_latency_hint(1) for the block.  Kernel selection: the deep operand rings
    are bit-identical; the short-M skinny tiles, the uneven split-K and the key-split attention change the fp32 association."""

    def __enter__(self):
        self.prev = _lib().vla_gemm_latency_hint(1)
        return self

    def __exit__(self, *exc):
        _lib().vla_gemm_latency_hint(self.prev)
        return False


def _scratch_f32(numel: int, device) -> torch.Tensor:
    """The current stream's scratch (scratch.ARENA) as floats: at least ``numel`` of them."""
    return ARENA.get(4 * numel, device).view(torch.float32)


def gemm_swiglu_bwd(d: torch.Tensor, w_downT: torch.Tensor, gu: torch.Tensor, out: Optional[torch.Tensor] = None,
                    gu_group=None, ext=None, fp8=None, query_plan: bool = False):
    """dGU[M, 2I] = swiglu'(GU) * (d[M, D] @ w_downT[I, D]^T): the dH GEMM with the SwiGLU backward in its epilogue.
    gu_group=(rows per group, element stride between groups): ``gu`` is then the first row-group window of a larger
    tensor (row m of the product reads gu row (m // g) * stride + (m % g) * ld).
    fp8=(d_scale [M], w_scale [I]) (with ext only): d and w_downT are uint8 e4m3 codes (quant_fp8_rows).
    query_plan=True: no launch, returns (kernel id, K slices) of this call."""
    if fp8 is not None:
        assert ext is not None and d.dtype == torch.uint8 and w_downT.dtype == torch.uint8
        _chk_bf16(gu, out)
    else:
        _chk_bf16(d, w_downT, gu, out)
    M, K = d.shape
    I = w_downT.shape[0]
    assert gu.shape[-1] == 2 * I and gu.stride(-1) == 1 and w_downT.shape[1] == K
    assert gu_group is not None or gu.shape[0] == M
    if out is None:
        out = torch.empty(M, 2 * I, device=d.device, dtype=BF16)
    assert out.shape == (M, 2 * I)
    desc = N.GemmDesc()
    desc.A, desc.B, desc.C, desc.R = d.data_ptr(), w_downT.data_ptr(), out.data_ptr(), gu.data_ptr()
    desc.M, desc.N, desc.K, desc.lda, desc.ldb, desc.ldc, desc.ldr, desc.batch = M, I, K, d.stride(0), w_downT.stride(0), out.stride(0), gu.stride(0), 1
    desc.act, desc.alpha = ACT_SWIGLU_BWD, 1.0
    if gu_group is not None:
        desc.r_group, desc.r_group_stride = gu_group
    if ext is not None:          # K extension: dH = d . W_down + dt . A_down (LoRA on down_proj)
        a2, b2 = ext
        _chk_bf16(a2, b2)
        assert a2.shape == (M, b2.shape[1]) and b2.shape[0] == I and a2.stride(1) == 1 and b2.stride(1) == 1 and a2.shape[1] % 64 == 0
        desc.A2, desc.B2, desc.K2, desc.lda2, desc.ldb2 = a2.data_ptr(), b2.data_ptr(), a2.shape[1], a2.stride(0), b2.stride(0)
    if fp8 is not None:
        sa, sb = fp8
        assert sa.dtype == torch.float32 and sb.dtype == torch.float32 and sa.numel() == M and sb.numel() == I and sa.is_contiguous() and sb.is_contiguous()
        desc.fp8, desc.a_scale, desc.b_scale = 1, sa.data_ptr(), sb.data_ptr()
    if query_plan:
        return _nt_plan(desc)
    N.check(_lib().vla_gemm_bf16_nt(_st(), C.byref(desc)), "gemm_bf16_nt(swiglu_bwd)")
    return out


def gemm_tn(a: torch.Tensor, b: torch.Tensor, *, out: Optional[torch.Tensor] = None, alpha: float = 1.0, accumulate: bool = False,
            a_group=None, b_group=None, a_cols=None, rows: Optional[int] = None, split: Optional[int] = None) -> torch.Tensor:
    """C[.., N1, N2] = alpha * a[.., M, N1]^T @ b[.., M, N2]  (contraction over the ROWS: dW = dY^T X, no operand transposes).
    a / b: [M, N] or [batch, M, N] views with last stride 1.  accumulate: C = bf16(bf16(product) + C).
    rows: contraction length when it differs from a.shape[-2] (row groups).  a_group / b_group = (rows per group, element stride
    between groups): a / b is then the first group's [g, N] view of a larger tensor.  a_cols = (n1, group, stride, offset): the
    product's N1 axis is the n1 columns {offset + (c // group) * stride + c % group} of a (gate / up halves of an interleaved dY).
    split: None = automatic (few-tile long-M products), 0 / 1 = off."""
    _chk_bf16(a, b, out)
    assert a.stride(-1) == 1 and b.stride(-1) == 1 and a.dim() == b.dim()
    batched = a.dim() == 3
    nb = a.shape[0] if batched else 1
    M = rows if rows is not None else a.shape[-2]
    assert rows is not None or b.shape[-2] == M
    N1, N2 = a.shape[-1], b.shape[-1]
    d = N.GemmTnDesc()
    a_ptr = a.data_ptr()
    if a_cols is not None:
        N1, cg, cgs, off = a_cols
        assert cg % 8 == 0 and cgs % 8 == 0 and off % 8 == 0
        d.a_col_group, d.a_col_group_stride = cg, cgs
        a_ptr += off * 2
    shape = (nb, N1, N2) if batched else (N1, N2)
    if out is None:
        assert not accumulate
        out = torch.empty(shape, device=a.device, dtype=BF16)
    assert tuple(out.shape) == shape and out.stride(-1) == 1, f"out shape {tuple(out.shape)} != {shape}"
    d.A, d.B, d.C = a_ptr, b.data_ptr(), out.data_ptr()
    d.M, d.N1, d.N2, d.lda, d.ldb, d.ldc, d.batch = M, N1, N2, a.stride(-2), b.stride(-2), out.stride(-2), nb
    d.sA, d.sB, d.sC = (a.stride(0), b.stride(0), out.stride(0)) if batched else (0, 0, 0)
    d.alpha = alpha
    if accumulate:
        d.R, d.ldr, d.sR = out.data_ptr(), out.stride(-2), d.sC
    if a_group is not None:
        d.a_group, d.a_group_stride = a_group
    if b_group is not None:
        d.b_group, d.b_group_stride = b_group
    if split is None and M >= 1024:                   # (shorter contractions never split)
        split_c = C.c_int(0)
        N.check(min(_lib().vla_gemm_tn_plan(C.byref(d), 0, C.byref(split_c)), 0), "gemm_tn_plan")
        split = split_c.value
    if split and split > 1:
        d.split, d.ws = split, _scratch_f32(nb * split * N1 * N2, a.device).data_ptr()
    N.check(_lib().vla_gemm_bf16_tn(_st(), C.byref(d)), "gemm_bf16_tn")
    return out


TN_GROUP_MAX = 48


def tn_problem(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, alpha: float = 1.0, a_cols=None) -> "N.GemmTnDesc":
    """Descriptor of one plain product out[N1, N2] = alpha a[M, N1]^T b[M, N2] for gemm_tn_grouped (2-D views, last stride 1)."""
    _chk_bf16(a, b, out)
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and a.shape[0] == b.shape[0]
    d = N.GemmTnDesc()
    N1, a_ptr = a.shape[1], a.data_ptr()
    if a_cols is not None:
        N1, cg, cgs, off = a_cols
        d.a_col_group, d.a_col_group_stride = cg, cgs
        a_ptr += off * 2
    assert tuple(out.shape) == (N1, b.shape[1]), f"out shape {tuple(out.shape)} != {(N1, b.shape[1])}"
    d.A, d.B, d.C = a_ptr, b.data_ptr(), out.data_ptr()
    d.M, d.N1, d.N2, d.lda, d.ldb, d.ldc, d.batch, d.alpha = a.shape[0], N1, b.shape[1], a.stride(0), b.stride(0), out.stride(0), 1, alpha
    d._keep = (a, b, out)                      # the descriptor holds raw pointers: keep the tensors alive with it
    return d


def gemm_tn_grouped(problems):
    """ONE launch (per 48 problems) over the concatenated tile lists of independent TN products (tn_problem descriptors)."""
    for i in range(0, len(problems), TN_GROUP_MAX):
        chunk = problems[i:i + TN_GROUP_MAX]
        arr = (N.GemmTnDesc * len(chunk))(*chunk)
        N.check(_lib().vla_gemm_bf16_tn_grouped(_st(), arr, len(chunk)), "gemm_bf16_tn_grouped")


def copy_rows3d(src: torch.Tensor, dst: torch.Tensor, groups: int, rows: int, cols: int, s_sg: int, s_sr: int, d_sg: int, d_sr: int):
    """dst[g][r][:cols] = src[g][r][:cols] over raw element strides (src / dst: tensors whose data_ptr is element [0][0][0])."""
    _chk_bf16(src, dst)
    N.check(_lib().vla_copy_rows3d(_st(), _p(src), _p(dst), groups, rows, cols, s_sg, s_sr, d_sg, d_sr), "copy_rows3d")
    return dst


def layerscale_fwd(a: torch.Tensor, ls: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = bf16(x + bf16(a * ls))  (modeling_prismatic.py:58-66 + the residual add); out may be x."""
    _chk_bf16(a, ls, x, out)
    assert a.is_contiguous() and x.is_contiguous() and a.shape == x.shape and ls.numel() == a.shape[-1]
    out = torch.empty_like(x) if out is None else out
    N.check(_lib().vla_layerscale_fwd(_st(), _p(a), _p(ls), _p(x), _p(out), a.numel() // a.shape[-1], a.shape[-1]), "layerscale_fwd")
    return out


def layerscale_bwd(dy: torch.Tensor, a: Optional[torch.Tensor], ls: torch.Tensor, dls_f32: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """da = bf16(dy * ls); dls_f32 (optional, +=) += column sums of dy * a."""
    _chk_bf16(dy, a, ls, out)
    assert dy.is_contiguous() and (a is None or (a.is_contiguous() and a.shape == dy.shape))
    out = torch.empty_like(dy) if out is None else out
    N.check(_lib().vla_layerscale_bwd(_st(), _p(dy), _p(a), _p(ls), _p(out), _p(dls_f32), dy.numel() // dy.shape[-1], dy.shape[-1]), "layerscale_bwd")
    return out


def transpose(x: torch.Tensor, ld_out: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [.., R, Cc] -> [.., Cc, ld_out] (columns R..ld_out-1 zero).  Returns the padded buffer."""
    _chk_bf16(x, out)
    assert x.stride(-1) == 1
    batched = x.dim() == 3
    nb = x.shape[0] if batched else 1
    R, Cc = x.shape[-2:]
    ld = ld_out or R
    if out is None:
        shape = (nb, Cc, ld) if batched else (Cc, ld)
        out = torch.empty(shape, device=x.device, dtype=BF16)
        if ld != R:
            zero_(out)                 # (native fill: the padding columns; torch.zeros would put an ATen kernel on the step)
    N.check(_lib().vla_transpose_bf16(_st(), _p(x), _p(out), R, Cc, x.stride(-2), out.stride(-2), nb,
                                      x.stride(0) if batched else 0, out.stride(0) if batched else 0), "transpose")
    return out


def layernorm_fwd(x, w, b, eps: float, want_stats: bool = False, out=None, stats=None):
    """out / stats: [rows, cols] bf16 / [rows, 2] f32 destinations (default: new tensors; stats only with want_stats)."""
    _chk_bf16(x, w, b)
    cols = x.shape[-1]
    x2 = x.reshape(-1, cols)
    assert x2.stride(-1) == 1
    y = torch.empty_like(x2) if out is None else out
    if want_stats and stats is None:
        stats = torch.empty(x2.shape[0], 2, device=x.device, dtype=torch.float32)
    N.check(_lib().vla_layernorm_fwd(_st(), _p(x2), _p(w), _p(b), _p(y), _p(stats), x2.shape[0], cols, x2.stride(0),
                                     y.stride(0), eps), "layernorm_fwd")
    return (y.view(x.shape), stats) if want_stats else y.view(x.shape)


def layernorm_bwd(dy, x, w, stats, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None,
                  want_dx: bool = True, out=None):
    _chk_bf16(dy, x, w)
    cols = x.shape[-1]
    x2, dy2 = x.reshape(-1, cols), dy.reshape(-1, cols)
    dx = out if out is not None else torch.empty_like(x2) if want_dx else None
    N.check(_lib().vla_layernorm_bwd(_st(), _p(dy2), _p(x2), _p(w), _p(stats), _p(dx), _p(dw), _p(db), x2.shape[0], cols,
                                     x2.stride(0), dy2.stride(0), dx.stride(0) if dx is not None else cols), "layernorm_bwd")
    return dx.view(x.shape) if dx is not None else None


def rmsnorm_fwd(x, w, eps: float, want_rstd: bool = False, out=None, rstd=None):
    """rstd: f32 [rows] destination of the reciprocal RMS (default: a new tensor with want_rstd, else not stored)."""
    _chk_bf16(x, w)
    cols = x.shape[-1]
    assert x.is_contiguous()
    rows = x.numel() // cols
    y = torch.empty_like(x) if out is None else out
    if want_rstd and rstd is None:
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    N.check(_lib().vla_rmsnorm_fwd(_st(), _p(x), _p(w), _p(y), _p(rstd), rows, cols, eps), "rmsnorm_fwd")
    return (y, rstd) if want_rstd else y


def rmsnorm_fwd_q8(x, w, eps: float, q8: torch.Tensor, qscale: torch.Tensor, rstd: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None):
    """RMSNorm with the row-wise e4m3 quantisation of its bf16 output fused behind it: fills q8 (uint8 [rows, cols]) and
    qscale (f32 [rows]); rstd / y (the bf16 output) are optional."""
    _chk_bf16(x, w, y)
    cols = x.shape[-1]
    assert x.is_contiguous() and q8.dtype == torch.uint8 and q8.stride(-1) == 1
    rows = x.numel() // cols
    N.check(_lib().vla_rmsnorm_fwd_q8(_st(), _p(x), _p(w), _p(y), _p(rstd), _p(q8), _p(qscale), rows, cols, q8.stride(-2), eps), "rmsnorm_fwd_q8")
    return q8, qscale


def layernorm_fwd_q8(x2, w, b, eps: float, q8: torch.Tensor, qscale: torch.Tensor, y: Optional[torch.Tensor] = None, stats=None):
    """LayerNorm (rows of x2 [rows, cols], row stride x2.stride(0)) + fused row-wise e4m3 quantisation of its bf16 output."""
    _chk_bf16(x2, w, b, y)
    rows, cols = x2.shape
    assert x2.stride(-1) == 1 and q8.dtype == torch.uint8 and q8.stride(-1) == 1
    N.check(_lib().vla_layernorm_fwd_q8(_st(), _p(x2), _p(w), _p(b), _p(y), _p(stats), _p(q8), _p(qscale), rows, cols, x2.stride(0),
                                        y.stride(0) if y is not None else 0, q8.stride(0), eps), "layernorm_fwd_q8")
    return q8, qscale


def rmsnorm_bwd(dy, x, w, rstd, dres=None, out=None, x_rows=None):
    """dy/dres/out compact [rows, cols].  x_rows=(group, group_rows, row0): x / rstd are the forward's full tensors and
    compact row r maps to row (r // group) * group_rows + row0 + r % group (live-row window of every sequence)."""
    _chk_bf16(dy, x, w, dres)
    cols = x.shape[-1]
    assert x.is_contiguous() and dy.is_contiguous()
    rows = dy.numel() // cols
    g, gr, r0 = x_rows if x_rows is not None else (0, 0, 0)
    if x_rows is None:
        assert x.numel() == dy.numel()
    else:
        assert rows % g == 0 and (rows // g) * gr * cols <= x.numel() and rstd.numel() * cols >= (rows // g) * gr * cols
    dx = torch.empty_like(dy) if out is None else out
    if dres is not None:
        assert dres.is_contiguous() and dres.numel() >= dy.numel()
    N.check(_lib().vla_rmsnorm_bwd(_st(), _p(dy), _p(x), _p(w), _p(rstd), _p(dres), _p(dx), rows, cols, g, gr, r0), "rmsnorm_bwd")
    return dx


def rmsnorm_dw(dy, x, rstd, acc_f32):
    """acc_f32 [cols] += sum over the rows of dy * x * rstd (the RMSNorm weight gradient; dy / x [rows, cols] contiguous)."""
    rows, cols = dy.shape
    N.check(_lib().vla_rmsnorm_dw(_st(), _p(dy), _p(x), _p(rstd), _p(acc_f32), rows, cols), "rmsnorm_dw")
    return acc_f32


def _attn_desc(q, k, v, o, lse, kmask, causal, scale, Hq, Hkv, dh):
    """q [B,Sq,>=Hq*dh], k/v [B,Sk,>=Hkv*dh] views (last-dim stride 1), o [B,Sq,Hq*dh]."""
    d = N.AttnDesc()
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.kmask = kmask.data_ptr() if kmask is not None else None
    d.q_sb, d.k_sb, d.v_sb, d.o_sb = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    d.q_ss, d.k_ss, d.v_ss, d.o_ss = q.stride(1), k.stride(1), v.stride(1), o.stride(1)
    d.B, d.Sq, d.Sk, d.Hq, d.Hkv, d.dh, d.causal, d.scale = B, Sq, Sk, Hq, Hkv, dh, int(causal), scale
    return d


def attn_fwd(q, k, v, Hq: int, Hkv: int, dh: int, causal: bool, kmask=None, scale: Optional[float] = None,
             want_lse: bool = False, out=None, lse=None):
    """out [B, Sq, Hq*dh] / lse f32 [B, Hq, Sq]: destinations (default: new tensors; lse only with want_lse)."""
    _chk_bf16(q, k, v)
    assert q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1
    B, Sq = q.shape[:2]
    if kmask is not None:
        assert kmask.dtype == torch.uint8 and kmask.is_contiguous() and tuple(kmask.shape) == (B, k.shape[1])
    o = torch.empty(B, Sq, Hq * dh, device=q.device, dtype=BF16) if out is None else out
    if want_lse and lse is None:
        lse = torch.empty(B, Hq, Sq, device=q.device, dtype=torch.float32)
    d = _attn_desc(q, k, v, o, lse, kmask, causal, scale if scale is not None else dh ** -0.5, Hq, Hkv, dh)
    N.check(_lib().vla_attn_fwd(_st(), C.byref(d)), "attn_fwd")
    return (o, lse) if want_lse else o


def attn_bwd(dout, q, k, v, o, lse, Hq: int, Hkv: int, dh: int, causal: bool, kmask=None,
             scale: Optional[float] = None, dq=None, dk=None, dv=None, rope=None, row0: int = 0, delta=None):
    """row0 > 0 (causal only, multiple of 32): live-row backward.  q/o/dout/dq are the [B, Sk - row0, ...] windows
    (views) of the rows >= row0, k/v the full [B, Sk, ...] tensors, lse the forward's full [B, Hq, Sk]; dk/dv are
    produced for the keys >= row0 only ([B, Sk - row0, ...]).  Exactly the gradients the rows >= row0 receive.
    delta: the f32 [B, Hq, Sq] scratch of the backward (default: a new tensor)."""
    _chk_bf16(dout, q, k, v, o)
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    assert Sq + row0 == Sk or row0 == 0
    dq = torch.empty(B, Sq, Hq * dh, device=q.device, dtype=BF16) if dq is None else dq
    dk = torch.empty(B, Sk - row0, Hkv * dh, device=q.device, dtype=BF16) if dk is None else dk
    dv = torch.empty(B, Sk - row0, Hkv * dh, device=q.device, dtype=BF16) if dv is None else dv
    if delta is None:
        delta = torch.empty(B, Hq, Sq, device=q.device, dtype=torch.float32)
    assert delta.dtype == torch.float32 and delta.is_contiguous() and delta.numel() >= B * Hq * Sq
    d = _attn_desc(q, k, v, o, lse, kmask, causal, scale if scale is not None else dh ** -0.5, Hq, Hkv, dh)
    if row0:
        assert causal and row0 % 32 == 0 and lse.shape == (B, Hq, Sk) and lse.is_contiguous()
        d.q_off, d.dkv_k0, d.lse_hs = row0, row0, Sk
        d.lse = lse.data_ptr() + 4 * row0
    d.dout, d.dq, d.dk, d.dv, d.delta = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    d.do_sb, d.dq_sb, d.dk_sb, d.dv_sb = dout.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
    d.do_ss, d.dq_ss, d.dk_ss, d.dv_ss = dout.stride(1), dq.stride(1), dk.stride(1), dv.stride(1)
    if rope is not None:          # (cos, sin) f32 [S, dh/2]: dq/dk come back through the inverse rotate_half RoPE
        assert rope[0].shape == (Sk, dh // 2) and rope[0].dtype == torch.float32
        d.rope_cos, d.rope_sin = rope[0].data_ptr(), rope[1].data_ptr()
    N.check(_lib().vla_attn_bwd(_st(), C.byref(d)), "attn_bwd")
    return dq, dk, dv


def rope_half_tables(S: int, dh: int, theta: float, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """f32 [S, dh/2] tables of bf16-rounded cos/sin (HF casts cos/sin to the activation dtype)."""
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    f = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    return (f.cos().to(BF16).float().to(device).contiguous(), f.sin().to(BF16).float().to(device).contiguous())


def rope_half_(x2d: torch.Tensor, cos_t, sin_t, S: int, nheads: int, dh: int, sign: int = 1):
    """In place on x2d [rows, >= nheads*dh] (a column window of the fused qkv buffer)."""
    _chk_bf16(x2d)
    assert x2d.stride(-1) == 1 and cos_t.shape == (S, dh // 2)
    N.check(_lib().vla_rope_half(_st(), _p(x2d), _p(cos_t), _p(sin_t), x2d.shape[0], S, nheads, dh, x2d.stride(0), sign),
            "rope_half")
    return x2d


def rope_inter_tables(T: int, dh: int, device, base: float = 10000.0):
    """action_heads.py:150-164: cos/sin of cat([f, f]) -> f32 [T, dh] tables holding the bf16 values the reference's bf16
    head computes.  finetune.py:280-281 casts the head with .to(torch.bfloat16), which casts the registered ``inv_freq``
    buffer too: positions are a bf16 arange (above 256 they collapse onto representable even numbers), the angle
    t * inv_freq is rounded to bf16 BEFORE cos / sin.  Host-side table construction (torch CPU as the array library),
    pinned by the reference-run fixtures tests/golden/head_bf16_*.npz."""
    inv = (1.0 / (base ** (torch.arange(0, dh, 2).float() / dh))).to(BF16)
    f = torch.einsum("i,j->ij", torch.arange(T, dtype=BF16), inv)
    e = torch.cat([f, f], dim=-1)
    return (e.cos().float().to(device).contiguous(), e.sin().float().to(device).contiguous())


def rope_inter_(x2d: torch.Tensor, cos_t, sin_t, T: int, nheads: int, dh: int, mode: int = 0):
    _chk_bf16(x2d)
    assert x2d.stride(-1) == 1 and cos_t.shape[0] >= T and cos_t.shape[1] == dh
    N.check(_lib().vla_rope_interleaved(_st(), _p(x2d), _p(cos_t), _p(sin_t), x2d.shape[0], T, nheads, dh, x2d.stride(0),
                                        mode), "rope_interleaved")
    return x2d


def im2col_patch(pixels: torch.Tensor, c0: int, P: int, ldo: int) -> torch.Tensor:
    assert pixels.is_cuda and pixels.is_contiguous() and pixels.dtype in (BF16, torch.float32)
    B, Ct, H, W = pixels.shape
    out = torch.empty(B * (H // P) * (W // P), ldo, device=pixels.device, dtype=BF16)
    N.check(_lib().vla_im2col_patch(_st(), _p(pixels), _p(out), B, Ct, c0, H, W, P, ldo,
                                    int(pixels.dtype == torch.float32)), "im2col_patch")
    return out


def action_mask(labels: torch.Tensor, shift: int):
    """-> qidx int32 [B, L-shift], pos int32 [B,64], count int32 [B] (device tensors; no host sync)."""
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous()
    B, L = labels.shape
    qidx = torch.empty(B, L - shift, device=labels.device, dtype=torch.int32)
    pos = torch.empty(B, 64, device=labels.device, dtype=torch.int32)
    cnt = torch.empty(B, device=labels.device, dtype=torch.int32)
    N.check(_lib().vla_action_mask(_st(), _p(labels), _p(qidx), _p(pos), _p(cnt), B, L, shift), "action_mask")
    return qidx, pos, cnt


def embed_splice(ids, attn_mask_u8, qidx, table, action_queries, out, mm_mask, Np: int):
    B, L = ids.shape
    D = table.shape[1]
    assert ids.dtype == torch.int64 and ids.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (B, L + Np, D)
    assert tuple(action_queries.shape) == (64, D) and qidx.shape == (B, L)
    N.check(_lib().vla_embed_splice(_st(), _p(ids), _p(attn_mask_u8), _p(qidx), _p(table), _p(action_queries), _p(out),
                                    _p(mm_mask), B, L, Np, D, table.shape[0]), "embed_splice")


def action_query_grad(dx, pos, Np: int, row0: int = 0) -> torch.Tensor:
    """dx [B, S - row0, D]: the rows >= row0 of the gradient w.r.t. inputs_embeds."""
    B, S, D = dx.shape
    assert dx.is_contiguous()
    dq = torch.empty(64, D, device=dx.device, dtype=torch.float32)
    N.check(_lib().vla_action_query_grad(_st(), _p(dx), _p(pos), _p(dq), B, S, Np, D, row0), "action_query_grad")
    return dq


def gather_rows(src2d, idx, out2d):
    N.check(_lib().vla_gather_rows(_st(), _p(src2d), _p(idx), _p(out2d), idx.numel(), out2d.shape[-1], src2d.stride(0),
                                   out2d.stride(0)), "gather_rows")
    return out2d


def scatter_add_rows(src2d, idx, out2d):
    N.check(_lib().vla_scatter_add_rows(_st(), _p(src2d), _p(idx), _p(out2d), idx.numel(), src2d.shape[-1], src2d.stride(0),
                                        out2d.stride(0)), "scatter_add_rows")
    return out2d


def add_(a, b):
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    N.check(_lib().vla_add_bf16(_st(), _p(a), _p(b), _p(a), a.numel()), "add_bf16")
    return a


def gelu_fwd(x, out=None):
    y = torch.empty_like(x) if out is None else out
    N.check(_lib().vla_gelu_fwd(_st(), _p(x), _p(y), x.numel()), "gelu_fwd")
    return y


def gelu_bwd(dy, x, out=None):
    """out may be dy itself (in place)."""
    dx = torch.empty_like(x) if out is None else out
    N.check(_lib().vla_gelu_bwd(_st(), _p(dy), _p(x), _p(dx), x.numel()), "gelu_bwd")
    return dx


def relu_bwd(dy, y, out=None):
    dx = torch.empty_like(y) if out is None else out
    N.check(_lib().vla_relu_bwd(_st(), _p(dy), _p(y), _p(dx), y.numel()), "relu_bwd")
    return dx


def swiglu_bwd(dh, gu, out=None):
    M, I = dh.shape
    assert gu.shape == (M, 2 * I) and dh.is_contiguous() and gu.is_contiguous()
    dgu = torch.empty_like(gu) if out is None else out
    N.check(_lib().vla_swiglu_bwd(_st(), _p(dh), _p(gu), _p(dgu), M, I), "swiglu_bwd")
    return dgu


def swiglu_fwd(gu, out=None):
    M, I2 = gu.shape
    assert gu.is_contiguous() and I2 % 32 == 0
    h = torch.empty(M, I2 // 2, device=gu.device, dtype=BF16) if out is None else out
    N.check(_lib().vla_swiglu_fwd(_st(), _p(gu), _p(h), M, I2 // 2), "swiglu_fwd")
    return h


def colsum_(x, out_f32):
    """x [rows, cols] or [batch, rows, cols] (bf16) -> out_f32 [cols] / [batch, cols] += column sums."""
    if x.dim() == 3:
        assert out_f32.shape == (x.shape[0], x.shape[2]) and out_f32.stride(-1) == 1 and x.stride(-1) == 1
        N.check(_lib().vla_colsum_bf16(_st(), _p(x), _p(out_f32), x.shape[1], x.shape[2], x.stride(1), x.shape[0], x.stride(0),
                                       out_f32.stride(0)), "colsum")
    else:
        N.check(_lib().vla_colsum_bf16(_st(), _p(x), _p(out_f32), x.shape[0], x.shape[1], x.stride(0), 1, 0, 0), "colsum")
    return out_f32


def cast_f32_bf16(x, out=None):
    y = torch.empty(x.shape, device=x.device, dtype=BF16) if out is None else out
    N.check(_lib().vla_cast_f32_bf16(_st(), _p(x), _p(y), x.numel()), "cast")
    return y


def head_attn_desc(q, ks, vs, ka, va, kt, vt, gate, probs, out, H: int):
    d = N.HeadAttnDesc()
    B, T = q.shape[:2]
    d.q, d.k_self, d.v_self, d.k_adp, d.v_adp, d.k_task, d.v_task = (t.data_ptr() for t in (q, ks, vs, ka, va, kt, vt))
    d.gate, d.probs, d.out = gate.data_ptr(), probs.data_ptr(), out.data_ptr()
    d.B, d.T, d.Ka, d.Kt, d.H, d.dh = B, T, ka.shape[1], kt.shape[1], H, out.shape[-1] // H
    d.ld_q, d.ld_self, d.ld_adp, d.ld_task, d.ld_out = q.stride(1), ks.stride(1), ka.stride(1), kt.stride(1), out.stride(1)
    for t, n in ((vs, ks), (va, ka), (vt, kt)):
        assert t.stride(1) == n.stride(1) and t.stride(-1) == 1
    return d


def head_attn_fwd(q, ks, vs, ka, va, kt, vt, gate, H: int = 8, ref_softmax: bool = False, out=None, probs=None):
    """q/ks/vs [B,T,D*], ka/va [B,Ka,D*], kt/vt [B,Kt,D*] (views, last stride 1) -> out [B,T,D], probs f32 [B,H,T,T+Ka+Kt]
    (given or new).  ref_softmax: weights rounded to bf16 after normalisation, as ATen's bf16 softmax emits them (two passes
    over the keys)."""
    _chk_bf16(q, ks, vs, ka, va, kt, vt, gate)
    B, T = q.shape[:2]
    D = q.shape[-1]
    Nn = T + ka.shape[1] + kt.shape[1]
    out = torch.empty(B, T, D, device=q.device, dtype=BF16) if out is None else out
    probs = torch.empty(B, H, T, Nn, device=q.device, dtype=torch.float32) if probs is None else probs
    d = head_attn_desc(q, ks, vs, ka, va, kt, vt, gate, probs, out, H)
    d.ref_softmax = int(ref_softmax)
    N.check(_lib().vla_head_attn_fwd(_st(), C.byref(d)), "head_attn_fwd")
    return out, probs


def head_attn_bwd(dout, out, q, ks, vs, ka, va, kt, vt, gate, probs, dgate_f32, dq, dks, dvs, dka, dva, dkt, dvt, H: int = 8,
                  rope=None):
    """``out`` = the forward output, ``probs`` = the forward's workspace.  Gradient tensors are caller-provided views
    with the SAME row strides as their forward counterparts.  The MFMA backward's workspace (B*H*ceil((T+Ka+Kt)/32)*(T*dh + 1)
    floats of dQ / gate partials, one set per 32-key tile) is REQUIRED by the library at the MFMA head widths - a descriptor without
    it is refused before anything is launched - and is passed here at exactly that size."""
    _chk_bf16(dout, out, dq, dks, dvs, dka, dva, dkt, dvt)
    d = head_attn_desc(q, ks, vs, ka, va, kt, vt, gate, probs, out, H)
    d.dout = dout.data_ptr()
    assert dout.stride(1) == out.stride(1) and dout.stride(-1) == 1
    for g, f in ((dq, q), (dks, ks), (dvs, vs), (dka, ka), (dva, va), (dkt, kt), (dvt, vt)):
        assert g.stride(1) == f.stride(1) and g.stride(-1) == 1, "grad views must mirror forward strides"
    d.dq, d.dk_self, d.dv_self, d.dk_adp, d.dv_adp, d.dk_task, d.dv_task = (t.data_ptr() for t in (dq, dks, dvs, dka, dva, dkt, dvt))
    d.dgate = dgate_f32.data_ptr()
    if rope is not None:          # (cos, sin) f32 [>= max(T,Ka,Kt), dh]: dq / dk come back through the RoPE transpose
        assert rope[0].shape[0] >= max(q.shape[1], ka.shape[1], kt.shape[1]) and rope[0].shape[1] == d.dh
        d.rope_cos, d.rope_sin = rope[0].data_ptr(), rope[1].data_ptr()
    ntile = (d.T + d.Ka + d.Kt + 31) // 32
    ws = _scratch_f32(d.B * d.H * ntile * (d.T * d.dh + 1), q.device)
    d.ws, d.ws_floats = ws.data_ptr(), ws.numel()
    N.check(_lib().vla_head_attn_bwd(_st(), C.byref(d)), "head_attn_bwd")


def l1_loss(pred, target, want_grad: bool = True, gscale: float = 1.0):
    _chk_bf16(pred, target)
    B, Cc, Da = pred.shape
    loss3 = torch.empty(3, device=pred.device, dtype=torch.float32)
    dpred = torch.empty_like(pred) if want_grad else None
    N.check(_lib().vla_l1_loss(_st(), _p(pred.contiguous()), _p(target.contiguous()), _p(loss3), _p(dpred), B, Cc, Da, gscale),
            "l1_loss")
    return loss3, dpred


def adamw_(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, gscale: float = 1.0):
    assert p.dtype == BF16 and m.dtype == BF16 and v.dtype == BF16 and g.dtype in (BF16, torch.float32)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert p.numel() == g.numel() == m.numel() == v.numel()
    N.check(_lib().vla_adamw_bf16(_st(), _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, step,
                                  int(g.dtype == torch.float32), gscale), "adamw")


# ---- global gradient-norm clipping (torch.nn.utils.clip_grad_norm_) without a host sync -----------------------------------
def grad_sumsq_slots(n: int) -> int:
    """fp32 partials grad_sumsq_ writes for n elements: host arithmetic, a function of n alone (callable without a GPU)."""
    return int(_lib().vla_grad_sumsq_slots(int(n)))


def grad_sumsq_(g, slots, gscale: float = 1.0) -> int:
    """slots[:grad_sumsq_slots(n)] <- fixed-order partial sums of squares of the gradients adamw_ would consume from ``g`` (a
    contiguous bf16 / f32 slice at any element offset) under the same ``gscale``.  Returns the slot count."""
    assert g.dtype in (BF16, torch.float32) and g.is_contiguous() and slots.dtype == torch.float32 and slots.is_contiguous()
    k = grad_sumsq_slots(g.numel())
    assert 0 < k <= slots.numel(), "grad_sumsq_: slot buffer too short"
    N.check(_lib().vla_grad_sumsq(_st(), _p(g), g.numel(), int(g.dtype == torch.float32), gscale, _p(slots)), "grad_sumsq")
    return k


def grad_norm_finalise_(slots, max_norm: float, out):
    """out[0] = total_norm, out[1] = min(1, max_norm / (total_norm + 1e-6)) from every partial in ``slots`` (f32, device)."""
    assert slots.dtype == torch.float32 and slots.is_contiguous() and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 2
    N.check(_lib().vla_grad_norm_finalise(_st(), _p(slots), slots.numel(), float(max_norm), _p(out)), "grad_norm_finalise")
    return out


def adamw_clipped_(p, g, m, v, coef, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, gscale: float = 1.0):
    """adamw_ with the gradients scaled by the device scalar ``coef`` (f32 [1], grad_norm_finalise_'s out[1:2]) after the gscale rounding."""
    assert p.dtype == BF16 and m.dtype == BF16 and v.dtype == BF16 and g.dtype in (BF16, torch.float32)
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    assert p.numel() == g.numel() == m.numel() == v.numel()
    assert coef.dtype == torch.float32 and coef.numel() == 1 and coef.device == p.device
    N.check(_lib().vla_adamw_clipped_bf16(_st(), _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, step,
                                          int(g.dtype == torch.float32), gscale, _p(coef)), "adamw_clipped")


# ---- host-glue replacements: no ATen kernel between the hand-written ones on the training step ---------------------------
_DT = {BF16: 0, torch.float32: 1}


def copy2d(src: torch.Tensor, dst: torch.Tensor, rows: int, cols: int, ld_src: int, ld_dst: int, src_mod: int = 0, d_group=None):
    """dst[r, :cols] = cast(src[r % src_mod or r, :cols]) over raw row strides (elements); d_group=(rows per group, group stride)."""
    g, gs = d_group if d_group is not None else (0, 0)
    N.check(_lib().vla_copy2d(_st(), _p(src), _p(dst), rows, cols, ld_src, ld_dst, _DT[src.dtype], _DT[dst.dtype], src_mod, g, gs), "copy2d")
    return dst


def quant_fp8_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None):
    """x bf16 [rows, cols] -> (uint8 [rows, cols] of OCP e4m3 codes, f32 [rows] dequantisation scales = amax / 448)."""
    assert x.dtype == BF16 and x.dim() == 2 and x.stride(1) == 1
    rows, cols = x.shape
    if out is None:
        out = torch.empty(rows, cols, device=x.device, dtype=torch.uint8)
    if scale is None:
        scale = torch.empty(rows, device=x.device, dtype=torch.float32)
    assert out.dtype == torch.uint8 and out.stride(1) == 1 and tuple(out.shape) == (rows, cols)
    N.check(_lib().vla_quant_fp8_rows(_st(), _p(x), _p(out), _p(scale), rows, cols, x.stride(0), out.stride(0)), "quant_fp8_rows")
    return out, scale


def dropout(x: torch.Tensor, out: torch.Tensor, p: float, seed: int, step: Optional[torch.Tensor] = None):
    """out = dropout(x, p) on 2-D bf16 views (last stride 1): vla_dropout_bf16.  step: device int32 [1] (the mask's second key) or None."""
    _chk_bf16(x, out)
    assert x.dim() == 2 and x.shape == out.shape and x.stride(1) == 1 and out.stride(1) == 1
    N.check(_lib().vla_dropout_bf16(_st(), _p(x), _p(out), x.shape[0], x.shape[1], x.stride(0), out.stride(0), float(p), int(seed) & (2 ** 64 - 1),
                                    _p(step) if step is not None else None), "dropout")
    return out


def dropout_bwd_add_(dx: torch.Tensor, u: torch.Tensor, p: float, seed: int, step: Optional[torch.Tensor] = None):
    """dx += dropout'(u) with the mask of dropout(., p, seed, step): vla_dropout_bwd_add_bf16."""
    _chk_bf16(dx, u)
    assert u.dim() == 2 and u.shape == dx.shape and u.stride(1) == 1 and dx.stride(1) == 1
    N.check(_lib().vla_dropout_bwd_add_bf16(_st(), _p(u), _p(dx), u.shape[0], u.shape[1], u.stride(0), dx.stride(0), float(p), int(seed) & (2 ** 64 - 1),
                                            _p(step) if step is not None else None), "dropout_bwd_add")
    return dx


def inc_i32_(t: torch.Tensor):
    assert t.dtype == torch.int32 and t.numel() >= 1
    N.check(_lib().vla_inc_i32(_st(), _p(t)), "inc_i32")
    return t


def zero_(t: torch.Tensor):
    assert t.is_contiguous()
    N.check(_lib().vla_fill_zero(_st(), _p(t), t.numel() * t.element_size()), "fill_zero")
    return t


def head_index_prep(pos1, pos0, cnt0, gather, scatter, guard, B: int, S: int, Np: int, row0: int):
    N.check(_lib().vla_head_index_prep(_st(), _p(pos1), _p(pos0), _p(cnt0), _p(gather), _p(scatter), _p(guard), B, S, Np, row0), "head_index_prep")


def embed_grad(dx, ids, qidx, out, Np: int):
    """Token-embedding gradient: out [V, D] += the rows of dx [B, L + Np, D] that hold a looked-up token (ids [B, L]; qidx: the
    action-query slots, which read no table row)."""
    B, L = ids.shape
    V, D = out.shape
    N.check(_lib().vla_embed_grad(_st(), _p(dx), _p(ids), _p(qidx), _p(out), B, L, Np, D, V), "embed_grad")
    return out


def token_ce(logits, tgt, out_f32):
    """out_f32[0] += sum of logsumexp(logits) - logits[tgt], out_f32[1] += count, over the rows of logits [rows, V] whose target
    (tgt int64 [rows]) is not IGNORE_INDEX."""
    V = logits.shape[-1]
    N.check(_lib().vla_token_ce(_st(), _p(logits), V, _p(tgt), logits.numel() // V, V, _p(out_f32)), "token_ce")
    return out_f32


TOKENIZER_LEN, N_BINS = 151643, 256          # GPUInputStage's defaults (Qwen2.5's tokenizer.vocab_size, ActionTokenizer's bins)
TOKEN_METRIC_NAMES = ("action_accuracy", "l1_loss", "next_actions_accuracy", "next_actions_l1_loss")    # base_strategy.py:350-356


def token_row_class(labels: torch.Tensor, shift: int = 1, tokenizer_len: int = TOKENIZER_LEN, n_bins: int = N_BINS,
                    action_dim: Optional[int] = None, out: Optional[torch.Tensor] = None):
    """-> uint8 [B, L - shift]: 1 where get_current_action_mask(labels[:, shift:]) holds, 2 where get_next_actions_mask does, else 0
    (train_utils.py:8-41 with ACTION_TOKEN_BEGIN_IDX = tokenizer_len - (n_bins + 1), action_tokenizer.py:57)."""
    from .constants import ACTION_DIM
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous() and labels.dim() == 2
    B, L = labels.shape
    if out is None:
        out = torch.empty(B, L - shift, device=labels.device, dtype=torch.uint8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == B * (L - shift)
    N.check(_lib().vla_token_row_class(_st(), _p(labels), _p(out), B, L, shift, tokenizer_len - (n_bins + 1),
                                       ACTION_DIM if action_dim is None else action_dim), "token_row_class")
    return out


def token_ce_metrics(logits, tgt, row_class, out_f32, counters_u64, pred_ids=None, tokenizer_len: int = TOKENIZER_LEN,
                     n_bins: int = N_BINS, terms: Optional[torch.Tensor] = None):
    """token_ce (out_f32 receives the same two sums) plus, for the rows of class 1 (current action) / 2 (next actions) of row_class
    (uint8 [rows]), the argmax over the vocabulary and the decoded-bin statistics: counters_u64 (6 64-bit integers, zeroed by the
    caller) += per class (rows, rows whose argmax is the target, sum of |bin(argmax) - bin(target)|).  pred_ids (int32 [rows],
    optional): the argmax of every action row, -1 elsewhere.  logits [rows, V] bf16, any row stride that is a multiple of 8.
    terms (f32 [rows] scratch): vla_token_ce_metrics_ordered - every row's loss term goes there and one workgroup adds them in a fixed
    order, so the sum has the same bits in every run (the atomic form's last bit depends on the order the workgroups finish in)."""
    _chk_bf16(logits)
    assert logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    assert tgt.dtype == torch.int64 and tgt.is_contiguous() and tgt.numel() == rows
    assert row_class.dtype == torch.uint8 and row_class.is_contiguous() and row_class.numel() == rows
    assert out_f32.dtype == torch.float32 and out_f32.numel() >= 2
    assert counters_u64.dtype in (torch.int64, torch.uint64) and counters_u64.is_contiguous() and counters_u64.numel() == 6
    assert pred_ids is None or (pred_ids.dtype == torch.int32 and pred_ids.is_contiguous() and pred_ids.numel() == rows)
    if terms is not None:
        assert terms.dtype == torch.float32 and terms.is_contiguous() and terms.numel() == rows and terms.device == logits.device
        N.check(_lib().vla_token_ce_metrics_ordered(_st(), _p(logits), logits.stride(0), _p(tgt), _p(row_class), rows, V, _p(out_f32),
                                                    _p(counters_u64), _p(pred_ids), tokenizer_len, n_bins, _p(terms)), "token_ce_metrics_ordered")
        return out_f32
    N.check(_lib().vla_token_ce_metrics(_st(), _p(logits), logits.stride(0), _p(tgt), _p(row_class), rows, V, _p(out_f32),
                                        _p(counters_u64), _p(pred_ids), tokenizer_len, n_bins), "token_ce_metrics")
    return out_f32


def token_metrics_finish(counters, n_bins: int = N_BINS, min_action: float = -1.0, max_action: float = 1.0, out=None) -> dict:
    """The reference's four metric values from token_ce_metrics' counters, divided on the device (no sync): accuracy = correct /
    rows, L1 = sum * spacing / rows with spacing = (max_action - min_action) / (n_bins - 1), the distance of neighbouring bin
    centres.  -> {name: 0-dim f32 tensor} (views of one [4] buffer, `out` if given); a class without rows gives NaN."""
    assert counters.dtype in (torch.int64, torch.uint64) and counters.is_contiguous() and counters.numel() == 6
    if out is None:
        out = torch.empty(4, device=counters.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 4
    N.check(_lib().vla_token_metrics_finish(_st(), _p(counters), (max_action - min_action) / (n_bins - 1), _p(out)), "token_metrics_finish")
    return {k: out[i] for i, k in enumerate(TOKEN_METRIC_NAMES)}


def token_ce_bwd(logits, tgt, sums_f32, gscale: float, out):
    """d loss / d logits = gscale (softmax - onehot) / count (sums_f32 from token_ce); out may be logits itself (in place)."""
    V = logits.shape[-1]
    N.check(_lib().vla_token_ce_bwd(_st(), _p(logits), V, _p(tgt), logits.numel() // V, V, _p(sums_f32), gscale, _p(out), V),
            "token_ce_bwd")
    return out


def add_scalar_f32_(x: torch.Tensor, s: torch.Tensor):
    N.check(_lib().vla_add_scalar_f32(_st(), _p(x), _p(s), x.numel()), "add_scalar_f32")
    return x


# ---- input stage ------------------------------------------------------------------------------------
def image_normalize_u8_(img_u8: torch.Tensor, out: torch.Tensor, c0: int, mean, std):
    """img_u8 [B, H, W, 3] uint8 -> out[:, c0:c0+3] = ((img / 255) - mean) / std  (out [B, Ctot, H, W] bf16 or f32)."""
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and img_u8.dim() == 4 and img_u8.shape[-1] == 3
    B, H, W, _ = img_u8.shape
    assert out.is_contiguous() and out.shape[0] == B and tuple(out.shape[2:]) == (H, W) and out.dtype in (BF16, torch.float32)
    m3, s3 = (C.c_float * 3)(*[float(x) for x in mean]), (C.c_float * 3)(*[float(x) for x in std])
    N.check(_lib().vla_image_normalize_u8(_st(), _p(img_u8), _p(out), B, H, W, out.shape[1], c0, m3, s3,
                                          int(out.dtype == torch.float32)), "image_normalize_u8")
    return out


# op mask bits and parameter columns of vla_augment_stats / vla_augment_apply (include/vla_native.h)
AUG_CROP, AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE, AUG_DRAW = 1, 2, 4, 8, 16, 32
AUG_NPARAM = 9
AUG_P_U, AUG_P_Y1, AUG_P_X1, AUG_P_Y2, AUG_P_X2, AUG_P_BRIGHT, AUG_P_CONTRAST, AUG_P_SAT, AUG_P_HUE = range(9)


def image_augment_normalize_(frames_u8: torch.Tensor, out: torch.Tensor, norms, ops_mask: int, cfg7, params: torch.Tensor,
                             seed: int = 0, rank: int = 0, step: int = 0, frames_out: Optional[torch.Tensor] = None):
    """frames_u8 [B, n_img, H, W, 3] uint8 -> crop / brightness / contrast / saturation / hue (the enabled bits of ``ops_mask``),
    uint8 quantisation, then out[:, 3 * (im * len(norms) + j) + c] = ((q / 255) - mean_j[c]) / std_j[c] for every backbone
    (mean_j, std_j) of ``norms``.  params f32 [B * n_img, AUG_NPARAM]: read, or drawn in the kernel from (seed, rank, step, sample,
    image) and written when AUG_DRAW is set.  cfg7: the draw mapping's settings (crop side, brightness, contrast lo / hi,
    saturation lo / hi, hue).  frames_out: optional uint8 [B, n_img, H, W, 3] copy of the augmented frames."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.dim() == 5 and frames_u8.shape[-1] == 3
    B, n_img, H, W, _ = frames_u8.shape
    nb = len(norms)
    assert out.is_contiguous() and tuple(out.shape) == (B, 3 * nb * n_img, H, W) and out.dtype in (BF16, torch.float32)
    assert params.dtype == torch.float32 and params.is_contiguous() and tuple(params.shape) == (B * n_img, AUG_NPARAM)
    assert frames_out is None or (frames_out.dtype == torch.uint8 and frames_out.is_contiguous() and frames_out.shape == frames_u8.shape)
    mean = (C.c_float * (3 * nb))(*[float(x) for mu, _ in norms for x in mu])
    std = (C.c_float * (3 * nb))(*[float(x) for _, sd in norms for x in sd])
    cfg = (C.c_float * 7)(*[float(x) for x in cfg7])
    n = B * n_img
    slab = None
    if ops_mask & AUG_CONTRAST:        # the statistics pass: per-chunk channel sums of the post-brightness image
        slab = torch.empty(_lib().vla_augment_slab_floats(n, H, W), device=frames_u8.device, dtype=torch.float32)
        N.check(_lib().vla_augment_stats(_st(), _p(frames_u8), _p(params), _p(slab), n, H, W, n_img, ops_mask, cfg, seed, rank, step),
                "augment_stats")
    N.check(_lib().vla_augment_apply(_st(), _p(frames_u8), _p(params), _p(slab), _p(out), _p(frames_out), n, H, W, n_img, nb, mean, std,
                                     int(out.dtype == torch.float32), ops_mask, cfg, seed, rank, step), "augment_apply")
    return out


def action_tokenize(actions_f32: torch.Tensor, bins_f64: torch.Tensor, tokenizer_len: int, lo: float = -1.0, hi: float = 1.0):
    """ActionTokenizer (use_minivlm): int64 ids of the same shape = tokenizer_len - np.digitize(np.clip(a, lo, hi), bins)."""
    assert actions_f32.dtype == torch.float32 and actions_f32.is_contiguous() and bins_f64.dtype == torch.float64 and bins_f64.is_contiguous()
    ids = torch.empty(actions_f32.shape, device=actions_f32.device, dtype=torch.int64)
    N.check(_lib().vla_action_tokenize(_st(), _p(actions_f32), _p(bins_f64), _p(ids), actions_f32.numel(), bins_f64.numel(), lo, hi,
                                       tokenizer_len), "action_tokenize")
    return ids


def normalize_bounds(x_f32: torch.Tensor, low: torch.Tensor, high: torch.Tensor, mask: Optional[torch.Tensor] = None,
                     zero_mask: Optional[torch.Tensor] = None):
    """normalize_action_and_proprio's BOUNDS / BOUNDS_Q99 branch (data_utils.py:67-90) on x f32 [..., D]: clip(2 (x - low) / (high - low +
    1e-8) - 1, -1, 1) where mask (u8 [D], None = everywhere), then 0 where zero_mask (u8 [D], None = nowhere).  low / high f32 [D]."""
    D = x_f32.shape[-1]
    assert x_f32.dtype == torch.float32 and x_f32.is_contiguous() and x_f32.numel() > 0
    for t, dt in ((low, torch.float32), (high, torch.float32), (mask, torch.uint8), (zero_mask, torch.uint8)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() == D and t.device == x_f32.device), "per-dimension statistics: [D] on x's device"
    out = torch.empty_like(x_f32)
    N.check(_lib().vla_normalize_bounds(_st(), _p(x_f32), _p(out), x_f32.numel(), D, _p(low), _p(high), _p(mask), _p(zero_mask)), "normalize_bounds")
    return out


def collate_tokens(prompt_flat: torch.Tensor, prompt_off: torch.Tensor, actions_f32: torch.Tensor, bins_f64: torch.Tensor, L: int, *,
                   tokenizer_len: int, lo: float = -1.0, hi: float = 1.0, pad_id: int, ignore_index: int = -100, num_tokens: int = 64,
                   seed: int = 0, rank: int = 0, step: int = 0):
    """vla_collate_tokens: prompt_flat int64 [n] + prompt_off int32 [B + 1] + normalised actions f32 [B, n_act] -> (input_ids int64 [B, L],
    labels int64 [B, L], attention_mask u8 [B, L]), one launch, nothing read back."""
    B, n_act = actions_f32.shape
    dev = actions_f32.device
    assert actions_f32.dtype == torch.float32 and actions_f32.is_contiguous() and bins_f64.dtype == torch.float64 and bins_f64.is_contiguous()
    assert prompt_flat.dtype == torch.int64 and prompt_flat.is_contiguous() and prompt_flat.dim() == 1
    assert prompt_off.dtype == torch.int32 and prompt_off.is_contiguous() and tuple(prompt_off.shape) == (B + 1,)
    assert prompt_flat.device == dev and prompt_off.device == dev and bins_f64.device == dev
    assert L > 0
    ids, labels = torch.empty(B, L, device=dev, dtype=torch.int64), torch.empty(B, L, device=dev, dtype=torch.int64)
    am = torch.empty(B, L, device=dev, dtype=torch.uint8)
    N.check(_lib().vla_collate_tokens(_st(), _p(prompt_flat) if prompt_flat.numel() else None, _p(prompt_off), prompt_flat.numel(), _p(actions_f32),
                                      _p(bins_f64), _p(ids), _p(labels), _p(am), B, n_act, L, bins_f64.numel(), lo, hi, tokenizer_len, pad_id,
                                      ignore_index, num_tokens, int(seed) & (2 ** 64 - 1), int(rank), int(step)), "collate_tokens")
    return ids, labels, am


# ---- serving a batch (include/vla_serve.h, csrc/serve.hip) --------------------------------------------------------------------------
def serve_tokens(prompt_flat: torch.Tensor, prompt_off: torch.Tensor, L: int, *, pad_id: int, num_tokens: int = 64, fill_id: int = 1,
                 stop_id: int = 2, action_label: int = 151387, ignore_index: int = -100):
    """vla_serve_tokens: prompt_flat int64 [n] + prompt_off int32 [B + 1] -> (input_ids int64 [B, L], labels int64 [B, L], attention_mask
    u8 [B, L], hid_row int32 [B], row_ok u8 [B]): the batch of prepare_inference_inputs, right-padded, one launch, nothing read back."""
    B, dev = prompt_off.numel() - 1, prompt_off.device
    assert prompt_flat.dtype == torch.int64 and prompt_flat.is_contiguous() and prompt_flat.dim() == 1
    assert prompt_off.dtype == torch.int32 and prompt_off.is_contiguous() and prompt_off.dim() == 1 and B >= 1
    assert prompt_flat.device == dev and prompt_off.is_cuda
    if L < num_tokens + 2:
        raise ValueError(f"serve_tokens: L = {L} cannot hold one prompt id, {num_tokens} placeholders and the stop id")
    ids, labels = torch.empty(B, L, device=dev, dtype=torch.int64), torch.empty(B, L, device=dev, dtype=torch.int64)
    am = torch.empty(B, L, device=dev, dtype=torch.uint8)
    hid_row, row_ok = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.uint8)
    N.check(_lib().vla_serve_tokens(_st(), _p(prompt_flat) if prompt_flat.numel() else None, _p(prompt_off), prompt_flat.numel(), _p(ids),
                                    _p(labels), _p(am), _p(hid_row), _p(row_ok), B, int(L), num_tokens, fill_id, stop_id, action_label, pad_id,
                                    ignore_index), "serve_tokens")
    return ids, labels, am, hid_row, row_ok


def _chk_stats64(D, dev, low, high, mask):
    for t, dt in ((low, torch.float64), (high, torch.float64), (mask, torch.uint8)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and t.numel() == D and t.device == dev), "per-dimension statistics: [D] on the operand's device"


def normalize_proprio_serve(x: torch.Tensor, low: torch.Tensor, high: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_normalize_proprio_serve: the evaluator's normalize_proprio on x f32 / f64 [..., D] -> f32; low / high f64 [D], mask u8 [D] or None."""
    D = x.shape[-1]
    assert x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.is_contiguous() and x.numel() > 0
    _chk_stats64(D, x.device, low, high, mask)
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    N.check(_lib().vla_normalize_proprio_serve(_st(), _p(x), int(x.dtype == torch.float64), _p(out), x.numel(), D, _p(low), _p(high), _p(mask)),
            "normalize_proprio_serve")
    return out


def unnormalize_actions(pred: torch.Tensor, low: torch.Tensor, high: torch.Tensor, mask: Optional[torch.Tensor] = None,
                        row_ok: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_unnormalize_actions: pred bf16 [B, chunk, Da] (or [B, chunk * Da]; rows may be strided) -> f64 of the same shape, the bits of
    OpenVLAForActionPrediction._unnormalize_actions; rows whose row_ok (u8 [B]) is 0 become NaN."""
    _chk_bf16(pred)
    B, Da = pred.shape[0], low.numel()
    p2 = pred.reshape(B, -1) if pred.dim() != 2 else pred
    assert p2.stride(1) == 1 and p2.shape[1] % Da == 0
    _chk_stats64(Da, pred.device, low, high, mask)
    assert row_ok is None or (row_ok.dtype == torch.uint8 and row_ok.is_contiguous() and row_ok.numel() == B and row_ok.device == pred.device)
    if out is None:
        out = torch.empty(pred.shape, device=pred.device, dtype=torch.float64)
    o2 = out.view(B, -1) if out.dim() != 2 else out
    assert out.dtype == torch.float64 and o2.stride(1) == 1 and o2.shape == p2.shape
    N.check(_lib().vla_unnormalize_actions(_st(), _p(p2), _p(o2), B, p2.shape[1], Da, p2.stride(0), o2.stride(0), _p(low), _p(high), _p(mask),
                                           _p(row_ok)), "unnormalize_actions")
    return out


def serve_gather_hidden(hs: torch.Tensor, hid_row: torch.Tensor, Np: int, T: int = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_serve_gather_hidden: hs bf16 [B, S, D] (one hidden state) + hid_row int32 [B] -> [B, 1, T, D]: rows [Np + hid_row[b], +T) of sample b."""
    _chk_bf16(hs)
    B, S, D = hs.shape
    assert hs.stride(2) == 1 and hid_row.dtype == torch.int32 and hid_row.is_contiguous() and hid_row.numel() == B and hid_row.device == hs.device
    if out is None:
        out = torch.empty(B, 1, T, D, device=hs.device, dtype=BF16)
    assert out.is_contiguous() and out.numel() == B * T * D and out.dtype == BF16
    N.check(_lib().vla_serve_gather_hidden(_st(), _p(hs), _p(hid_row), _p(out), B, S, Np, T, D, hs.stride(0), hs.stride(1)), "serve_gather_hidden")
    return out


# ---- device-resident episodes (include/vla_episodes.h, csrc/episodes.hip) -----------------------------------------------------------
def _chk_vectors(op: str, dev, *operands) -> None:
    """The window pickers' operand check: every (tensor, dtype, length) is 1-D, contiguous, on ``dev``; a None tensor is skipped."""
    for t, dt, n in operands:
        assert t is None or (t.is_cuda and t.device == dev and t.dtype == dt and t.dim() == 1 and t.numel() == n and t.is_contiguous()), \
            f"{op}: bad operand"


def episode_sample(valid_off: torch.Tensor, episode_off: torch.Tensor, prompt_off: torch.Tensor, seed: int, rank: int, world: int, step: int,
                   Pmax: int, ep: torch.Tensor, row: torch.Tensor, out_off: torch.Tensor) -> None:
    """vla_episode_sample: the windows of the batch of (rank, step) -> ep int32 [B], row int64 [B], out_off int32 [B + 1] (all given)."""
    E, B, dev = valid_off.numel() - 1, ep.numel(), valid_off.device
    _chk_vectors("episode_sample", dev, (valid_off, torch.int64, E + 1), (episode_off, torch.int64, E + 1), (prompt_off, torch.int32, E + 1),
                 (ep, torch.int32, B), (row, torch.int64, B), (out_off, torch.int32, B + 1))
    N.check(_lib().vla_episode_sample(_st(), _p(valid_off), _p(episode_off), _p(prompt_off), E, int(seed) & (2 ** 64 - 1), int(rank), int(world),
                                      int(step), B, int(Pmax), _p(ep), _p(row), _p(out_off)), "episode_sample")


def episode_gather(frames: torch.Tensor, actions: torch.Tensor, proprio: torch.Tensor, episode_off: torch.Tensor, prompt_flat: torch.Tensor,
                   prompt_off: torch.Tensor, ep: torch.Tensor, row: torch.Tensor, out_off: torch.Tensor, out_frames: torch.Tensor,
                   out_actions: torch.Tensor, out_proprio: torch.Tensor, out_prompt: torch.Tensor, Pmax: int) -> None:
    """vla_episode_gather: the store's tensors + the sampler's index vectors -> the raw batch (all outputs given): out_frames u8
    [B, *frame], out_actions f32 [B, chunk, A], out_proprio f32 [B, Pd], out_prompt int64 [B * Pmax]."""
    B, E, T, dev = ep.numel(), episode_off.numel() - 1, frames.shape[0], frames.device
    chunk, A, Pd = out_actions.shape[1], actions.shape[1], proprio.shape[1]
    row_bytes = frames[0].numel()
    for t in (frames, actions, proprio, episode_off, prompt_flat, prompt_off, ep, row, out_off, out_frames, out_actions, out_proprio, out_prompt):
        assert t.is_cuda and t.device == dev and t.is_contiguous(), "episode_gather: operands are contiguous tensors on one device"
    assert frames.dtype == torch.uint8 and out_frames.dtype == torch.uint8 and tuple(out_frames.shape) == (B,) + tuple(frames.shape[1:])
    assert actions.dtype == torch.float32 and tuple(actions.shape) == (T, A) and out_actions.dtype == torch.float32 and tuple(out_actions.shape) == (B, chunk, A)
    assert proprio.dtype == torch.float32 and tuple(proprio.shape) == (T, Pd) and out_proprio.dtype == torch.float32 and tuple(out_proprio.shape) == (B, Pd)
    assert episode_off.dtype == torch.int64 and prompt_off.dtype == torch.int32 and prompt_off.numel() == E + 1 and prompt_flat.dtype == torch.int64
    assert ep.dtype == torch.int32 and row.dtype == torch.int64 and row.numel() == B and out_off.dtype == torch.int32 and out_off.numel() == B + 1
    assert out_prompt.dtype == torch.int64 and out_prompt.numel() == B * Pmax
    N.check(_lib().vla_episode_gather(_st(), _p(frames), _p(actions), _p(proprio), _p(episode_off), _p(prompt_flat) if prompt_flat.numel() else None,
                                      _p(prompt_off), _p(ep), _p(row), _p(out_off), _p(out_frames), _p(out_actions), _p(out_proprio),
                                      _p(out_prompt) if out_prompt.numel() else None, B, E, T, row_bytes, chunk, A, Pd, prompt_flat.numel(), int(Pmax)),
            "episode_gather")


# ---- JPEG frames of a device-resident store (include/vla_jpeg.h, csrc/jpeg.hip) --------------------------------------------------------
def jpeg_workspace_bytes(slots: int, H: int, W: int, h2v2: int) -> int:
    """vla_jpeg_workspace_bytes: what vla_jpeg_decode_rows needs for ``slots`` = B * n_img images (host arithmetic)."""
    n = _lib().vla_jpeg_workspace_bytes(int(slots), int(H), int(W), int(h2v2))
    if n < 0:
        raise ValueError(f"jpeg_workspace_bytes: {slots} images of {H} x {W} (sampling flag {h2v2}) are refused: H and W are multiples of 16")
    return n


def jpeg_decode_rows(data: torch.Tensor, img_seg: torch.Tensor, seg_tab: torch.Tensor, img_tab: torch.Tensor, qt_pool: torch.Tensor,
                     ht_pool: torch.Tensor, episode_off: torch.Tensor, T: int, ep: torch.Tensor, row: torch.Tensor, n_img: int, H: int, W: int,
                     h2v2: int, max_seg: int, mapping: int, workspace: torch.Tensor, out_frames: torch.Tensor, status: torch.Tensor,
                     seg_ent: Optional[torch.Tensor] = None) -> None:
    """vla_jpeg_decode_rows: the store's bytes and tables (jpeg_store.JpegFrames) + the sampler's index vectors -> out_frames u8
    [B, n_img, H, W, 3] and status u8 [B, n_img, max_seg] (both given; out_frames may be strided between images).  ``seg_ent`` (int32
    [S, 4], the entry state of every segment: a store with a scan index): vla_jpeg_decode_rows_at (include/vla_jpeg_index.h)."""
    B, E, dev, n_all = ep.numel(), episode_off.numel() - 1, data.device, int(T) * int(n_img)
    for t in (data, img_seg, seg_tab, img_tab, qt_pool, ht_pool, episode_off, ep, row, workspace, status):
        assert t.is_cuda and t.device == dev and t.is_contiguous(), "jpeg_decode_rows: operands are contiguous tensors on one device"
    assert data.dtype == torch.uint8 and data.dim() == 1 and workspace.dtype == torch.uint8
    assert img_seg.dtype == torch.int64 and img_seg.numel() == n_all + 1 and seg_tab.dtype == torch.int64 and seg_tab.dim() == 2 and seg_tab.shape[1] == 4
    assert img_tab.dtype == torch.int32 and tuple(img_tab.shape) == (n_all, 12)
    assert qt_pool.dtype == torch.int16 and qt_pool.dim() == 2 and qt_pool.shape[1] == 64 and ht_pool.dtype == torch.int32 and ht_pool.dim() == 2 and ht_pool.shape[1] == 548
    assert episode_off.dtype == torch.int64 and ep.dtype == torch.int32 and row.dtype == torch.int64 and row.numel() == B
    assert status.dtype == torch.uint8 and tuple(status.shape) == (B, n_img, max_seg)
    assert out_frames.is_cuda and out_frames.device == dev and out_frames.dtype == torch.uint8 and tuple(out_frames.shape) == (B, n_img, H, W, 3)
    image = out_frames.stride(1) if n_img > 1 else (out_frames.stride(0) if B > 1 else H * W * 3)          # elements between two images
    assert out_frames[0, 0].is_contiguous() and (B == 1 or out_frames.stride(0) == n_img * image), "jpeg_decode_rows: out_frames: contiguous images, one stride between them"
    tail = (_p(img_tab), _p(qt_pool), qt_pool.shape[0], _p(ht_pool), ht_pool.shape[0], _p(episode_off), E, int(T), _p(ep), _p(row), B, int(n_img),
            int(H), int(W), int(h2v2), int(max_seg), int(mapping), _p(workspace), workspace.numel(), _p(out_frames), int(image), _p(status))
    if seg_ent is None:
        N.check(_lib().vla_jpeg_decode_rows(_st(), _p(data), data.numel(), _p(img_seg), _p(seg_tab), seg_tab.shape[0], *tail), "jpeg_decode_rows")
        return
    assert seg_ent.is_cuda and seg_ent.device == dev and seg_ent.is_contiguous() and seg_ent.dtype == torch.int32 and tuple(seg_ent.shape) == (seg_tab.shape[0], 4)
    N.check(_lib().vla_jpeg_decode_rows_at(_st(), _p(data), data.numel(), _p(img_seg), _p(seg_tab), _p(seg_ent), seg_tab.shape[0], *tail),
            "jpeg_decode_rows_at")


def jpeg_index_build(data: torch.Tensor, img_seg: torch.Tensor, seg_tab: torch.Tensor, img_tab: torch.Tensor, qt_pool: torch.Tensor,
                     ht_pool: torch.Tensor, H: int, W: int, h2v2: int, piece_mcus: int, piece_off: torch.Tensor, s_begin: int, s_end: int,
                     mapping: int, out_seg_tab: torch.Tensor, out_seg_ent: torch.Tensor, out_status: torch.Tensor) -> None:
    """vla_jpeg_index_build (include/vla_jpeg_index.h): the segments [s_begin, s_end) of the store walked once and cut into pieces of
    ``piece_mcus`` MCUs - rows piece_off[s] .. piece_off[s + 1] of out_seg_tab int64 [S', 4] and out_seg_ent int32 [S', 4], and
    out_status u8 [S] (all given; only the slice's rows are written)."""
    dev, S, n_all = data.device, seg_tab.shape[0], img_tab.shape[0]
    for t in (data, img_seg, seg_tab, img_tab, qt_pool, ht_pool, piece_off, out_seg_tab, out_seg_ent, out_status):
        assert t.is_cuda and t.device == dev and t.is_contiguous(), "jpeg_index_build: operands are contiguous tensors on one device"
    assert data.dtype == torch.uint8 and data.dim() == 1
    assert img_seg.dtype == torch.int64 and img_seg.numel() == n_all + 1 and seg_tab.dtype == torch.int64 and seg_tab.dim() == 2 and seg_tab.shape[1] == 4
    assert img_tab.dtype == torch.int32 and img_tab.dim() == 2 and img_tab.shape[1] == 12
    assert qt_pool.dtype == torch.int16 and qt_pool.dim() == 2 and qt_pool.shape[1] == 64 and ht_pool.dtype == torch.int32 and ht_pool.dim() == 2 and ht_pool.shape[1] == 548
    assert piece_off.dtype == torch.int64 and piece_off.numel() == S + 1
    assert out_seg_tab.dtype == torch.int64 and out_seg_tab.dim() == 2 and out_seg_tab.shape[1] == 4
    assert out_seg_ent.dtype == torch.int32 and tuple(out_seg_ent.shape) == tuple(out_seg_tab.shape)
    assert out_status.dtype == torch.uint8 and out_status.numel() == S
    N.check(_lib().vla_jpeg_index_build(_st(), _p(data), data.numel(), _p(img_seg), _p(seg_tab), S, _p(img_tab), _p(qt_pool), qt_pool.shape[0],
                                        _p(ht_pool), ht_pool.shape[0], n_all, int(H), int(W), int(h2v2), int(piece_mcus), _p(piece_off),
                                        int(s_begin), int(s_end), int(mapping), _p(out_seg_tab), _p(out_seg_ent), out_seg_tab.shape[0],
                                        _p(out_status)), "jpeg_index_build")


# ---- a weighted mixture of device-resident datasets (include/vla_mixture.h, csrc/mixture.hip) ----------------------------------------
def mixture_sample(valid_off: torch.Tensor, episode_off: torch.Tensor, prompt_off: torch.Tensor, dataset_off: torch.Tensor,
                   quota_off: torch.Tensor, seed: int, rank: int, world: int, step: int, Pmax: int, ds: torch.Tensor, ep: torch.Tensor,
                   row: torch.Tensor, out_off: torch.Tensor) -> None:
    """vla_mixture_sample: the windows of the batch of (rank, step) -> ds int32 [B], ep int32 [B], row int64 [B], out_off int32 [B + 1]
    (all given)."""
    E, D, B, dev = valid_off.numel() - 1, dataset_off.numel() - 1, ep.numel(), valid_off.device
    _chk_vectors("mixture_sample", dev, (valid_off, torch.int64, E + 1), (episode_off, torch.int64, E + 1), (prompt_off, torch.int32, E + 1),
                 (dataset_off, torch.int32, D + 1), (quota_off, torch.int64, D + 1), (ds, torch.int32, B), (ep, torch.int32, B),
                 (row, torch.int64, B), (out_off, torch.int32, B + 1))
    N.check(_lib().vla_mixture_sample(_st(), _p(valid_off), _p(episode_off), _p(prompt_off), _p(dataset_off), _p(quota_off), E, D,
                                      int(seed) & (2 ** 64 - 1), int(rank), int(world), int(step), B, int(Pmax), _p(ds), _p(ep), _p(row),
                                      _p(out_off)), "mixture_sample")


def normalize_bounds_rows(x_f32: torch.Tensor, sel: torch.Tensor, low: torch.Tensor, high: torch.Tensor, mask: Optional[torch.Tensor] = None,
                          zero_mask: Optional[torch.Tensor] = None):
    """vla_normalize_bounds_rows: normalize_bounds on x f32 [R, ..., D] with the statistics set sel[r] (int32 [R], clamped into the
    tables) for row r; low / high f32 [n_sets, D], mask / zero_mask u8 [n_sets, D] or None.  A row equals normalize_bounds on that row."""
    R, D = x_f32.shape[0], x_f32.shape[-1]
    assert x_f32.dim() >= 2 and x_f32.dtype == torch.float32 and x_f32.is_contiguous() and x_f32.numel() > 0
    assert low.dim() == 2 and low.shape[1] == D, "per-set statistics: [n_sets, D]"
    n_sets, dev = low.shape[0], x_f32.device
    assert sel.dtype == torch.int32 and sel.is_contiguous() and tuple(sel.shape) == (R,) and sel.device == dev, "sel: int32 [R] on x's device"
    for t, dt in ((low, torch.float32), (high, torch.float32), (mask, torch.uint8), (zero_mask, torch.uint8)):
        assert t is None or (t.dtype == dt and t.is_contiguous() and tuple(t.shape) == (n_sets, D) and t.device == dev), \
            "per-set statistics: [n_sets, D] on x's device"
    out = torch.empty_like(x_f32)
    N.check(_lib().vla_normalize_bounds_rows(_st(), _p(x_f32), _p(out), R, x_f32.numel() // R, D, _p(sel), n_sets, _p(low), _p(high), _p(mask),
                                             _p(zero_mask)), "normalize_bounds_rows")
    return out


# ---- validation on held-out episodes (include/vla_heldout.h, csrc/heldout.hip) -------------------------------------------------------
def heldout_sweep(val_off: torch.Tensor, episode_off: torch.Tensor, prompt_off: torch.Tensor, dataset_off: Optional[torch.Tensor], rank: int,
                  world: int, batch_j: int, stride: int, Pmax: int, ds: torch.Tensor, ep: torch.Tensor, row: torch.Tensor, out_off: torch.Tensor,
                  valid: torch.Tensor) -> None:
    """vla_heldout_sweep: the held-out windows of validation batch batch_j of this rank, in order -> ds int32 [B], ep int32 [B], row int64
    [B], out_off int32 [B + 1], valid u8 [B] (all given).  dataset_off int32 [D + 1], or None for a single dataset."""
    E, B, dev = val_off.numel() - 1, ep.numel(), val_off.device
    D = 1 if dataset_off is None else dataset_off.numel() - 1
    _chk_vectors("heldout_sweep", dev, (val_off, torch.int64, E + 1), (episode_off, torch.int64, E + 1), (prompt_off, torch.int32, E + 1),
                 (dataset_off, torch.int32, D + 1), (ds, torch.int32, B), (ep, torch.int32, B), (row, torch.int64, B),
                 (out_off, torch.int32, B + 1), (valid, torch.uint8, B))
    N.check(_lib().vla_heldout_sweep(_st(), _p(val_off), _p(episode_off), _p(prompt_off), _p(dataset_off), E, D, int(rank), int(world),
                                     int(batch_j), int(stride), B, int(Pmax), _p(ds), _p(ep), _p(row), _p(out_off), _p(valid)), "heldout_sweep")


def heldout_l1_accumulate(pred: torch.Tensor, target: torch.Tensor, ds: Optional[torch.Tensor], valid: torch.Tensor, acc: torch.Tensor,
                          cnt: torch.Tensor) -> None:
    """vla_heldout_l1_accumulate: acc f64 [D, C, A] += per-dataset sums over the valid rows of |pred - target| (bf16 [B, C, A]), cnt int64
    [D] += their number; ds int32 [B] or None (all rows dataset 0), valid u8 [B]."""
    _chk_bf16(pred, target)
    B, Cc, A = pred.shape
    D, dev = acc.shape[0], pred.device
    assert pred.is_contiguous() and target.is_contiguous() and tuple(target.shape) == (B, Cc, A) and target.device == dev
    assert acc.dtype == torch.float64 and acc.is_contiguous() and tuple(acc.shape) == (D, Cc, A) and acc.device == dev
    assert cnt.dtype == torch.int64 and cnt.is_contiguous() and tuple(cnt.shape) == (D,) and cnt.device == dev
    assert valid.dtype == torch.uint8 and valid.is_contiguous() and tuple(valid.shape) == (B,) and valid.device == dev
    assert ds is None or (ds.dtype == torch.int32 and ds.is_contiguous() and tuple(ds.shape) == (B,) and ds.device == dev)
    N.check(_lib().vla_heldout_l1_accumulate(_st(), _p(pred), _p(target), _p(ds), _p(valid), B, Cc, A, D, _p(acc), _p(cnt)), "heldout_l1_accumulate")


# ---- state digest (include/vla_digest.h, csrc/digest.hip) ---------------------------------------------------------------------------
def state_digest(t: torch.Tensor, salt: int = 0, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_state_digest: the position-weighted 64-bit digest of the contiguous tensor ``t`` of 16-bit elements (bf16,
    fp16, int16) -> int64 [1] on t's device holding the u64's bits (``out``: given, 8-byte aligned).  Launched on the current stream;
    nothing synchronises - digest_value() reads it.  ``scratch``: int64 [>= 1] for the workgroups' partial sums; by default the current
    stream's scratch (scratch.ARENA)."""
    assert t.is_cuda and t.element_size() == 2 and t.is_contiguous(), f"state_digest: a contiguous CUDA tensor of 16-bit elements, got {t.dtype} {t.device}"
    n = t.numel()
    if n == 0:
        raise ValueError("state_digest: an empty view has no digest")
    if out is None:
        out = torch.empty(1, device=t.device, dtype=torch.int64)
    assert out.dtype == torch.int64 and out.numel() == 1 and out.device == t.device, "state_digest: out is int64 [1] on t's device"
    if scratch is None:
        slots = _lib().vla_state_digest_slots()
        scratch = ARENA.get(8 * slots, t.device).view(torch.int64)[:slots]
    assert scratch.dtype == torch.int64 and scratch.is_contiguous() and scratch.device == t.device and scratch.numel() >= 1
    N.check(_lib().vla_state_digest(_st(), _p(t), n, int(salt) & (2 ** 64 - 1), _p(scratch), scratch.numel(), _p(out)), "state_digest")
    return out


def digest_value(d) -> int:
    """The unsigned 64-bit value of a digest (an int64 [1] tensor of state_digest, or its .item()): a host sync for a tensor."""
    return int(d.item() if isinstance(d, torch.Tensor) else d) & (2 ** 64 - 1)


# ---- the evaluator's frame pipeline (include/vla_policy_image.h, csrc/policy_image.hip) ----------------------------------------------
def _frames_nhwc(frames: torch.Tensor, what: str):
    """uint8 [N, H, W, 3] on the device whose images are contiguous (the images themselves may be a stride apart) -> (N, H, W, stride)."""
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
        raise ValueError(f"{what}: frames are uint8 [N, H, W, 3] on the device, got {frames.dtype} {tuple(frames.shape)} on {frames.device}")
    n, H, W, _ = frames.shape
    if n < 1 or frames.stride()[1:] != (W * 3, 3, 1) or (n > 1 and frames.stride(0) < H * W * 3):
        raise ValueError(f"{what}: every image must be contiguous ({H} x {W} x 3), at least one image apart; strides {frames.stride()}")
    return n, H, W, (frames.stride(0) if n > 1 else H * W * 3)


def policy_jpeg_round_trip(frames: torch.Tensor, qtab: torch.Tensor, out: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_policy_jpeg_round_trip: uint8 [N, H, W, 3] (images a stride apart) -> uint8 of the same shape, the pixels a 4:2:0 baseline
    JPEG file of each frame decodes to.  qtab: int16 [2, 64] on the device, the luminance and chrominance quantisation tables in
    natural order (input_stage.jpeg_quant_tables).  H and W must be multiples of 16: ValueError otherwise."""
    n, H, W, stride = _frames_nhwc(frames, "policy_jpeg_round_trip")
    need = _lib().vla_policy_image_workspace_bytes(n, H, W, 0, 0, 1)
    if need < 0:
        raise ValueError(f"policy_jpeg_round_trip: {n} frames of {H} x {W} are refused: H and W must be multiples of 16 inside [16, 4096] "
                         "(a frame whose edge MCUs are partial would need libjpeg's edge replication, which is not built)")
    assert qtab.is_cuda and qtab.dtype == torch.int16 and tuple(qtab.shape) == (2, 64) and qtab.is_contiguous(), "qtab: int16 [2, 64] on the device"
    if out is None:
        out = torch.empty(n, H, W, 3, device=frames.device, dtype=torch.uint8)
    _, oh, ow, ostride = _frames_nhwc(out, "policy_jpeg_round_trip (out)")
    assert (out.shape[0], oh, ow) == (n, H, W) and out.device == frames.device
    if workspace is None:
        workspace = torch.empty(need, device=frames.device, dtype=torch.uint8)
    assert workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == frames.device
    N.check(_lib().vla_policy_jpeg_round_trip(_st(), _p(frames), stride, n, H, W, _p(qtab), _p(workspace), workspace.numel(), _p(out), ostride),
            "policy_jpeg_round_trip")
    return out


def policy_lanczos3_resize(frames: torch.Tensor, out_h: int, out_w: int, spans_v, spans_h, out: Optional[torch.Tensor] = None,
                           workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_policy_lanczos3_resize: uint8 [N, H, W, 3] (images a stride apart) -> uint8 [N, out_h, out_w, 3], tf.image.resize(method =
    "lanczos3", antialias=True) rounded and clamped.  spans_v / spans_h: (starts int32 [out_len], weights f32 [out_len, span]) on the
    device for H -> out_h and W -> out_w (input_stage.tf_lanczos3_spans); None for a side that does not change.  At least one side
    must change (the caller returns the frames as they are otherwise)."""
    n, H, W, stride = _frames_nhwc(frames, "policy_lanczos3_resize")
    need = _lib().vla_policy_image_workspace_bytes(n, H, W, int(out_h), int(out_w), 0)
    if need < 0:
        raise ValueError(f"policy_lanczos3_resize: {n} frames of {H} x {W} -> {out_h} x {out_w} are refused (sides inside [1, 4096], one must change)")

    def tab(sp, n_out, changes):
        if not changes:
            return None, None, 0
        st, w = sp
        assert st.is_cuda and st.dtype == torch.int32 and st.is_contiguous() and st.numel() == n_out, "starts: int32 [out_len] on the device"
        assert w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2 and w.shape[0] == n_out, "weights: f32 [out_len, span]"
        return st, w, int(w.shape[1])
    sv, wv, kv = tab(spans_v, out_h, H != out_h)
    sh, wh, kh = tab(spans_h, out_w, W != out_w)
    if out is None:
        out = torch.empty(n, out_h, out_w, 3, device=frames.device, dtype=torch.uint8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (n, out_h, out_w, 3)
    if workspace is None and need:
        workspace = torch.empty(need, device=frames.device, dtype=torch.uint8)
    N.check(_lib().vla_policy_lanczos3_resize(_st(), _p(frames), stride, n, H, W, int(out_h), int(out_w), _p(sv), _p(wv), kv, _p(sh), _p(wh), kh,
                                              _p(workspace), workspace.numel() if workspace is not None else 0, _p(out)), "policy_lanczos3_resize")
    return out


# ---- the JPEG encoder (include/vla_jpeg_encode.h, csrc/jpeg_encode.hip) -------------------------------------------------------------
_ENC_QTABS = {}


def _encode_qtab(quality: int, device) -> torch.Tensor:
    """input_stage.jpeg_quant_tables(quality) on the device, int16 [2, 64] (the same bits as its uint16), uploaded once per quality."""
    key = (int(quality), str(device))
    if key not in _ENC_QTABS:
        import numpy as np
        from .input_stage import jpeg_quant_tables
        _ENC_QTABS[key] = torch.from_numpy(jpeg_quant_tables(int(quality)).view(np.int16).copy()).to(device)
    return _ENC_QTABS[key]


def jpeg_encode(frames_u8: torch.Tensor, quality: int = 95, restart_rows: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 [N, H, W, 3] on the device (images a stride apart), or [T, n_img, H, W, 3] taken in (t, cam) order -> (frames_jpeg uint8
    [n_bytes], frame_off int64 [N + 1]) on the device: the baseline 4:2:0 files of the frames back to back, every one byte for byte
    what Pillow saves with quality, subsampling=2 and restart_marker_rows=restart_rows.  H and W must be multiples of 16 and
    restart_rows >= 1: ValueError otherwise.  The byte count is read back once, between the two calls of the encode."""
    if frames_u8.dim() == 5:
        T, n_img = frames_u8.shape[:2]
        if T > 1 and n_img > 1 and frames_u8.stride(0) != n_img * frames_u8.stride(1):
            raise ValueError(f"jpeg_encode: [T, n_img, H, W, 3] frames must be one image stride apart in (t, cam) order; strides {frames_u8.stride()}")
        st = frames_u8.stride(1) if n_img > 1 else frames_u8.stride(0)
        frames_u8 = frames_u8.as_strided((T * n_img,) + tuple(frames_u8.shape[2:]), (st,) + tuple(frames_u8.stride()[2:]))
    n, H, W, stride = _frames_nhwc(frames_u8, "jpeg_encode")
    need = _lib().vla_jpeg_encode_workspace_bytes(n, H, W, int(restart_rows))
    if need < 0:
        raise ValueError(f"jpeg_encode: {n} frames of {H} x {W} with restart_rows {restart_rows} are refused: H and W must be multiples of 16 "
                         "inside [16, 4096] and restart_rows >= 1 (a file without restart markers is coded serially: Pillow writes those)")
    qtab = _encode_qtab(quality, frames_u8.device)
    workspace = torch.empty(need, device=frames_u8.device, dtype=torch.uint8)
    frame_off = torch.empty(n + 1, device=frames_u8.device, dtype=torch.int64)
    N.check(_lib().vla_jpeg_encode_plan(_st(), _p(frames_u8), stride, n, H, W, _p(qtab), int(restart_rows), _p(workspace), need, _p(frame_off)),
            "jpeg_encode_plan")
    total = int(frame_off[-1].item())               # the one read-back of the encode: load time, not the step
    out = torch.empty(total, device=frames_u8.device, dtype=torch.uint8)
    N.check(_lib().vla_jpeg_encode_write(_st(), n, H, W, _p(qtab), int(restart_rows), _p(workspace), need, _p(frame_off), _p(out), total),
            "jpeg_encode_write")
    return out, frame_off


# ---- greedy decoding with a key/value cache (include/vla_decode.h, csrc/decode.hip) -------------------------------------------------
def _cache_view(name: str, k_cache: torch.Tensor, v_cache: torch.Tensor, B: int, Hkv: int, dh: int):
    """(S_cap, sample stride, row stride) of one layer's cache pair [B, S_cap, Hkv * dh] (same strides, unit inner stride)."""
    _chk_bf16(k_cache, v_cache)
    if k_cache.dim() != 3 or k_cache.shape != v_cache.shape or k_cache.stride() != v_cache.stride():
        raise ValueError(f"{name}: k_cache and v_cache must be [B, S_cap, Hkv * dh] views of one layout, got {tuple(k_cache.shape)} / {tuple(v_cache.shape)}")
    if k_cache.shape[0] != B or k_cache.shape[2] != Hkv * dh or k_cache.stride(2) != 1:
        raise ValueError(f"{name}: the cache is [B = {B}, S_cap, Hkv * dh = {Hkv * dh}] with unit inner stride, got {tuple(k_cache.shape)}")
    return k_cache.shape[1], k_cache.stride(0), k_cache.stride(1)


def _chk_pos(name: str, pos: torch.Tensor, B: int, dev):
    if pos.dtype != torch.int32 or not pos.is_contiguous() or pos.numel() != B or pos.device != dev:
        raise ValueError(f"{name}: pos must be a contiguous int32 [{B}] on {dev}, got {pos.dtype} {tuple(pos.shape)} on {pos.device}")


def decode_prompt(prompt_flat: torch.Tensor, prompt_off: torch.Tensor, L: int, Np: int, *, pad_id: int):
    """vla_decode_prompt: prompt_flat int64 [n] + prompt_off int32 [B + 1] -> (input_ids int64 [B, L], attention_mask u8 [B, L], pos int32
    [B] = Np + P - 1, last_row int32 [B] = b (Np + L) + pos, row_ok u8 [B]): the prompt-only batch of a generation, right-padded."""
    B, dev = prompt_off.numel() - 1, prompt_off.device
    if prompt_flat.dtype != torch.int64 or prompt_flat.dim() != 1 or not prompt_flat.is_contiguous():
        raise ValueError("decode_prompt: prompt_flat must be a contiguous int64 vector")
    if prompt_off.dtype != torch.int32 or prompt_off.dim() != 1 or not prompt_off.is_contiguous() or B < 1 or not prompt_off.is_cuda or prompt_flat.device != dev:
        raise ValueError("decode_prompt: prompt_off must be a contiguous int32 [B + 1] on the device of prompt_flat, B >= 1")
    if L < 1 or Np < 0:
        raise ValueError(f"decode_prompt: L >= 1 and Np >= 0, got L = {L}, Np = {Np}")
    ids, am = torch.empty(B, L, device=dev, dtype=torch.int64), torch.empty(B, L, device=dev, dtype=torch.uint8)
    pos, last_row = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
    row_ok = torch.empty(B, device=dev, dtype=torch.uint8)
    N.check(_lib().vla_decode_prompt(_st(), _p(prompt_flat) if prompt_flat.numel() else None, _p(prompt_off), prompt_flat.numel(), _p(ids), _p(am),
                                     _p(pos), _p(last_row), _p(row_ok), B, int(L), int(Np), int(pad_id)), "decode_prompt")
    return ids, am, pos, last_row, row_ok


def decode_rope_append_(qkv: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor, pos: torch.Tensor, k_cache: torch.Tensor,
                        v_cache: torch.Tensor, Hq: int, Hkv: int, dh: int):
    """vla_decode_rope_append: qkv bf16 [B, (Hq + 2 Hkv) dh] (rows may be strided) - q rotated in place at pos[b], the rotated k and
    the v written to row pos[b] of sample b of k_cache / v_cache [B, S_cap, Hkv dh]; tables f32 [S_cap, dh / 2]."""
    _chk_bf16(qkv)
    B = qkv.shape[0]
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] != (Hq + 2 * Hkv) * dh:
        raise ValueError(f"decode_rope_append: qkv must be [B, (Hq + 2 Hkv) dh = {(Hq + 2 * Hkv) * dh}] with unit inner stride, got {tuple(qkv.shape)}")
    S_cap, sb, ss = _cache_view("decode_rope_append", k_cache, v_cache, B, Hkv, dh)
    _chk_pos("decode_rope_append", pos, B, qkv.device)
    for t in (cos_t, sin_t):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (S_cap, dh // 2) or t.device != qkv.device:
            raise ValueError(f"decode_rope_append: the tables are contiguous f32 [S_cap = {S_cap}, dh / 2 = {dh // 2}], got {t.dtype} {tuple(t.shape)}")
    N.check(_lib().vla_decode_rope_append(_st(), _p(qkv), _p(cos_t), _p(sin_t), _p(pos), _p(k_cache), _p(v_cache), B, Hq, Hkv, dh, qkv.stride(0),
                                          S_cap, sb, ss), "decode_rope_append")
    return qkv


def decode_attn(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, pos: torch.Tensor, Hq: int, Hkv: int, dh: int,
                out: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """vla_decode_attn: q bf16 [B, Hq dh] (one rotated query row per sample; rows may be strided) against keys / values 0 .. pos[b] of
    the cache -> out bf16 [B, Hq dh]."""
    _chk_bf16(q, out)
    B = q.shape[0]
    if q.dim() != 2 or q.stride(1) != 1 or q.shape[1] != Hq * dh:
        raise ValueError(f"decode_attn: q must be [B, Hq dh = {Hq * dh}] with unit inner stride, got {tuple(q.shape)}")
    if dh not in (64, 128) or Hq % Hkv or Hq // Hkv > 8:
        raise ValueError(f"decode_attn: head dim 64 or 128 and at most 8 query heads per kv head, got Hq = {Hq}, Hkv = {Hkv}, dh = {dh}")
    S_cap, sb, ss = _cache_view("decode_attn", k_cache, v_cache, B, Hkv, dh)
    _chk_pos("decode_attn", pos, B, q.device)
    if out is None:
        out = torch.empty(B, Hq * dh, device=q.device, dtype=BF16)
    if tuple(out.shape) != (B, Hq * dh) or out.stride(1) != 1:
        raise ValueError(f"decode_attn: out must be [B, Hq dh] with unit inner stride, got {tuple(out.shape)}")
    N.check(_lib().vla_decode_attn(_st(), _p(q), _p(k_cache), _p(v_cache), _p(pos), _p(out), B, Hq, Hkv, dh, q.stride(0), out.stride(0), S_cap, sb,
                                   ss, float(dh ** -0.5 if scale is None else scale)), "decode_attn")
    return out


def decode_argmax_workspace(B: int, V: int, device):
    """(part_val f32 [B, slabs], part_idx int32 [B, slabs]) of decode_lm_head_argmax for a vocabulary of V rows."""
    n = _lib().vla_decode_argmax_slabs(int(V))
    if n < 1 or B < 1:
        raise ValueError(f"decode_argmax_workspace: B >= 1 and V >= 1, got B = {B}, V = {V}")
    return torch.empty(B, n, device=device, dtype=torch.float32), torch.empty(B, n, device=device, dtype=torch.int32)


def decode_lm_head_argmax(x: torch.Tensor, W: torch.Tensor, ws, ids: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None,
                          advance=None, pos_from: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_decode_lm_head_argmax: x bf16 [B, D], W bf16 [V, D] -> ids int64 [B], the argmax of bf16(x W^T) in torch.argmax's order, no
    [B, V] tensor formed unless logits_out (bf16 [B, V], rows may be strided) asks for the compared values.  ws: decode_argmax_workspace.
    advance = (out_ids int64 [B, T], step int32 [1], pos int32 [B], embed bf16 [vocab, D], x_next bf16 [B, D]): out_ids[:, step] = ids,
    x_next = embed[ids], pos += 1, step += 1 in the finishing pass.  pos_from int32 [B] (with advance): the first advance of a generation -
    step counts from 0 and pos = pos_from + 1."""
    _chk_bf16(x, W, logits_out)
    if x.dim() != 2 or W.dim() != 2 or x.stride(1) != 1 or W.stride(1) != 1 or x.shape[1] != W.shape[1]:
        raise ValueError(f"decode_lm_head_argmax: x [B, D] and W [V, D] with unit inner strides, got {tuple(x.shape)} / {tuple(W.shape)}")
    (B, D), V, dev = x.shape, W.shape[0], x.device
    if not 1 <= B <= 64 or D % 8 or D > 4096:
        raise ValueError(f"decode_lm_head_argmax: B in [1, 64] and D a multiple of 8 up to 4096, got B = {B}, D = {D}")
    pv, pi = ws
    n = _lib().vla_decode_argmax_slabs(V)
    if pv.dtype != torch.float32 or pi.dtype != torch.int32 or not pv.is_contiguous() or not pi.is_contiguous() or pv.numel() < B * n or pi.numel() < B * n:
        raise ValueError(f"decode_lm_head_argmax: the workspace holds f32 and int32 [B = {B}, slabs = {n}] (decode_argmax_workspace)")
    if ids is None:
        ids = torch.empty(B, device=dev, dtype=torch.int64)
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() != B:
        raise ValueError(f"decode_lm_head_argmax: ids must be a contiguous int64 [{B}]")
    ldl = 0
    if logits_out is not None:
        if tuple(logits_out.shape) != (B, V) or logits_out.stride(1) != 1:
            raise ValueError(f"decode_lm_head_argmax: logits_out must be [B, V] = [{B}, {V}] with unit inner stride, got {tuple(logits_out.shape)}")
        ldl = logits_out.stride(0)
    a = [None, 0, None, None, None, None, 0, 0, None, 0]
    if pos_from is not None and advance is None:
        raise ValueError("decode_lm_head_argmax: pos_from belongs to an advance")
    if advance is not None:
        out_ids, step, pos, embed, x_next = advance
        _chk_bf16(embed, x_next)
        _chk_pos("decode_lm_head_argmax", pos, B, dev)
        if out_ids.dtype != torch.int64 or not out_ids.is_contiguous() or out_ids.dim() != 2 or out_ids.shape[0] != B:
            raise ValueError(f"decode_lm_head_argmax: out_ids must be a contiguous int64 [B = {B}, T], got {out_ids.dtype} {tuple(out_ids.shape)}")
        if step.dtype != torch.int32 or step.numel() != 1:
            raise ValueError("decode_lm_head_argmax: step must be one int32 on the device")
        if embed.dim() != 2 or embed.shape[1] != D or embed.stride(1) != 1 or tuple(x_next.shape) != (B, D) or x_next.stride(1) != 1:
            raise ValueError(f"decode_lm_head_argmax: embed [vocab, D = {D}] and x_next [B, D] with unit inner strides, got {tuple(embed.shape)} / {tuple(x_next.shape)}")
        if pos_from is not None:
            _chk_pos("decode_lm_head_argmax", pos_from, B, dev)
        a = [_p(out_ids), out_ids.shape[1], _p(step), _p(pos), _p(pos_from), _p(embed), embed.shape[0], embed.stride(0), _p(x_next), x_next.stride(0)]
    N.check(_lib().vla_decode_lm_head_argmax(_st(), _p(x), x.stride(0), _p(W), W.stride(0), B, D, V, _p(pv), _p(pi), _p(ids), _p(logits_out), ldl, *a),
            "decode_lm_head_argmax")
    return ids


# ---- sampling of action tokens (include/vla_sample.h, csrc/sample.hip) ---------------------------------------------------------------
SAMPLE_PARAM_BYTES = 24


def sample_params(*, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0, greedy: bool = False) -> torch.Tensor:
    """The parameter block of vla_sample_tokens as a uint8 [24] tensor on the host (f32 temperature, f32 top_p, i32 top_k, i32 greedy,
    u64 seed): copied into the device block a captured graph reads.  Refuses what the rule does not define."""
    import struct
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature > 0:
        raise ValueError(f"sample_params: temperature must be a number above 0, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < 2 ** 31:
        raise ValueError(f"sample_params: top_k must be an int >= 0 (0 switches the filter off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1:
        raise ValueError(f"sample_params: top_p must lie in (0, 1], got {top_p!r}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"sample_params: seed must be an int, got {seed!r}")
    raw = struct.pack("<ffiiQ", float(temperature), float(top_p), int(top_k), 1 if greedy else 0, seed & (2 ** 64 - 1))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8)


def sample_tokens(logits: torch.Tensor, params: torch.Tensor, step: torch.Tensor, ids: Optional[torch.Tensor] = None,
                  streams: Optional[torch.Tensor] = None, logprob_out: Optional[torch.Tensor] = None, probs_out: Optional[torch.Tensor] = None,
                  advance=None, pos_from: Optional[torch.Tensor] = None) -> torch.Tensor:
    """vla_sample_tokens: logits bf16 [B, V] (rows may be strided; what decode_lm_head_argmax stores in logits_out) -> ids int64 [B], one
    decoding step of the rule of include/vla_sample.h.  params: the device copy of sample_params() (uint8 [24], 8-B aligned).  step: the
    int32 [1] device step counter t (read; advanced only by an advance).  streams int64 [B] or None (row b draws from stream b).
    logprob_out f32 [B, T] (column t is written), probs_out f32 [B, V] (the filtered, renormalised probabilities; rows may be strided).
    advance = (out_ids, step, pos, embed, x_next) and pos_from: as decode_lm_head_argmax takes them."""
    if logits.dtype != BF16 or logits.dim() != 2 or logits.stride(1) != 1 or not logits.is_cuda:
        raise ValueError(f"sample_tokens: logits must be a bf16 [B, V] device tensor with unit inner stride, got {tuple(logits.shape)}")
    (B, V), dev = logits.shape, logits.device
    if not 1 <= B <= 64 or V < 1 or (B > 1 and logits.stride(0) < V):
        raise ValueError(f"sample_tokens: B in [1, 64], V >= 1 and a row stride of at least V, got B = {B}, V = {V}")
    if params.dtype != torch.uint8 or params.numel() != SAMPLE_PARAM_BYTES or not params.is_contiguous() or params.device != dev or params.data_ptr() % 8:
        raise ValueError("sample_tokens: params must be the 8-B aligned uint8 [24] device copy of ops.sample_params()")
    if step.dtype != torch.int32 or step.numel() != 1 or step.device != dev:
        raise ValueError("sample_tokens: step must be one int32 on the device")
    if ids is None:
        ids = torch.empty(B, device=dev, dtype=torch.int64)
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() != B or ids.device != dev:
        raise ValueError(f"sample_tokens: ids must be a contiguous int64 [{B}]")
    if streams is not None and (streams.dtype != torch.int64 or not streams.is_contiguous() or streams.numel() != B or streams.device != dev):
        raise ValueError(f"sample_tokens: streams must be a contiguous int64 [{B}] on {dev}")
    T = 0
    if logprob_out is not None:
        if logprob_out.dtype != torch.float32 or logprob_out.dim() != 2 or logprob_out.shape[0] != B or not logprob_out.is_contiguous() or logprob_out.device != dev:
            raise ValueError(f"sample_tokens: logprob_out must be a contiguous f32 [B = {B}, T]")
        T = logprob_out.shape[1]
    ldp = 0
    if probs_out is not None:
        if probs_out.dtype != torch.float32 or tuple(probs_out.shape) != (B, V) or probs_out.stride(1) != 1 or probs_out.device != dev:
            raise ValueError(f"sample_tokens: probs_out must be f32 [B, V] = [{B}, {V}] with unit inner stride")
        ldp = probs_out.stride(0)
    if pos_from is not None and advance is None:
        raise ValueError("sample_tokens: pos_from belongs to an advance")
    a = [None, T, _p(step), None, None, None, 0, 0, None, 0, 0]
    if advance is not None:
        out_ids, step_a, pos, embed, x_next = advance
        _chk_bf16(embed, x_next)
        _chk_pos("sample_tokens", pos, B, dev)
        if step_a is not step:
            raise ValueError("sample_tokens: the advance moves the step counter the draw reads")
        if out_ids.dtype != torch.int64 or not out_ids.is_contiguous() or out_ids.dim() != 2 or out_ids.shape[0] != B:
            raise ValueError(f"sample_tokens: out_ids must be a contiguous int64 [B = {B}, T], got {out_ids.dtype} {tuple(out_ids.shape)}")
        if logprob_out is not None and out_ids.shape[1] != T:
            raise ValueError("sample_tokens: out_ids and logprob_out hold the same T columns")
        D = embed.shape[1] if embed.dim() == 2 else 0
        if embed.dim() != 2 or D % 8 or embed.stride(1) != 1 or tuple(x_next.shape) != (B, D) or x_next.stride(1) != 1:
            raise ValueError(f"sample_tokens: embed [vocab, D] and x_next [B, D] with unit inner strides and D a multiple of 8, got {tuple(embed.shape)} / {tuple(x_next.shape)}")
        if pos_from is not None:
            _chk_pos("sample_tokens", pos_from, B, dev)
        a = [_p(out_ids), out_ids.shape[1], _p(step), _p(pos), _p(pos_from), _p(embed), embed.shape[0], embed.stride(0), _p(x_next), x_next.stride(0), D]
    N.check(_lib().vla_sample_tokens(_st(), _p(logits), logits.stride(0), B, V, _p(params), _p(streams), _p(ids), _p(logprob_out), _p(probs_out),
                                     ldp, *a), "sample_tokens")
    return ids
