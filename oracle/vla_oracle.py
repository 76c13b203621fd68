"""CPU restatement (oracle) of the VLA-Adapter fine-tune hot path.  TEST INFRASTRUCTURE ONLY.

This file is the *checker* for the HIP kernels in ``vla_adapter_amd/csrc``: only ``tests/``,
``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import it.  The product path
(``vla_adapter_amd``) never imports anything from ``oracle/`` and fails loudly when the HIP extension is
missing.

Every function restates, as explicit tensor arithmetic on CPU (torch is used here as a numpy-like array
library + reverse-mode differentiation of the restated math), one row of SURVEY.md §8(a).  Citations are
``path:line`` relative to the reference checkout (``/root/reference``).

Pinning: the reference ships no tests/golden vectors.  ``tools/make_golden.py`` imports the
reference's own leaf modules (``prismatic/models/action_heads.py``, ``prismatic/models/projectors.py``,
``prismatic/training/train_utils.py``, ``prismatic/vla/constants.py``) and the installed ``transformers``
Qwen2 (the reference's pinned fork is absent) and writes ``tests/golden/*.npz``; ``tests/test_oracle_golden.py``
checks this file against them.  Rows a1, a7, a8, a9, a10 are therefore pinned by reference code run here;
a5 is pinned by installed-transformers Qwen2 (third-party, version differs from the reference's pin);
a3 (ViT; timm absent) is pinned by third-party stand-ins too since round 4: installed transformers' SiglipVisionModel and
Dinov2WithRegistersModel (tools/make_golden_vit.py).  a2, a4, a6 (VLM glue) and the batch-1 predict_action restatement are pinned
by the reference's own modeling_prismatic.py forward / predict_action and finetune.py's run_forward_pass, run in fp32 with the
stand-ins above (tools/make_golden_vla.py -> tests/golden/vla_*.npz).  a11 (LoRA; peft is not importable) is pinned
through the full-weight gradient: the same run with W_eff = W + 2 B A (tests/golden/vla_lora_*.npz; peft's bf16 rounding order stays unpinned); the fp8 registry restates the NATIVE build's arithmetic
(the reference has no fp8 code).  token_ce is pinned like a5: against the loss / logits of installed transformers'
Qwen2ForCausalLM (tools/make_golden_ce.py -> tests/golden/qwen2_tiny_ce.npz) and torch's cross_entropy.

Precision: ``emu=False`` is straight fp32.  ``emu=True`` rounds to bf16 at the points where the reference's
bf16 autocast / bf16 modules round (after every Linear, activation, residual add, norm output), with fp32
accumulation inside each op - the same rounding points the HIP kernels use.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F  # only: erf-GELU / softmax primitives used as array math

IGNORE_INDEX = -100                 # prismatic/vla/constants.py:11
ACTION_TOKEN_BEGIN_IDX = 151386     # prismatic/vla/constants.py:13
STOP_INDEX = 2                      # prismatic/vla/constants.py:14
NUM_TOKENS = 64                     # prismatic/vla/constants.py:15
ACTION_DIM = 7                      # prismatic/vla/constants.py:28-33 (LIBERO)
NUM_ACTIONS_CHUNK = 8
PROPRIO_DIM = 8


def rnd(x: torch.Tensor, emu: bool) -> torch.Tensor:
    """bf16 rounding point (identity in fp32 mode)."""
    return x.to(torch.bfloat16).to(torch.float32) if emu else x


def linear(x, w, b=None, emu=False, strided_input=False):
    """nn.Linear: y = x W^T + b, one rounding after bias (fp32 accumulate).
    strided_input (bf16 emulation only): torch's CPU nn.Linear on a NON-CONTIGUOUS 3-D bf16 input does not take the fused
    addmm path - it runs matmul, rounds the product to bf16, then adds the bias and rounds again.  That is how the reference
    run computes k_task / v_task (k_proj / v_proj in the original block): h_t is a strided slice of the [B, 25, K+64, D] tensor
    (action_heads.py:57, 118) - for batch size > 1 only: with B = 1 the slice [1, K, D] counts as contiguous (size-1
    dimensions are ignored) and the fused path is taken (batch-1 inference!).  Verified op by op against the reference module in this container and pinned by
    tests/golden/head_bf16_*.npz; every other Linear of the head sees a contiguous input (cat / view outputs)."""
    if id(w) in FP8:             # opt-in fp8 weight path: both operands fake-quantised per row (e4m3, scale amax / 448)
        base = lambda: _Fp8Product.apply(x, w, FP8_BWD)      # (the low-rank branch below reads the UN-quantised input)
    else:
        base = lambda: x @ w.t()
    y = base()
    if b is not None:
        y = (rnd(y, emu) if strided_input else y) + b
    y = rnd(y, emu)
    l = LORA.get(id(w))
    xl = x
    if l is not None and id(w) in LORA_DROP:       # peft: lora_A(lora_dropout(x)) - the module's own mask over its input (training mode)
        mask, p = LORA_DROP[id(w)]
        xl = rnd(x * mask.reshape(x.shape) * (1.0 / (1.0 - p)), emu)
    if l is not None and LORA_FUSED:
        # the native build's form (vla_adapter_amd/trainers.py): the low-rank branch inside the base product's fp32 accumulator -
        # t = bf16(scale x A^T), y = bf16(x W^T + t B^T + b): ONE rounding of y where peft's module-by-module evaluation has three
        A, Bm, scale = l
        y = base() + rnd(scale * (xl @ A.t()), emu) @ Bm.t()
        return rnd(y + b, emu) if b is not None else rnd(y, emu)
    if l is not None:            # peft Linear.forward: result = base(x) + lora_B(lora_A(x)) * scaling, every step a bf16 tensor
        A, Bm, scale = l
        y = rnd(y + rnd(rnd(rnd(xl @ A.t(), emu) @ Bm.t(), emu) * scale, emu), emu)
    return y


def linear_group(x, wbs, emu=False):
    """Several Linears on the SAME input (q / k / v; gate / up): one ``linear`` each - except when their base products run on fp8
    operands INCLUDING the backward (FP8_BWD): the native build forms them as one product on a fused weight, so the gradient row
    that is quantised for dx = Q(dy) Q(W^T)^T is the CONCATENATION of their output gradients (one scale per row over q | k | v),
    and a row of W^T spans all of their output channels.  Forward values are the same either way (per-output-channel weight
    scales, shared input).  The fused LoRA form only (LORA_FUSED) or no LoRA."""
    ws = [w for w, _ in wbs]
    if not (FP8_BWD and all(id(w) in FP8 for w in ws)):
        return [linear(x, w, b, emu) for w, b in wbs]
    base = _Fp8Product.apply(x, torch.cat([w.detach() for w in ws], 0), True)
    outs, o = [], 0
    for w, b in wbs:
        y = base[..., o:o + w.shape[0]]
        o += w.shape[0]
        l = LORA.get(id(w))
        if l is not None:
            assert LORA_FUSED, "fp8 base products: the fused single-rounding LoRA form"
            A, Bm, scale = l
            y = y + rnd(scale * (x @ A.t()), emu) @ Bm.t()
        outs.append(rnd(y + b, emu) if b is not None else rnd(y, emu))
    return outs


# fp8 registry (BASELINE configs[4] "fp8 MFMA weight path"; the reference has no fp8 code: PARITY UNPINNED): ids of the weight
# tensors whose Linear runs on e4m3 operands in the native build (vla_quant_fp8_rows semantics: per-row dynamic scale for the
# input, per-output-channel scale for the weight, fp32 accumulation of the dequantised values).
FP8: set = set()
FP8_BWD = False       # True: the dX product of a registered Linear runs on e4m3 operands too (LoRAFinetune(fp8_backward=True))


class _Fp8Product(torch.autograd.Function):
    """y = Q(x) Q(W)^T with rows of x and rows of W (output channels) quantised to e4m3; the weight is frozen (no dW).  Backward:
    dx = dy W through the un-quantised weight (the engine's adapter-only step: bf16 W^T), or - bwd_fp8 - dx = Q(dy) Q(W^T)^T with
    rows of dy and rows of W^T (INPUT channels) quantised: the arithmetic of trainers.LoRAFinetune._lin_bwd on fp8 operands."""

    @staticmethod
    def forward(ctx, x, w, bwd_fp8):
        ctx.save_for_backward(w)
        ctx.bwd_fp8 = bool(bwd_fp8)
        return fake_quant_e4m3_rows(x) @ fake_quant_e4m3_rows(w).t()

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        if ctx.bwd_fp8:
            return fake_quant_e4m3_rows(dy) @ fake_quant_e4m3_rows(w.detach().t().contiguous()).t(), None, None
        return dy @ w.detach(), None, None


def fake_quant_e4m3_rows(t):
    """Quantise-dequantise every row of the last dimension to OCP e4m3 with the scale amax / 448 (vla_quant_fp8_rows)."""
    a = t.detach().abs().amax(dim=-1, keepdim=True)
    inv = torch.where(a > 0, 448.0 / a, torch.ones_like(a))
    q = (t.detach() * inv).to(torch.float8_e4m3fn).to(t.dtype)
    return q * torch.where(a > 0, a / 448.0, torch.ones_like(a))


# LoRA registry (a11, pinned through the full-weight gradient: tests/test_oracle_golden.py): id(base weight tensor) -> (A [r, in], B [out, r], alpha / r).  Tests fill it
# to evaluate the LoRA-wrapped model (vla-scripts/finetune.py:832-844) through the unchanged restated forward.
LORA: Dict[int, Tuple[torch.Tensor, torch.Tensor, float]] = {}
LORA_FUSED = False     # True: restate the native build's single-rounding evaluation instead of peft's module-by-module one
# lora_dropout > 0 (vla-scripts/finetune.py:110): id(base weight tensor) -> (keep mask of the module's input, 0/1 floats, any shape that
# reshapes to the input's; p).  Tests fill it with the masks the native kernel generated (torch's Philox stream is not reproduced).
LORA_DROP: Dict[int, Tuple[torch.Tensor, float]] = {}


def gelu(x, emu=False, tanh=False):
    return rnd(F.gelu(x, approximate="tanh" if tanh else "none"), emu)


def layer_norm(x, w, b, eps, emu=False):
    """nn.LayerNorm over the last dim, fp32 statistics (biased variance)."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return rnd((x - mu) * torch.rsqrt(var + eps) * w + b, emu)


# ----------------------------------------------------------------------------------------------
# a1  action masks  (prismatic/training/train_utils.py:8-23, 26-41; modeling_prismatic.py:456-461)
# ----------------------------------------------------------------------------------------------
def current_action_mask(token_ids: torch.Tensor) -> torch.Tensor:
    cumsum = torch.cumsum((token_ids != IGNORE_INDEX).to(torch.int64), dim=1)
    return ((1 <= cumsum) & (cumsum <= ACTION_DIM)) & (token_ids > ACTION_TOKEN_BEGIN_IDX)


def next_actions_mask(token_ids: torch.Tensor) -> torch.Tensor:
    cumsum = torch.cumsum((token_ids != IGNORE_INDEX).to(torch.int64), dim=1)
    return (cumsum > ACTION_DIM) & (token_ids > ACTION_TOKEN_BEGIN_IDX)


def all_actions_mask(labels: torch.Tensor) -> torch.Tensor:
    return current_action_mask(labels) | next_actions_mask(labels)


# ----------------------------------------------------------------------------------------------
# a2  embedding + action-query splice (modeling_prismatic.py:601, 418-454, 486-510)
# ----------------------------------------------------------------------------------------------
def embed_splice(input_ids, labels, attention_mask, embed_table, action_queries, patches):
    """-> (multimodal_embeddings [B, L+Np, D], multimodal_mask [B, L+Np] bool).

    k-th True position of the (current|next) mask on ``labels`` receives ``action_queries[k]``;
    sequence = [tok0 | patches | tok1..]; mask = attention_mask with ones for the patches.
    """
    B, L = input_ids.shape
    emb = embed_table[input_ids]                                  # :601
    mask = all_actions_mask(labels)                               # :605
    out = emb.clone()
    for b in range(B):                                            # :439-447 (k-th True <- k-th query)
        idx = torch.where(mask[b])[0]
        assert idx.numel() == action_queries.shape[0], "mask must select NUM_TOKENS positions per row"
        out[b, idx] = action_queries
    mm = torch.cat([out[:, :1], patches, out[:, 1:]], dim=1)      # :499-501
    ones = torch.ones(B, patches.shape[1], dtype=torch.bool)
    mm_mask = torch.cat([attention_mask[:, :1].bool(), ones, attention_mask[:, 1:].bool()], dim=1)  # :505-508
    return mm, mm_mask


def attention(q, k, v, causal: bool, kmask=None, scale=None, emu=False):
    """softmax(scale q k^T + mask) v.  q [B,H,Sq,dh], k/v [B,Hkv,Sk,dh] (GQA: H % Hkv == 0), kmask [B,Sk] bool.
    fp32 softmax, probabilities rounded to bf16 before P@V (transformers eager_attention_forward)."""
    H, KV, dh = q.shape[1], k.shape[1], q.shape[-1]
    if KV != H:
        k, v = k.repeat_interleave(H // KV, dim=1), v.repeat_interleave(H // KV, dim=1)
    s = (q @ k.transpose(-1, -2)) * (scale if scale is not None else dh ** -0.5)
    Sq, Sk = s.shape[-2:]
    allow = torch.ones(Sq, Sk, dtype=torch.bool)
    if causal:
        allow = torch.tril(allow)
    allow = allow[None, None]
    if kmask is not None:
        allow = allow & kmask[:, None, None, :].bool()
    s = s.masked_fill(~allow, float("-inf"))
    return rnd(rnd(torch.softmax(s, dim=-1), emu) @ v, emu)


def im2col(pixels, P: int):
    """[B,C,H,W] -> [B, (H/P)(W/P), C*P*P] in the (c, py, px) order of a conv weight [d, C, P, P]."""
    B, C, H, W = pixels.shape
    gh, gw = H // P, W // P
    return pixels.reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * P * P)


# ----------------------------------------------------------------------------------------------
# a3  ViT featurizer (timm VisionTransformer semantics; evidence film_vit_wrapper.py:69-75,114-168;
#     modeling_prismatic.py:120-144, 196-237).  Pinned since round 4 by third-party stand-ins (transformers' SiglipVisionModel /
#     Dinov2WithRegistersModel: tests/golden/vit_*_tiny.npz); timm itself is absent.
# ----------------------------------------------------------------------------------------------
def vit_forward(pixels, p: Dict[str, torch.Tensor], cfg: Dict, emu=False) -> torch.Tensor:
    """pixels [B,3,H,W] -> patch features [B, Np, d] = output of block ``depth-2``, prefix tokens dropped,
    no final norm (get_intermediate_layers(n={depth-2}), norm=False).

    cfg: dict(d, depth, heads, mlp, patch, n_prefix (0 SigLIP / 5 DINOv2 cls+4reg), layerscale, eps, gelu_tanh)
    params: timm names (patch_embed.proj.weight [d,3,P,P], pos_embed [1,Np,d], cls_token, reg_token,
            blocks.N.{norm1,attn.qkv,attn.proj,ls1.scale_factor,norm2,mlp.fc1,mlp.fc2,ls2.scale_factor}).
    """
    d, heads, P = cfg["d"], cfg["heads"], cfg["patch"]
    B = pixels.shape[0]
    cols = im2col(pixels, P)   # patch embed = conv PxP stride P == GEMM over im2col'd patches
    x = linear(rnd(cols, emu), p["patch_embed.proj.weight"].reshape(d, -1), p["patch_embed.proj.bias"], emu)
    x = rnd(x + p["pos_embed"], emu)                               # _pos_embed (no_embed_class / no cls)
    if cfg.get("n_prefix", 0):
        pref = [p["cls_token"].expand(B, -1, -1)]
        if "reg_token" in p:
            pref.append(p["reg_token"].expand(B, -1, -1))
        x = torch.cat(pref + [x], dim=1)
    last = cfg["depth"] - 2                                        # modeling_prismatic.py:141-142
    for i in range(last + 1):                                      # blocks after `last` are dead work
        x = vit_block(x, p, f"blocks.{i}.", cfg, emu)
    return x[:, cfg.get("n_prefix", 0):]


def vit_block(x, p: Dict[str, torch.Tensor], pre: str, cfg: Dict, emu=False):
    """One timm Block: x + ls1(attn(norm1 x)); x + ls2(mlp(norm2 x))  (film_vit_wrapper.py:69-75; LayerScale modeling_prismatic.py:58-66)."""
    d, heads = cfg["d"], cfg["heads"]
    B, T, dh = x.shape[0], x.shape[1], d // heads
    h = layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], cfg["eps"], emu)
    qkv = linear(h, p[pre + "attn.qkv.weight"], p[pre + "attn.qkv.bias"], emu)
    q, k, v = qkv.reshape(B, T, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = attention(q, k, v, False, None, dh ** -0.5, emu).transpose(1, 2).reshape(B, T, d)
    a = linear(a, p[pre + "attn.proj.weight"], p[pre + "attn.proj.bias"], emu)
    if cfg.get("layerscale"):
        a = rnd(a * p[pre + "ls1.scale_factor"], emu)              # modeling_prismatic.py:58-66
    x = rnd(x + a, emu)
    h = layer_norm(x, p[pre + "norm2.weight"], p[pre + "norm2.bias"], cfg["eps"], emu)
    h = gelu(linear(h, p[pre + "mlp.fc1.weight"], p[pre + "mlp.fc1.bias"], emu), emu, cfg.get("gelu_tanh", False))
    h = linear(h, p[pre + "mlp.fc2.weight"], p[pre + "mlp.fc2.bias"], emu)
    if cfg.get("layerscale"):
        h = rnd(h * p[pre + "ls2.scale_factor"], emu)
    return rnd(x + h, emu)


# ----------------------------------------------------------------------------------------------
# a4  projector (modeling_prismatic.py:242-273).  Pinned by tests/golden/vla_*.npz (tools/make_golden_vla.py).
# ----------------------------------------------------------------------------------------------
def projector(x, p: Dict[str, torch.Tensor], fused: bool, emu=False):
    h = gelu(linear(x, p["fc1.weight"], p["fc1.bias"], emu), emu)
    h = linear(h, p["fc2.weight"], p["fc2.bias"], emu)
    if fused:
        h = linear(gelu(h, emu), p["fc3.weight"], p["fc3.bias"], emu)
    return h


# ----------------------------------------------------------------------------------------------
# a5  Qwen2 decoder stack (transformers Qwen2ForCausalLM; call site modeling_prismatic.py:644-655)
# ----------------------------------------------------------------------------------------------
def rms_norm(x, w, eps, emu=False):
    """Qwen2RMSNorm: w * bf16(x * rsqrt(mean(x^2)+eps))  (two rounding points in bf16)."""
    n = rnd(x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps), emu)
    return rnd(w * n, emu)


def rope_half_tables(S: int, dh: int, theta: float, emu=False):
    inv = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    f = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    e = torch.cat([f, f], dim=-1)
    return rnd(e.cos(), emu), rnd(e.sin(), emu)


def rope_half(x, cos, sin, emu=False):
    """HF rotate_half convention: pairs (i, i+dh/2). x [B,H,S,dh], cos/sin [S,dh]."""
    h = x.shape[-1] // 2
    rot = torch.cat([-x[..., h:], x[..., :h]], dim=-1)
    return rnd(rnd(x * cos, emu) + rnd(rot * sin, emu), emu)


def qwen2_forward(x, mask, p: Dict[str, torch.Tensor], cfg: Dict, emu=False) -> List[torch.Tensor]:
    """x [B,S,D] inputs_embeds, mask [B,S] bool key-padding mask -> hidden_states (n_layers+1 tensors):
    [0]=inputs_embeds, [i]=output of layer i (i<n), [n]=final-norm output (HF convention).

    cfg: dict(n_layers, heads, kv_heads, dh, eps, theta).  Params use HF names under ``layers.N.``.
    Attention: causal AND key-padding, softmax fp32, P rounded to bf16 before P@V (eager path).
    """
    S = x.shape[1]
    hs = [x]
    for i in range(cfg["n_layers"]):
        x = qwen2_layer(x, mask, p, f"layers.{i}.", cfg, emu)
        hs.append(x)
    hs[-1] = rms_norm(x, p["norm.weight"], cfg["eps"], emu)
    return hs


def qwen2_layer(x, mask, p: Dict[str, torch.Tensor], pre: str, cfg: Dict, emu=False):
    """One Qwen2DecoderLayer (transformers): x + o(attn(rope(q, k), v)) ; x + down(silu(gate) * up)."""
    B, S, D = x.shape
    H, KV, dh = cfg["heads"], cfg["kv_heads"], cfg["dh"]
    cos, sin = rope_half_tables(S, dh, cfg["theta"], emu)
    h = rms_norm(x, p[pre + "input_layernorm.weight"], cfg["eps"], emu)
    q, k, v = linear_group(h, [(p[pre + f"self_attn.{n}_proj.weight"], p[pre + f"self_attn.{n}_proj.bias"]) for n in "qkv"], emu)
    q = rope_half(q.reshape(B, S, H, dh).transpose(1, 2), cos, sin, emu)
    k = rope_half(k.reshape(B, S, KV, dh).transpose(1, 2), cos, sin, emu)
    v = v.reshape(B, S, KV, dh).transpose(1, 2)
    a = attention(q, k, v, True, mask, dh ** -0.5, emu).transpose(1, 2).reshape(B, S, H * dh)
    x = rnd(x + linear(a, p[pre + "self_attn.o_proj.weight"], None, emu), emu)
    h = rms_norm(x, p[pre + "post_attention_layernorm.weight"], cfg["eps"], emu)
    g, u = linear_group(h, [(p[pre + "mlp.gate_proj.weight"], None), (p[pre + "mlp.up_proj.weight"], None)], emu)
    m = rnd(rnd(g * torch.sigmoid(g), emu) * u, emu)
    return rnd(x + linear(m, p[pre + "mlp.down_proj.weight"], None, emu), emu)


# ----------------------------------------------------------------------------------------------
# a6  hidden-state regroup (vla-scripts/finetune.py:396-409)
# ----------------------------------------------------------------------------------------------
def regroup_hidden_states(hidden_states: List[torch.Tensor], labels, num_patches: int) -> torch.Tensor:
    """-> [B, n_states, num_patches + 64, D].  task = item[:, :num_patches] (tok0 + first num_patches-1
    patches: reference off-by-one kept); actions = item[:, num_patches:-1][mask(labels[:,1:])]."""
    gt = labels[:, 1:]
    m = current_action_mask(gt) | next_actions_mask(gt)            # finetune.py:351-353
    outs = []
    for item in hidden_states:
        B = item.shape[0]
        text = item[:, num_patches:-1]
        act = text[m].reshape(B, 1, NUM_TOKENS, -1)
        task = item[:, :num_patches].reshape(B, 1, num_patches, -1)
        outs.append(torch.cat([task, act], dim=2))
    return torch.cat(outs, dim=1)


# ----------------------------------------------------------------------------------------------
# a7  proprio projector (prismatic/models/projectors.py:19-24)
# ----------------------------------------------------------------------------------------------
def proprio_projector(proprio, p: Dict[str, torch.Tensor], emu=False):
    return linear(gelu(linear(rnd(proprio, emu), p["fc1.weight"], p["fc1.bias"], emu), emu),
                  p["fc2.weight"], p["fc2.bias"], emu)


# ----------------------------------------------------------------------------------------------
# a8/a9  action head (prismatic/models/action_heads.py)
# ----------------------------------------------------------------------------------------------
def head_rope_tables(T: int, dh: int, emu=False, base: float = 10000.0):
    """RotaryPositionEmbedding.forward (action_heads.py:150-164): cos/sin of cat([f, f]).
    emu: the tables as the reference's bf16 run builds them.  finetune.py:280-281 casts the whole head with
    ``.to(torch.bfloat16)``, which also casts the registered ``inv_freq`` BUFFER (:158): ``t = arange(seq_len, dtype=bf16)``
    (positions above 256 are not representable and collapse onto even numbers), ``freqs = einsum(t, inv_freq)`` is rounded
    to bf16 BEFORE cos / sin, and those round again.  Pinned by tests/golden/head_bf16_*.npz (reference run in bf16)."""
    inv = 1.0 / (base ** (torch.arange(0, dh, 2).float() / dh))
    if emu:
        inv_b = inv.to(torch.bfloat16)
        t = torch.arange(T, dtype=torch.bfloat16)
        f = torch.einsum("i,j->ij", t, inv_b)                      # bf16 product, rounded
        e = torch.cat([f, f], dim=-1)
        return e.cos().float(), e.sin().float()                    # bf16 cos/sin of the bf16 angle
    f = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    e = torch.cat([f, f], dim=-1)
    return e.cos(), e.sin()


def head_rope(x, cos, sin, emu=False):
    """apply_rope (action_heads.py:125-146): rotation pairs (2i, 2i+1) but cos/sin laid out as cat([f,f])
    (the reference's mixed convention, kept).  x [B,H,T,dh]."""
    x1, x2 = x[..., ::2], x[..., 1::2]
    rot = torch.stack((-x2, x1), dim=-1).reshape_as(x)
    return rnd(rnd(x * cos, emu) + rnd(rot * sin, emu), emu)


def _heads(t, B, L, H):
    return t.reshape(B, L, H, -1).transpose(1, 2)


def head_attention_core(q, segs, ratio_g, emu=False):
    """Scores over [self | second | third] key segments, tanh-gate on the THIRD (h_t) segment, softmax over all
    (action_heads.py:391-401 Pro; :262-275 original).  q [B,H,T,dh]; segs = [(k,v)]*3 -> [B,H,T,dh]."""
    dh = q.shape[-1]
    sc = [rnd(q @ k.transpose(-1, -2), emu) for k, _ in segs]
    sc[2] = rnd(sc[2] * rnd(ratio_g, emu), emu)
    s = rnd(torch.cat(sc, dim=-1) / math.sqrt(dh), emu)
    w = rnd(torch.softmax(s, dim=-1), emu)
    return rnd(w @ torch.cat([v for _, v in segs], dim=2), emu)


def head_block_pro(x, h_t, h_a, pp, p: Dict[str, torch.Tensor], pre: str, emu=False, H: int = 8, relu_mask=None):
    """MLPResNetBlock_Pro.forward (action_heads.py:337-410).
    relu_mask (tests only): evaluate the closing ReLU with THIS 0/1 pattern instead of the sign of the recomputed pre-activation -
    a single-block gradient check compares backward arithmetic at the SAME activation pattern as the run under test (a
    pre-activation within rounding of zero that falls on the other side is a forward difference, not a backward one)."""
    B, T, C = x.shape
    dh = C // H
    ratio_g = torch.tanh(p[pre + "gating_factor"])                 # :343-344
    h_ad = torch.cat([h_a, pp], dim=1)                             # :347
    Ka, Kt = h_ad.shape[1], h_t.shape[1]
    L = lambda n, t: linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"], emu)
    q = _heads(L("q_proj", x), B, T, H)
    ks, vs = _heads(L("k_self", x), B, T, H), _heads(L("v_self", x), B, T, H)
    ka, va = _heads(L("k_adapter", h_ad), B, Ka, H), _heads(L("v_adapter", h_ad), B, Ka, H)
    Ls = lambda n, t: linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"], emu, strided_input=B > 1)
    kt, vt = _heads(Ls("k_task", h_t), B, Kt, H), _heads(Ls("v_task", h_t), B, Kt, H)      # h_t: strided slice (see linear())
    cm, sm = head_rope_tables(T, dh, emu)                          # :383-388 positions restart per segment
    q, ks = head_rope(q, cm, sm, emu), head_rope(ks, cm, sm, emu)
    ca, sa = head_rope_tables(Ka, dh, emu)
    ka = head_rope(ka, ca, sa, emu)
    ct, st = head_rope_tables(Kt, dh, emu)
    kt = head_rope(kt, ct, st, emu)
    o = head_attention_core(q, [(ks, vs), (ka, va), (kt, vt)], ratio_g, emu)     # :391-401
    o = L("o_proj", o.transpose(1, 2).reshape(B, T, C))
    y = rnd(o + x, emu)                                            # :409 (no outer residual)
    y = layer_norm(y, p[pre + "ffn.0.weight"], p[pre + "ffn.0.bias"], 1e-5, emu)
    z = L("ffn.1", y)
    return rnd(torch.relu(z) if relu_mask is None else z * relu_mask, emu)


def head_block_orig(x, h_t, h_a, pp, p: Dict[str, torch.Tensor], pre: str, emu=False, H: int = 8):
    """MLPResNetBlock.forward (action_heads.py:218-283): shared k/v proj, no RoPE, tanh gate on the h_t segment,
    order [self, (h_a,p), h_t]."""
    B, T, C = x.shape
    dh = C // H
    ratio_g = torch.tanh(p[pre + "gating_factor"])
    h = torch.cat([h_a, pp], dim=1)
    L = lambda n, t: linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"], emu)
    q = _heads(L("q_proj", x), B, T, H)
    kx, vx = _heads(L("k_proj", x), B, T, H), _heads(L("v_proj", x), B, T, H)
    kh, vh = _heads(L("k_proj", h), B, h.shape[1], H), _heads(L("v_proj", h), B, h.shape[1], H)
    Ls = lambda n, t: linear(t, p[pre + n + ".weight"], p[pre + n + ".bias"], emu, strided_input=B > 1)
    kt, vt = _heads(Ls("k_proj", h_t), B, h_t.shape[1], H), _heads(Ls("v_proj", h_t), B, h_t.shape[1], H)   # h_t: strided slice
    o = head_attention_core(q, [(kx, vx), (kh, vh), (kt, vt)], ratio_g, emu)     # :262-275
    o = L("o_proj", o.transpose(1, 2).reshape(B, T, C))
    y = layer_norm(rnd(o + x, emu), p[pre + "ffn.0.weight"], p[pre + "ffn.0.bias"], 1e-5, emu)
    return rnd(torch.relu(L("ffn.1", y)), emu)


def head_predict_action(mlhs, proprio, head_p: Dict[str, torch.Tensor], proprio_p: Dict[str, torch.Tensor],
                        num_task_tokens: int, pro: bool = True, noise: Optional[torch.Tensor] = None,
                        emu=False, num_blocks: int = 24, taps: Optional[dict] = None) -> torch.Tensor:
    """L1RegressionActionHead.predict_action + MLPResNet.forward (action_heads.py:43-81, 111-121).

    mlhs [B, n_states, num_task_tokens+64, D]; ``noise`` [8, 7*D] is the Training-phase perturbation
    (action_heads.py:14-17, 69-72) injected explicitly; None == phase "Inference" (zeros input).
    head_p keys are the reference state-dict keys under ``model.``.
    """
    B, D = mlhs.shape[0], mlhs.shape[-1]
    pf = proprio_projector(proprio.reshape(B, -1), proprio_p, emu)[:, None, :]           # :53-55
    h_t_all, h_a_all = mlhs[:, :, :num_task_tokens], mlhs[:, :, num_task_tokens:]        # :57-58
    x = torch.zeros(B, NUM_ACTIONS_CHUNK, ACTION_DIM * D)                                 # :60-66
    if noise is not None:
        x = rnd(x + noise, emu)
    x = layer_norm(x, head_p["model.layer_norm1.weight"], head_p["model.layer_norm1.bias"], 1e-5, emu)
    x = rnd(torch.relu(linear(x, head_p["model.fc1.weight"], head_p["model.fc1.bias"], emu)), emu)
    blk = head_block_pro if pro else head_block_orig
    for i in range(num_blocks):                                                           # :117-118
        x = blk(x, h_t_all[:, i + 1], h_a_all[:, i + 1], pf, head_p, f"model.mlp_resnet_blocks.{i}.", emu)
        if taps is not None:
            taps[i] = x.detach()                                                              # block outputs (tests)
    x = layer_norm(x, head_p["model.layer_norm2.weight"], head_p["model.layer_norm2.bias"], 1e-5, emu)
    return linear(x, head_p["model.fc2.weight"], head_p["model.fc2.bias"], emu)


# ----------------------------------------------------------------------------------------------
# a10  loss + metrics (finetune.py:418-444)
# ----------------------------------------------------------------------------------------------
def l1_loss(pred, target, emu=False):
    return (pred - rnd(target, emu)).abs().mean()


def l1_metrics(pred, target):
    return dict(loss_value=(pred - target).abs().mean(),
                curr_action_l1_loss=(pred[:, 0] - target[:, 0]).abs().mean(),
                next_actions_l1_loss=(pred[:, 1:] - target[:, 1:]).abs().mean())


# ----------------------------------------------------------------------------------------------
# 8f-2  image resize of PrismaticImageProcessor.apply_transform (prismatic/extern/hf/processing_prismatic.py:128-145):
#       TVF.resize(PIL image, (224, 224), BICUBIC, antialias=True) == PIL.Image.resize(..., resample=BICUBIC).
#       The arithmetic lives in Pillow (third-party, pinned by the reference at pillow via torchvision; 12.2.0 installed here):
#       restated below from its published algorithm (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
#       ImagingResampleHorizontal/Vertical_8bpc) and pinned BIT-EXACTLY against PIL.Image.resize in tests/test_oracle_golden.py.
# ----------------------------------------------------------------------------------------------
def _bicubic_filter(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_coeffs(in_size: int, out_size: int):
    """-> (bounds int32 [out, 2] = (first source index, count), coefs int32 [out, ksize]): Pillow's 8-bit fixed-point bicubic
    taps (22 fractional bits) with antialiasing (filter support scaled by the downscale factor)."""
    import numpy as np
    PREC = 32 - 8 - 2
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coefs = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coefs[xx, x] = int(-0.5 + v * (1 << PREC)) if v < 0 else int(0.5 + v * (1 << PREC))
    return bounds, coefs


def resize_bicubic_u8(img, out_h: int, out_w: int):
    """img uint8 [H, W, C] (numpy) -> uint8 [out_h, out_w, C]: horizontal pass into an 8-bit intermediate, then vertical pass."""
    import numpy as np
    PREC = 32 - 8 - 2
    H, W, Cc = img.shape

    def one_pass(src, bounds, coefs, axis):
        n_out = bounds.shape[0]
        shape = list(src.shape)
        shape[axis] = n_out
        out = np.empty(shape, np.uint8)
        s64 = src.astype(np.int64)
        for o in range(n_out):
            lo, cnt = int(bounds[o, 0]), int(bounds[o, 1])
            k = coefs[o, :cnt].astype(np.int64)
            seg = s64[:, lo:lo + cnt] if axis == 1 else s64[lo:lo + cnt]
            acc = (1 << (PREC - 1)) + (np.tensordot(seg, k, axes=([1], [0])) if axis == 1 else np.tensordot(k, seg, axes=([0], [0])))
            val = np.clip(acc >> PREC, 0, 255).astype(np.uint8)
            if axis == 1:
                out[:, o] = val
            else:
                out[o] = val
        return out
    cur = img
    if W != out_w:
        cur = one_pass(cur, *pil_bicubic_coeffs(W, out_w), axis=1)
    if H != out_h:
        cur = one_pass(cur, *pil_bicubic_coeffs(H, out_h), axis=0)
    return cur


# ----------------------------------------------------------------------------------------------
# 8f-4  token cross-entropy of the native VLM path (prismatic/models/vlms/prismatic.py:411-422, 469-481 -> HF causal-LM loss)
# ----------------------------------------------------------------------------------------------
def token_ce(hidden_last, lm_head, labels, num_patches: int, emu=False):
    """hidden_last [B, S, D] = hidden_states[-1]; labels [B, L] (text positions); -> (loss, logits [B, S, V]).
    multimodal labels = [labels[:, :1] | -100 x num_patches | labels[:, 1:]]; HF shifts by one and averages over labels != -100,
    on the fp32 upcast of the (bf16) logits."""
    B = hidden_last.shape[0]
    logits = linear(hidden_last, lm_head, None, emu)
    mm = torch.cat([labels[:, :1], torch.full((B, num_patches), IGNORE_INDEX, dtype=labels.dtype), labels[:, 1:]], dim=1)
    lg, tg = logits[:, :-1].reshape(-1, logits.shape[-1]).float(), mm[:, 1:].reshape(-1)
    valid = tg != IGNORE_INDEX
    lse = torch.logsumexp(lg[valid], dim=-1)
    return (lse - lg[valid].gather(1, tg[valid][:, None])[:, 0]).mean(), logits


# ----------------------------------------------------------------------------------------------
# a11  LoRA linear (peft LoraConfig r, alpha=2r; finetune.py:832-844).  Pinned via W_eff = W + 2 B A (test_oracle_golden.py).
# ----------------------------------------------------------------------------------------------
def lora_linear(x, w, b, A, Bm, scale: float, emu=False):
    return rnd(linear(x, w, b, emu) + rnd(linear(linear(x, A, None, emu), Bm, None, emu) * scale, emu), emu)


# ----------------------------------------------------------------------------------------------
# a12  AdamW (torch.optim.AdamW defaults as used at finetune.py:910) + LR schedule (:917, 1061-1065)
# ----------------------------------------------------------------------------------------------
def adamw_step(p, g, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, emu=False):
    """One AdamW update; returns (p, m, v).  With ``emu`` every elementwise op rounds to bf16, which is what
    torch's (foreach) AdamW does on bf16 params/states: lerp_, mul_/addcmul_, sqrt/div/add, addcdiv_."""
    def fma(a, b, c):  # fp32 fused multiply-add (a*b exact in f64), as the vectorised ATen kernels contract it
        return (a.double() * b.double() + c.double()).float()
    f32 = lambda s: torch.tensor(s, dtype=torch.float32)
    p = rnd(p * f32(1.0 - lr * wd), emu)
    m = rnd(fma(f32(1.0 - beta1), g - m, m), emu)                  # exp_avg.lerp_(grad, 1-beta1)
    v = rnd(fma(f32(1.0 - beta2) * g, g, rnd(v * f32(beta2), emu)), emu)   # mul_(beta2).addcmul_(g, g, 1-beta2)
    bc1 = 1.0 - beta1 ** step
    bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
    denom = rnd(rnd(rnd(v.sqrt(), emu) / f32(bc2_sqrt), emu) + f32(eps), emu)
    p = rnd(fma(f32(-(lr / bc1)), m / denom, p), emu)              # addcdiv_(exp_avg, denom, -step_size)
    return p, m, v


def lr_at(step: int, base_lr: float, warmup_steps: float = 0.1, decay_at: int = 100000, gamma: float = 0.1):
    """Learning rate of optimizer step ``step`` (finetune.py:917, 1061-1065, 1078-1082).  With warmup_steps > 0 the warm-up
    block rewrites param_group['lr'] = base * (0.1 + 0.9 * min((step+1)/warmup, 1)) on every iteration BEFORE
    optimizer.step(), which also undoes MultiStepLR's decay from the previous scheduler.step(): the decay only exists with
    warmup_steps <= 0 (pinned by tests/test_host_api_cpu.py against a torch AdamW + MultiStepLR loop)."""
    if warmup_steps > 0:
        return base_lr * (0.1 + 0.9 * min((step + 1) / warmup_steps, 1.0))
    return base_lr * (gamma if step >= decay_at else 1.0)


def vision_features(px, vit_w: List[Dict[str, torch.Tensor]], cfg: Dict, emu=False):
    """PrismaticVisionBackbone.forward (modeling_prismatic.py:196-237): pixels [B, 3 * n_backbones * n_img, H, W] -> [B, Np * n_img,
    sum of widths].  Per image, channels [0, 3) go to the featurizer and [3, 6) to the fused featurizer; features concatenated
    [featurizer | fused] along the width, images along the patches."""
    n_img, nb = cfg["n_img"], len(cfg["vit"])
    feats = []
    for im in range(n_img):
        chans = px[:, im * 3 * nb:(im + 1) * 3 * nb]
        f = [vit_forward(chans[:, 3 * j:3 * j + 3], vit_w[j], cfg["vit"][j], emu) for j in range(nb)]
        feats.append(torch.cat(f, dim=2))
    return torch.cat(feats, dim=1)


# ----------------------------------------------------------------------------------------------
# Composite: the whole fine-tune forward of run_forward_pass (finetune.py:288-447) on the oracle pieces.
# ----------------------------------------------------------------------------------------------
def vla_forward(batch: Dict[str, torch.Tensor], W: Dict[str, Dict[str, torch.Tensor]], cfg: Dict, emu=False,
                noise: Optional[torch.Tensor] = None):
    """-> dict(pred [B,8,7], loss, hidden_states, mlhs).  ``W`` = dict(vit=[..one dict per backbone..],
    proj, llm, embed, action_queries, head, proprio); cfg = dict(vit=[...], fused, llm, n_img, pro)."""
    patches = projector(vision_features(batch["pixel_values"], W["vit"], cfg, emu), W["proj"], cfg["fused"], emu)
    mm, mm_mask = embed_splice(batch["input_ids"], batch["labels"], batch["attention_mask"],
                               W["embed"], W["action_queries"], patches)
    hs = qwen2_forward(mm, mm_mask, W["llm"], cfg["llm"], emu)
    npatch = patches.shape[1]
    mlhs = regroup_hidden_states(hs, batch["labels"], npatch)
    pred = head_predict_action(mlhs, batch["proprio"], W["head"], W["proprio"], npatch, cfg.get("pro", True),
                               noise, emu, cfg.get("num_blocks", 24))
    loss = l1_loss(pred, batch["actions"], emu)
    return dict(pred=pred, loss=loss, hidden_states=hs, mlhs=mlhs, patches=patches)


def prepare_predict_inputs(input_ids, attention_mask):
    """_prepare_input_for_action_prediction + _prepare_labels_for_action_prediction (modeling_prismatic.py:748-784) -> (ids, mask,
    labels): the prompt ids, 64 placeholder ids (1) and the stop id; the mask extended with ones; IGNORE_INDEX over the prompt,
    an action id over the placeholders, the stop id last."""
    B, L0 = input_ids.shape
    ids = torch.cat([input_ids, torch.ones(B, NUM_TOKENS, dtype=input_ids.dtype),
                     torch.full((B, 1), STOP_INDEX, dtype=input_ids.dtype)], dim=1)
    am = torch.cat([attention_mask.bool(), torch.ones(B, ids.shape[1] - L0, dtype=torch.bool)], dim=1)
    labels = torch.full_like(ids, IGNORE_INDEX)
    labels[:, L0:] = ACTION_TOKEN_BEGIN_IDX + 1
    labels[:, -1] = STOP_INDEX
    return ids, am, labels


def predict_action_batch1(input_ids, attention_mask, pixels, proprio, W, cfg: Dict, action_stats: Dict, emu=False):
    """OpenVLAForActionPrediction.predict_action with the L1 regression head, batch 1, phase Inference (modeling_prismatic.py:892-972):
    the batch of prepare_predict_inputs; the fine-tune forward on that batch; the
    returned hidden states are the last state's rows [NUM_PATCHES + NUM_PROMPT_TOKENS, +64) with NUM_PROMPT_TOKENS = prompt
    length - 1 (:855, :927); q01 / q99 un-normalisation where the stats' mask is set (:786-805).
    -> (un-normalised actions [chunk, action_dim] float64 ndarray, normalised [1, chunk, action_dim], hidden [1, 1, 64, D])."""
    import numpy as np
    L0 = input_ids.shape[1]
    assert input_ids.shape[0] == 1
    ids, am, labels = prepare_predict_inputs(input_ids, attention_mask)
    batch = dict(input_ids=ids, labels=labels, attention_mask=am, pixel_values=pixels, proprio=proprio.reshape(1, -1),
                 actions=torch.zeros(1, NUM_ACTIONS_CHUNK, ACTION_DIM))
    out = vla_forward(batch, W, cfg, emu)
    s0 = out["patches"].shape[1] + L0 - 1
    hid = out["hidden_states"][-1][:, s0:s0 + NUM_TOKENS].reshape(1, 1, NUM_TOKENS, -1)
    norm = out["pred"].detach().reshape(NUM_ACTIONS_CHUNK, ACTION_DIM).double().numpy()
    lo, hi = np.array(action_stats["q01"]), np.array(action_stats["q99"])
    mask = np.array(action_stats.get("mask", np.ones_like(lo, dtype=bool)))
    return np.where(mask, 0.5 * (norm + 1) * (hi - lo + 1e-8) + lo, norm), out["pred"], hid
