"""Native execution engine of the VLA-Adapter fine-tune hot path on MI355X.

Orchestrates the HIP kernels of ``libvla_native.so`` (through ``ops``) for the whole training step of
``vla-scripts/finetune.py:run_forward_pass`` + backward + AdamW (reference citations per method).  PyTorch is used
for device memory, streams and (in ``ddp.py``) RCCL only; every FLOP and every byte moved on the hot path is a
hand-written gfx950 kernel.  No autograd: backward is explicit, activations live in buffers allocated once and
reused every step (static shapes -> the step is hipGraph-capturable).

Layout decisions (MI355X-first, 288 GB HBM):
  * frozen weights are stored twice: [out,in] for the forward NT GEMM and pre-transposed [in,out] for dX, so every
    product is the K-contiguous NT form the MFMA kernel wants;
  * q/k/v and gate/up projections are fused ([1152,896] and a 16-row interleaved [9728,896]) so the SwiGLU product
    is formed in the GEMM epilogue;
  * ViT MLP width 4304 is zero-padded to 4352 (=34*128) so every GEMM dim is tile-aligned;
  * LLM hidden states for all layers live in one [n+2, B, S, D] buffer that the action head reads in place
    (no [B,25,576,896] regroup copy, finetune.py:396-409); the lm_head (modeling_prismatic.py:680-686, discarded by
    the reference) and the last ViT block (output unused) are never computed;
  * trainable parameters (action head, proprio projector, action queries) are views into ONE flat bf16 buffer
    grouped by kind across the 24 blocks -> batched GEMMs over layers, one AdamW launch, one gradient bucket.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from . import ops, schedule
from .ops import ACT_GELU, ACT_GELU_TANH, ACT_NONE, ACT_RELU, ACT_SWIGLU, BF16
from .schedule import Segment, capture_graph, chunks, turnaround_chunks

NUM_TOKENS = 64          # prismatic/vla/constants.py:15
IGNORE_INDEX = -100


def rup(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def copy_flat(dst: torch.Tensor, src: torch.Tensor):
    """dst <- src, contiguous tensors of one size, by the native copy (no ATen / runtime copy kernel on the step)."""
    n = src.numel()
    ops.copy2d(src, dst, 1, n, n, n)


# ------------------------------------------------------------------------------------------------ configs
@dataclass
class ViTCfg:
    d: int = 1152
    depth: int = 27
    heads: int = 16
    mlp: int = 4304
    patch: int = 14
    img: int = 224
    n_prefix: int = 0          # 0 SigLIP; 5 DINOv2 (cls + 4 reg)
    layerscale: bool = False
    eps: float = 1e-6
    gelu_tanh: bool = False

    @property
    def n_patches(self):
        return (self.img // self.patch) ** 2

    def as_oracle(self):
        return dict(d=self.d, depth=self.depth, heads=self.heads, mlp=self.mlp, patch=self.patch, n_prefix=self.n_prefix,
                    layerscale=self.layerscale, eps=self.eps, gelu_tanh=self.gelu_tanh)


SIGLIP_SO400M = ViTCfg(1152, 27, 16, 4304, 14, 224, 0, False)
DINOV2_L_REG4 = ViTCfg(1024, 24, 16, 4096, 14, 224, 5, True)


@dataclass
class LLMCfg:
    d: int = 896
    n_layers: int = 24
    heads: int = 14
    kv_heads: int = 2
    dh: int = 64
    inter: int = 4864
    eps: float = 1e-6
    theta: float = 1e6
    vocab: int = 151936

    def as_oracle(self):
        return dict(n_layers=self.n_layers, heads=self.heads, kv_heads=self.kv_heads, dh=self.dh, eps=self.eps, theta=self.theta)


@dataclass
class VLACfg:
    vit: List[ViTCfg] = field(default_factory=lambda: [SIGLIP_SO400M])
    llm: LLMCfg = field(default_factory=LLMCfg)
    n_img: int = 1
    num_blocks: int = 24       # MLPResNet(num_blocks=24), action_heads.py:35
    action_dim: int = 7
    chunk: int = 8
    proprio_dim: int = 8
    pro: bool = True

    @property
    def fused(self):
        return len(self.vit) == 2

    @property
    def n_patches(self):
        return self.vit[0].n_patches * self.n_img

    @property
    def vis_dim(self):
        return sum(v.d for v in self.vit)


def config2() -> VLACfg:
    """BASELINE.json configs[1]: SigLIP-224 + Qwen2.5-0.5B, adapter-only, 1 image."""
    return VLACfg()


def tiny_config() -> VLACfg:
    """BASELINE.json configs[0] 'prismatic-tiny': 2 useful ViT-T blocks + 2-layer 256-d LLM + adapter.
    The head reads hidden_states[i+1] for every block i (action_heads.py:117-118), so it can have at most
    n_layers blocks: 2 here (the reference hard-codes 24 and therefore needs >= 24 LLM layers)."""
    return VLACfg(vit=[ViTCfg(192, 3, 3, 768, 14, 56, 0, False)],
                  llm=LLMCfg(256, 2, 4, 2, 64, 512, 1e-6, 1e6, 1024), num_blocks=2)


def config5_backbone() -> VLACfg:
    """BASELINE.json configs[4]'s backbone at full size: DINOv2-L/14 (reg4) + SigLIP-so400m fused vision, Qwen2.5-1.5B language
    model (28 layers, d 1536, 12 heads of 128, 2 KV heads, MLP 8960), Pro action head on 24 of the 28 hidden states.  (The
    config's LoRA + fp8 training mode is a separate matter: bench.py runs this backbone adapter-only.)"""
    return VLACfg(vit=[DINOV2_L_REG4, SIGLIP_SO400M], llm=LLMCfg(1536, 28, 12, 2, 128, 8960, 1e-6, 1e6, 151936))


def qwen15b_geometry_config(n_layers: int = 2) -> VLACfg:
    """BASELINE.json configs[4]'s language-model GEOMETRY at plumbing depth: Qwen2.5-1.5B's layer (d 1536, 12 heads of 128,
    2 KV heads, MLP 8960) - head dim 128 (unfused RoPE, the 128-wide attention kernels) and a 7 x 1536-wide first head
    LayerNorm - under a tiny ViT, `n_layers` layers and as many head blocks."""
    return VLACfg(vit=[ViTCfg(192, 3, 3, 768, 14, 56, 0, False)],
                  llm=LLMCfg(1536, n_layers, 12, 2, 128, 8960, 1e-6, 1e6, 1024), num_blocks=n_layers)


def tiny_fused_config() -> VLACfg:
    """Plumbing-size version of the reference's default setup: DINOv2-like backbone (cls + 4 register tokens,
    LayerScale) + SigLIP-like backbone, fused 3-layer projector, two images per sample."""
    return VLACfg(vit=[ViTCfg(192, 3, 3, 768, 14, 56, 5, True), ViTCfg(128, 3, 2, 512, 14, 56, 0, False)], n_img=2,
                  llm=LLMCfg(256, 2, 4, 2, 64, 512, 1e-6, 1e6, 1024), num_blocks=2)


def tiny_twin_config() -> VLACfg:
    """Plumbing-size fused vision with two backbones of IDENTICAL geometry (d 128, 2 blocks, 2 heads, MLP 512, cls + 4 register
    tokens: equal token counts and widths, as DINOv2-L + CLIP-L), the first with LayerScale; two images per sample.  Every ViT
    contraction length is a multiple of 128, so LoRAFinetune(fp8=True) runs their base products on e4m3 operands.  The two
    backbones' per-shape scratch coincides: the configuration that exposes sharing between the trainer's stream kinds."""
    return VLACfg(vit=[ViTCfg(128, 2, 2, 512, 14, 56, 5, True), ViTCfg(128, 2, 2, 512, 14, 56, 5, False)], n_img=2,
                  llm=LLMCfg(256, 2, 4, 2, 64, 512, 1e-6, 1e6, 1024), num_blocks=2)


def dinosiglip_05b_config(n_img: int = 2) -> VLACfg:
    """The reference's documented recipe (README.md:254-274: ``--vlm_path .../prism-qwen25-extra-dinosiglip-224px-0_5b
    --num_images_in_input 2``): DINOv2-L/14 reg4 + SigLIP-so400m fused vision, 3-layer projector, Qwen2.5-0.5B."""
    return VLACfg(vit=[DINOV2_L_REG4, SIGLIP_SO400M], llm=LLMCfg(), n_img=n_img)


def _config5_two_images() -> VLACfg:
    c = config5_backbone()
    c.n_img = 2
    return c


# names accepted by ``finetune.py --backbone`` / ``bench.py --backbone`` (n_img follows --num_images_in_input where given)
NAMED_CONFIGS = {"config2": config2, "dinosiglip-0_5b": dinosiglip_05b_config, "config5": config5_backbone, "tiny": tiny_config,
                 "tiny_fused": tiny_fused_config, "tiny_twin": tiny_twin_config, "qwen15b-geometry": qwen15b_geometry_config}


# ------------------------------------------------------------------------------------------------ what a Linear does
class Linear:
    """What a Linear does on a frozen backbone: y = x W^T + b through the GEMM's fused epilogues, dx = dy W on the kept W^T.  The
    layer bodies (ViT.block, LLM.fwd_layer / bwd_layer) call ``_lin`` / ``_lin_bwd`` / ``_ln`` / ``_rms`` on the Linear they are
    given: this one, or a trainer (trainers.BackboneTrainer subclasses it), which adds the weight-gradient or LoRA work.

    fp8: ``Q`` maps a Linear's key ("llm.3.qkv", "vit0.5.fc1") to the OCP e4m3 codes and per-output-channel scales of its weight;
    such a Linear runs on the fp8 MFMA with its input quantised per row.  A norm whose output feeds one quantises inside the norm
    kernel (the row is still in registers: bit-identical to norm + quantise) and hands the codes over to the ``_lin`` that follows
    within the same segment call (``_xq``); anything else is quantised by one pass over it.  Scratch is per shape and per stream
    kind (``_lane``): one Linear serves each frozen backbone, and the trainers run two kinds at once on different streams."""

    trains_vectors = False       # (trainers: norm / bias / LayerScale gradients)
    taps = None                  # (trainers' test hook, see BackboneTrainer)
    keep_norm_out = False        # fp8: the bf16 norm output is written too (a trainer reads it again for a weight gradient)
    _lane = "M"

    def __init__(self, device):
        self.dev = device
        self.fp8 = False
        self.Q: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._qbuf, self._xq = {}, None

    def _q8_norm(self, x) -> bool:
        """Does the norm producing rows like x quantise them for the Linear it feeds?"""
        return self.fp8

    def _qscratch(self, rows: int, cols: int, slot: str):
        k = (rows, cols, slot, self._lane)
        b = self._qbuf.get(k)
        if b is None:
            b = self._qbuf[k] = (torch.empty(rows, cols, device=self.dev, dtype=torch.uint8), torch.empty(rows, device=self.dev, dtype=torch.float32))
        return b

    def _hand_over(self, y, q, s_):
        """Record the norm's quantised output for the next _lin; returns what stands for the norm's output (y, or the codes
        when the bf16 output is not written)."""
        h = q if y is None else y
        self._xq = ((h.data_ptr(), tuple(h.shape)), q, s_)
        return h

    def _quant(self, x, slot: str):
        """(codes, scales) of the rows of x: taken from the norm that just produced x, else one pass over x (vla_quant_fp8_rows)."""
        if self._xq is not None and self._xq[0] == (x.data_ptr(), tuple(x.shape)):
            hit, self._xq = self._xq, None               # (consumed: the scratch is overwritten by the next norm of this shape)
            return hit[1], hit[2]
        q, s_ = self._qscratch(x.shape[0], x.shape[1], slot)
        return ops.quant_fp8_rows(x, q, s_)

    def _ln(self, x, w, b, y, st, eps):
        """LayerNorm of the rows of x into y (None: a new tensor) with statistics st (None: not stored) -> its output."""
        if not self._q8_norm(x):
            return ops.layernorm_fwd(x, w, b, eps, out=y, stats=st)
        q, s_ = self._qscratch(x.shape[0], x.shape[1], "n")
        y = y if self.keep_norm_out else None
        ops.layernorm_fwd_q8(x, w, b, eps, q, s_, y=y, stats=st)
        return self._hand_over(y, q, s_)

    def _rms(self, x, w, out, rstd, eps):
        if not self._q8_norm(x):
            return ops.rmsnorm_fwd(x, w, eps, out=out, rstd=rstd)
        q, s_ = self._qscratch(x.shape[0], x.shape[1], "n")
        ops.rmsnorm_fwd_q8(x, w, eps, q, s_, rstd=rstd, y=out if self.keep_norm_out else None)
        return self._hand_over(out, q, s_)

    def _lin(self, key, x, W, bias=None, **kw):
        wq = self.Q.get(key)
        if wq is not None:
            xq, xs = self._quant(x, "f")
            return ops.gemm_nt(xq, wq[0], bias=bias, fp8=(xs, wq[1]), **kw)
        return ops.gemm_nt(x, W, bias=bias, **kw)

    def _lin_bwd(self, key, dy, x, WT, out=None, swiglu_gu=None, **kw):
        """dx = dy W (x: the layer's input, for a weight gradient); down_proj (swiglu_gu): dGU = swiglu'(GU) * (dy W_down) in the
        dX GEMM's epilogue (kw: its gu_group)."""
        if swiglu_gu is not None:
            return ops.gemm_swiglu_bwd(dy, WT, swiglu_gu, out=out, **kw)
        return ops.gemm_nt(dy, WT, out=out)


# ------------------------------------------------------------------------------------------------ frozen ViT
class ViT:
    """timm VisionTransformer forward up to block depth-2, no final norm (modeling_prismatic.py:120-144,196-237;
    block structure film_vit_wrapper.py:69-75).  Frozen: forward only (the trainers run the same blocks with Linears of their own)."""

    def __init__(self, cfg: ViTCfg, sd: Dict[str, torch.Tensor], device, j: int = 0):
        self.cfg, self.key = cfg, f"vit{j}."
        self.lin = Linear(device)
        d, P = cfg.d, cfg.patch
        g = lambda k: sd[k].to(device=device, dtype=BF16).contiguous()
        self.kpe = rup(3 * P * P, 64)
        wpe = torch.zeros(d, self.kpe, device=device, dtype=BF16)
        wpe[:, :3 * P * P] = g("patch_embed.proj.weight").reshape(d, -1)
        self.wpe, self.bpe = wpe, g("patch_embed.proj.bias")
        self.pos = g("pos_embed").reshape(-1, d)
        assert self.pos.shape[0] == cfg.n_patches, "pos_embed covers patches only (no_embed_class / no cls token)"
        self.prefix = None
        if cfg.n_prefix:
            toks = [g("cls_token").reshape(1, d)] + ([g("reg_token").reshape(-1, d)] if "reg_token" in sd else [])
            self.prefix = torch.cat(toks, 0)
            assert self.prefix.shape[0] == cfg.n_prefix
        self.mlp_pad = rup(cfg.mlp, 128)
        self.blocks = []
        for i in range(cfg.depth - 1):          # the last block's output is never used
            p = f"blocks.{i}."
            w1 = torch.zeros(self.mlp_pad, d, device=device, dtype=BF16)
            w1[:cfg.mlp] = g(p + "mlp.fc1.weight")
            b1 = torch.zeros(self.mlp_pad, device=device, dtype=BF16)
            b1[:cfg.mlp] = g(p + "mlp.fc1.bias")
            w2 = torch.zeros(d, self.mlp_pad, device=device, dtype=BF16)
            w2[:, :cfg.mlp] = g(p + "mlp.fc2.weight")
            wproj, bproj, b2 = g(p + "attn.proj.weight"), g(p + "attn.proj.bias"), g(p + "mlp.fc2.bias")
            blk = dict(n1w=g(p + "norm1.weight"), n1b=g(p + "norm1.bias"), wqkv=g(p + "attn.qkv.weight"),
                       bqkv=g(p + "attn.qkv.bias"), wproj=wproj, bproj=bproj, n2w=g(p + "norm2.weight"),
                       n2b=g(p + "norm2.bias"), w1=w1, b1=b1, w2=w2, b2=b2)
            if cfg.layerscale:                  # LayerScale (modeling_prismatic.py:58-66): the parameters themselves ...
                blk["ls1"], blk["ls2"] = g(p + "ls1.scale_factor"), g(p + "ls2.scale_factor")
            self.blocks.append(blk)
        # ... and, for the FROZEN forward (adapter-only fine-tune, inference), folded into the projections: y = ls * (W x + b) =
        # (ls W) x + ls b - one bf16 rounding point moves (scale applied to the weight instead of to the bf16 output), no extra
        # kernel on the step.  A trainer of the backbone (LoRA / full fine-tune) calls fold_layerscale(False): the blocks then
        # apply the scale as the reference does (vla_layerscale_fwd), on the weights that are being trained.
        self.ls_folded = False
        self.fold_layerscale(True)

    def fold_layerscale(self, on: bool):
        if not self.cfg.layerscale or on == self.ls_folded:
            self.ls_folded = on and self.cfg.layerscale
            return
        for b in self.blocks:
            if on:
                ls1, ls2 = b["ls1"].float(), b["ls2"].float()
                b["wproj_f"], b["bproj_f"] = (b["wproj"].float() * ls1[:, None]).to(BF16), (b["bproj"].float() * ls1).to(BF16)
                b["w2_f"], b["b2_f"] = (b["w2"].float() * ls2[:, None]).to(BF16), (b["b2"].float() * ls2).to(BF16)
            else:
                for k in ("wproj_f", "bproj_f", "w2_f", "b2_f"):
                    b.pop(k, None)
        self.ls_folded = on

    def enable_fp8(self):
        """BASELINE configs[4] 'fp8 MFMA weight path', first part: the frozen qkv and fc1 weights as OCP e4m3 with one scale per
        output channel; their inputs come out of LayerNorm already quantised per row (vla_layernorm_fwd_q8), the products run on
        the fp8 MFMA.  proj / fc2 (inputs produced by attention / a GEMM epilogue: no row statistics at hand) stay bf16."""
        for i, b in enumerate(self.blocks):
            self.lin.Q[f"{self.key}{i}.qkv"] = ops.quant_fp8_rows(b["wqkv"])
            self.lin.Q[f"{self.key}{i}.fc1"] = ops.quant_fp8_rows(b["w1"])
        self.lin.fp8 = True

    def forward(self, pixels: torch.Tensor, c0: int, out: Optional[torch.Tensor] = None, lin: Optional[Linear] = None, st=None):
        """pixels [Bv, C, H, W] (channels c0..c0+2 used) -> the last block's output [Bv * T, d] (prefix tokens included).
        out: the frozen last block writes its fc2 product straight into it (no prefix tokens: out is then the [Bv * Np, d] patch
        features).  lin / st: a trainer and its per-block keeps (trainers.BackboneTrainer.V[j])."""
        cfg = self.cfg
        lin = self.lin if lin is None else lin
        Bv, Np, d, T = pixels.shape[0], cfg.n_patches, cfg.d, cfg.n_patches + cfg.n_prefix
        cols = ops.im2col_patch(pixels, c0, cfg.patch, self.kpe)
        x = st["X"][0] if st is not None else torch.empty(Bv * T, d, device=pixels.device, dtype=BF16)
        if cfg.n_prefix:
            pe = ops.gemm_nt(cols, self.wpe, bias=self.bpe, residual=self.pos, res_mod=Np, out=st["pe"] if st is not None else None)
            x3 = x.view(Bv, T, d)
            ops.copy_rows3d(pe, x3[0, cfg.n_prefix:], Bv, Np, d, Np * d, d, T * d, d)
            ops.copy_rows3d(self.prefix, x3, Bv, cfg.n_prefix, d, 0, d, T * d, d)     # cls + register tokens, broadcast over the batch
        else:
            ops.gemm_nt(cols, self.wpe, bias=self.bpe, residual=self.pos, res_mod=Np, out=x)
        if st is not None:
            st["cols"] = cols                      # (the patch-embedding weight gradient reads it)
        nb = len(self.blocks)
        for i in range(nb):
            if st is not None:
                x = self.block(i, x, lin, st, st["X"][i + 1])
            else:                                  # frozen: the residual stream is updated in place
                x = self.block(i, x, lin, None, out if i == nb - 1 and out is not None else x)
        return x

    def block(self, i: int, x: torch.Tensor, lin: Linear, st, x_out: torch.Tensor) -> torch.Tensor:
        """Block i: x [Bv * T, d] -> x_out.  st: a trainer's per-block keeps (every activation its backward reads; the fc1
        pre-activation apart from the GELU), None on the frozen path (temporaries; GELU in the fc1 epilogue)."""
        cfg, b, k = self.cfg, self.blocks[i], f"{self.key}{i}."
        d, T = cfg.d, cfg.n_patches + cfg.n_prefix
        Bv = x.shape[0] // T
        keep = lambda name: st[name][i] if st is not None and name in st else None
        sfx = "_f" if self.ls_folded else ""       # (folded LayerScale: the scaled projections)
        # x_mid = x + ls1 * proj(attn(qkv(LN1(x))))
        h = lin._ln(x, b["n1w"], b["n1b"], keep("H1"), keep("S1"), cfg.eps)
        qkv = lin._lin(k + "qkv", h, b["wqkv"], b["bqkv"], out=keep("QKV")).view(Bv, T, 3 * d)
        a = ops.attn_fwd(qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:], cfg.heads, cfg.heads, d // cfg.heads, False,
                         out=st["A"][i].view(Bv, T, d) if st is not None else None, lse=keep("LSE")).view(Bv * T, d)
        xm = x if st is None else st["Xm"][i]
        self._residual(lin, k + "proj", a, b["wproj" + sfx], b["bproj" + sfx], b.get("ls1"), x, xm, keep("PA"))
        # x_out = x_mid + ls2 * fc2(gelu(fc1(LN2(x_mid))))
        h = lin._ln(xm, b["n2w"], b["n2b"], keep("H2"), keep("S2"), cfg.eps)
        if st is None:
            m = lin._lin(k + "fc1", h, b["w1"], b["b1"], act=ACT_GELU_TANH if cfg.gelu_tanh else ACT_GELU)
        else:
            m = ops.gelu_fwd(lin._lin(k + "fc1", h, b["w1"], b["b1"], out=st["Mpre"][i]), out=st["Mact"][i])
        self._residual(lin, k + "fc2", m, b["w2" + sfx], b["b2" + sfx], b.get("ls2"), xm, x_out, keep("PM"))
        return x_out

    def _residual(self, lin, key, a, w, bias, ls, x, out, pre):
        """out = x + ls * (a W^T + bias): LayerScale applied to the bf16 product as the reference does (pre: a trainer's slot
        for the unscaled product), or - folded / none - the residual added in the GEMM's epilogue."""
        if ls is not None and not self.ls_folded:
            ops.layerscale_fwd(lin._lin(key, a, w, bias, out=pre), ls, x, out=out)
        else:
            lin._lin(key, a, w, bias, out=out, residual=x)


# ------------------------------------------------------------------------------------------------ frozen LLM
class _BufferSets:
    """Base of the classes that work on one set of activation buffers per shape (LLM, Head).  THE rule: a captured
    graph holds the addresses of the set it was captured on, so whoever keeps a graph keeps that set (buffer_set() after the capture) and
    binds it (bind_buffer_set()) before every replay: the tensors stay allocated, and the attributes the host reads afterwards (llm.HS,
    ...) are the replayed shape's.  A set is the dict ``build_buffer_set`` declares: its keys are the attribute names.  What a forward
    records about a set's contents (``_FWD_FIELDS``, declared beside the fwd_begin that sets them) is taken and bound with it."""
    _bound = _buf_key = None             # the set whose members are this object's attributes, and its key

    def _alloc(self, *key):
        if self._buf_key != key:
            self.bind_buffer_set(self.build_buffer_set(*key))

    def buffer_set(self) -> Optional[dict]:  # the bound set (None: nothing is bound) with the per-forward fields as they stand now
        if self._bound is not None:
            self._bound = dict(self._bound, **{k: getattr(self, k) for k in self._FWD_FIELDS if hasattr(self, k)})
        return self._bound

    def bind_buffer_set(self, bufs: dict):
        if bufs is not self._bound:          # (an identity check when it is the bound one)
            self.__dict__.update(bufs)
            self._bound = bufs

    def unbind(self):                        # nothing is bound: the next _alloc builds a fresh set (holders of the old one keep it alive)
        self._bound = self._buf_key = None


class LLM(_BufferSets):
    """Qwen2 decoder stack (transformers Qwen2ForCausalLM; reference call site modeling_prismatic.py:644-655),
    forward with hidden-state taps and explicit dX backward (weights frozen: adapter-only fine-tune).  The trainers run the
    same layer bodies with themselves as the Linear and per-layer slots for what their gradient work reads (keep_per_layer)."""

    def __init__(self, cfg: LLMCfg, sd: Dict[str, torch.Tensor], device):
        self.cfg, self.device = cfg, device
        self.lin = Linear(device)
        D, H, KV, dh, I = cfg.d, cfg.heads, cfg.kv_heads, cfg.dh, cfg.inter
        assert D % 64 == 0 and I % 64 == 0 and (H + 2 * KV) * dh % 64 == 0 and I % 16 == 0
        g = lambda k: sd[k].to(device=device, dtype=BF16).contiguous()
        self.layers = []
        for i in range(cfg.n_layers):
            p = f"layers.{i}."
            wqkv = torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")], 0)
            bqkv = torch.cat([g(p + "self_attn.q_proj.bias"), g(p + "self_attn.k_proj.bias"), g(p + "self_attn.v_proj.bias")], 0)
            wg, wu = g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")
            wgu = torch.stack([wg.view(I // 16, 16, D), wu.view(I // 16, 16, D)], 1).reshape(2 * I, D).contiguous()
            wo, wd = g(p + "self_attn.o_proj.weight"), g(p + "mlp.down_proj.weight")
            self.layers.append(dict(n1=g(p + "input_layernorm.weight"), n2=g(p + "post_attention_layernorm.weight"),
                                    wqkv=wqkv.contiguous(), bqkv=bqkv.contiguous(), wo=wo, wgu=wgu, wd=wd,
                                    wqkvT=wqkv.t().contiguous(), woT=wo.t().contiguous(), wguT=wgu.t().contiguous(),
                                    wdT=wd.t().contiguous()))
        self.norm = g("norm.weight")
        self.embed = g("embed_tokens.weight")
        self.gu_row0 = 0
        self.per_layer, self.norm_grads = False, False
        self._flin = self._blin = self.lin

    def keep_per_layer(self, norm_grads: bool):
        """Training of the layers: the norm / SwiGLU outputs of every layer (N1, N2, Hs) and the dY of every Linear (G_res, G_d1,
        G_gu, G_qkv; norm_grads: of the two RMSNorms too, G_n1 / G_n2) in slots of their own - the gradient stream reads them any
        time after the dX chain has moved on (3.4 GB at batch 16)."""
        self.per_layer, self.norm_grads = True, norm_grads
        self.unbind()

    def build_buffer_set(self, B: int, S: int) -> dict:
        c, dev = self.cfg, self.device
        n, M, D = c.n_layers, B * S, c.d
        W = (c.heads + 2 * c.kv_heads) * c.dh
        e = lambda *s, dt=BF16: torch.empty(*s, device=dev, dtype=dt)
        # slots 0..n-1: residual stream entering layer i (slot 0 = inputs_embeds); slot n = FINAL-NORM output
        # (= hidden_states[n] of the HF convention); slot n+1 = raw output of the last layer.
        b = dict(HS=e(n + 2, B, S, D), X1=e(n, M, D), QKV=e(n, M, W), AO=e(n, M, c.heads * c.dh), GU=e(n, M, 2 * c.inter),
                 LSE=e(n, B, c.heads, S, dt=torch.float32), R1=e(n, M, dt=torch.float32), R2=e(n, M, dt=torch.float32), RF=e(M, dt=torch.float32),
                 nbuf=e(M, D), hbuf=e(M, c.inter), d_a=e(M, D), d_b=e(M, D), d_gu=e(M, 2 * c.inter), d_qkv=e(M, W), d_n=e(M, D))
        if self.per_layer:
            b.update(N1=e(n, M, D), N2=e(n, M, D), Hs=e(n, M, c.inter),
                     G_res=e(n, M, D), G_d1=e(n, M, D), G_gu=e(n, M, 2 * c.inter), G_qkv=e(n, M, W), d_last=e(M, D))
            if self.norm_grads:
                b.update(G_n1=e(n, M, D), G_n2=e(n, M, D))
        b["cos"], b["sin"] = ops.rope_half_tables(S, c.dh, c.theta, dev)
        return dict(b, _buf_key=(B, S))

    def out_slot(self, i: int) -> int:
        """HS slot holding the output of layer i (0-based)."""
        n = self.cfg.n_layers
        return i + 1 if i < n - 1 else n + 1

    def forward(self, B: int, S: int, kmask_u8: torch.Tensor, keep_from_row: int = 0, n_run: Optional[int] = None):
        """HS[0] must already hold inputs_embeds [B,S,D].  Fills HS[1..n] (HF hidden_states semantics).  n_run < n_layers: only the
        first n_run layers (hidden_states[1..n_run]: all the action head reads when it has fewer blocks than the LLM has layers)."""
        self.fwd_begin(B, S, kmask_u8, keep_from_row)
        self.fwd_layers(0, self.cfg.n_layers if n_run is None else n_run)

    def fwd_layers(self, lo: int, hi: int):
        """Layers lo .. hi - 1, and behind the top layer the final norm."""
        for i in range(lo, hi):
            self.fwd_layer(i)
        if hi == self.cfg.n_layers:
            self.fwd_final()

    _FWD_FIELDS = ("kmask", "B", "S", "gu_row0", "_flin")      # what fwd_begin records about the bound set's contents

    def fwd_begin(self, B: int, S: int, kmask_u8: torch.Tensor, keep_from_row: int = 0, lin: Optional[Linear] = None):
        """keep_from_row: the backward of this forward will only visit the rows >= keep_from_row of every sequence
        (LLM.backward row0 >= keep_from_row); backward-only tensors skip the rows below it.  lin: the Linear the layers of this
        forward run with (default: the frozen one)."""
        self.kmask, self.B, self.S = kmask_u8, B, S
        self.gu_row0 = keep_from_row
        self._flin = self.lin if lin is None else lin

    def _keeps(self, i: int):
        """(RMSNorm 1 output, RMSNorm 2 output, SwiGLU output) of layer i: per-layer slots, else shared scratch."""
        return (self.N1[i], self.N2[i], self.Hs[i]) if self.per_layer else (self.nbuf, self.nbuf, self.hbuf)

    def _attn_views(self, t3):
        c = self.cfg
        a, b = c.heads * c.dh, (c.heads + c.kv_heads) * c.dh
        return t3[:, :, :a], t3[:, :, a:b], t3[:, :, b:]

    def _layer(self, i: int, lin: Linear, x, x1, y, n1, n2, h, gu, r1, r2, attend, c_live=None):
        """The ONE statement of decoder layer i, rows x -> y: which weights, norms and GEMM epilogues it runs.  ``attend(n1)`` is the
        part that differs between the full-sequence forward (fwd_layer) and the cached single-token step (decode_step): the q|k|v
        projection with its RoPE and the attention, returning the rows that enter o_proj."""
        c, L, k = self.cfg, self.layers[i], f"llm.{i}."
        # (RMSNorm folded into the neighbouring GEMMs - 47 launches fewer, built and measured SLOWER in round 3 - left the tree in
        #  round 4: DESIGN section 4, tools/diag/gemm256_pruned_paths.patch)
        n1 = lin._rms(x, L["n1"], n1, r1, c.eps)
        ao = attend(n1)
        lin._lin(k + "o", ao, L["wo"], None, out=x1, residual=x)
        n2 = lin._rms(x1, L["n2"], n2, r2, c.eps)
        # the pre-activations are kept for the backward only: rows below the live window are never read again
        lin._lin(k + "gu", n2, L["wgu"], None, act=ACT_SWIGLU, out=gu, out2=h, c_live=c_live)
        lin._lin(k + "down", h, L["wd"], None, out=y, residual=x1)

    def fwd_layer(self, i: int):
        """Layer i over the whole batch."""
        c, B, S, lin = self.cfg, self.B, self.S, self._flin
        D, H, KV, dh = c.d, c.heads, c.kv_heads, c.dh
        L, k = self.layers[i], f"llm.{i}."
        qkv = self.QKV[i]
        n1, n2, h = self._keeps(i)

        def attend(n1):
            if dh in (64, 128):   # RoPE fused into the projection's epilogue (head dim 128: the 128-row kernel's column map, round 4)
                lin._lin(k + "qkv", n1, L["wqkv"], L["bqkv"], out=qkv, rope=(1, self.cos, self.sin, S, dh, (H + KV) * dh))
            else:
                lin._lin(k + "qkv", n1, L["wqkv"], L["bqkv"], out=qkv)
                ops.rope_half_(qkv[:, :H * dh], self.cos, self.sin, S, H, dh)
                ops.rope_half_(qkv[:, H * dh:(H + KV) * dh], self.cos, self.sin, S, KV, dh)
            ops.attn_fwd(*self._attn_views(qkv.view(B, S, -1)), H, KV, dh, True, self.kmask, out=self.AO[i].view(B, S, -1), lse=self.LSE[i])
            return self.AO[i]

        self._layer(i, lin, self.HS[i].view(-1, D), self.X1[i], self.HS[self.out_slot(i)].view(-1, D), n1, n2, h, self.GU[i], self.R1[i],
                    self.R2[i], attend, c_live=(S, self.gu_row0) if self.gu_row0 else None)

    # ---- greedy decoding with a key/value cache (VLAEngine.generate; include/vla_decode.h) ------------------------------------------
    def decode_alloc(self, B: int, S: int, T: int, sample: bool = False) -> dict:
        """Everything T cached single-token steps behind a prefill of S rows own: the cache K / V [n, B, S_cap, KV dh] with
        S_cap = S + T, the RoPE tables at that capacity (the values of a position do not depend on the table's length), the M = B
        activations of a step, the per-row positions, the device step counter and the tokens.  sample: also what the sampler of
        include/vla_sample.h works on - the step's logits bf16 [B, V], the log-probabilities f32 [B, T], the parameter block and the
        stream id of every row (row b draws from stream b until the caller says otherwise)."""
        c, dev = self.cfg, self.device
        n, D, kvw = c.n_layers, c.d, c.kv_heads * c.dh
        W = getattr(self, "lm_head", None)
        W = self.embed if W is None else W
        e = lambda *s, dt=BF16: torch.empty(*s, device=dev, dtype=dt)
        cos, sin = ops.rope_half_tables(S + T, c.dh, c.theta, dev)
        st = dict(B=B, S=S, T=T, S_cap=S + T, W=W, cos=cos, sin=sin, K=e(n, B, S + T, kvw), V=e(n, B, S + T, kvw),
                  X=e(n + 1, B, D), X1=e(B, D), NB=e(B, D), NF=e(B, D), QKV=e(B, (c.heads + 2 * c.kv_heads) * c.dh), AO=e(B, c.heads * c.dh),
                  GU=e(B, 2 * c.inter), H=e(B, c.inter), R=e(3, rup(B, 4), dt=torch.float32)[:, :B], XG=e(B, D),
                  pos=torch.zeros(B, device=dev, dtype=torch.int32), step=torch.zeros(1, device=dev, dtype=torch.int32),
                  ids=e(B, dt=torch.int64), out_ids=torch.zeros(B, T, device=dev, dtype=torch.int64), ws=ops.decode_argmax_workspace(B, W.shape[0], dev))
        if sample:
            st.update(logits=e(B, W.shape[0]), logprobs=torch.zeros(B, T, device=dev, dtype=torch.float32),
                      sparams=ops.sample_params(greedy=True).to(dev), streams=torch.arange(B, device=dev, dtype=torch.int64))
        return st

    def _decode_choose(self, st: dict, x: torch.Tensor, logits_out, pos_from=None):
        """The last launches of a decoding step: the greedy lm_head argmax with its advance - or, on a state with a sampler
        (decode_alloc(sample=True)), the lm_head pass storing the logits, then vla_sample_tokens with the advance."""
        advance = (st["out_ids"], st["step"], st["pos"], self.embed, st["X"][0])
        if "sparams" not in st:
            ops.decode_lm_head_argmax(x, st["W"], st["ws"], st["ids"], logits_out, advance=advance, pos_from=pos_from)
            return
        ops.decode_lm_head_argmax(x, st["W"], st["ws"], st["ids"], st["logits"])
        ops.sample_tokens(st["logits"], st["sparams"], st["step"], st["ids"], st["streams"], st["logprobs"], advance=advance, pos_from=pos_from)
        if logits_out is not None:
            logits_out.copy_(st["logits"])                       # (eager return_logits: the logits the sampler saw)

    def cache_fill(self, st: dict):
        """The rotated k and the v of every prefill row, from QKV[i] into rows 0 .. S - 1 of the cache (a strided copy per layer and
        operand; the rows behind a sample's prompt hold its padding and are overwritten one per step before they are read)."""
        c, B, S = self.cfg, st["B"], st["S"]
        W, kvw, q = (c.heads + 2 * c.kv_heads) * c.dh, c.kv_heads * c.dh, c.heads * c.dh
        for i in range(c.n_layers):
            for dst, col in ((st["K"], q), (st["V"], q + kvw)):
                ops.copy_rows3d(self.QKV[i][:, col:], dst[i], B, S, kvw, S * W, W, st["S_cap"] * kvw, kvw)

    def decode_first(self, st: dict, last_row: torch.Tensor, pos0: torch.Tensor, logits_out=None):
        """Behind the prefill: the final-norm rows of every sample's last prompt id -> the first token, the embedding of it as the
        first step's input, pos = pos0 + 1, step = 1."""
        n, D = self.cfg.n_layers, self.cfg.d
        ops.gather_rows(self.HS[n].view(-1, D), last_row, st["XG"])
        self._decode_choose(st, st["XG"], logits_out, pos_from=pos0)

    def decode_step(self, st: dict, logits_out=None):
        """One cached single-token step for all B rows: the layers of _layer at M = B with the cache attention, the final norm, the
        lm_head argmax and the advance.  Nothing here depends on the host knowing a position or the step index."""
        c, lin = self.cfg, self.lin
        H, KV, dh = c.heads, c.kv_heads, c.dh
        for i in range(c.n_layers):
            L, k = self.layers[i], f"llm.{i}."

            def attend(n1):
                lin._lin(k + "qkv", n1, L["wqkv"], L["bqkv"], out=st["QKV"])
                ops.decode_rope_append_(st["QKV"], st["cos"], st["sin"], st["pos"], st["K"][i], st["V"][i], H, KV, dh)
                return ops.decode_attn(st["QKV"][:, :H * dh], st["K"][i], st["V"][i], st["pos"], H, KV, dh, out=st["AO"])

            self._layer(i, lin, st["X"][i], st["X1"], st["X"][i + 1], st["NB"], st["NB"], st["H"], st["GU"], st["R"][0], st["R"][1], attend)
        ops.rmsnorm_fwd(st["X"][c.n_layers], self.norm, c.eps, out=st["NF"], rstd=st["R"][2])
        self._decode_choose(st, st["NF"], logits_out)

    def fwd_final(self):
        """hidden_states[n] = final RMSNorm of the last layer's output (HF convention)."""
        n, D = self.cfg.n_layers, self.cfg.d
        ops.rmsnorm_fwd(self.HS[n + 1].view(-1, D), self.norm, self.cfg.eps, out=self.HS[n].view(-1, D), rstd=self.RF)

    def enable_fp8(self):
        """fp8 weight path (see ViT.enable_fp8): the frozen q|k|v and gate/up weights in e4m3, their inputs quantised inside
        RMSNorm (vla_rmsnorm_fwd_q8); o-proj / down stay bf16.  Forward only: the dX products keep the bf16 W^T."""
        for i, L in enumerate(self.layers):
            self.lin.Q[f"llm.{i}.qkv"] = ops.quant_fp8_rows(L["wqkv"])
            self.lin.Q[f"llm.{i}.gu"] = ops.quant_fp8_rows(L["wgu"])
        self.lin.fp8 = True

    # ---- backward: dX (frozen weights: adapter-only), restricted to the LIVE rows ------------------------------------------
    # The only trainable tensor upstream of the LLM is `action_queries`, spliced in at sequence positions >= r_first
    # (after tok0 + patches + prompt).  Causal attention makes row i of every hidden state a function of the input rows
    # <= i only, so d loss / d inputs_embeds[rows >= r0] depends on d loss / d hidden[rows >= r0] alone, for any
    # r0 <= r_first: the gradient rows < r0 flow exclusively into frozen inputs (patch / prompt embeddings) and are dead.
    # torch.autograd (the reference) computes them anyway because it prunes by tensor, not by row.  `row0` selects the
    # window; every op below works on compact [B * (S - row0), .] gradients and reads the forward's tensors through
    # row-window addressing.  row0 = 0 is the plain full-sequence backward (needed as soon as ViT / projector / LoRA
    # weights train).  The surviving gradients are the same numbers either way (tests/test_engine_gpu.py).
    def backward(self, dHS: torch.Tensor, B: int, S: int, row0: int = 0, n_run: Optional[int] = None) -> torch.Tensor:
        """dHS [n+1, B, S - row0, D]: gradient w.r.t. rows >= row0 of hidden_states[i] (i = 0..n, HF convention; [0]
        unused).  Returns the gradient w.r.t. rows >= row0 of inputs_embeds, [B, S - row0, D] (frozen weights: no dW).
        n_run < n_layers: the layers above n_run never reached the loss (forward(n_run=)): the chain starts at layer n_run - 1."""
        n_run = self.cfg.n_layers if n_run is None else n_run
        self.bwd_begin(dHS, row0, n_run)
        for i in range(n_run - 1, -1, -1):
            self.bwd_layer(i, dHS)
        return self.bwd_result()

    def bwd_begin(self, dHS: torch.Tensor, row0: Optional[int] = 0, n_run: Optional[int] = None, lin: Optional[Linear] = None):
        """Gradient w.r.t. the output of the top layer that reached the loss.  row0: the live-row window (any row0 runs the
        windowed kernels); None: the trainers' whole-sequence backward without a window.  lin: as in fwd_begin."""
        n, S, D = self.cfg.n_layers, self.S, self.cfg.d
        self._n_run = n if n_run is None else n_run
        self._blin = lin = self.lin if lin is None else lin
        if row0 is None:
            self.r0, self.Rl, self._win = 0, S, None
        else:
            assert 0 <= row0 < S and row0 % 32 == 0, "live-row window must start on a multiple of 32"
            assert row0 >= self.gu_row0, "the forward dropped backward-only rows this window needs"
            self.r0, self.Rl = row0, S - row0
            self._win = (self.Rl, S, row0)                    # (rows per sequence, sequence rows, first row)
        Mr = self.B * self.Rl
        assert tuple(dHS.shape[1:]) == (self.B, self.Rl, D)
        d = (self.G_res[self._n_run - 1] if self.per_layer else self.d_a)[:Mr]
        if self._n_run == n:
            self._d = ops.rmsnorm_bwd(dHS[n].view(Mr, D), self.HS[n + 1].view(-1, D), self.norm, self.RF, out=d, x_rows=self._win)
            if lin.trains_vectors:
                ops.rmsnorm_dw(dHS[n].view(Mr, D), self.HS[n + 1].view(-1, D), self.RF, lin.A("llm.norm"))
        else:           # hidden_states[n_run] is a raw layer output (no final norm behind it): its gradient is the head's alone
            self._d = ops.copy2d(dHS[self._n_run].view(Mr, D), d, Mr, D, D, D)

    def bwd_layer(self, i: int, dHS: torch.Tensor):
        """dX through layer i: self._d (gradient w.r.t. its output, without the head's share) -> w.r.t. its input.  Per-layer
        slots: every dY in the layer's own slot and everything that only feeds a parameter gradient handed to the trainer
        (_lin_bwd, _defer); scratch: one buffer per role, reused by every layer."""
        c, B, S, r0, R, lin = self.cfg, self.B, self.S, self.r0, self.Rl, self._blin
        M, D, H, KV, dh, I = B * S, c.d, c.heads, c.kv_heads, c.dh, c.inter
        Mr, tv, win = B * R, lin.trains_vectors, self._win
        L, k, d = self.layers[i], f"llm.{i}.", self._d
        _, n2, h = self._keeps(i)
        if self.per_layer:
            d1_out, d_out = self.G_d1[i], (self.G_res[i - 1] if i > 0 else self.d_last)[:Mr]
            d_gu, d_qkv = self.G_gu[i][:Mr], self.G_qkv[i][:Mr]
        else:
            d1_out, d_out, d_gu, d_qkv = self.d_b[:Mr], d, self.d_gu[:Mr], self.d_qkv[:Mr]
        if i < self._n_run - 1:                         # head contribution to the output of layer i (the top layer's came in bwd_begin)
            ops.add_(d, dHS[i + 1].view(Mr, D))
        tap = lin.taps.get(("llm", i)) if lin.taps is not None else None
        if tap is not None:
            tap["d_out"] = d.clone()
        # the first sequence's window of GU; the others by row-group addressing
        d_gu = lin._lin_bwd(k + "down", d, h, L["wdT"], out=d_gu, swiglu_gu=self.GU[i][r0:], **({"gu_group": (R, S * 2 * I)} if win else {}))
        d_n = lin._lin_bwd(k + "gu", d_gu, n2, L["wguT"], out=self.G_n2[i] if tv else self.d_n[:Mr])
        if tv:
            lin._defer(lambda dy=d_n, x=self.X1[i], r=self.R2[i], acc=lin.A(k + "n2"): ops.rmsnorm_dw(dy, x, r, acc))
        d1 = ops.rmsnorm_bwd(d_n, self.X1[i], L["n2"], self.R2[i], dres=d, out=d1_out, x_rows=win)
        dao = lin._lin_bwd(k + "o", d1, self.AO[i], L["woT"], out=self.d_n[:Mr])
        q, kk, v = self._attn_views(self.QKV[i].view(B, S, -1))
        dq, dk, dv = self._attn_views(d_qkv.view(B, R, -1))
        ops.attn_bwd(dao.view(B, R, -1), q[:, r0:], kk, v, self.AO[i].view(B, S, -1)[:, r0:], self.LSE[i], H, KV, dh, True,
                     self.kmask, dq=dq, dk=dk, dv=dv, rope=(self.cos, self.sin) if dh in (64, 128) else None, row0=r0)
        if dh not in (64, 128):
            cs, sn = self.cos[r0:], self.sin[r0:]
            ops.rope_half_(d_qkv[:, :H * dh], cs, sn, R, H, dh, sign=-1)
            ops.rope_half_(d_qkv[:, H * dh:(H + KV) * dh], cs, sn, R, KV, dh, sign=-1)
        d_n = lin._lin_bwd(k + "qkv", d_qkv, self._keeps(i)[0], L["wqkvT"], out=self.G_n1[i] if tv else self.d_n[:Mr])
        if tv:
            lin._defer(lambda dy=d_qkv, acc=lin.A(k + "bqkv"): ops.colsum_(dy, acc))
            lin._defer(lambda dy=d_n, x=self.HS[i].view(M, D), r=self.R1[i], acc=lin.A(k + "n1"): ops.rmsnorm_dw(dy, x, r, acc))
        self._d = ops.rmsnorm_bwd(d_n, self.HS[i].view(M, D), L["n1"], self.R1[i], dres=d1, out=d_out, x_rows=win)
        if tap is not None:
            tap["d_in"] = self._d.clone()

    def bwd_result(self) -> torch.Tensor:
        return self._d.view(self.B, self.Rl, self.cfg.d)


# ------------------------------------------------------------------------------------------------ trainable params
class FlatParams:
    """Named bf16 views into one flat buffer (+ matching flat grad / AdamW state buffers)."""

    def __init__(self, spec: List[Tuple[str, Tuple[int, ...]]], device):
        self.offsets, off = {}, 0
        for name, shape in spec:
            n = math.prod(shape)
            self.offsets[name] = (off, shape)
            off += rup(n, 8)                      # every region 16-B aligned
        self.numel = off
        self.data = torch.zeros(off, device=device, dtype=BF16)
        self.grad = torch.zeros(off, device=device, dtype=BF16)
        self.m = torch.zeros(off, device=device, dtype=BF16)
        self.v = torch.zeros(off, device=device, dtype=BF16)

    def view(self, name, buf=None):
        off, shape = self.offsets[name]
        return (self.data if buf is None else buf)[off:off + math.prod(shape)].view(shape)

    def g(self, name):
        return self.view(name, self.grad)


class Head(_BufferSets):
    """L1RegressionActionHead + ProprioProjector + action_queries: the trainable set of the adapter-only fine-tune
    (action_heads.py:21-121; projectors.py:6-24; modeling_prismatic.py:375-376).  cfg.pro selects the block:
    MLPResNetBlock_Pro (:287-410, the reference default) - separate k/v projections per segment, RoPE on q/k - or the
    original MLPResNetBlock (:168-283) - ONE k_proj / v_proj shared by the three segments, no RoPE.  Both put the
    tanh(gating_factor) on the task-token segment and share every kernel; the original block simply reads its k|v
    weights (rows D..3D of the fused q|k|v matrix) for all three segments and sums their three gradients."""

    H = 8

    def __init__(self, cfg: VLACfg, device):
        self.cfg, self.device, self.pro = cfg, device, cfg.pro
        D, nb, Da, Pd = cfg.llm.d, cfg.num_blocks, cfg.action_dim, cfg.proprio_dim
        assert D % 64 == 0 and (D // self.H) % 8 == 0
        self.D, self.nb, self.Din = D, nb, Da * D
        assert self.Din % 64 == 0
        seg = [("w_adp", (nb, 2 * D, D)), ("b_adp", (nb, 2 * D)),    # k_adapter | v_adapter
               ("w_task", (nb, 2 * D, D)), ("b_task", (nb, 2 * D))] if cfg.pro else []   # k_task | v_task
        spec = [("w_x", (nb, 3 * D, D)), ("b_x", (nb, 3 * D))] + seg + [   # q_proj | k_self | v_self   (orig: q | k | v)
                ("w_o", (nb, D, D)), ("b_o", (nb, D)), ("w_ffn", (nb, D, D)), ("b_ffn", (nb, D)),
                ("ln_w", (nb, D)), ("ln_b", (nb, D)), ("gate", (nb, 8)),
                ("ln1_w", (self.Din,)), ("ln1_b", (self.Din,)), ("fc1_w", (D, self.Din)), ("fc1_b", (D,)),
                ("ln2_w", (D,)), ("ln2_b", (D,)), ("fc2_w", (Da, D)), ("fc2_b", (Da,)),
                ("p_fc1_w", (D, Pd)), ("p_fc1_b", (D,)), ("p_fc2_w", (D, D)), ("p_fc2_b", (D,)),
                ("action_queries", (NUM_TOKENS, D))]
        self.P = FlatParams(spec, device)
        self.film = {}            # film_gen.0.{weight,bias}: in the state dict, never used, never updated (:327-329)
        # transposed copies for the dX products (rebuilt after every optimiser step)
        z = lambda *s: torch.zeros(*s, device=device, dtype=BF16)
        self.T = dict(w_x=z(nb, D, 3 * D), w_o=z(nb, D, D), w_ffn=z(nb, D, D), p_fc2_w=z(D, D))
        if cfg.pro:
            self.T.update(w_adp=z(nb, D, 2 * D), w_task=z(nb, D, 2 * D))
        self.fc2T = z(D, 64)                       # fc2^T zero-padded to K=64
        self.pfc1_pad = z(D, 64)                   # proprio fc1 weight zero-padded to K=64
        self.dirty = True
        self.rope_tab = None     # f32 [max(T, Ka, Kt), dh] cos/sin tables (positions restart per segment: one table serves all)
        # attention weights rounded to bf16 AFTER normalisation, as the reference's bf16 softmax emits them (action_heads.py:397): a second
        # pass over the keys (vla_head_attn_desc.ref_softmax).  Off by default: +N us per block on a chain the step's turn-around waits
        # for; the reference-run fixture tests switch it on (tests/test_head_fixture_gpu.py prints both distances)
        self.ref_softmax = bool(int(os.environ.get("VLA_HEAD_REF_SOFTMAX", "0")))

    # ---- reference state-dict interop (file names / keys: finetune.py:527-572) -------------------------
    _BLK_PRO = [("q_proj", "w_x", "b_x", 0), ("k_self", "w_x", "b_x", 1), ("v_self", "w_x", "b_x", 2),
                ("k_adapter", "w_adp", "b_adp", 0), ("v_adapter", "w_adp", "b_adp", 1),
                ("k_task", "w_task", "b_task", 0), ("v_task", "w_task", "b_task", 1),
                ("o_proj", "w_o", "b_o", 0), ("ffn.1", "w_ffn", "b_ffn", 0)]
    _BLK_ORIG = [("q_proj", "w_x", "b_x", 0), ("k_proj", "w_x", "b_x", 1), ("v_proj", "w_x", "b_x", 2),
                 ("o_proj", "w_o", "b_o", 0), ("ffn.1", "w_ffn", "b_ffn", 0)]

    @property
    def _BLK(self):
        return self._BLK_PRO if self.pro else self._BLK_ORIG

    def _kv(self, which: str, i: int):
        """(weight [2D, D], bias [2D], transposed weight [D, 2D]) of the k|v projection of segment `which` in block i."""
        D = self.D
        if self.pro:
            return self.P.view("w_" + which)[i], self.P.view("b_" + which)[i], self.T["w_" + which][i]
        return self.P.view("w_x")[i, D:], self.P.view("b_x")[i, D:], self.T["w_x"][i][:, D:]

    def named_views(self, buf=None) -> Dict[str, torch.Tensor]:
        """Reference-named views ('model.mlp_resnet_blocks.N.q_proj.weight', ...) into the flat buffer."""
        P, D, out = self.P, self.D, {}
        v = lambda n: P.view(n, buf)
        for i in range(self.nb):
            pre = f"model.mlp_resnet_blocks.{i}."
            for name, w, b, k in self._BLK:
                out[pre + name + ".weight"] = v(w)[i, k * D:(k + 1) * D]
                out[pre + name + ".bias"] = v(b)[i, k * D:(k + 1) * D]
            out[pre + "ffn.0.weight"], out[pre + "ffn.0.bias"] = v("ln_w")[i], v("ln_b")[i]
            out[pre + "gating_factor"] = v("gate")[i, :1]
        for a, b in (("model.layer_norm1.weight", "ln1_w"), ("model.layer_norm1.bias", "ln1_b"), ("model.fc1.weight", "fc1_w"),
                     ("model.fc1.bias", "fc1_b"), ("model.layer_norm2.weight", "ln2_w"), ("model.layer_norm2.bias", "ln2_b"),
                     ("model.fc2.weight", "fc2_w"), ("model.fc2.bias", "fc2_b")):
            out[a] = v(b)
        return out

    def proprio_views(self, buf=None):
        v = lambda n: self.P.view(n, buf)
        return {"fc1.weight": v("p_fc1_w"), "fc1.bias": v("p_fc1_b"), "fc2.weight": v("p_fc2_w"), "fc2.bias": v("p_fc2_b")}

    def load_state_dicts(self, head_sd: Dict[str, torch.Tensor], proprio_sd: Dict[str, torch.Tensor],
                         action_queries: Optional[torch.Tensor] = None):
        nv = self.named_views()
        for k, t in nv.items():
            t.copy_(head_sd[k].to(self.device, BF16).reshape(t.shape))
        for k, t in head_sd.items():
            if "film_gen" in k:
                self.film[k] = t.to(self.device, BF16)
        for k, t in self.proprio_views().items():
            t.copy_(proprio_sd[k].to(self.device, BF16))
        if action_queries is not None:
            self.P.view("action_queries").copy_(action_queries.to(self.device, BF16))
        self.dirty = True

    def head_state_dict(self):
        sd = {k: v.clone() for k, v in self.named_views().items()}
        sd.update(self.film)
        return sd

    # `dirty` is raised whenever the flat parameter buffer changed (AdamW, checkpoint load); it expands into two stale
    # marks: the K-padded proprio fc1 weight the FORWARD reads, and the W^T operands only the BACKWARD reads.
    @property
    def dirty(self) -> bool:
        return self._stale_fwd or self._stale_bwd

    @dirty.setter
    def dirty(self, v: bool):
        self._stale_fwd = self._stale_bwd = bool(v)

    def refresh_forward_operands(self):
        if self._stale_fwd:
            pd = self.cfg.proprio_dim                  # (native strided copy: a sliced assignment is an ATen kernel on the step)
            ops.copy2d(self.P.view("p_fc1_w"), self.pfc1_pad, self.D, pd, pd, self.pfc1_pad.stride(0))
            self._stale_fwd = False

    def refresh_transposes(self):
        if not self._stale_bwd:
            return
        P = self.P
        for k in (("w_x", "w_adp", "w_task", "w_o", "w_ffn") if self.pro else ("w_x", "w_o", "w_ffn")):
            ops.transpose(P.view(k), out=self.T[k])
        ops.transpose(P.view("p_fc2_w"), out=self.T["p_fc2_w"])
        ops.transpose(P.view("fc2_w"), out=self.fc2T)             # [7, D] -> columns 0..6 of the zero-padded [D, 64]
        self._stale_bwd = False

    def build_buffer_set(self, B: int, Kt: int) -> dict:
        D, nb, T, dev = self.D, self.nb, self.cfg.chunk, self.device
        Ka = NUM_TOKENS + 1
        e = lambda *s, dt=BF16: torch.empty(*s, device=dev, dtype=dt)
        z = lambda *s, dt=BF16: torch.zeros(*s, device=dev, dtype=dt)
        R = B * T
        b = dict(Ka=Ka, Kt=Kt, R=R, h_adp=e(nb, B, Ka, D),
                 KV_adp=e(nb, B * Ka, 2 * D), KV_task=e(nb, B * Kt, 2 * D), dKV_adp=e(nb, B * Ka, 2 * D), dKV_task=e(nb, B * Kt, 2 * D),
                 X=e(nb + 1, R, D),                    # block inputs; X[nb] = output of the last block
                 QKVx=e(nb, R, 3 * D), dQKVx=e(nb, R, 3 * D), AOx=e(nb, R, D), O2=e(nb, R, D), LNo=e(nb, R, D), dO2=e(nb, R, D), dFF=e(nb, R, D),
                 probs=e(nb, B, self.H, T, T + Ka + Kt, dt=torch.float32), stats=e(nb, R, 2, dt=torch.float32))
        # fp32 gradient accumulators (bias column sums, LayerNorm dw/db, gate): views of ONE buffer, zeroed by one fill
        bkeys = tuple(k for k in ("b_x", "b_adp", "b_task", "b_o", "b_ffn", "fc1_b", "fc2_b", "p_fc1_b", "p_fc2_b") if k in self.P.offsets)
        shapes = [("dgate", (nb,)), ("ln_dw", (nb, D)), ("ln_db", (nb, D)), ("ln1_dw", (self.Din,)), ("ln1_db", (self.Din,)),
                  ("ln2_dw", (D,)), ("ln2_db", (D,)), ("d_pf", (B, D))] + [("b:" + k, tuple(self.P.offsets[k][1])) for k in bkeys]
        acc32 = b["acc32"] = z(sum(rup(math.prod(sh), 4) for _, sh in shapes), dt=torch.float32)
        off, views = 0, {}
        for name, sh in shapes:
            views[name] = acc32[off:off + math.prod(sh)].view(sh)
            off += rup(math.prod(sh), 4)
        b.update({k: views[k] for k in ("dgate", "ln_dw", "ln_db", "ln1_dw", "ln1_db", "ln2_dw", "ln2_db")}, b_f32={k: views["b:" + k] for k in bkeys}, d_pf32=views["d_pf"])
        i32 = lambda: torch.empty(B, Ka, device=dev, dtype=torch.int32)
        b.update(
            # gather / scatter row indices of the action-query hidden states (+ proprio slot) and the live-row guard: static buffers
            # filled by vla_head_index_prep (a captured step replays the kernel on the new batch's mask positions)
            row_idx_ka=i32(), row_idx_live_ka=i32(), _idx_scratch=i32(), guard=torch.zeros(1, device=dev, dtype=torch.float32),
            x_in=z(R, self.Din), pr_in=z(B, 64),
            # (the dW products read dY and X as they lie: vla_gemm_bf16_tn contracts over their rows - no transposed operand copies)
            h_task_c=e(nb, B * Kt, D) if Kt % 64 else None,      # plumbing sizes only: task rows compacted (row groups need Kt % 64 == 0)
            dfc2=e(64, D), dpfc1=e(D, 64),             # (dpfc1: proprio fc1 weight gradient against the 64-column padded input, any proprio_dim)
            dh_adp=e(nb, B * Ka, D), dpad=z(R, 64), rope_tab=ops.rope_inter_tables(max(T, Ka, Kt), D // self.H, dev),
            _buf_key=(B, Kt), _prep_key=None)          # (the scatter indices of a backward were those of the buffers just replaced)
        return b

    # ---- forward (action_heads.py:43-81, 111-121, 337-410) -------------------------------------------------
    def forward(self, HS: torch.Tensor, pos1: torch.Tensor, proprio: torch.Tensor, Np: int,
                noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HS [>=nb+1, B, S, D] hidden states (HF indexing: block i reads HS[i+1]); pos1 int32 [B,64] = positions of
        the action-query hidden states in text coordinates (mask on labels[:,1:], finetune.py:351-353, 399-405);
        proprio [B, Pd]; noise [chunk, 7*D] or None (phase Inference).  Returns predicted actions [B, chunk, 7].
        Sequential composition of the per-layer pieces the pipelined schedule (VLAEngine.step_pipelined) interleaves
        with the LLM on a second stream."""
        self.fwd_begin(HS, pos1, proprio, Np, noise)
        for i in range(self.nb):
            self.fwd_layer(i)
        return self.fwd_end()

    _FWD_FIELDS = ("HSref", "Np", "S", "B", "pos1", "_prep_key")      # what fwd_begin / prep_backward record about the bound set

    def fwd_begin(self, HS, pos1, proprio, Np, noise=None):
        """Everything that does not depend on the LLM's output: buffers, proprio projector, input stage
        (zeros/noise -> LN -> fc1 -> ReLU, action_heads.py:60-72, 113-115)."""
        cfg, P = self.cfg, self.P
        B, S = HS.shape[1], HS.shape[2]
        T = cfg.chunk
        self._alloc(B, Np)
        self.refresh_forward_operands()
        self.HSref, self.Np, self.S, self.B, self.pos1 = HS, Np, S, B, pos1
        # proprio projector (projectors.py:19-24); proprio rounded to bf16 first (action_heads.py:53)
        assert proprio.dim() == 2 and proprio.stride(1) == 1 and proprio.dtype in (BF16, torch.float32)
        ops.copy2d(proprio, self.pr_in, B, cfg.proprio_dim, proprio.stride(0), 64)
        self.pp_pre = ops.gemm_nt(self.pr_in, self.pfc1_pad, bias=P.view("p_fc1_b"))
        self.pp_act = ops.gelu_fwd(self.pp_pre)
        self.pf = ops.gemm_nt(self.pp_act, P.view("p_fc2_w"), bias=P.view("p_fc2_b"))       # [B, D]
        # rows of the 64 action-query hidden states inside one [B*S, D] layer slab.  The adapter segment of every block =
        # [64 action-query hidden states | proprio token]: the gather writes straight into h_adp[i] (index -2 = leave the row
        # alone), the proprio token is filled in once for all blocks
        ops.head_index_prep(pos1, pos1, pos1, self.row_idx_ka, self._idx_scratch, None, B, S, Np, 0)
        ops.copy2d(self.pf, self.h_adp[0, 0, NUM_TOKENS], self.nb * B, self.D, self.D, self.Ka * self.D, src_mod=B)
        if noise is not None:
            assert tuple(noise.shape) == (T, self.Din) and noise.is_contiguous()
            ops.copy2d(noise, self.x_in, B * T, self.Din, self.Din, self.Din, src_mod=T)
        else:
            ops.zero_(self.x_in)
        self.x_ln, self.st1 = ops.layernorm_fwd(self.x_in, P.view("ln1_w"), P.view("ln1_b"), 1e-5, want_stats=True)
        ops.gemm_nt(self.x_ln, P.view("fc1_w"), bias=P.view("fc1_b"), act=ACT_RELU, out=self.X[0])

    def fwd_layer(self, i: int):
        """Block i (action_heads.py:337-410): needs hidden_states[i+1] of the LLM and the previous block's output."""
        cfg, P, D, H = self.cfg, self.P, self.D, self.H
        HS, B, S, Kt, Ka, T = self.HSref, self.B, self.S, self.Kt, self.Ka, cfg.chunk
        dh = D // H
        rc, rs_ = self.rope_tab
        hs2 = HS[i + 1].view(B * S, D)
        # adapter tokens: the 64 action-query hidden states + the proprio token (:347); K/V projections, RoPE on K
        ops.gather_rows(hs2, self.row_idx_ka.view(-1), self.h_adp[i].view(B * Ka, D))
        # RoPE (positions restart per segment, action_heads.py:383-388) on q and on every segment's k rides in the projections'
        # epilogues (columns [0, D) of the k|v outputs: the K halves; position = row % segment length); the original block has none
        fuse = self.pro and D % 64 == 0 and not os.environ.get("VLA_NO_KV_ROPE_FUSE")
        wa, ba, _ = self._kv("adp", i)
        ops.gemm_nt(self.h_adp[i].view(B * Ka, D), wa, bias=ba, out=self.KV_adp[i], rope=(2, rc, rs_, Ka, dh, D) if fuse else None)
        # task tokens = HS[i+1][:, :Np] read in place (row-group addressing)
        wt, bt, _ = self._kv("task", i)
        # the reference feeds a STRIDED slice here: torch's CPU Linear then rounds the product before adding the bias, for B > 1
        # only (oracle.linear, vla_native.h bias_post_round) - reproduced so that the head tracks the reference's bf16 run
        # (the task segment's RoPE rides in the 256-row kernel's epilogue since the end of round 3; before, fusing it sent the
        #  8192 x 1792 product to the 128-row kernel: 76 us in situ against 39 + the stand-alone pass)
        ops.gemm_nt(hs2[:B * Kt], wt, bias=bt, out=self.KV_task[i], a_group=(Kt, S * D), bias_post_round=B > 1,
                    rope=(2, rc, rs_, Kt, dh, D) if fuse else None)
        x = self.X[i]
        if self.pro:
            if not fuse:
                ops.rope_inter_(self.KV_adp[i][:, :D], rc, rs_, Ka, H, dh, 0)
                ops.rope_inter_(self.KV_task[i][:, :D], rc, rs_, Kt, H, dh, 0)
            ops.gemm_nt(x, P.view("w_x")[i], bias=P.view("b_x")[i], out=self.QKVx[i], rope=(2, rc, rs_, T, dh, 2 * D))  # q, k_self
        else:
            ops.gemm_nt(x, P.view("w_x")[i], bias=P.view("b_x")[i], out=self.QKVx[i])
        self._attn(i, fwd=True)
        ops.gemm_nt(self.AOx[i], P.view("w_o")[i], bias=P.view("b_o")[i], residual=x, out=self.O2[i])
        ops.layernorm_fwd(self.O2[i], P.view("ln_w")[i], P.view("ln_b")[i], 1e-5, out=self.LNo[i], stats=self.stats[i])
        ops.gemm_nt(self.LNo[i], P.view("w_ffn")[i], bias=P.view("b_ffn")[i], act=ACT_RELU, out=self.X[i + 1])

    def fwd_end(self) -> torch.Tensor:
        P, nb = self.P, self.nb
        self.xf_ln, self.st2 = ops.layernorm_fwd(self.X[nb], P.view("ln2_w"), P.view("ln2_b"), 1e-5, want_stats=True)
        self.pred = ops.gemm_nt(self.xf_ln, P.view("fc2_w"), bias=P.view("fc2_b"))
        return self.pred.view(self.B, self.cfg.chunk, self.cfg.action_dim)

    def _attn(self, i: int, fwd: bool, dout=None):
        B, T, D, Ka, Kt, H = self.B, self.cfg.chunk, self.D, self.Ka, self.Kt, self.H
        qkv = self.QKVx[i].view(B, T, 3 * D)
        ka = self.KV_adp[i].view(B, Ka, 2 * D)
        kt = self.KV_task[i].view(B, Kt, 2 * D)
        args = (qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], ka[:, :, :D], ka[:, :, D:], kt[:, :, :D], kt[:, :, D:])
        gate = self.P.view("gate")[i]
        out = self.AOx[i].view(B, T, D)
        if fwd:
            ops.head_attn_fwd(*args, gate, H, self.ref_softmax, out=out, probs=self.probs[i])
        else:
            g = self.dQKVx[i].view(B, T, 3 * D)
            ga = self.dKV_adp[i].view(B, Ka, 2 * D)
            gt = self.dKV_task[i].view(B, Kt, 2 * D)
            ops.head_attn_bwd(dout.view(B, T, D), out, *args, gate, self.probs[i], self.dgate[i:i + 1], g[:, :, :D], g[:, :, D:2 * D],
                              g[:, :, 2 * D:], ga[:, :, :D], ga[:, :, D:], gt[:, :, :D], gt[:, :, D:], H,
                              rope=self.rope_tab if self.pro else None)

    # ---- backward ---------------------------------------------------------------------------------------------
    def backward(self, dpred: torch.Tensor, dHS: torch.Tensor, row0: int = 0):
        """dpred [B, chunk, 7] bf16.  Writes parameter gradients into the flat grad buffer and the hidden-state
        gradients into dHS [nb+1, B, S - row0, D] (HF indexing; rows not touched by the head must be pre-zeroed).
        Sequential composition of bwd_begin / bwd_layer / bwd_end."""
        self.prep_backward(self.pos1, self.Np, self.B, self.S, row0)
        self.bwd_begin(dpred, row0)
        for i in range(self.nb - 1, -1, -1):
            self.bwd_layer(i, dHS)
        self.bwd_end()

    def prep_backward(self, pos1: torch.Tensor, Np: int, B: int, S: int, row0: int, pos0=None, cnt0=None):
        """Scatter indices of the action-row gradients inside the live window [row0, S) of every sequence (-1: dead row; the
        proprio token's row scatters nowhere) and - given the unshifted mask positions - the NaN guard of a frozen window.
        Depends on the batch only, so the step schedule runs it long before the backward."""
        self._alloc(B, Np)
        g = self.guard if pos0 is not None else None
        ops.head_index_prep(pos1, pos0 if pos0 is not None else pos1, cnt0 if cnt0 is not None else pos1, self._idx_scratch,
                            self.row_idx_live_ka, g, B, S, Np, row0)
        self._prep_key = (B, S, Np, row0)

    def bwd_begin(self, dpred: torch.Tensor, row0: int = 0):
        """row0: first live row of the LLM backward (LLM.backward); dHS handed to bwd_layer is [nb+1, B, S - row0, D].
        row0 > 0 also means nothing upstream of the task tokens trains: their dX is dead and skipped."""
        cfg, P, nb = self.cfg, self.P, self.nb
        R, Da = self.R, cfg.action_dim
        self.row0 = row0
        assert self._prep_key == (self.B, self.S, self.Np, row0), "prep_backward() first"
        self.refresh_transposes()                                  # W^T operands of the dX products (stale after AdamW)
        ops.zero_(self.acc32)                                      # every fp32 gradient accumulator in one fill
        dp = dpred.reshape(R, Da)
        ops.zero_(self.dpad)
        ops.copy2d(dp, self.dpad, R, Da, Da, 64)
        ops.colsum_(dp, self.b_f32["fc2_b"])
        self._dw(self.dpad, self.xf_ln, out=self.dfc2)                         # action_dim 7 rides zero-padded to 64 columns
        ops.copy2d(self.dfc2, P.g("fc2_w"), Da, self.D, self.D, self.D)
        d_ln2 = ops.gemm_nt(self.dpad, self.fc2T)                              # [R, D]
        self.dx = ops.layernorm_bwd(d_ln2, self.X[nb], P.view("ln2_w"), self.st2, self.ln2_dw, self.ln2_db)

    def bwd_layer(self, i: int, dHS: torch.Tensor):
        """Backward of block i: the x-chain (critical path), then this layer's hidden-state gradients
        dHS[i+1] (task rows written in place, action rows scattered) - all the LLM backward of layer i waits for."""
        P, D = self.P, self.D
        B, S, Kt, Ka = self.B, self.S, self.Kt, self.Ka
        dff = self.dFF[i]
        ops.relu_bwd(self.dx, self.X[i + 1], out=dff)
        d_ln = ops.gemm_nt(dff, self.T["w_ffn"][i])
        do2 = self.dO2[i]
        ops.layernorm_bwd(d_ln, self.O2[i], P.view("ln_w")[i], self.stats[i], self.ln_dw[i], self.ln_db[i], out=do2)
        d_ao = ops.gemm_nt(do2, self.T["w_o"][i])
        self._attn(i, fwd=False, dout=d_ao)          # returns dq / dk already through the RoPE transpose
        self.dx = ops.gemm_nt(self.dQKVx[i], self.T["w_x"][i], residual=do2)
        # d h_adapter -> action rows of dHS[i+1] (+ the proprio token's gradient); d h_task -> dHS[i+1][:, :Np] in place
        ops.gemm_nt(self.dKV_adp[i], self._kv("adp", i)[2], out=self.dh_adp[i])
        ops.scatter_add_rows(self.dh_adp[i], self.row_idx_live_ka.view(-1), dHS[i + 1].view(-1, D))
        if self.row0 == 0:
            ops.gemm_nt(self.dKV_task[i], self._kv("task", i)[2], out=dHS[i + 1].view(B * S, D)[:B * Kt], c_group=(Kt, S * D))

    def bwd_end(self):
        """Off the critical path: input stage, proprio projector, and every dW as batched NT GEMMs on transposed operands."""
        cfg, P, D, nb = self.cfg, self.P, self.D, self.nb
        B, Ka = self.B, self.Ka
        G = P.g
        # input stage: relu -> fc1 -> layer_norm1 (input is noise/zeros: only parameter gradients)
        dy1 = ops.relu_bwd(self.dx, self.X[0])
        ops.colsum_(dy1, self.b_f32["fc1_b"])
        self._dw(dy1, self.x_ln, out=G("fc1_w"))
        d_xln = ops.gemm_nt(dy1, self._t(P.view("fc1_w")))
        ops.layernorm_bwd(d_xln, self.x_in, P.view("ln1_w"), self.st1, self.ln1_dw, self.ln1_db, want_dx=False)
        # proprio projector backward (its token's gradient = sum over the blocks)
        ops.colsum_(self.dh_adp.view(nb, B, Ka, D)[:, :, NUM_TOKENS].transpose(0, 1), self.d_pf32)      # [B, nb, D] strided -> sum over the blocks
        d_pf = ops.cast_f32_bf16(self.d_pf32)
        ops.colsum_(d_pf, self.b_f32["p_fc2_b"])
        self._dw(d_pf, self.pp_act, out=G("p_fc2_w"))
        d_act = ops.gemm_nt(d_pf, self.T["p_fc2_w"])
        d_pre = ops.gelu_bwd(d_act, self.pp_pre)
        ops.colsum_(d_pre, self.b_f32["p_fc1_b"])
        # proprio_dim is 8 (LIBERO), 7 (BRIDGE) or 14 (ALOHA) - prismatic/vla/constants.py:38-52: the TN product wants 8-element
        # column chunks, so it contracts against the zero-padded 64-column input (as the forward does) and the first proprio_dim
        # columns are copied out (the fc2_w gradient above takes the same route for action_dim 7)
        self._dw(d_pre, self.pr_in, out=self.dpfc1)
        ops.copy2d(self.dpfc1, G("p_fc1_w"), D, cfg.proprio_dim, 64, cfg.proprio_dim)
        # batched dW products over the nb blocks: dW = dY^T . X as TN GEMMs on dY and X as they lie in memory (the contraction
        # runs over their rows); the task tokens are read in place from the hidden states (row groups: Kt rows of every sequence)
        Kt, S = self.Kt, self.S
        h_adp = self.h_adp.view(nb, B * Ka, D)
        if self.h_task_c is None:
            h_task, tg = self.HSref[1:nb + 1, 0, :Kt], (Kt, S * D)
        else:
            for i in range(nb):
                ops.copy_rows3d(self.HSref[i + 1], self.h_task_c[i], B, Kt, D, S * D, D, Kt * D, D)
            h_task, tg = self.h_task_c, None
        ops.gemm_tn(self.dQKVx, self.X[:nb], out=G("w_x"))
        ops.gemm_tn(self.dO2, self.AOx, out=G("w_o"))
        ops.gemm_tn(self.dFF, self.LNo, out=G("w_ffn"))
        ops.colsum_(self.dQKVx, self.b_f32["b_x"]); ops.colsum_(self.dO2, self.b_f32["b_o"]); ops.colsum_(self.dFF, self.b_f32["b_ffn"])
        if self.pro:
            ops.gemm_tn(self.dKV_adp, h_adp, out=G("w_adp"))
            ops.gemm_tn(self.dKV_task, h_task, out=G("w_task"), rows=B * Kt, b_group=tg)
            ops.colsum_(self.dKV_adp, self.b_f32["b_adp"]); ops.colsum_(self.dKV_task, self.b_f32["b_task"])
        else:             # shared k_proj / v_proj: the three segments' gradients add up (autograd accumulates them in bf16 too)
            gkv = G("w_x")[:, self.D:]
            ops.gemm_tn(self.dKV_adp, h_adp, out=gkv, accumulate=True)
            ops.gemm_tn(self.dKV_task, h_task, out=gkv, accumulate=True, rows=B * Kt, b_group=tg)
            bkv = self.b_f32["b_x"][:, self.D:]
            ops.colsum_(self.dKV_adp, bkv); ops.colsum_(self.dKV_task, bkv)
        for k, t in self.b_f32.items():
            ops.cast_f32_bf16(t, out=G(k))
        ops.cast_f32_bf16(self.ln_dw, out=G("ln_w")); ops.cast_f32_bf16(self.ln_db, out=G("ln_b"))
        ops.cast_f32_bf16(self.ln1_dw, out=G("ln1_w")); ops.cast_f32_bf16(self.ln1_db, out=G("ln1_b"))
        ops.cast_f32_bf16(self.ln2_dw, out=G("ln2_w")); ops.cast_f32_bf16(self.ln2_db, out=G("ln2_b"))
        ops.copy2d(self.dgate, G("gate"), nb, 1, 1, 8)

    def _t(self, w2d):
        return ops.transpose(w2d.contiguous())

    def _dw(self, dy, x, out=None):
        """dW[N, K] = dY[R, N]^T . X[R, K] for the small one-off layers."""
        return ops.gemm_tn(dy, x, out=out, split=0)


# ------------------------------------------------------------------------------------------------ whole model
class Workspace:
    """What one input shape owns (_BufferSets' rule at engine level): the LLM's buffer set (None: nothing bound), the head's (None: left
    as it is - generation runs no head), the engine's fields (_vis_bufs: the pairs per (B, Np) that all but generation share)."""
    FIELDS = ("feats", "patches", "_vis_bufs", "B", "S", "Np", "qidx0", "pos0", "cnt0", "pos1", "cnt1", "_pred_out", "_dHS")

    def __init__(self, llm: Optional[dict] = None, head: Optional[dict] = None, fields: Optional[dict] = None):
        self.llm, self.head, self.fields = llm, head, fields or dict.fromkeys(self.FIELDS)


class VLAEngine(schedule.StepControls):
    """Adapter-only fine-tune step of VLA-Adapter (finetune.py:288-447 + 1039-1082) on one GPU."""

    def __init__(self, cfg: VLACfg, weights: Dict, device="cuda"):
        """weights = dict(vit=[sd...], proj=sd, llm=sd (HF names without 'model.' prefix incl. embed_tokens/norm),
        head=sd, proprio=sd, action_queries=tensor)."""
        self.cfg, self.device = cfg, device
        self.vits = [ViT(c, sd, device, j) for j, (c, sd) in enumerate(zip(cfg.vit, weights["vit"]))]
        self.llm = LLM(cfg.llm, weights["llm"], device)
        self.head = Head(cfg, device)
        self.head.load_state_dicts(weights["head"], weights["proprio"], weights.get("action_queries"))
        g = lambda k: weights["proj"][k].to(device=device, dtype=BF16).contiguous()
        self.proj = {k: g(k) for k in weights["proj"]}
        self.step_count = 0
        self._ws = None
        self.bind_workspace(Workspace())             # nothing is bound
        # adapter-only fine-tune: the LLM backward only has to cover the rows that can reach `action_queries`
        # (LLM.backward).  VLA_FULL_LLM_BWD=1 / full_llm_backward=True runs the reference-shaped full-sequence backward.
        self.full_llm_backward = bool(int(os.environ.get("VLA_FULL_LLM_BWD", "0")))
        self._row0 = None          # frozen by capture(); None = derive from every batch (one host sync)
        self.reducer = None        # ddp.FlatGradReducer when world_size > 1
        self._init_step_controls(copy_flat, ops.add_)
        self.executed_steps = 0    # forward+backward passes enqueued so far (eager, pipelined or replayed): profile bookkeeping
        # LLM layers above the head's last block (Qwen2.5-1.5B: 28 layers, 24 blocks - action_heads.py:117-118 reads hidden_states[1..24])
        # never reach the loss or the predicted actions: the training step and predict() run the first n_act layers only, as the
        # LoRA / full trainers do; forward_vlm() - the API twin that RETURNS every hidden state - runs them all
        self.n_act = min(cfg.llm.n_layers, cfg.num_blocks)
        self.fp8_frozen = False
        self.side = None           # head stream: the streams are created on first use (_ensure_streams)
        self._vis_bufs = {}        # (feats, patches) per (batch, patches): captured graphs keep their addresses
        self._val_pred = None
        self._predict_graphs, self._val_graphs = {}, None      # predict(): dict(graphs, static, segs, ws) per input shape; val_step_graphed()
        self._generate_sets = {}   # generate(): buffers, static batch and the two graphs per (B, L, T, pixel shape)
        self._timeline = None      # a list collects (kind, index, start, end) events of every segment run (tools/*_timeline.py)
        # captured step (capture()): its graphs, the vision graph, events of the vision stage in flight / of its pixel copy, pending update, exchange events
        self._graphs = self._g_vis = self._vis_ev = self._px_copied = self._pending_lr = self._reduced = None
        if os.environ.get("VLA_FP8_FROZEN"):
            self.enable_fp8_frozen()

    def enable_fp8_frozen(self):
        """Opt-in, NOT the reference's arithmetic (it is bf16 throughout; BASELINE configs[4] names an fp8 weight path, the
        reference has no code for it): run the frozen backbones' LayerNorm/RMSNorm-fed projections (ViT qkv / fc1, LLM q|k|v /
        gate|up) on e4m3 weights and row-quantised inputs.  Adapter-only training and inference; the backward is unchanged."""
        for v in self.vits:
            v.enable_fp8()
        self.llm.enable_fp8()
        self.fp8_frozen = True

    def _grad_buffers(self):
        return [self.head.P.grad]                    # (schedule.StepControls)

    def _state_buffers(self):
        return [("head", self.head.P)]               # (schedule.StepControls: optimizer_state / load_optimizer_state / state digests)

    @property
    def frozen_row0(self) -> Optional[int]:
        """The live-row window capture() froze (None: eager, derived from every batch)."""
        return self._row0

    def _set_clip(self, clip):
        self.flush()                                 # (a pending update belongs to the setting it ran under)
        self._clip = clip
        if clip is not None:                         # slots and the two events of _apply_update() reserved here: no step allocates
            clip.begin(self._clip_ranges())
            self._clip_events = (torch.cuda.Event(), torch.cuda.Event())

    def _clip_ranges(self):
        """The two ranges of head.P.grad that become final apart (head + proprio projector | action queries): one slot layout for
        the eager and the captured update, so both give the same norm bit for bit."""
        g, aq_off = self.head.P.grad, self.head.P.offsets["action_queries"][0]
        return [(g, 0, aq_off), (g, aq_off, self.head.P.numel)]

    def workspace(self, head: bool = True) -> Workspace:
        """The workspace that is bound now: every holder of captured graphs keeps theirs and binds it before a replay."""
        self._ws = Workspace(self.llm.buffer_set(), self.head.buffer_set() if head else None, {k: getattr(self, k) for k in Workspace.FIELDS})
        return self._ws

    def bind_workspace(self, ws: Workspace):
        """The LLM's set, the head's and the engine's fields together; identity checks alone when ``ws`` is still bound (a steady replay)."""
        if ws is self._ws and ws.llm is self.llm._bound and (ws.head is None or ws.head is self.head._bound):
            return
        self.llm.unbind() if ws.llm is None else self.llm.bind_buffer_set(ws.llm)
        if ws.head is not None:
            self.head.bind_buffer_set(ws.head)
        for k, v in ws.fields.items():
            setattr(self, k, v)
        self._ws = ws

    @contextlib.contextmanager
    def bound_workspace(self, ws: Workspace):
        """``ws`` for the duration of a call; what was bound before is bound after."""
        prev = self.workspace()
        try:
            yield self.bind_workspace(ws)
        finally:
            self.bind_workspace(prev)

    def forward(self, batch: Dict[str, torch.Tensor], noise: Optional[torch.Tensor] = None, for_training: bool = False):
        """VLM forward + action head (finetune.py:336-411) -> predicted actions [B, chunk, 7]."""
        self.forward_vlm(batch, for_training)
        return self.head.forward(self.llm.HS, self.pos1, batch["proprio"], self.Np, noise)

    # ---- inference (modeling_prismatic.py:892-972; batched: OpenVLAForActionPrediction.predict_actions): forward only, captured per input shape
    def predict(self, batch: Dict[str, torch.Tensor], latency_hint: Optional[bool] = None) -> torch.Tensor:
        """Forward pass in phase "Inference" (no input perturbation) -> normalised actions [B, chunk, action_dim] bf16, for any B.
        At batch 1 every kernel is a handful of workgroups and the ~1000 launches form dependent chains, so the forward is
        cut into single-stream segments like the training step: one stream per vision backbone (they are independent),
        the LLM on the caller's stream with the action head trailing it on the head stream; each segment is a linear
        hipGraph captured on first use of an input shape and replayed on static input buffers afterwards.

        B > 1 (a serving batch: right-padded rows, every sample's 64 action rows found from its labels by the mask / splice /
        head-index kernels, attention masking the padding): one cache entry - dict(graphs, static inputs, segs, ws: the workspace they
        were captured on, _BufferSets' rule) - per (B, L, pixel shape).  The workspace is bound before the replay and stays bound: calls
        of different shapes may alternate, and llm.HS read after a call is that call's.  The cache therefore grows by one workspace per
        shape served (DESIGN, "Serving a batch"); callers bound the number of shapes by rounding L (input_stage.serve_layout).

        latency_hint: capture under ops.latency_hint() - kernel variants for sub-chip launches on an idle chip (deep-ring GEMMs,
        short-M skinny tiles, uneven split-K, key-split attention), baked into the graphs.  Default (None): at B == 1 only, where it
        was measured; the setting is part of the cache key.  The warm-up always runs under the same
        setting as the capture, so that every kernel the graphs use has been launched and its LDS attribute set before the capture,
        and the capture streams' scratch is reserved at the size the warm-up asked for (schedule.graph_capture, scratch.ARENA)."""
        hint = batch["input_ids"].shape[0] == 1 if latency_hint is None else bool(latency_hint)
        key = (tuple(batch["input_ids"].shape), tuple(batch["pixel_values"].shape), batch["pixel_values"].dtype, hint)
        cache = self._predict_graphs
        if os.environ.get("VLA_PREDICT_EAGER"):
            return self.forward(batch, None)
        self._ensure_streams()
        if key not in cache:
            static = {k: v.clone() for k, v in batch.items()}
            with (ops.latency_hint() if hint else contextlib.nullcontext()):
                for _ in range(2):
                    self.forward(static, None)
                torch.cuda.synchronize()
                segs = self._predict_segments(static)
                graphs = schedule.capture(segs, {}, self._cap_stream)
            torch.cuda.synchronize()
            cache[key] = dict(graphs=graphs, static=static, segs=segs, ws=self.workspace())
        graphs, static, segs, ws = cache[key].values()
        self.bind_workspace(ws)                  # stays bound: callers read llm.HS and the returned tensor
        for k, v in batch.items():
            static[k].copy_(v)
        self.head.refresh_forward_operands()     # parameters may have changed since the capture (no-op when fresh)
        ev = schedule.run(segs, self._stream_of, graphs, timeline=self._timeline)
        torch.cuda.current_stream().wait_event(ev[("end", 0)])
        return self._pred_out

    def _predict_segments(self, batch, noise: Optional[torch.Tensor] = None, loss_of: Optional[torch.Tensor] = None):
        """Forward-only segments (predict()).  noise: the head's input perturbation (phase "Training"); loss_of: actions whose L1
        loss against the prediction ends the last head segment (-> self._val_loss3: the validation pass)."""
        llm, head = self.llm, self.head
        self._vision_begin(batch)                                 # host-side bookkeeping only
        segs = [Segment(f"V{j}", (lambda j=j: self._vision_backbone(j, batch)), None, ("v", j)) for j in range(len(self.vits))]
        # (layers above the head's last block do not reach the actions; few launches: the caller blocks on every call)
        ch = turnaround_chunks(self.n_act, 6, [4, 2], 1)

        def llm_fwd(c, lo, hi):
            if c == 0:
                self._vision_project()
                llm.fwd_begin(self.B, self.S, self._embed(batch), 0)
            llm.fwd_layers(lo, hi)

        def at_end():
            self._pred_out = head.fwd_end()
            if loss_of is not None:
                self._val_pred = self._pred_out
                self._val_loss3 = ops.l1_loss(self._pred_out, self._to_bf16(loss_of), want_grad=False)[0]

        return segs + schedule.pipeline_forward(head, ch, llm_fwd, lambda: (llm.HS, self.pos1, batch["proprio"], self.Np, noise), at_end,
                                                wait=[sg.signal for sg in segs], signal=("end", 0))

    # ---- greedy decoding of action tokens (prismatic/models/vlas/openvla.py:81-94: `generate`, do_sample off) ---------------------------
    def generate(self, batch: Dict[str, torch.Tensor], max_new_tokens: int, return_logits: bool = False, sample: Optional[dict] = None,
                 return_logprobs: bool = False):
        """Greedy decoding of T = max_new_tokens tokens behind B right-padded prompts of different lengths -> int64 [B, T] on the
        device, no host synchronisation.  batch: input_ids int64 [B, L], attention_mask [B, L], pixel_values, and from
        ops.decode_prompt ``pos`` int32 [B] (sequence row of each sample's last prompt id) and ``last_row`` int32 [B] (the same row in
        the flattened hidden states).  One prefill - the plain VLM forward of forward_vlm(action_queries=False), every layer and the
        final norm, no [B, S, V] logits: the last valid row of every sample is gathered and goes through the fused lm_head argmax -
        then T - 1 cached single-token steps (LLM.decode_step).  There is no early stop at an end-of-sequence id: T tokens are
        always produced.

        Captured by default: one prefill graph and ONE step graph per (B, L, T, pixel shape), the step graph replayed T - 1 times
        (positions and the step index live in device memory).  VLA_PREDICT_EAGER=1 runs both parts eagerly; return_logits (eager
        only) also returns the bf16 logits the argmax compared, [B, T, V].
        Generation owns its workspace - LLM activations, vision features; no head - and runs inside bound_workspace(): what was bound
        before is bound after, and the buffers a captured predict() or training graph holds are not written.

        sample = dict(temperature=, top_k=, top_p=, seed=, streams=None): every token is drawn by the rule of include/vla_sample.h
         instead - streams: B ints, the stream id of every row (default 0 .. B - 1); K samples of one observation
        are that row repeated under K stream ids.  return_logprobs: the log-probability of every emitted token, f32 [B, T], comes last in
        the returned tuple; without `sample` the tokens are the greedy ones, bit for bit, and the log-probability is log_softmax of the
        logits.  Either of the two takes a second cache entry (the key gains a flag) whose prefill and step graphs end in the lm_head
        pass storing the logits and vla_sample_tokens; the settings, the seed and the greedy flag live in a device block filled by a
        small copy in front of the prefill, so changing them never captures again.  With neither, the path, the key and the graphs
        are the greedy ones."""
        T = int(max_new_tokens)
        if T < 1:
            raise ValueError(f"generate: max_new_tokens must be at least 1, got {max_new_tokens}")
        if self.fp8_frozen or self.llm.lin.fp8:
            raise NotImplementedError("generate: the fp8 weight path (enable_fp8_frozen) is not covered by the cached decoder")
        eager = bool(os.environ.get("VLA_PREDICT_EAGER"))
        if return_logits and not eager:
            raise ValueError("generate: return_logits needs the eager path (VLA_PREDICT_EAGER=1): the captured graphs store no logits")
        ids, px = batch["input_ids"], batch["pixel_values"]
        B, L = ids.shape
        for k in ("pos", "last_row"):
            if k not in batch or batch[k].dtype != torch.int32 or batch[k].numel() != B:
                raise ValueError(f"generate: batch[{k!r}] must be the int32 [{B}] vector of ops.decode_prompt")
        sampled = sample is not None or return_logprobs
        key = (B, L, T, tuple(px.shape), px.dtype, eager) + (("sample",) if sampled else ())
        if sampled:                                  # refusals and the host copy of the block before any device work
            opts = dict(sample or {})
            streams = opts.pop("streams", None)
            block = ops.sample_params(greedy=sample is None, **opts)
            streams = list(range(B)) if streams is None else [int(v) for v in streams]
            if len(streams) != B:
                raise ValueError(f"generate: sample['streams'] must hold B = {B} ints, got {len(streams)}")
        ent = self._generate_sets.get(key)
        with self.bound_workspace(Workspace() if ent is None else ent["ws"]):
            if ent is None:
                ent = self._generate_sets[key] = self._generate_build(batch, T, eager, sampled)
            static, st = ent["static"], ent["state"]
            for k, v in static.items():
                v.copy_(batch[k])
            if sampled:
                st["sparams"].copy_(block)
                st["streams"].copy_(torch.tensor(streams, dtype=torch.int64))
            logits = torch.empty(B, T, st["W"].shape[0], device=self.device, dtype=BF16) if return_logits else None
            if eager:
                self._generate_prefill(static, st, None if logits is None else logits[:, 0])
                for t in range(1, T):
                    self._generate_step(st, None if logits is None else logits[:, t])
            else:
                ent["prefill"].replay()
                for _ in range(T - 1):
                    ent["step"].replay()
            out = st["out_ids"].clone()
            logprobs = st["logprobs"].clone() if return_logprobs else None
        res = (out,) + ((logits,) if return_logits else ()) + ((logprobs,) if return_logprobs else ())
        return res if len(res) > 1 else out

    # Kernel selection is part of the arithmetic (ops.latency_hint: the short-M tiles and the uneven split-K associate the fp32 sums
    # differently), so the eager and the captured path run under ONE rule and give the same tokens: the prefill as predict() has it (the
    # hint at batch 1, where it was measured), the steps - M = B rows, every launch a fraction of the chip - always.
    def _generate_prefill(self, static, st, logits0=None):
        with (ops.latency_hint() if st["B"] == 1 else contextlib.nullcontext()):
            self.forward_vlm(static, action_queries=False)
            self.llm.cache_fill(st)
            self.llm.decode_first(st, static["last_row"], static["pos"], logits0)

    def _generate_step(self, st, logits_t=None):
        with ops.latency_hint():
            self.llm.decode_step(st, logits_t)

    def _generate_build(self, batch, T: int, eager: bool, sampled: bool = False) -> dict:
        """The cache entry of one generate() shape: a workspace of its own (a fresh allocation, whatever is bound; the caller puts
        the previous one back), the decode state, static inputs, and - unless eager - the prefill graph and the step graph,
        captured on one stream behind two eager warm-up runs (every kernel launched and its LDS attribute set before the capture)."""
        llm = self.llm
        B, L = batch["input_ids"].shape
        static = {k: batch[k].clone() for k in ("input_ids", "attention_mask", "pixel_values", "pos", "last_row")}
        self._vis_bufs = {}
        llm.unbind()
        self._vision_begin(static)                   # allocates the workspace this entry keeps
        st = llm.decode_alloc(B, self.S, T, sample=sampled)
        ent = dict(static=static, state=st, ws=self.workspace(head=False))
        if eager:
            return ent
        self._ensure_streams()
        for _ in range(2):
            self._generate_prefill(static, st)
            if T > 1:
                self._generate_step(st)
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        ent["prefill"] = capture_graph(lambda: self._generate_prefill(static, st), pool, self._cap_main)
        ent["step"] = capture_graph(lambda: self._generate_step(st), pool, self._cap_main) if T > 1 else None
        torch.cuda.synchronize()
        return ent

    # modeling_prismatic.py:596-655 (multimodal forward): fills llm.HS with the n+1 hidden states
    def forward_vlm(self, batch: Dict[str, torch.Tensor], for_training: bool = False, action_queries: bool = True):
        """for_training: a loss_and_backward() follows - backward-only tensors are kept for its live rows only
        (reads the mask positions back: one host sync, eager path).  action_queries=False: the plain VLM forward of
        prismatic/models/vlms/prismatic.py:312-481 (embedding gather + patch splice only; ``labels`` not needed)."""
        self._vision(batch)
        mm = self._embed(batch, action_queries)
        self.llm.forward(self.B, self.S, mm, self.live_row0() if (for_training and action_queries) else 0,
                         n_run=self.n_act if for_training else None)

    def token_ce(self, labels: torch.Tensor):
        """HF shifted token cross-entropy of the last forward_vlm (prismatic/models/vlms/prismatic.py:469-481):
        logits = lm_head(hidden_states[-1]) over ALL positions (bf16, returned like the reference does), multimodal labels =
        [labels[:, :1] | IGNORE for the patches | labels[:, 1:]] (:411-422), loss = mean over the positions whose NEXT label is
        valid of logsumexp(float(logits)) - logits[label].  lm_head = the checkpoint's ``lm_head.weight`` or, when tied
        (Qwen2.5-0.5B: tie_word_embeddings), the embedding table.  Returns (loss f32 scalar tensor, logits [B, S, V])."""
        llm, B, S, Np = self.llm, self.B, self.S, self.Np
        n, D = self.cfg.llm.n_layers, self.cfg.llm.d
        W = getattr(llm, "lm_head", None)
        W = llm.embed if W is None else W
        V = W.shape[0]
        assert V % 8 == 0 and tuple(labels.shape) == (B, S - Np)
        logits = ops.gemm_nt(llm.HS[n].view(B * S, D), W, split_k=0).view(B, S, V)
        # target of sequence row s = multimodal label of row s + 1; the last row has none
        tgt = torch.full((B, S), IGNORE_INDEX, device=self.device, dtype=torch.int64)
        tgt[:, Np:S - 1] = labels[:, 1:]                  # rows Np .. S-2 predict text tokens 1 .. L-1 (row 0 predicts a patch: ignored)
        out2 = ops.token_ce(logits, tgt, torch.zeros(2, device=self.device, dtype=torch.float32))
        return out2[0] / out2[1], logits

    def _vision_and_embed(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        """ViT(s) -> projector -> action masks -> embedding/query splice into llm.HS[0]; returns the key mask [B,S] u8."""
        self._vision(batch)
        return self._embed(batch)

    def _vision(self, batch: Dict[str, torch.Tensor]):
        """Frozen part that reads NO trainable tensor: ViT(s) + projector -> self.patches [B, Np, D] (its own buffer, so
        that the vision stage of the NEXT step can run while the current step is still using llm.HS)."""
        self._vision_begin(batch)
        for j in range(len(self.vits)):
            self._vision_backbone(j, batch)
        self._vision_project()

    def _vision_begin(self, batch: Dict[str, torch.Tensor]):
        cfg = self.cfg
        B, L = batch["input_ids"].shape
        Np = cfg.n_patches
        self._ws = None                              # (the fields below change: no workspace is known to be bound)
        self.llm._alloc(B, L + Np)
        bufs = self._vis_bufs
        if (B, Np) not in bufs:
            bufs[(B, Np)] = (torch.empty(B, Np, cfg.vis_dim, device=self.device, dtype=BF16),
                             torch.empty(B, Np, cfg.llm.d, device=self.device, dtype=BF16))
        self.feats, self.patches = bufs[(B, Np)]
        self.B, self.S, self.Np = B, L + Np, Np

    def _vision_backbone(self, j: int, batch: Dict[str, torch.Tensor]):
        """Backbone j over ALL images of the batch in one pass (modeling_prismatic.py:196-237 runs them one by one) -> its
        column block of feats.  One backbone, one image, no prefix tokens: the last block writes the features in place."""
        vit = self.vits[j]
        direct = len(self.vits) == 1 and self.cfg.n_img == 1 and vit.cfg.n_prefix == 0
        x = vit.forward(*self._stacked_pixels(j, batch["pixel_values"]), out=self.feats.view(self.B * self.Np, -1) if direct else None)
        if not direct:
            self._scatter_feats(j, x)

    def _stacked_pixels(self, j: int, px: torch.Tensor):
        """Images of backbone j stacked along the batch: ([n_img * B, C, H, W] tensor, first channel).  Image `im` uses channels
        3*(im*n_backbones + j) .. +2."""
        cfg, nbk = self.cfg, len(self.cfg.vit)
        if cfg.n_img == 1:
            return px, 3 * j
        return torch.cat([px[:, 3 * (im * nbk + j):3 * (im * nbk + j) + 3] for im in range(cfg.n_img)], 0).contiguous(), 0

    def _scatter_feats(self, j: int, x: torch.Tensor):
        """Patch features of backbone j (its last block's output [n_img * B * T, d]; prefix tokens dropped, no final norm) ->
        feats[:, im*npi:(im+1)*npi, column block of backbone j] for every image im."""
        cfg, vc, B, feats = self.cfg, self.vits[j].cfg, self.B, self.feats
        npi, T, d, vis = vc.n_patches, vc.n_patches + vc.n_prefix, vc.d, cfg.vis_dim
        col = sum(v.cfg.d for v in self.vits[:j])
        x3 = x.view(-1, T, d)
        for im in range(cfg.n_img):
            ops.copy_rows3d(x3[im * B, vc.n_prefix:], feats[0, im * npi:, col:], B, npi, d, T * d, d, feats.shape[1] * vis, vis)

    def _vision_project(self):
        """PrismaticProjector (modeling_prismatic.py:261-273) -> self.patches."""
        cfg, B, Np = self.cfg, self.B, self.Np
        f2 = self.feats.view(B * Np, -1)
        h = ops.gemm_nt(f2, self.proj["fc1.weight"], bias=self.proj["fc1.bias"], act=ACT_GELU)
        dst = self.patches.view(B * Np, cfg.llm.d)
        if cfg.fused:
            h = ops.gemm_nt(h, self.proj["fc2.weight"], bias=self.proj["fc2.bias"], act=ACT_GELU)
            ops.gemm_nt(h, self.proj["fc3.weight"], bias=self.proj["fc3.bias"], out=dst)
        else:
            ops.gemm_nt(h, self.proj["fc2.weight"], bias=self.proj["fc2.bias"], out=dst)

    def _embed(self, batch: Dict[str, torch.Tensor], action_queries: bool = True) -> torch.Tensor:
        """Action masks + embedding gather + action-query splice (train_utils.py:8-41; modeling_prismatic.py:601-636)
        into rows 0 and Np+1.. of llm.HS[0] (reads the trainable `action_queries`); returns the key mask [B,S] u8."""
        cfg, llm = self.cfg, self.llm
        ids, labels, am = batch["input_ids"], batch.get("labels"), batch["attention_mask"]
        B, L = ids.shape
        Np = cfg.n_patches
        S = L + Np
        llm._alloc(B, S)
        X0 = llm.HS[0]
        ops.copy2d(self.patches, X0[0, 1], B * Np, cfg.llm.d, cfg.llm.d, cfg.llm.d, d_group=(Np, S * cfg.llm.d))   # patches: rows 1..Np
        if action_queries:
            self.qidx0, self.pos0, self.cnt0 = ops.action_mask(labels, 0)
            _, self.pos1, self.cnt1 = ops.action_mask(labels, 1)
        else:                                                     # plain VLM forward: no slot is overwritten
            self.qidx0 = torch.full((B, L), -1, device=self.device, dtype=torch.int32)
        mm = torch.empty(B, S, device=self.device, dtype=torch.uint8)
        am8 = am.view(torch.uint8) if am.dtype == torch.bool and am.is_contiguous() else am.to(torch.uint8).contiguous()
        ops.embed_splice(ids, am8, self.qidx0, llm.embed, self.head.P.view("action_queries"), X0, mm, Np)
        self.B, self.S, self.Np = B, S, Np
        return mm

    def live_row0(self) -> int:
        """First sequence row the backward has to cover: the largest multiple of 32 not above the first action-query
        position of any sample of the current batch (0 = whole sequence).  Reads the mask positions back (host sync)."""
        if self.full_llm_backward:
            return 0
        first = self.pos0[:, 0]
        if bool((self.cnt0 < 1).any()):
            return 0
        return (self.Np + int(first.min())) // 32 * 32

    def _to_bf16(self, t: torch.Tensor) -> torch.Tensor:
        """bf16 copy of a small contiguous fp32 / bf16 tensor (targets) by the native cast-copy."""
        if t.dtype == BF16:
            return t
        t = t.contiguous()
        out = torch.empty(t.shape, device=t.device, dtype=BF16)
        n = t.shape[-1]
        return ops.copy2d(t, out, t.numel() // n, n, n, n)

    def _dhs(self, row0: int) -> torch.Tensor:
        B, S, D, n = self.B, self.S, self.cfg.llm.d, self.cfg.llm.n_layers
        if self._dHS is None or tuple(self._dHS.shape[1:3]) != (B, S - row0):
            self._dHS = torch.empty(n + 1, B, S - row0, D, device=self.device, dtype=BF16)
        ops.zero_(self._dHS)
        return self._dHS

    def _prep_backward(self, actions, row0: Optional[int] = None):
        """Everything the backward needs that depends only on the batch (the step schedule runs it at the start of the step, off
        the forward->backward turn-around): live-row window, zeroed dHS, guard, scatter indices, bf16 targets.  row0: the window
        capture() froze; None: derived from this batch (one host sync) - no action block can start before it, so no guard."""
        frozen = row0 is not None
        self._row0_used = row0 = row0 if frozen else self.live_row0()
        self._dhs(row0)
        self.head.prep_backward(self.pos1, self.Np, self.B, self.S, row0, self.pos0, self.cnt0)
        self._guard = self.head.guard if frozen and row0 else None      # NaN when a sample's action block starts before the frozen window
        self._actions_bf = self._to_bf16(actions)

    def _turn_around(self, pred, gscale: float) -> torch.Tensor:
        """Forward -> backward turn-around: L1 loss (finetune.py:418) with its gradient scaled by gscale, the frozen window's
        guard folded into the reported loss, the head's backward begun -> loss3."""
        loss3, dpred = ops.l1_loss(pred, self._actions_bf, True, gscale)
        if self._guard is not None:
            ops.add_scalar_f32_(loss3, self._guard)
        self.head.bwd_begin(dpred, self._row0_used)
        return loss3

    def _query_grad(self):
        """Tail of the backward: the LLM's input gradient at the action-query rows -> the ``action_queries`` gradient."""
        dq = ops.action_query_grad(self.llm.bwd_result().contiguous(), self.pos0, self.Np, self._row0_used)
        ops.cast_f32_bf16(dq, out=self.head.P.g("action_queries"))

    def loss_and_backward(self, pred, actions, gscale: float = 1.0, exchange: bool = True):
        """L1 loss + backward into the flat grad buffer: the pieces of the step schedule (_segments) one after the other on the
        current stream.  gscale scales the gradient (loss / grad-accumulation steps); exchange=False leaves the data-parallel
        exchange to the caller (non-boundary micro-steps)."""
        llm, head = self.llm, self.head
        exchange = exchange and self.reducer is not None
        self._prep_backward(actions)
        loss3 = self._turn_around(pred, gscale)
        for i in range(head.nb - 1, -1, -1):
            head.bwd_layer(i, self._dHS)
        head.bwd_end()
        aq_off = head.P.offsets["action_queries"][0]
        if exchange:                                    # head/proprio grads are final: exchange them under the LLM backward
            self.reducer.reduce_async(head.P.grad, 0, aq_off)
        llm.backward(self._dHS, self.B, self.S, self._row0_used, n_run=self.n_act)
        self._query_grad()
        if exchange:
            self.reducer.reduce_async(head.P.grad, aq_off, None)
        return loss3

    def optimizer_step(self, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01):
        """torch.optim.AdamW semantics on the flat trainable buffer (finetune.py:910, 1078-1082), on the current stream."""
        self._apply_update(lr, beta1, beta2, eps, wd, two_stream=False, join=False)

    def train_step(self, batch, lr: float, noise=None):
        """One micro-batch; the optimizer steps on every ``ga``-th call (set_grad_accumulation)."""
        self.executed_steps += 1
        pred = self.forward(batch, noise, for_training=True)
        loss3 = self.loss_and_backward(pred, batch["actions"], 1.0 / self.ga, exchange=self.ga == 1)
        if self._accum.fold():
            if self.ga > 1 and self.reducer is not None:
                self.reducer.reduce_async(self.head.P.grad, 0, None)
            self.optimizer_step(lr)
        return loss3

    # ---- pipelined two-stream schedule + hipGraph replay -----------------------------------------------------------
    # The action head is 3 % of the FLOPs but a chain of ~300 small dependent kernels (~9 ms when run alone): block i
    # only needs hidden_states[i+1], so its forward trails the LLM forward on a SECOND stream and its backward runs AHEAD
    # of the LLM backward (which needs dHS[i+1] from block i).  The head's kernels fill the idle CUs / tile-quantisation
    # tails of the LLM's large GEMMs instead of serialising with them.
    #
    # The step is a list of single-stream segments ("M": vision / LLM, "H": head) built, run and captured by schedule.py.
    def _ensure_streams(self):
        if self.side is None:
            self.side = torch.cuda.Stream()            # head stream (a high-priority stream measured 0.7 % slower on the step in round 1)
            self._cap_main = torch.cuda.Stream()       # capture stream of the "M" graphs (replayed on the current stream)
            self.vis_stream = torch.cuda.Stream()      # vision stage of the NEXT step (fills the backward's idle CUs)
            self._vstreams = [self.vis_stream] + [torch.cuda.Stream() for _ in range(max(0, len(self.vits) - 1))]   # one per backbone

    def _segments(self, batch, noise):
        """[Segment(stream 'M'|'H', fn, wait_key|None, signal_key|None)] for everything after the vision stage."""
        llm, head = self.llm, self.head
        n = self.n_act                                  # layers that reach the loss
        fch = turnaround_chunks(n, 4, [2, 1, 1], 1)           # (the backward walks the same ranges top-down)
        if os.environ.get("VLA_FWD_CHUNKS"):                  # A/B knob: "4,4,4,4,4,2,1,1"
            fch = chunks(n, [int(x) for x in os.environ["VLA_FWD_CHUNKS"].split(",")])

        def llm_fwd(c, lo, hi):
            if c == 0:
                mm = self._embed(batch)
                self._prep_backward(batch["actions"], self._row0)
                llm.fwd_begin(self.B, self.S, mm, self._row0_used)
            llm.fwd_layers(lo, hi)

        def turn_around():
            self._loss3 = self._turn_around(head.fwd_end(), 1.0 / self.ga)

        def llm_bwd(k, lo, hi):
            if k == 0:
                llm.bwd_begin(self._dHS, self._row0_used, n)
            for i in range(hi - 1, lo - 1, -1):
                llm.bwd_layer(i, self._dHS)
            if k == len(fch) - 1:
                self._query_grad()

        # ONE whole-batch forward pipeline (round 1's two half-batch pipelines left the tree in round 4: DESIGN section 5b)
        return (schedule.pipeline_forward(head, fch, llm_fwd, lambda: (llm.HS, self.pos1, batch["proprio"], self.Np, noise), turn_around,
                                          refresh=True)
                + schedule.pipeline_backward(head, fch, llm_bwd, lambda: self._dHS)
                + [Segment("H", head.bwd_end, None, ("end", 0))])      # the caller joins on this event (head gradients final)

    def _stream_of(self, name: str, main):
        return main if name == "M" else self.side if name == "H" else self._vstreams[int(name[1:])]

    def _cap_stream(self, name: str):
        """Capture stream of a segment kind: the "M" graphs replay on the caller's stream and are captured on one of their own."""
        return self._cap_main if name == "M" else self._stream_of(name, None)

    def _fwd_bwd(self, batch, noise, vision: bool = True):
        """Eager run of the two-stream schedule (vision stage first unless the vision graph already ran)."""
        self.executed_steps += 1
        if vision:
            self._vision(batch)
        torch.cuda.current_stream().wait_event(schedule.run(self._segments(batch, noise), self._stream_of)[("end", 0)])   # join
        return self._loss3

    # Data-parallel schedule of the captured step.  The gradient exchange of step k (one bucketed RCCL all-reduce of the
    # flat gradient buffer on its own stream) is NOT waited for at the end of step k: step k+1 first replays the vision
    # graph - ViT + projector, ~25 % of the step, which read no trainable tensor - and only then waits for the exchange,
    # applies AdamW and replays the rest.  Same arithmetic as synchronous DP (every use of a parameter sees the updated
    # value); the all-reduce is hidden under the next step's ViT instead of under a backward tail that the live-row
    # LLM backward has made too short to hide it.  `flush()` applies the last pending update.
    def capture(self, batch: Dict[str, torch.Tensor], noise: Optional[torch.Tensor] = None, warmup: int = 2,
                conservative_rows: bool = False, row0: Optional[int] = None):
        """``batch``/``noise`` become the static input buffers: copy new data INTO them before each replay.
        The live-row window of the LLM backward is frozen here: from the capture batch's first action-query row, or - with
        ``conservative_rows`` - from the first text row (valid for ANY later batch of the same shape: the action block
        cannot start before tok0 + patches + one prompt token).  ``row0``: the window an earlier run froze (a resumed run captures
        with the window of the run it continues, not with the one its own first batch would give)."""
        self._ensure_streams()
        self._static_batch, self._static_noise = batch, noise
        self._row0 = None
        self._vision_and_embed(batch)                # masks of the capture batch -> the frozen live-row window
        self._row0 = self.live_row0()
        if conservative_rows and not self.full_llm_backward:
            self._row0 = min(self._row0, (self.cfg.n_patches + 1) // 32 * 32)
        if row0 is not None:
            assert 0 <= int(row0) < self.S and int(row0) % 32 == 0, f"row0 {row0}: a multiple of 32 inside the sequence"
            self._row0 = int(row0)
        for _ in range(warmup):                      # allocate every buffer / set kernel attributes outside capture (kernel scratch: graph_capture reserves it)
            self.head.dirty = True
            self._fwd_bwd(batch, noise)
        torch.cuda.synchronize()
        self.head.dirty = True
        # vision stage: reads the staged pixels of the NEXT batch (stage_next_pixels), writes self.patches; a memory pool of its own
        self._next_px = batch["pixel_values"].clone()
        self._px_stage = batch["pixel_values"].clone()
        self._g_vis = capture_graph(lambda: self._vision(dict(batch, pixel_values=self._px_stage)), torch.cuda.graph_pool_handle(),
                                    self.vis_stream)
        self._vis_ev = None
        self._segs = self._segments(batch, noise)
        self._graphs = schedule.capture(self._segs, {}, self._cap_stream)
        torch.cuda.synchronize()
        self._step_ws = self.workspace()             # kept for the graphs' lifetime, bound before every replay
        self._pending_lr = None
        # the vision stage of step k+1 starts behind this forward segment of step k: it runs under the backward, whose two
        # dependent kernel chains leave most CUs idle.  Default: the third-last forward segment (the last two hold one LLM
        # layer each and are latency-bound with the head trailing them); same-box sweep at B = 32: last 31.52 ms/step,
        # second-last 31.33, third-last 31.14, fourth-last 31.35.  VLA_VIS_AFTER overrides.
        m_fwd = [k for k, sg in enumerate(self._segs) if sg.stream == "M" and sg.signal is not None and sg.signal[0] == "f"]
        # (fourth-last forward segment: 26.51 vs 26.64-26.69 ms for the third-last with the one-pipeline forward, same box)
        self._vis_after = m_fwd[min(len(m_fwd) - 1, max(0, int(os.environ.get("VLA_VIS_AFTER", len(m_fwd) - 4))))]
        assert self._segs[self._vis_after].signal is not None      # (schedule.run hands after() the event of a signalling segment)
        self._launch_vision()                        # vision stage of the FIRST step (the pixels given to capture)

    def stage_next_pixels(self, pixel_values: torch.Tensor):
        """Captured mode: pixels of the batch AFTER the one the next train_step_graphed() call trains on (its vision stage
        runs during that call).  Without staging, the pixels given to capture() are reused."""
        if self._px_copied is not None:
            torch.cuda.current_stream().wait_event(self._px_copied)   # the vision stream has taken its copy of the old pixels
        self._next_px.copy_(pixel_values)

    def _launch_vision(self, after_event=None):
        """Enqueue the vision stage (ViT + projector -> self.patches) of the staged pixels on the vision stream."""
        V, cur = self.vis_stream, torch.cuda.current_stream()
        if after_event is not None:
            V.wait_event(after_event)           # self.patches of the running step has been consumed (_embed)
        else:
            V.wait_stream(cur)
        tl = self._timeline
        with torch.cuda.stream(V):
            if tl is not None:
                t0 = torch.cuda.Event(enable_timing=True)
                t0.record(V)
            copy_flat(self._px_stage, self._next_px)
            self._px_copied = torch.cuda.Event()
            self._px_copied.record(V)
            self._g_vis.replay()
            self._vis_ev = torch.cuda.Event(enable_timing=tl is not None)
            self._vis_ev.record(V)
            if tl is not None:
                tl.append(("V", -1, t0, self._vis_ev))

    def train_step_pipelined(self, batch, lr: float, noise=None):
        """Eager (un-captured) run of the two-stream schedule."""
        self._ensure_streams()
        loss3 = self._fwd_bwd(batch, noise)
        if self.reducer is not None:
            self.reducer.reduce_async(self.head.P.grad, 0, None)
        self.optimizer_step(lr)
        return loss3

    def train_step_graphed(self, lr: float):
        """Replay of the captured step on the static buffers.  The parameter update of THIS step (RCCL exchange +
        AdamW) is left pending and applied inside the next call, after that step's vision graph - or by flush()."""
        cur = torch.cuda.current_stream()
        self.executed_steps += 1
        self.bind_workspace(self._step_ws)
        self.flush(join=False)
        cur.wait_event(self._vis_ev)          # patches of THIS step (computed during the previous call)
        def after(k, seg, ev):
            if k == self._vis_after:
                self._launch_vision(ev)
        self._h_end = schedule.run(self._segs, self._stream_of, self._graphs, after=after,
                                   timeline=self._timeline)[("end", 0)]
        cur.wait_event(self._px_copied)        # later writes to the staging source are ordered behind the vision copy
        if self.ga > 1:                        # gradient accumulation: join, fold, update only on the boundary micro-step
            cur.wait_event(self._h_end)
            if not self._accum.fold():
                return self._loss3
            self._h_end = torch.cuda.Event()
            self._h_end.record(cur)            # the summed gradient is final on the current stream
        if self.reducer is not None:
            aq_off = self.head.P.offsets["action_queries"][0]
            # head / proprio gradients are final when the head stream ends: their exchange starts there, underneath the
            # rest of the LLM backward and the next step's vision stage; the action-query gradient follows the LLM backward
            # (the action queries go first on the exchange stream: the LLM backward ends before the head's tail does, and
            # the next step's LLM stream only waits for them - flush())
            ev_aq = self.reducer.reduce_async(self.head.P.grad, aq_off, None)
            ev_head = self.reducer.reduce_async(self.head.P.grad, 0, aq_off, after_event=self._h_end)
            self._reduced = (ev_aq, ev_head)
        self._pending_lr = lr
        return self._loss3

    def flush(self, join: bool = True):
        """Apply the pending parameter update of the last train_step_graphed (no-op if none), in the two-stream placement of
        _apply_update().  ``join`` (default) makes the current stream wait for the head-stream half too, so that callers may
        read any parameter afterwards (checkpoints, evaluation); the captured step passes False: its head segments run on the
        head stream anyway."""
        if self._pending_lr is None:
            return
        lr, self._pending_lr = self._pending_lr, None
        self._apply_update(lr, two_stream=True, join=join)

    def _apply_update(self, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, *, two_stream: bool, join: bool):
        """THE parameter update: reducer join, step count, clip passes, AdamW.  It is two AdamW launches: the action queries (64 x
        D, the only trainable tensor the LLM stream reads, in _embed) on the current stream, everything else (head + proprio
        projector, 99.97 % of the bytes) on the head stream ``hs`` - with ``two_stream`` the engine's (behind that stream's last
        backward kernel and ahead of its first forward kernel of the next step: the 0.5 ms of optimiser traffic runs beside the
        first LLM forward segment instead of in front of it), else the current one too.  join: the current stream waits for hs."""
        cur, P, clip = torch.cuda.current_stream(), self.head.P, self._clip
        hs = self.side if two_stream else cur
        aq_off = P.offsets["action_queries"][0]
        assert aq_off + rup(math.prod(P.offsets["action_queries"][1]), 8) == P.numel, "action_queries must close the flat buffer"
        self.step_count += 1
        gscale = 1.0
        if self.reducer is not None:
            ev_aq, ev_head = self._reduced or (None, None)
            if ev_aq is not None and ev_head is not None:
                cur.wait_event(ev_aq)                 # the LLM stream needs the action queries only ...
                hs.wait_event(ev_head)                # ... the 437 MB head exchange is joined by the head stream
                self.reducer.joined()
            else:
                self.reducer.wait(*((cur, hs) if two_stream else (cur,)))
            self._reduced = None
            gscale = self.reducer.grad_scale          # DDP averages: sum-all-reduce then 1/N, folded into AdamW
        if two_stream and self.ga > 1:                # accumulated gradient was assembled on the current stream
            hs.wait_event(self._h_end)
        if clip is not None:
            # clipped: each stream takes the sum of squares of its own range where that range is final; the current stream adds the
            # two (it waits for the head stream's pass: the one new edge), and each stream runs its AdamW behind the coefficient
            r_head, r_aq = self._clip_ranges()
            head_summed, finalised = self._clip_events
            clip.begin([r_head, r_aq])
            with torch.cuda.stream(hs):
                clip.sumsq(*r_head, gscale)
                head_summed.record(hs)
            clip.sumsq(*r_aq, gscale)
            cur.wait_event(head_summed)
            clip.finalise()
            finalised.record(cur)
            hs.wait_event(finalised)

        def adam(sl):
            args = (self.step_count, lr, beta1, beta2, eps, wd)
            if clip is None:
                ops.adamw_(P.data[sl], P.grad[sl], P.m[sl], P.v[sl], *args, gscale=gscale)
            else:
                ops.adamw_clipped_(P.data[sl], P.grad[sl], P.m[sl], P.v[sl], clip.coef, *args, gscale=gscale)
        with torch.cuda.stream(hs):
            adam(slice(None, aq_off))
            side_done = torch.cuda.Event()
            side_done.record()
        adam(slice(aq_off, None))
        if join:
            cur.wait_event(side_done)
        self.head.dirty = True

    # ---- validation pass (vla-scripts/finetune.py:605-685: eval mode, no_grad, run_forward_pass per held-out batch) ----------
    # A sweep runs between two training steps at the TRAINING batch shape, so it shares the step's activation buffers - none of
    # which carries state from one step to the next - and its vision buffers (feats / patches).  What does carry over in the
    # captured step: the pending parameter update (applied by begin_validation) and the vision stage of the NEXT training batch,
    # in flight on the vision stream.  The sweep waits for that stage, overwrites its patches, and end_validation() runs it
    # again on the pixels still staged in _next_px (the same graph on the same input: the same bits).
    def begin_validation(self):
        """Before a sweep: apply the pending update, order the sweep behind the in-flight vision stage, refresh the head's
        forward operands (the captured validation graphs do not carry that refresh)."""
        self.flush()
        if self._vis_ev is not None:
            torch.cuda.current_stream().wait_event(self._vis_ev)
        self.head.refresh_forward_operands()

    def end_validation(self):
        """After a sweep: recompute the next training batch's patches (captured step only)."""
        if self._g_vis is not None:
            self._launch_vision()

    def val_forward(self, batch: Dict[str, torch.Tensor], noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Eager validation of one batch: forward() + the L1 loss without gradient -> f32 [3] (loss, current, next actions)."""
        pred = self._val_pred = self.forward(batch, noise)
        return ops.l1_loss(pred, self._to_bf16(batch["actions"]), want_grad=False)[0]

    @property
    def val_pred(self) -> torch.Tensor:
        """The prediction of the last validation forward (val_forward / val_step_graphed): bf16 [B, chunk, action_dim] on the device,
        final in stream order when that call returns - what a per-sample reduction of the sweep reads (heldout.HeldOutSweep)."""
        return self._val_pred.view(self.B, self.cfg.chunk, self.cfg.action_dim)

    def val_step_graphed(self, batch: Dict[str, torch.Tensor], noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Captured validation of the static ``batch`` / ``noise`` buffers (copy each batch INTO them first): the forward-only
        segments of predict() ending in the L1 loss, captured on the first call.  No ops.latency_hint(): its GEMM variant
        changes the fp32 association, and the values must be the eager forward's."""
        self._ensure_streams()

        def make():
            segs = self._predict_segments(batch, noise, loss_of=batch["actions"])
            return schedule.capture(segs, {}, self._cap_stream), segs, self.workspace()

        def replay(graphs, segs, ws):
            self.bind_workspace(ws)
            self.head.refresh_forward_operands()
            torch.cuda.current_stream().wait_event(schedule.run(segs, self._stream_of, graphs)[("end", 0)])
        return schedule.captured_validation(self, batch, noise, make, replay)
