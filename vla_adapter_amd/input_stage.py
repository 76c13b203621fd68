"""On-GPU input stage for the fine-tune path: raw frames / actions / prompt ids -> the batch dict
the model consumes, following the reference's CPU pipeline step by step:

  * ``RLDSBatchTransform.__call__`` (prismatic/vla/datasets/datasets.py:29-143, ``use_minivlm`` branch): action chunk
    -> 56 token ids with ``ActionTokenizer`` (action_tokenizer.py:60-74), extended to NUM_TOKENS = 64 by
    ``random.choices`` over the 56, appended to the prompt ids minus their last three; labels = ids with everything but the
    last 65 positions set to IGNORE_INDEX;
  * ``PrismaticImageProcessor.apply_transform`` (processing_prismatic.py:128-145): ToTensor + Normalize per backbone,
    channel-stacked, after ``TVF.resize(img, (224, 224), BICUBIC, antialias=True)`` ("resize-naive", preprocessor_config.json)
    = ``PIL.Image.resize``: Pillow's two-pass 8-bit fixed-point bicubic resampler, reproduced bit for bit by
    ``vla_resample_u8`` with host-computed taps (``pil_bicubic_coeffs``);
  * ``PaddedCollatorForActionPrediction`` (prismatic/util/data_utils.py:95-175): right padding, attention mask,
    primary || wrist images on the channel dimension, stacked actions / proprio.

The heavy parts (pixels, binning) run as HIP kernels on the device; the variable-length id bookkeeping is a few hundred
integers per batch and stays on the host, using Python's ``random`` exactly like the reference so that a seeded run draws
the same 8 filler tokens.  That is ``build()``.  ``collate()`` produces the same batch without the host: the reference's
``normalize_action_and_proprio`` (rlds/utils/data_utils.py:52-90) and the whole id / label / padding assembly run as two more
kernels (csrc/collate.hip), nothing is read back, and the filler tokens come from the device's counter-based generator
(DESIGN.md section 12).
"""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .constants import IGNORE_INDEX, NUM_TOKENS

# timm data configs of the two backbones (pretrained_models/configs/preprocessor_config.json: means / stds)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # DINOv2 (featurizer, channels 0-2)
SIGLIP_MEAN, SIGLIP_STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)                          # SigLIP (fused_featurizer, channels 3-5)


def backbone_norms(mcfg) -> Tuple[str, ...]:
    """Which Normalize each vision backbone of a model config gets (the ``backbones`` argument of GPUInputStage): a DINOv2-like
    ViT - register / cls prefix tokens or LayerScale - takes ImageNet's mean / std, anything else SigLIP's 0.5 / 0.5 (the timm
    data configs of the reference's two featurizers, preprocessor_config.json)."""
    return tuple("dino" if (v.layerscale or v.n_prefix > 0) else "siglip" for v in mcfg.vit)


AUG_ORDER = ("random_resized_crop", "random_brightness", "random_contrast", "random_saturation", "random_hue")


@dataclass
class ImageAugment:
    """The reference's training augmentation (prismatic/vla/datasets/datasets.py:204-218 -> dlimp augment_image): defaults are its
    settings - random_resized_crop(scale=[0.9, 0.9], ratio=[1, 1]), random_brightness(0.2), random_contrast(0.8, 1.2),
    random_saturation(0.8, 1.2), random_hue(0.05) - applied in that order; ``ops`` names the ones that run (a disabled op is
    skipped).  Per image one uniform u is drawn on the device from (seed, rank, step, sample, image) and mapped to all five
    parameters.  ``params``: f32 [B * n_img, 9] supplied instead of drawn (columns: ops.AUG_P_*)."""
    crop_scale: float = 0.9
    brightness: float = 0.2
    contrast: Tuple[float, float] = (0.8, 1.2)
    saturation: Tuple[float, float] = (0.8, 1.2)
    hue: float = 0.05
    ops: Tuple[str, ...] = AUG_ORDER
    seed: int = 0
    rank: int = 0
    step: int = 0
    params: Optional[torch.Tensor] = None

    def mask(self) -> int:
        bad = [o for o in self.ops if o not in AUG_ORDER]
        if bad:
            raise ValueError(f"unknown augmentation ops {bad}: known {AUG_ORDER}")
        bits = (ops.AUG_CROP, ops.AUG_BRIGHTNESS, ops.AUG_CONTRAST, ops.AUG_SATURATION, ops.AUG_HUE)
        m = sum(b for o, b in zip(AUG_ORDER, bits) if o in self.ops)
        return m | (0 if self.params is not None else ops.AUG_DRAW)

    def cfg7(self):
        """Settings of the draw mapping, f32: crop side = sqrt(area scale) (tf.sqrt of the f32 scale), then the ranges."""
        side = np.sqrt(np.float32(self.crop_scale))
        return [float(side), self.brightness, *self.contrast, *self.saturation, self.hue]


def center_crop_params(n: int, crop_scale: float = 0.9) -> torch.Tensor:
    """Per-image parameters of the evaluator's center crop (experiments/robot/openvla_utils.py:568-648): the centred box of area
    ``crop_scale``, in f32 as TF computes it - side = clip(sqrt(scale), 0, 1), offset = (1 - side) / 2."""
    side = np.clip(np.sqrt(np.float32(crop_scale)), np.float32(0), np.float32(1))
    off = (np.float32(1) - side) / np.float32(2)
    p = np.zeros((n, ops.AUG_NPARAM), np.float32)
    p[:, ops.AUG_P_Y1] = p[:, ops.AUG_P_X1] = off
    p[:, ops.AUG_P_Y2] = p[:, ops.AUG_P_X2] = off + side
    return torch.from_numpy(p)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_coeffs(in_size: int, out_size: int):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BICUBIC filter (src/libImaging/Resample.c): per output position
    the first source index, the tap count and the taps in 22-bit fixed point; the support widens with the downscale factor
    (antialiasing).  Same double arithmetic, same rounding, so that the device pass is bit-identical to PIL.Image.resize."""
    import math
    prec = 32 - 8 - 2
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coefs = np.zeros((out_size, ksize), np.int32)
    inv = 1.0 / fscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * inv) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, cnt)
        for x, v in enumerate(w):
            coefs[xx, x] = int(-0.5 + v * (1 << prec)) if v < 0 else int(0.5 + v * (1 << prec))
    return bounds, coefs


# ---- the evaluator's frame pipeline: resize_image_for_policy (experiments/robot/openvla_utils.py:542-565), DESIGN.md section 20 ----
RESIZE_MODES = ("bicubic", "lanczos3")
# libjpeg's two standard quantisation tables (jcparam.c: std_luminance_quant_tbl, std_chrominance_quant_tbl), natural order
JPEG_STD_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
JPEG_STD_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def jpeg_quant_tables(quality: int = 95) -> np.ndarray:
    """uint16 [2, 64]: the luminance and the chrominance quantisation table of a baseline file of ``quality`` (1 .. 100), natural
    order - libjpeg's jpeg_set_quality: its standard tables scaled by jpeg_quality_scaling (5000 / quality below 50, else 200 - 2 *
    quality), q = clamp((base * scale + 50) / 100, 1, 255), integer arithmetic.  95 is tf.image.encode_jpeg's default."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quant_tables: quality is 1 .. 100, got {quality}")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = np.array([JPEG_STD_LUMA, JPEG_STD_CHROMA], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


_SPANS = {}


def tf_lanczos3_spans(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """The spans of tf.image.resize(method="lanczos3", antialias=True) along one side, n_in -> n_out samples (TF's ScaleAndTranslate:
    ComputeSpansCore with the Lanczos3 kernel, scale = n_out / n_in, translation 0), float32 throughout -> (starts int32 [n_out],
    weights f32 [n_out, span], zero-padded behind a span that the source's edge cuts short).  Cached per (n_in, n_out).

    scale = f32(n_out) / f32(n_in), inv = 1 / scale, ks = max(inv, 1) (the kernel widens with the downscale factor: the antialiasing);
    span = min(2 ceil(3 ks) + 1, n_in).  Output x samples the source at s = (x + 0.5) inv; its span is [ceil(s - 3 ks - 0.5), floor(s +
    3 ks - 0.5)] clamped into the source; source i weighs k(|(i + 0.5 - s) (1 / ks)|), k(x) = 0 beyond 3, 1 up to 1e-3, else 3 sin(pi x)
    sin(pi x / 3) / (pi^2 x^2) with pi = f32(3.14159265359); the weights are summed one after the other in float32 and every one is
    multiplied by 1 / sum (when |sum| >= 1000 FLT_MIN).  numpy's float32 sin stands where TF calls sinf: their last bits may differ."""
    key = (int(n_in), int(n_out))
    if key in _SPANS:
        return _SPANS[key]
    n_in, n_out = key
    if n_in < 1 or n_out < 1:
        raise ValueError(f"tf_lanczos3_spans: sizes must be positive, got {n_in} -> {n_out}")
    f32 = np.float32
    scale = f32(n_out) / f32(n_in)
    inv = f32(1.0) / scale
    ks = max(inv, f32(1.0))
    oks, rad, pi = f32(1.0) / ks, f32(3.0), f32(3.14159265359)
    span = min(2 * int(np.ceil(rad * ks)) + 1, n_in)
    s = (np.arange(n_out, dtype=f32) + f32(0.5)) * inv                                # f32 [n_out]
    first = np.clip(np.ceil((s - rad * ks) - f32(0.5)).astype(np.int64), 0, n_in - 1)
    last = np.clip(np.floor((s + rad * ks) - f32(0.5)).astype(np.int64), 0, n_in - 1)
    src = first[:, None] + np.arange(span)[None, :]                                    # [n_out, span]
    x = np.abs(((src.astype(f32) + f32(0.5)) - s[:, None]) * oks).astype(f32)
    with np.errstate(all="ignore"):
        v = (rad * np.sin(pi * x) * np.sin(pi * x / rad) / (pi * pi * x * x)).astype(f32)
    w = np.where(x > rad, f32(0), np.where(x <= f32(1e-3), f32(1), v)).astype(f32)
    w[src > last[:, None]] = 0                                                        # behind the span: padding
    tot = np.zeros(n_out, f32)
    for k in range(span):                                                              # summed one after the other, as TF does
        tot = (tot + w[:, k]).astype(f32)
    norm = np.where(np.abs(tot) >= f32(1000.0) * np.finfo(f32).tiny, f32(1.0) / np.where(tot == 0, f32(1), tot), f32(1.0)).astype(f32)
    w = (w * norm[:, None]).astype(f32)
    out = (np.ascontiguousarray(first.astype(np.int32)), np.ascontiguousarray(w))
    for a in out:
        a.setflags(write=False)
    _SPANS[key] = out
    return out


NORMALIZATION_KINDS = ("bounds", "bounds_q99")     # NormalizationType.BOUNDS / BOUNDS_Q99 (rlds/utils/data_utils.py:44-49)


def collate_layout(prompt_lens: Sequence[int], max_len: int, num_tokens: int = NUM_TOKENS) -> Tuple[List[int], int]:
    """Host side of ``GPUInputStage.collate``, from the prompt lengths alone: the offset table [B + 1] of the concatenated prompts
    and the batch's token length L = min(longest row, max_len), a row being its prompt minus the three trailing ids (kept whole
    when shorter than three, datasets.py:76-79) plus the ``num_tokens`` action ids."""
    off = [0]
    for n in prompt_lens:
        off.append(off[-1] + int(n))
    rows = [(n - 3 if n >= 3 else n) + num_tokens for n in map(int, prompt_lens)]
    return off, min(max(rows), max_len)


def serve_layout(prompt_lens: Sequence[int], len_multiple: int = 32, num_tokens: int = NUM_TOKENS) -> Tuple[List[int], int]:
    """Host side of ``GPUInputStage.serve_tokens``, from the prompt lengths alone: the offset table [B + 1] of the concatenated prompts
    and the batch's token length L = the longest row - its whole prompt, the ``num_tokens`` placeholders and the stop id
    (prepare_inference_inputs) - rounded up to ``len_multiple``.  32 is the granularity live_row0 already uses: a stream of calls
    whose longest prompts differ lands on few captured shapes."""
    if len_multiple < 1:
        raise ValueError("serve_layout: len_multiple must be at least 1")
    off = [0]
    for n in prompt_lens:
        off.append(off[-1] + int(n))
    longest = max(int(n) for n in prompt_lens) + num_tokens + 1
    return off, -(-longest // len_multiple) * len_multiple


def serve_prompt_lens(prompt_ids) -> Optional[List[int]]:
    """The prompt lengths where the host knows them - id lists, or (flat, offsets) tensors with the offsets on the host - else None."""
    if isinstance(prompt_ids, (tuple, list)) and len(prompt_ids) == 2 and all(isinstance(t, torch.Tensor) for t in prompt_ids):
        return None if prompt_ids[1].is_cuda else prompt_ids[1].diff().tolist()
    return [len(r) for r in prompt_ids]


def serve_check(prompt_ids, L: Optional[int] = None, len_multiple: int = 32) -> Tuple[Optional[List[int]], Optional[int]]:
    """Host-side validation of a serving batch's prompts -> (offsets or None, L).  Known lengths: ValueError on an empty prompt or
    one that does not fit L (default serve_layout's).  Offsets on the device: L is required (nothing is read back)."""
    lens = serve_prompt_lens(prompt_ids)
    if lens is None:
        if L is None:
            raise ValueError("serve_tokens: prompt offsets on the device need an explicit L (the default would read them back)")
        return None, int(L)
    if len(lens) < 1 or min(lens) < 1:
        raise ValueError("serve_tokens: every sample needs a prompt of at least one id")
    off, L_nat = serve_layout(lens, len_multiple)
    L = L_nat if L is None else int(L)
    if max(lens) + NUM_TOKENS + 1 > L:
        raise ValueError(f"serve_tokens: a prompt of {max(lens)} ids needs L >= {max(lens) + NUM_TOKENS + 1}, got L = {L}")
    return off, L


PAD_TOKEN_ID = 151643                               # Qwen2.5's <|endoftext|>, the processor's pad id
SERVE_STATS_KINDS = {"bounds": ("min", "max"), "bounds_q99": ("q01", "q99")}     # openvla_utils.py:682-687, modeling_prismatic.py:787-796


class GPUInputStage:
    def __init__(self, device="cuda", tokenizer_len: int = 151643, n_bins: int = 256, min_action: float = -1.0, max_action: float = 1.0,
                 pad_token_id: int = PAD_TOKEN_ID, model_max_length: int = 2048, backbones: Sequence[str] = ("siglip",),
                 out_dtype=torch.bfloat16, image_size: int = 224, resize: str = "bicubic"):
        """``resize``: how pixels() brings frames that are not at ``image_size`` there - "bicubic", the processor's Pillow resize
        (resize()), or "lanczos3", the RLDS stage's tf.image.resize(method="lanczos3", antialias=True) (lanczos3_resize(), DESIGN.md
        section 20)."""
        if resize not in RESIZE_MODES:
            raise ValueError(f"GPUInputStage: resize is one of {RESIZE_MODES}, got {resize!r}")
        self.resize_mode = resize
        self.device, self.tokenizer_len, self.pad, self.max_len = device, tokenizer_len, pad_token_id, model_max_length
        self.lo, self.hi = float(min_action), float(max_action)
        self.bins = torch.from_numpy(np.linspace(min_action, max_action, n_bins)).to(device)       # f64, numpy's own edges
        self.n_bins = n_bins
        self.bin_centers = (self.bins[:-1] + self.bins[1:]) / 2.0                                    # f64 [n_bins - 1] (action_tokenizer.py:47)
        self.norm = [dict(dino=(IMAGENET_MEAN, IMAGENET_STD), siglip=(SIGLIP_MEAN, SIGLIP_STD))[b] for b in backbones]
        self.out_dtype = out_dtype
        self.image_size = image_size
        self._taps = {}
        self._stats = {}
        self._spans = {}
        self._qtabs = {}

    def resize(self, frames_u8: torch.Tensor, out_h: int = 224, out_w: int = 224) -> torch.Tensor:
        """uint8 [B, H, W, 3] -> uint8 [B, out_h, out_w, 3], bit-identical to PIL.Image.resize((out_w, out_h), BICUBIC): horizontal
        pass into an 8-bit intermediate, then the vertical pass (Pillow's order)."""
        fr = frames_u8.to(self.device).contiguous()
        B, H, W, Cc = fr.shape
        assert fr.dtype == torch.uint8 and Cc == 3

        def taps(n_in, n_out):
            key = (n_in, n_out)
            if key not in self._taps:
                b, c = pil_bicubic_coeffs(n_in, n_out)
                self._taps[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(c).to(self.device), c.shape[1])
            return self._taps[key]
        cur = fr
        if W != out_w:
            b, c, ks = taps(W, out_w)
            nxt = torch.empty(B, H, out_w, 3, device=self.device, dtype=torch.uint8)
            ops.N.check(ops._lib().vla_resample_u8(ops._st(), ops._p(cur), ops._p(nxt), B * H, W, out_w, 3, ops._p(b), ops._p(c), ks), "resample_u8")
            cur = nxt
        if H != out_h:
            b, c, ks = taps(H, out_h)
            nxt = torch.empty(B, out_h, out_w, 3, device=self.device, dtype=torch.uint8)
            ops.N.check(ops._lib().vla_resample_u8(ops._st(), ops._p(cur), ops._p(nxt), B, H, out_h, out_w * 3, ops._p(b), ops._p(c), ks), "resample_u8")
            cur = nxt
        return cur

    def lanczos3_resize(self, frames_u8: torch.Tensor, out_h: int = 224, out_w: int = 224) -> torch.Tensor:
        """uint8 [B, H, W, 3] -> uint8 [B, out_h, out_w, 3]: tf.image.resize(method="lanczos3", antialias=True), rounded half to even
        and clipped, as the reference's RLDS stage (obs_transforms.py:75) and its evaluators (resize_image_for_policy) apply it.  Two
        HIP passes, the vertical one first, float32 sums over the spans of tf_lanczos3_spans(); bit-identical to the numpy rule of
        tests/policy_image_rule_np.py.  TF itself is not pinned: its last bits and its pass order are unconfirmed (DESIGN.md section
        20).  A side that does not change is not resampled; frames already at the size come back as they are, nothing launched."""
        fr = frames_u8.to(self.device)
        if fr.dim() != 4 or fr.dtype != torch.uint8 or fr.shape[3] != 3:
            raise ValueError(f"lanczos3_resize: frames are uint8 [B, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
        B, H, W, _ = fr.shape
        if (H, W) == (out_h, out_w):
            return fr

        def spans(n_in, n_out):
            if n_in == n_out:
                return None
            key = (n_in, n_out)
            if key not in self._spans:
                st, w = tf_lanczos3_spans(n_in, n_out)
                self._spans[key] = (torch.from_numpy(st.copy()).to(self.device), torch.from_numpy(w.copy()).to(self.device))
            return self._spans[key]
        return ops.policy_lanczos3_resize(fr.contiguous(), out_h, out_w, spans(H, out_h), spans(W, out_w))

    def jpeg_round_trip(self, frames_u8: torch.Tensor, quality: int = 95) -> torch.Tensor:
        """uint8 [B, H, W, 3] -> uint8 of the same shape: what saving every frame as a baseline 4:2:0 JPEG file of ``quality`` and
        decoding it again gives (tf.image.encode_jpeg, then tf.io.decode_image, of resize_image_for_policy), bit-identical to Pillow /
        libjpeg-turbo.  No file is written: the entropy coding is lossless and left out.  H and W must be multiples of 16 (ValueError)."""
        fr = frames_u8.to(self.device)
        if fr.dim() != 4 or fr.dtype != torch.uint8 or fr.shape[3] != 3:
            raise ValueError(f"jpeg_round_trip: frames are uint8 [B, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
        if fr.shape[1] % 16 or fr.shape[2] % 16 or fr.shape[1] < 16 or fr.shape[2] < 16:
            raise ValueError(f"jpeg_round_trip: frames of {fr.shape[1]} x {fr.shape[2]}: H and W must be multiples of 16 (libjpeg's edge "
                             "replication for partial MCUs is not built)")
        q = int(quality)
        if q not in self._qtabs:
            self._qtabs[q] = torch.from_numpy(jpeg_quant_tables(q).view(np.int16).copy()).to(self.device)
        return ops.policy_jpeg_round_trip(fr.contiguous(), self._qtabs[q])

    def policy_frames(self, frames_u8, size: Optional[int] = None, quality: int = 95) -> torch.Tensor:
        """The evaluator's resize_image_for_policy (experiments/robot/openvla_utils.py:542-565) for a batch, on the device: frames_u8
        uint8 [B, n_img, H, W, 3], or the list form pixels() takes -> uint8 [B, n_img, size, size, 3] (default size: image_size):
        jpeg_round_trip(quality), then lanczos3_resize.  Nothing is read back.  Pinned: the round trip to Pillow / libjpeg-turbo, the
        resize to the numpy rule; not pinned: TF's own bits."""
        size = self.image_size if size is None else int(size)
        if isinstance(frames_u8, torch.Tensor) and frames_u8.dim() == 5:
            fr = frames_u8.to(self.device)
        else:
            fr = torch.stack([f.to(self.device) for f in frames_u8], 1)
        if fr.dim() != 5 or fr.dtype != torch.uint8 or fr.shape[4] != 3:
            raise ValueError(f"policy_frames: frames are uint8 [B, n_img, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
        B, n_img, H, W, _ = fr.shape
        flat = fr.contiguous().view(B * n_img, H, W, 3)
        return self.lanczos3_resize(self.jpeg_round_trip(flat, quality), size, size).view(B, n_img, size, size, 3)

    def tokenize_actions(self, actions: torch.Tensor) -> torch.Tensor:
        """[..., action_dim] f32 on the device -> int64 token ids (same shape)."""
        return ops.action_tokenize(actions.to(self.device, torch.float32).contiguous(), self.bins, self.tokenizer_len, self.lo, self.hi)

    def decode_token_ids_to_actions(self, ids: torch.Tensor) -> torch.Tensor:
        """ActionTokenizer.decode_token_ids_to_actions (action_tokenizer.py:76-95): int64 token ids (any shape) -> f64 bin centres
        (same shape), centre[clip(tokenizer_len - id - 1, 0, n_bins - 2)].  The clip makes every id decodable; on ids that
        tokenize_actions made it inverts the binning (the last bin edge shares the last interval)."""
        d = (self.tokenizer_len - ids.to(self.bin_centers.device, torch.int64) - 1).clamp_(0, self.bin_centers.numel() - 1)
        return self.bin_centers[d]

    def pixels(self, frames_u8, augment: Optional[ImageAugment] = None, center_crop: bool = False, return_aux: bool = False):
        """frames_u8: list over images per sample (primary first, then wrist ...) of uint8 [B, H, W, 3] tensors, or one uint8
        [B, n_img, H, W, 3] tensor -> [B, 3 * n_backbones * n_images, H, W]: per image, one 3-channel block per backbone
        (apply_transform's vstack).  ``augment``: the reference's training augmentation first (ImageAugment); ``center_crop``: the
        evaluator's center_crop_image first (crop_scale 0.9).  Both run as one fused HIP pass that ends in the same normalise.
        ``return_aux``: also return dict(frames_u8=uint8 [B, n_img, H, W, 3] as normalised, params=f32 [B, n_img, 9] applied or None)."""
        if augment is not None and center_crop:
            raise ValueError("augment and center_crop are the training and the serving path: pass one of them")
        if isinstance(frames_u8, torch.Tensor) and frames_u8.dim() == 5:
            stacked = frames_u8
            frames_u8 = list(frames_u8.unbind(1))
        else:
            stacked = None
        if tuple(frames_u8[0].shape[1:3]) != (self.image_size, self.image_size):       # apply_transform: resize first
            first = self.lanczos3_resize if self.resize_mode == "lanczos3" else self.resize
            frames_u8 = [first(f, self.image_size, self.image_size) for f in frames_u8]
            stacked = None
        B, H, W, _ = frames_u8[0].shape
        nb = len(self.norm)
        out = torch.empty(B, 3 * nb * len(frames_u8), H, W, device=self.device, dtype=self.out_dtype)
        if augment is None and not center_crop:
            for im, fr in enumerate(frames_u8):
                fr = fr.to(self.device).contiguous()
                for j, (mean, std) in enumerate(self.norm):
                    ops.image_normalize_u8_(fr, out, 3 * (im * nb + j), mean, std)
            if not return_aux:
                return out
            return out, dict(frames_u8=torch.stack([f.to(self.device) for f in frames_u8], 1), params=None)
        fr = (stacked if stacked is not None else torch.stack(frames_u8, 1)).to(self.device).contiguous()
        n_img = fr.shape[1]
        if center_crop:
            augment = ImageAugment(ops=("random_resized_crop",), params=center_crop_params(B * n_img))
        params = augment.params
        params = (torch.empty(B * n_img, ops.AUG_NPARAM, device=self.device, dtype=torch.float32) if params is None
                  else params.to(self.device, torch.float32).reshape(B * n_img, ops.AUG_NPARAM).contiguous())
        fr_out = torch.empty_like(fr) if return_aux else None
        ops.image_augment_normalize_(fr, out, self.norm, augment.mask(), augment.cfg7(), params, seed=augment.seed, rank=augment.rank,
                                     step=augment.step, frames_out=fr_out)
        if not return_aux:
            return out
        return out, dict(frames_u8=fr_out, params=params.view(B, n_img, ops.AUG_NPARAM))

    def build(self, frames_u8: Sequence[torch.Tensor], prompt_ids: List[List[int]], actions: torch.Tensor,
              proprio: Optional[torch.Tensor] = None, rng: Optional[random.Random] = None, augment: Optional[ImageAugment] = None,
              center_crop: bool = False) -> Dict[str, torch.Tensor]:
        """prompt_ids: tokenizer output of the chat prompt per sample (still carrying the three trailing ids the reference
        deletes); actions [B, chunk, action_dim] normalised continuous actions (window: current + future); augment /
        center_crop: see pixels()."""
        rng = rng or random
        B = actions.shape[0]
        tok = self.tokenize_actions(actions.reshape(B, -1)).cpu().tolist()           # 56 ids per sample (8 x 7)
        rows, labels = [], []
        for b in range(B):
            ids = list(prompt_ids[b])
            if len(ids) >= 3:
                del ids[-3:]                                                         # datasets.py:76-79
            flat = tok[b]
            if NUM_TOKENS < len(flat):
                ids = ids + flat[:NUM_TOKENS]
            else:
                ids = ids + flat + rng.choices(flat, k=NUM_TOKENS - len(flat))       # datasets.py:81-87
            lab = list(ids)
            for k in range(len(lab) - (NUM_TOKENS + 1)):                             # labels[: -(action_chunk_len + 1)] = IGNORE
                lab[k] = IGNORE_INDEX
            rows.append(ids)
            labels.append(lab)
        L = min(max(len(r) for r in rows), self.max_len)
        ids_t = torch.full((B, L), self.pad, dtype=torch.int64)
        lab_t = torch.full((B, L), IGNORE_INDEX, dtype=torch.int64)
        for b in range(B):                                                           # right padding + truncation
            n = min(len(rows[b]), L)
            ids_t[b, :n] = torch.tensor(rows[b][:n])
            lab_t[b, :n] = torch.tensor(labels[b][:n])
        ids_t, lab_t = ids_t.to(self.device), lab_t.to(self.device)
        batch = dict(pixel_values=self.pixels(frames_u8, augment=augment, center_crop=center_crop), input_ids=ids_t, labels=lab_t, attention_mask=ids_t.ne(self.pad),
                     actions=actions.to(self.device))
        if proprio is not None:
            batch["proprio"] = proprio.to(self.device, torch.float32).reshape(B, -1)
        return batch

    def normalize(self, x: torch.Tensor, stats: dict, kind: str = "bounds_q99") -> torch.Tensor:
        """normalize_action_and_proprio (rlds/utils/data_utils.py:52-90) on the device: raw actions / proprio [..., D] -> f32 of the
        same shape.  ``stats``: one entry of dataset_statistics.json (e.g. norm_stats[name]["action"]) - q01 / q99 for "bounds_q99",
        min / max for "bounds", optional mask; dimensions whose min == max become 0 under both kinds (:87-89; skipped when the entry
        has no min / max).  The statistics are uploaded once per (stats object, kind)."""
        if kind not in NORMALIZATION_KINDS:
            raise NotImplementedError(f"normalisation type {kind!r}: only {NORMALIZATION_KINDS} are built (NORMAL, mean / std, is used by "
                                      "no shipped configuration)")
        key = (id(stats), kind)
        if key not in self._stats:
            lo_k, hi_k = ("min", "max") if kind == "bounds" else ("q01", "q99")
            if lo_k not in stats or hi_k not in stats:
                raise KeyError(f"normalisation type {kind!r} needs {lo_k!r} and {hi_k!r} in the statistics, got {sorted(stats)}")
            f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(self.device)
            u8 = lambda v: torch.as_tensor(np.asarray(v, dtype=bool).astype(np.uint8)).to(self.device)
            zero = None
            if "min" in stats and "max" in stats:
                zero = u8(np.asarray(stats["min"], dtype=np.float32) == np.asarray(stats["max"], dtype=np.float32))
            mask = u8(stats["mask"]) if "mask" in stats else None
            self._stats[key] = (stats, f32(stats[lo_k]), f32(stats[hi_k]), mask, zero)      # (stats itself: its id stays taken)
        _, low, high, mask, zero = self._stats[key]
        x = x.to(self.device, torch.float32).contiguous()
        if x.shape[-1] != low.numel():
            raise ValueError(f"last dimension {x.shape[-1]} does not match the statistics' {low.numel()}")
        return ops.normalize_bounds(x, low, high, mask, zero)

    def normalize_rows(self, x: torch.Tensor, stats_list, sel: torch.Tensor, kind: str = "bounds_q99") -> torch.Tensor:
        """normalize() with one statistics entry per row: x [R, ..., D], sel int32 [R] on the device names the entry of ``stats_list``
        (a list / tuple of entries as normalize() takes them) row r is normalised with - a mixture of datasets, every sample with its
        own dataset's statistics (rlds/dataset.py:544-550).  A row is bit-identical to normalize() on that row with that entry.  The
        stacked tables are uploaded once per (list object, kind); an entry without ``mask`` gets all ones, ``zero`` is min == max
        where an entry has both."""
        if kind not in NORMALIZATION_KINDS:
            raise NotImplementedError(f"normalisation type {kind!r}: only {NORMALIZATION_KINDS} are built (NORMAL, mean / std, is used by "
                                      "no shipped configuration)")
        if not isinstance(stats_list, (list, tuple)) or not stats_list:
            raise ValueError("normalize_rows: stats_list is a non-empty list / tuple of statistics entries")
        key = (id(stats_list), kind, "rows")
        if key not in self._stats:
            lo_k, hi_k = ("min", "max") if kind == "bounds" else ("q01", "q99")
            for n, st in enumerate(stats_list):
                if lo_k not in st or hi_k not in st:
                    raise KeyError(f"normalisation type {kind!r} needs {lo_k!r} and {hi_k!r} in the statistics, entry {n} has {sorted(st)}")
            f32 = lambda k: np.stack([np.asarray(st[k], dtype=np.float32) for st in stats_list])
            low, high = f32(lo_k), f32(hi_k)
            if low.ndim != 2 or low.shape != high.shape:
                raise ValueError(f"normalize_rows: the entries' {lo_k!r} / {hi_k!r} must share one length")
            D = low.shape[1]
            mask = np.stack([np.asarray(st["mask"], dtype=bool) if "mask" in st else np.ones(D, dtype=bool) for st in stats_list])
            zero = np.stack([np.asarray(st["min"], dtype=np.float32) == np.asarray(st["max"], dtype=np.float32)
                             if "min" in st and "max" in st else np.zeros(D, dtype=bool) for st in stats_list])
            if mask.shape != low.shape or zero.shape != low.shape:
                raise ValueError("normalize_rows: the entries' mask / min / max must have the length of the bounds")
            up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a.astype(dt))).to(self.device)
            self._stats[key] = (stats_list, up(low, np.float32), up(high, np.float32), up(mask, np.uint8), up(zero, np.uint8))   # (the list itself: its id stays taken)
        _, low, high, mask, zero = self._stats[key]
        x = x.to(self.device, torch.float32).contiguous()
        if x.shape[-1] != low.shape[1]:
            raise ValueError(f"last dimension {x.shape[-1]} does not match the statistics' {low.shape[1]}")
        if sel.dtype != torch.int32 or tuple(sel.shape) != (x.shape[0],):
            raise ValueError(f"normalize_rows: sel must be int32 [{x.shape[0]}], got {sel.dtype} {tuple(sel.shape)}")
        return ops.normalize_bounds_rows(x, sel.to(self.device).contiguous(), low, high, mask, zero)

    def serve_tokens(self, prompt_ids, L: Optional[int] = None, len_multiple: int = 32) -> Dict[str, torch.Tensor]:
        """The batch of prepare_inference_inputs for B prompts of different lengths, right-padded to L, in one launch (vla_serve_tokens):
        dict(input_ids, labels int64 [B, L], attention_mask bool [B, L], hid_row int32 [B], row_ok u8 [B]).  prompt_ids: list of id lists, or
        (prompt_flat int64 [n], prompt_off int32 [B + 1]) tensors.  L: static token length; default serve_layout's, from the prompt
        lengths on the host - offsets already on the device therefore need L (nothing is read back, exactly as collate() has it), and a
        row that is empty or does not fit is then reported by row_ok alone.  Host-side lengths are checked here: ValueError."""
        off_l, L = serve_check(prompt_ids, L, len_multiple)
        if isinstance(prompt_ids, (tuple, list)) and len(prompt_ids) == 2 and all(isinstance(t, torch.Tensor) for t in prompt_ids):
            flat, off = prompt_ids
        else:
            flat = torch.tensor([t for r in prompt_ids for t in r], dtype=torch.int64)
            off = torch.tensor(off_l, dtype=torch.int32)
        flat, off = flat.to(self.device, torch.int64).contiguous(), off.to(self.device, torch.int32).contiguous()
        from .constants import ACTION_TOKEN_BEGIN_IDX, STOP_INDEX
        ids, labels, am, hid_row, row_ok = ops.serve_tokens(flat, off, int(L), pad_id=self.pad, num_tokens=NUM_TOKENS, fill_id=1,
                                                            stop_id=STOP_INDEX, action_label=ACTION_TOKEN_BEGIN_IDX + 1, ignore_index=IGNORE_INDEX)
        return dict(input_ids=ids, labels=labels, attention_mask=am.view(torch.bool), hid_row=hid_row, row_ok=row_ok)

    def decode_prompt(self, prompt_ids, n_patches: int, len_multiple: int = 32) -> Dict[str, torch.Tensor]:
        """The prompt-only batch of a generation (VLAEngine.generate), right-padded to the longest prompt rounded up to
        ``len_multiple``, in one launch (vla_decode_prompt): dict(input_ids int64 [B, L], attention_mask bool [B, L], pos int32 [B],
        last_row int32 [B], row_ok u8 [B]).  Unlike serve_tokens no placeholders and no stop id stand behind the prompt: the decoder
        writes its own tokens there.  prompt_ids: list of id lists, or (prompt_flat, prompt_off) tensors with the offsets on the host."""
        lens = serve_prompt_lens(prompt_ids)
        if lens is None or len(lens) < 1 or min(lens) < 1:
            raise ValueError("decode_prompt: host-side prompt lengths, every one at least 1")
        if len_multiple < 1:
            raise ValueError("decode_prompt: len_multiple must be at least 1")
        L = -(-max(lens) // len_multiple) * len_multiple
        if isinstance(prompt_ids, (tuple, list)) and len(prompt_ids) == 2 and all(isinstance(t, torch.Tensor) for t in prompt_ids):
            flat, off = prompt_ids
        else:
            flat = torch.tensor([t for r in prompt_ids for t in r], dtype=torch.int64)
            off = torch.tensor(serve_layout(lens, len_multiple)[0], dtype=torch.int32)
        flat, off = flat.to(self.device, torch.int64).contiguous(), off.to(self.device, torch.int32).contiguous()
        ids, am, pos, last_row, row_ok = ops.decode_prompt(flat, off, L, int(n_patches), pad_id=self.pad)
        return dict(input_ids=ids, attention_mask=am.view(torch.bool), pos=pos, last_row=last_row, row_ok=row_ok)

    def _serve_stats(self, stats: dict, kind: str):
        """(low f64 [D], high f64 [D], mask u8 [D] or None) on the device, uploaded once per (stats object, kind)."""
        if kind not in SERVE_STATS_KINDS:
            raise ValueError(f"Unsupported action/proprio normalization type {kind!r}: known {sorted(SERVE_STATS_KINDS)}")
        key = (id(stats), kind, "serve")
        if key not in self._stats:
            lo_k, hi_k = SERVE_STATS_KINDS[kind]
            if lo_k not in stats or hi_k not in stats:
                raise KeyError(f"normalisation type {kind!r} needs {lo_k!r} and {hi_k!r} in the statistics, got {sorted(stats)}")
            f64 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float64)).to(self.device)
            mask = torch.as_tensor(np.asarray(stats["mask"], dtype=bool).astype(np.uint8)).to(self.device) if "mask" in stats else None
            self._stats[key] = (stats, f64(stats[lo_k]), f64(stats[hi_k]), mask)               # (stats itself: its id stays taken)
        return self._stats[key][1:]

    def normalize_proprio(self, x, stats: dict, kind: str = "bounds_q99") -> torch.Tensor:
        """The evaluator's normalize_proprio (experiments/robot/openvla_utils.py:671-701) on the device: raw proprio [..., D], f32 or f64
        (tensor or ndarray) -> f32, clip(mask ? 2 (x - low) / (high - low + 1e-8) - 1 : x, -1, 1) in f64, rounded once.  Unlike
        normalize() - the training pipeline's - it clips the unmasked dimensions too and zeroes none.  stats: norm_stats[key]["proprio"]."""
        low, high, mask = self._serve_stats(stats, kind)
        x = torch.as_tensor(x)
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        x = x.to(self.device).contiguous()
        if x.shape[-1] != low.numel():
            raise ValueError(f"last dimension {x.shape[-1]} does not match the statistics' {low.numel()}")
        return ops.normalize_proprio_serve(x, low, high, mask)

    def unnormalize_actions(self, pred: torch.Tensor, stats: dict, kind: str = "bounds_q99", row_ok: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """_unnormalize_actions (modeling_prismatic.py:784-805) on the device: the head's bf16 predictions [B, chunk, action_dim] -> f64 of
        the same shape, bit-identical to the host function on pred.float(); rows with row_ok == 0 become NaN.  stats:
        norm_stats[key]["action"]."""
        low, high, mask = self._serve_stats(stats, kind)
        if pred.shape[-1] != low.numel():
            raise ValueError(f"last dimension {pred.shape[-1]} does not match the statistics' {low.numel()}")
        return ops.unnormalize_actions(pred, low, high, mask, row_ok, out)

    def collate(self, frames_u8, prompt_ids, actions: torch.Tensor, proprio: Optional[torch.Tensor] = None, *, action_stats: Optional[dict] = None,
                proprio_stats: Optional[dict] = None, L: Optional[int] = None, seed: int = 0, rank: int = 0, step: int = 0,
                augment: Optional[ImageAugment] = None, center_crop: bool = False, stats_index: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """build() without the host: the same batch dict from kernels only (vla_normalize_bounds, vla_collate_tokens, pixels()).
        prompt_ids: list of id lists, or (prompt_flat int64 [n], prompt_off int32 [B + 1]) tensors - with tensors on the device nothing
        is copied, read back or looped over.  action_stats / proprio_stats: raw values are normalised first (normalize(), "bounds_q99")
        and batch["actions"] holds the normalised window.  L: static token length (rows are padded or cut to it); default
        min(longest row, model_max_length), from the prompt lengths on the host - device-resident offsets therefore need L.  The
        filler ids of the action block are drawn on the device from (seed, rank, step, sample, slot), not from Python's random.
        A list / tuple of entries as action_stats / proprio_stats with stats_index (int32 [B] on the device): sample b is normalised
        with entry stats_index[b] (normalize_rows(): a batch of a dataset mixture); a single dict keeps the one-set kernel."""
        B = actions.shape[0]
        per_row = [isinstance(s, (list, tuple)) for s in (action_stats, proprio_stats) if s is not None]
        if any(per_row) and stats_index is None:
            raise ValueError("collate: a list of statistics entries needs stats_index= (which entry each sample takes)")
        if stats_index is not None and not (per_row and all(per_row)):
            raise ValueError("collate: stats_index= goes with lists of statistics entries as action_stats / proprio_stats")

        def norm(x, st):
            return self.normalize_rows(x, st, stats_index) if isinstance(st, (list, tuple)) else self.normalize(x, st)
        if isinstance(prompt_ids, (tuple, list)) and len(prompt_ids) == 2 and all(isinstance(t, torch.Tensor) for t in prompt_ids):
            flat, off = prompt_ids
            if L is None:
                if off.is_cuda:
                    raise ValueError("collate: prompt offsets on the device need an explicit L (the default would read them back)")
                L = collate_layout(off.diff().tolist(), self.max_len)[1]
        else:
            lens = [len(r) for r in prompt_ids]
            off_l, L_nat = collate_layout(lens, self.max_len)
            L = L_nat if L is None else L
            flat = torch.tensor([t for r in prompt_ids for t in r], dtype=torch.int64)
            off = torch.tensor(off_l, dtype=torch.int32)
        if off.numel() != B + 1:
            raise ValueError(f"collate: {off.numel()} prompt offsets for {B} samples (expected B + 1)")
        flat, off = flat.to(self.device, torch.int64).contiguous(), off.to(self.device, torch.int32).contiguous()
        act = norm(actions, action_stats) if action_stats is not None else actions.to(self.device)
        ids, labels, am = ops.collate_tokens(flat, off, act.to(torch.float32).reshape(B, -1).contiguous(), self.bins, int(L),
                                             tokenizer_len=self.tokenizer_len, lo=self.lo, hi=self.hi, pad_id=self.pad, ignore_index=IGNORE_INDEX,
                                             num_tokens=NUM_TOKENS, seed=seed, rank=rank, step=step)
        batch = dict(pixel_values=self.pixels(frames_u8, augment=augment, center_crop=center_crop), input_ids=ids, labels=labels,
                     attention_mask=am.view(torch.bool), actions=act)
        if proprio is not None:
            pr = norm(proprio, proprio_stats) if proprio_stats is not None else proprio.to(self.device, torch.float32)
            batch["proprio"] = pr.reshape(B, -1)
        return batch
