"""Case definitions shared by tools/make_golden_vla.py (which runs the reference's own model glue on them) and the tests that
read its fixtures (tests/test_oracle_golden.py, tests/test_vla_golden_gpu.py).

The weights and the batch are regenerated from seeds on CPU on both sides (a full state dict of the smallest geometry the
engine builds is several MB, over the size limit of a committed file); every fixture keeps a digest of what was generated,
and the tests refuse to compare against a fixture whose inputs differ.  What the fixture records is the reference run:
the one input it decides (the targets, placed away from its own prediction), every output, and the gradients.
"""
import hashlib
import os

import numpy as np
import torch

from vla_adapter_amd import checkpoints as CK, engine as E, synthetic as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (configuration, batch size, prompt length, ragged, weight seed, batch seed).  All three use geometries that
# checkpoints.infer_config reads back off the reference-layout state dict (plus n_img / pro, which a state dict does not hold).
CASES = {
    # (a) fused DINOv2-like (cls + 4 registers, LayerScale) + SigLIP-like vision, one image, 3-layer projector, Pro head
    "fused1": (lambda: _with(E.tiny_fused_config(), n_img=1), 3, 12, True, 11, 12),
    # (b) the same backbones, two images per sample: channels [img0: featurizer | fused_featurizer | img1: ... | ...]
    "fused2": (lambda: _with(E.tiny_fused_config(), n_img=2), 2, 12, True, 21, 22),
    # (c) SigLIP only, 2-layer projector, the original (non-Pro) head block
    "siglip": (lambda: _with(E.tiny_config(), pro=False), 2, 12, True, 31, 32),
}

# batch-1 predict_action: q01 / q99 un-normalisation with the gripper (last dimension) left normalised by its mask
NORM_STATS = {"golden": {"action": {"q01": [-0.5, -0.4, -0.3, -0.2, -0.1, -0.6, 0.0], "q99": [0.5, 0.6, 0.7, 0.8, 0.9, 0.4, 1.0],
                                    "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
PREDICT_PROMPT = 13            # prompt ids of the batch-1 call (token 0 included)


def _with(cfg, **kw):
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def case(name):
    """-> (cfg, W, batch, predict inputs), all on CPU.  W: bf16 tensors under the engine's / oracle's names; batch: the
    collator's fields with pixels and proprio already bf16-representable (finetune.py:339 and action_heads.py:53 round them;
    the fixture's targets replace batch["actions"]); predict: (ids [1, PREDICT_PROMPT], pixels [1, C, H, W], proprio ndarray)."""
    make_cfg, B, P, ragged, ws, bs = CASES[name]
    cfg = make_cfg()
    W = S.make_weights(cfg, "cpu", seed=ws, std=0.05)
    batch = S.make_batch(cfg, B, "cpu", seed=bs, P=P, ragged=ragged)
    batch["pixel_values"], batch["proprio"] = bf16(batch["pixel_values"]), bf16(batch["proprio"])
    g = torch.Generator().manual_seed(bs + 1000)
    ids = torch.randint(3, cfg.llm.vocab - 300, (1, PREDICT_PROMPT), generator=g)
    px = bf16(torch.randn(1, batch["pixel_values"].shape[1], cfg.vit[0].img, cfg.vit[0].img, generator=g).clamp_(-3, 3))
    proprio = bf16(torch.rand(cfg.proprio_dim, generator=g) * 2 - 1).numpy()
    return cfg, W, batch, (ids, px, proprio)


def reference_state_dict(W, cfg):
    """The VLM weights under the reference's HF key layout (what vla.state_dict() holds), fp32."""
    return {k: v.float() for k, v in CK.merge_reference_state_dict(W, cfg).items()}


def digest(cfg, W, batch, predict):
    h = hashlib.sha256()
    items = [("w." + k, v) for k, v in sorted(reference_state_dict(W, cfg).items())]
    items += [("head." + k, v) for k, v in sorted(W["head"].items())] + [("proprio." + k, v) for k, v in sorted(W["proprio"].items())]
    items += [("b." + k, v) for k, v in sorted(batch.items()) if k != "actions"]
    items += [("p.ids", predict[0]), ("p.px", predict[1]), ("p.proprio", torch.from_numpy(predict[2]))]
    for k, v in items:
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().float().cpu().numpy() if v.is_floating_point() else v.cpu().numpy()).tobytes())
    return h.hexdigest()


def load(name):
    """Both files of one fixture as one dict: tensors, strings as numpy."""
    out = {}
    for suffix in ("", "_hs"):
        z = np.load(os.path.join(GOLDEN, f"vla_{name}{suffix}.npz"))
        for k in z.files:
            out[k] = z[k] if z[k].dtype.kind == "U" else torch.from_numpy(z[k])
    return out


def fixture(name):
    """(cfg, W, batch, predict inputs, fixture) with the fixture's targets in the batch; fails if the seeds drifted."""
    cfg, W, batch, pred_in = case(name)
    z = load(name)
    assert str(z["digest"]) == digest(cfg, W, batch, pred_in), f"vla_{name}: regenerated inputs differ from the fixture's"
    batch["actions"] = z["actions"].clone()
    return cfg, W, batch, pred_in, z


def hidden_states(z):
    return [z[f"hs.{i}"] for i in range(int(z["n_states"]))]


def regroup_from_rows(hs, rows):
    """The reference's regrouped multi-layer states rebuilt from its recorded row selection: [B, n+1, Np + 64, D]."""
    B = rows.shape[0]
    return torch.stack([torch.stack([h[b, rows[b].long()] for b in range(B)]) for h in hs], dim=1)


def grad_keys(z):
    """Reference names of the gradients the fixture keeps element by element (8-row slices of the larger matrices)."""
    return sorted(k[2:] for k in z if k.startswith("g."))


def norm_keys(z):
    return sorted(k[3:] for k in z if k.startswith("gn."))


# ---------------------------------------------------------------------------------------------- the oracle on a fixture's weights
def oracle_cfg(cfg):
    return dict(vit=[v.as_oracle() for v in cfg.vit], fused=cfg.fused, llm=cfg.llm.as_oracle(), n_img=cfg.n_img, pro=cfg.pro,
                num_blocks=cfg.num_blocks)


def oracle_weights(W, requires_grad=False):
    """W (engine names) as the oracle's fp32 weight dict; requires_grad: every tensor a fresh leaf."""
    leaf = lambda t: t.float().clone().requires_grad_(requires_grad)
    sd = lambda d: {k: leaf(v) for k, v in d.items()}
    llm = sd(W["llm"])
    return dict(vit=[sd(s) for s in W["vit"]], proj=sd(W["proj"]), llm=llm, embed=llm["embed_tokens.weight"],
                action_queries=leaf(W["action_queries"]), head=sd(W["head"]), proprio=sd(W["proprio"]))


def oracle_grad(OW, name):
    """The gradient of the oracle leaf behind a reference state-dict name (the fixture's names, and those of
    FullFinetune.reference_named_gradients)."""
    for pre, d in (("head.", OW["head"]), ("proprio.", OW["proprio"]), ("projector.", OW["proj"]), ("language_model.model.", OW["llm"]),
                   ("vision_backbone.featurizer.", OW["vit"][0]), ("vision_backbone.fused_featurizer.", OW["vit"][-1])):
        if name.startswith(pre):
            return d[name[len(pre):]].grad
    assert name == "action_queries.weight", f"no oracle tensor behind {name}"
    return OW["action_queries"].grad


# ---------------------------------------------------------------------------------------------- LoRA on the same geometries
# peft LoraConfig(r, lora_alpha=2r, target_modules="all-linear") (vla-scripts/finetune.py:832-844) computes y = W x + b + 2 B(A x):
# in exact arithmetic the plain Linear with W_eff = W + 2 B A.  tools/make_golden_vla.py runs the reference's glue with W_eff in every
# adapted Linear and derives the adapter gradients from that run's weight gradient: dA = 2 B^T dW_eff, dB = 2 dW_eff A^T.
# name -> (geometry case, rank, seed of A and B, B scale: 0 is the state right after init_lora_weights="gaussian")
LORA_CASES = {
    "lora_fused1_r8": ("fused1", 8, 41, 1.0),       # rank 8: zero-padded to 64 in the native build (the padding path)
    "lora_siglip_r8": ("siglip", 8, 42, 1.0),       # the original (non-Pro) head block
    "lora_fused2_r64": ("fused2", 64, 43, 1.0),     # two images, rank 64 (no padding)
    "lora_siglip_b0": ("siglip", 8, 44, 0.0),       # B = 0: the wrapped model is the base model, dA = 0 exactly
}
LORA_SCALE = 2.0                                    # lora_alpha / r
# B ~ N(0, (B_STD sqrt(r))^2) and A ~ N(0, (1/r)^2): |2 B A| ~ 2 B_STD |W| / 0.05 ~ 0.3 |W| for the std-0.05 weights of case()
B_STD = 0.0075
# rows of W_eff kept for the merge check (merge_and_unload's result): module -> first row
MERGED_ROWS = 16
LORA_ROWS = 4        # adapter gradients kept element by element: 4 rows of every dA [r, in] and dB [out, r], spread over the rows


def lora_rows(n):
    """The rows of an n-row adapter gradient the fixture keeps (dB: across q | k | v and every projection)."""
    return slice(0, None, max(1, n // LORA_ROWS))
MERGED = {"projector.fc1": 0, "language_model.model.layers.0.self_attn.k_proj": 0, "language_model.model.layers.1.mlp.up_proj": 0,
          "vision_backbone.featurizer.blocks.0.attn.qkv": None}          # None: the first rows of the k block


def lora_targets(cfg, W):
    """[(module name under the reference's layout, base weight tensor of W)] for every Linear of the VLM that "all-linear" wraps:
    each ViT block's attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 (timm names; the last block too, which no forward reaches), the
    projector's fc layers, each LLM layer's seven projections; not lm_head (the output embedding)."""
    out = []
    for pre, w in zip(("vision_backbone.featurizer.", "vision_backbone.fused_featurizer."), W["vit"]):
        for i in range(len([k for k in w if k.endswith(".attn.qkv.weight")])):
            out += [(f"{pre}blocks.{i}.{n}", w[f"blocks.{i}.{n}.weight"]) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
    out += [(f"projector.{k[:-7]}", v) for k, v in W["proj"].items() if k.endswith(".weight")]
    for i in range(cfg.llm.n_layers):
        out += [(f"language_model.model.layers.{i}.{n}", W["llm"][f"layers.{i}.{n}.weight"]) for n in (
            "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")]
    return out


def lora_case(name):
    """-> (cfg, W, batch, predict inputs, rank, AB): the geometry case's weights and batch, and per adapted module (A [r, in], B [out, r])
    drawn from the case's seed, bf16-representable fp32 (the native trainer holds them in bf16)."""
    geo, r, seed, bscale = LORA_CASES[name]
    cfg, W, batch, pred_in = case(geo)
    g = torch.Generator().manual_seed(seed)
    AB = {}
    for mod, w in lora_targets(cfg, W):
        A = bf16(torch.randn(r, w.shape[1], generator=g) / r)                                  # init_lora_weights="gaussian"
        AB[mod] = (A, bf16(torch.randn(w.shape[0], r, generator=g) * (B_STD * r ** 0.5 * bscale)))
    return cfg, W, batch, pred_in, r, AB


def effective_weights(W, AB):
    """W with W_eff = W + 2 B A (float64, then fp32) in every adapted Linear: what a peft Linear computes, as one plain Linear."""
    We = dict(W, vit=[dict(w) for w in W["vit"]], proj=dict(W["proj"]), llm=dict(W["llm"]))
    groups = {"vision_backbone.featurizer.": We["vit"][0], "projector.": We["proj"], "language_model.model.": We["llm"]}
    if len(We["vit"]) > 1:
        groups["vision_backbone.fused_featurizer."] = We["vit"][1]
    for mod, (A, B) in AB.items():
        pre = next(p for p in groups if mod.startswith(p))
        k = mod[len(pre):] + ".weight"
        groups[pre][k] = (groups[pre][k].double() + LORA_SCALE * (B.double() @ A.double())).float()
    return We


def lora_digest(cfg, W, batch, predict, AB):
    h = hashlib.sha256(digest(cfg, W, batch, predict).encode())
    for k in sorted(AB):
        for t in AB[k]:
            h.update(k.encode())
            h.update(np.ascontiguousarray(t.numpy()).tobytes())
    return h.hexdigest()


def lora_key(mod, which):
    """peft's saved adapter key (lora_adapter/adapter_model.safetensors): which in ("A", "B")."""
    return f"base_model.model.{mod}.lora_{which}.weight"


def lora_fixture(name):
    """(cfg, W, batch, rank, AB, fixture) with the fixture's targets in the batch; fails if the seeds drifted."""
    cfg, W, batch, pred_in, r, AB = lora_case(name)
    z = load(name)
    assert str(z["digest"]) == lora_digest(cfg, W, batch, pred_in, AB), f"vla_{name}: regenerated inputs differ from the fixture's"
    batch["actions"] = z["actions"].clone()
    return cfg, W, batch, r, AB, z


def merged_rows(cfg, mod):
    """First row of the kept W_eff slice of MERGED's module."""
    lo = MERGED[mod]
    return cfg.vit[0].d if lo is None else lo


def oracle_lora(OW, AB, requires_grad=False):
    """Register AB with the oracle (oracle.LORA: id of the base weight leaf -> (A, B, 2)); returns {module: (A, B)} as fresh fp32
    leaves.  The caller clears O.LORA."""
    from oracle import vla_oracle as O
    groups = {"vision_backbone.featurizer.": OW["vit"][0], "vision_backbone.fused_featurizer.": OW["vit"][-1], "projector.": OW["proj"],
              "language_model.model.": OW["llm"]}
    leaves = {}
    for mod, (A, B) in AB.items():
        pre = next(p for p in groups if mod.startswith(p))
        a, b = (t.float().clone().requires_grad_(requires_grad) for t in (A, B))
        O.LORA[id(groups[pre][mod[len(pre):] + ".weight"])] = (a, b, LORA_SCALE)
        leaves[mod] = (a, b)
    return leaves


def half_ulp_excess(got, ref):
    """max over elements of |got - ref| / (half a bf16 ulp at ref): <= 1 when got is ONE rounding to bf16 of an fp32 value of ref
    (plus fp32 slack of 2^-20 relative)."""
    ref = ref.double()
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return ((got.double() - ref).abs() / (2.0 ** (e - 8) + 2.0 ** -20 * ref.abs())).max().item()
