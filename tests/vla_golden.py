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
