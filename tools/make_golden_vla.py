#!/usr/bin/env python3
"""tests/golden/vla_{fused1,fused2,siglip}{,_hs}.npz: the reference's OWN multimodal glue, run on CPU in fp32 (build container only:
the reference checkout does not exist on the GPU machines).  The fixtures are data; no reference text is copied into this file
or into them.

What runs is the reference's code:
  * prismatic/extern/hf/modeling_prismatic.py: OpenVLAForActionPrediction.forward (action queries written over the action
    positions, patches after token 0, multimodal attention mask), PrismaticVisionBackbone.forward (fused and multi-image
    channel split, feature concatenation), PrismaticProjector, and predict_action (placeholder and stop ids, fake labels,
    the NUM_PATCHES + NUM_PROMPT_TOKENS slice, q01 / q99 un-normalisation under the mask).  The module imports once `timm` is a
    small stand-in in sys.modules (a version string, a module spec, a LayerScale class and a create_model that is never
    called); the model objects are assembled with __new__ + nn.Module.__init__, so no timm backbone is ever asked for.
  * vla-scripts/finetune.py: run_forward_pass, taken out of the script with `ast` in memory and executed against that model
    (the script itself needs draccus, tensorflow and more); its free names are bound here.
  * prismatic/models/action_heads.py L1RegressionActionHead, prismatic/models/projectors.py ProprioProjector.
Third-party stand-ins where the reference needs what is absent: installed transformers' Qwen2ForCausalLM for the language model,
SiglipVisionModel / Dinov2WithRegistersModel wrapped to return the hidden state behind block depth-2 without the prefix tokens
(timm's get_intermediate_layers(n={depth-2}) convention, pinned by tools/make_golden_vit.py), the timm-layout weights mapped in
by the inverse of that script's mapping.

The run is fp32: the bf16 casts the reference places on this path (autocast; `.to(torch.bfloat16)` of pixels, targets, proprio
and the action hidden states) are precision points, not glue, so the reference modules see a `torch` whose bfloat16 is float32
and whose autocast does nothing (a CUDA autocast does nothing to CPU tensors either).  Pixels, proprio and targets are
bf16-representable, so the native engine sees the same inputs.  The targets are placed 0.1 - 0.5 away from the reference's own
prediction (a no-grad pass first), so every run compared with this one has the same L1 gradient signs.

Weights and batches come from seeds (tests/vla_golden.py); each fixture keeps their digest.  Stored: the targets; the hidden
states (vla_*_hs.npz); projector input and output; the multimodal attention mask; the row of the hidden states each regrouped
state was taken from; predicted actions, loss_value and the two L1 metrics; after loss.backward(), the gradient of the action
head, proprio projector, projector, action queries, LLM layer 0 and ViT block 0 of each backbone element by element (8-row
slices of matrices above 16384 elements), the norm of every parameter's gradient and the row norms of the embedding table's;
one batch-1 predict_action call: its prepared ids, attention mask, fake labels and multimodal mask, un-normalised and normalised
actions and actions_hidden_states.

vla_lora_*.npz (tests/vla_golden.LORA_CASES): the same run with W_eff = W + 2 B A in every Linear peft's target_modules="all-linear"
wraps (adapted_modules: every nn.Linear of the VLM but get_output_embeddings()), A and B drawn from seeds; stored: the forward taps,
loss and metrics as above, per adapted module dA = 2 B^T dW_eff and dB = 2 dW_eff A^T (float64 from the run's fp32 weight gradients;
4 rows each and the norm), the gradients of the head, proprio projector and action queries, 16 rows of W_eff of a few Linears, the
adapted module list, the modules no forward reaches, and the trainable parameter names under peft (finetune.py:832-844).
    python tools/make_golden_vla.py [--ref PATH]
"""
import argparse
import ast
import contextlib
import importlib
import importlib.machinery
import io
import os
import sys
import types
import zipfile
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vla_golden as VG  # noqa: E402

FULL = 16384          # gradients kept whole up to this many elements, else their first ROWS rows
ROWS = 8
CASE_SEEDS = {"fused1": 101, "fused2": 102, "siglip": 103}      # target placement
LORA_SEEDS = {"lora_fused1_r8": 111, "lora_siglip_r8": 113, "lora_fused2_r64": 112, "lora_siglip_b0": 114}


class _Fp32Torch(types.ModuleType):
    """`torch` as the reference modules see it in the fp32 run: bfloat16 is float32, autocast does nothing."""

    def __getattr__(self, name):
        if name == "bfloat16":
            return torch.float32
        if name == "autocast":
            return lambda *a, **k: contextlib.nullcontext()
        return getattr(torch, name)


F32 = _Fp32Torch("torch")


def import_reference(ref):
    import transformers  # noqa: F401  (first: its optional-dependency probes must not see the stand-in)
    sys.path.insert(0, ref)
    for name in ("prismatic", "prismatic.vla", "prismatic.models", "prismatic.training", "prismatic.extern", "prismatic.extern.hf"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref, *name.split("."))]
        sys.modules[name] = m
    timm, models, vt = (types.ModuleType(n) for n in ("timm", "timm.models", "timm.models.vision_transformer"))
    timm.__version__, timm.__spec__ = "0.9.10", importlib.machinery.ModuleSpec("timm", None)

    class LayerScale(nn.Module):
        pass

    def create_model(*a, **k):
        raise RuntimeError("the featurizers are stand-ins: no timm model is built")

    vt.LayerScale, timm.create_model, timm.models, models.vision_transformer = LayerScale, create_model, models, vt
    sys.modules.update({"timm": timm, "timm.models": models, "timm.models.vision_transformer": vt})
    return {n.split(".")[-1]: importlib.import_module(n) for n in (
        "prismatic.vla.constants", "prismatic.training.train_utils", "prismatic.models.action_heads", "prismatic.models.projectors",
        "prismatic.extern.hf.modeling_prismatic")}


def extract_run_forward_pass(ref, R):
    tree = ast.parse(open(os.path.join(ref, "vla-scripts", "finetune.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run_forward_pass")
    tu = R["train_utils"]
    g = dict(torch=F32, NUM_TOKENS=R["constants"].NUM_TOKENS, get_current_action_mask=tu.get_current_action_mask,
             get_next_actions_mask=tu.get_next_actions_mask, compute_token_accuracy=None, compute_actions_l1_loss=None,
             CausalLMOutputWithPast=None, Dict=Dict, Tuple=Tuple)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "run_forward_pass", "exec"), g)
    return g["run_forward_pass"]


# ---------------------------------------------------------------------------------------------- third-party stand-ins
class Featurizer(nn.Module):
    """A timm featurizer as the reference patches it (modeling_prismatic.py:140-142) over an HF model of the same architecture."""

    def __init__(self, hf, c):
        super().__init__()
        self.hf, self.depth, self.n_prefix = hf, c.depth, c.n_prefix
        self.embed_dim = c.d
        self.patch_embed = types.SimpleNamespace(num_patches=c.n_patches)

    def forward(self, x):
        return self.hf(pixel_values=x, output_hidden_states=True).hidden_states[self.depth - 1][:, self.n_prefix:]


def vit_stand_in(c, w):
    """-> (Featurizer over an HF model holding the timm-layout weights w, function returning its gradients in timm layout)."""
    from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel, SiglipVisionConfig, SiglipVisionModel
    siglip = c.n_prefix == 0
    if siglip:
        hc = SiglipVisionConfig(hidden_size=c.d, intermediate_size=c.mlp, num_hidden_layers=c.depth, num_attention_heads=c.heads,
                                image_size=c.img, patch_size=c.patch, hidden_act="gelu", layer_norm_eps=c.eps, attention_dropout=0.0,
                                vision_use_head=False)
        m = SiglipVisionModel._from_config(hc, attn_implementation="eager")
        pre = "" if "embeddings.patch_embedding.weight" in m.state_dict() else "vision_model."
        emb = {"patch_embed.proj.weight": pre + "embeddings.patch_embedding.weight", "patch_embed.proj.bias": pre + "embeddings.patch_embedding.bias",
               "pos_embed": pre + "embeddings.position_embedding.weight"}
        L = lambda i: f"{pre}encoder.layers.{i}."
        blk = {"norm1": "layer_norm1", "norm2": "layer_norm2", "attn.proj": "self_attn.out_proj", "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
        qkv, ls = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), {}
    else:
        assert c.layerscale and c.mlp % c.d == 0
        hc = Dinov2WithRegistersConfig(hidden_size=c.d, num_hidden_layers=c.depth, num_attention_heads=c.heads, mlp_ratio=c.mlp // c.d,
                                       image_size=c.img, patch_size=c.patch, num_register_tokens=c.n_prefix - 1, hidden_act="gelu",
                                       layer_norm_eps=c.eps, layerscale_value=1.0, qkv_bias=True, use_swiglu_ffn=False,
                                       attention_probs_dropout_prob=0.0, hidden_dropout_prob=0.0, drop_path_rate=0.0)
        m = Dinov2WithRegistersModel._from_config(hc, attn_implementation="eager")
        emb = {"patch_embed.proj.weight": "embeddings.patch_embeddings.projection.weight", "patch_embed.proj.bias": "embeddings.patch_embeddings.projection.bias",
               "pos_embed": "embeddings.position_embeddings", "cls_token": "embeddings.cls_token", "reg_token": "embeddings.register_tokens"}
        L = lambda i: f"encoder.layer.{i}."
        blk = {"norm1": "norm1", "norm2": "norm2", "attn.proj": "attention.output.dense", "mlp.fc1": "mlp.fc1", "mlp.fc2": "mlp.fc2"}
        qkv = ("attention.attention.query", "attention.attention.key", "attention.attention.value")
        ls = {"ls1.scale_factor": "layer_scale1.lambda1", "ls2.scale_factor": "layer_scale2.lambda1"}
    m = m.float().eval()
    pairs = [(t, h, None) for t, h in emb.items()]            # (timm key, HF key, rows of the timm tensor)
    for i in range(c.depth):
        t, h = f"blocks.{i}.", L(i)
        for a, b in blk.items():
            pairs += [(t + a + s, h + b + s, None) for s in (".weight", ".bias")]
        pairs += [(t + a, h + b, None) for a, b in ls.items()]
        for j, b in enumerate(qkv):
            pairs += [(t + "attn.qkv" + s, h + b + s, (j * c.d, (j + 1) * c.d)) for s in (".weight", ".bias")]
    sd = m.state_dict()
    for t, h, rows in pairs:
        src = w[t].float()
        if rows is not None:
            src = src[rows[0]:rows[1]]
        if t == "pos_embed" and not siglip:                   # HF's DINOv2 has a position for the cls token: zero (timm reg4: none)
            src = torch.cat([torch.zeros(1, 1, c.d), src], dim=1)
        sd[h] = src.reshape(sd[h].shape).clone()
    assert {t for t, _, _ in pairs} == set(w), set(w) ^ {t for t, _, _ in pairs}
    m.load_state_dict(sd)

    def timm_grads():
        P, out = dict(m.named_parameters()), {}
        for t, h, rows in pairs:
            g = P[h].grad
            if g is None:
                continue
            if t == "pos_embed":
                g = g.reshape(1, -1, c.d)[:, 0 if siglip else 1:]
            out.setdefault(t, []).append(g.reshape(-1, *w[t].shape[1:]) if rows is not None else g.reshape(w[t].shape))
        return {t: torch.cat(v, 0) for t, v in out.items()}

    f = Featurizer(m, c)
    f.timm_modules = {"hf." + h[:-7]: t[:-7] for t, h, _ in pairs if t.endswith(".weight")}      # HF module -> timm module
    return f, timm_grads


def qwen2(cfg, w):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    c = cfg.llm
    qc = Qwen2Config(hidden_size=c.d, intermediate_size=c.inter, num_hidden_layers=c.n_layers, num_attention_heads=c.heads,
                     num_key_value_heads=c.kv_heads, vocab_size=c.vocab, rms_norm_eps=c.eps, rope_theta=c.theta, max_position_embeddings=512,
                     tie_word_embeddings=False, attention_dropout=0.0)
    lm = Qwen2ForCausalLM._from_config(qc, attn_implementation="eager").eval().float()
    lm.model.load_state_dict({k: v.float() for k, v in w.items()})
    return lm


class _Ddp(nn.Module):
    """What finetune.py's DDP wrapper gives run_forward_pass: the head under `.module`."""

    def __init__(self, m):
        super().__init__()
        self.module = m


def build_reference(R, cfg, W):
    MP, ah, pj = R["modeling_prismatic"], R["action_heads"], R["projectors"]
    D = cfg.llm.d
    f32 = lambda d: {k: v.float() for k, v in d.items()}
    vb = MP.PrismaticVisionBackbone.__new__(MP.PrismaticVisionBackbone)
    nn.Module.__init__(vb)
    stand = [vit_stand_in(c, w) for c, w in zip(cfg.vit, W["vit"])]
    vb.use_fused_vision_backbone, vb.num_images_in_input, vb.embed_dim = cfg.fused, cfg.n_img, cfg.vis_dim
    vb.featurizer = stand[0][0]
    if cfg.fused:
        vb.fused_featurizer = stand[1][0]
    vla = MP.OpenVLAForActionPrediction.__new__(MP.OpenVLAForActionPrediction)
    nn.Module.__init__(vla)
    vla.config = types.SimpleNamespace(output_attentions=False, output_hidden_states=False, use_return_dict=True)
    vla.vision_backbone = vb
    vla.projector = MP.PrismaticProjector(cfg.fused, vision_dim=cfg.vis_dim, llm_dim=D)
    vla.projector.load_state_dict(f32(W["proj"]))
    vla.language_model = qwen2(cfg, W["llm"])
    vla.action_queries = nn.Embedding(R["constants"].NUM_TOKENS, D)
    with torch.no_grad():
        vla.action_queries.weight.copy_(W["action_queries"].float())
    vla.llm_dim, vla.norm_stats = D, VG.NORM_STATS
    vla.eval()
    head = ah.L1RegressionActionHead(input_dim=D, hidden_dim=D, action_dim=cfg.action_dim, num_task_tokens=cfg.n_patches,
                                     use_pro_version=cfg.pro)
    head.model = ah.MLPResNet(num_blocks=cfg.num_blocks, input_dim=D * cfg.action_dim, hidden_dim=D, output_dim=cfg.action_dim,
                              use_pro_version=cfg.pro)
    head.load_state_dict(f32(W["head"]))
    pp = pj.ProprioProjector(llm_dim=D, proprio_dim=cfg.proprio_dim)
    pp.load_state_dict(f32(W["proprio"]))
    return vla, head, pp, [s[1] for s in stand]


def _tap_head(head, taps, key):
    orig = head.predict_action

    def predict_action(mlhs, **kw):
        out = orig(mlhs, **kw)
        taps.update({"mlhs": mlhs.detach(), key: out.detach()})
        return out
    head.predict_action = predict_action


def train_run(R, rfp, cfg, W, batch, seed):
    """The reference's run_forward_pass on W: a no-grad pass that places the targets (seed), then the pass with loss.backward().
    -> (targets, taps, metrics, (vla, head, pp, ViT gradient getters))."""
    Np = cfg.n_patches

    def one_pass(actions, grad):
        vla, head, pp, vit_grads = build_reference(R, cfg, W)
        taps = {}
        vla.projector.register_forward_hook(lambda m, i, o: taps.update(vis=i[0].detach(), patches=o.detach()))
        vla.language_model.register_forward_pre_hook(lambda m, a, k: taps.update(mm_mask=k["attention_mask"].detach()), with_kwargs=True)
        vla.register_forward_hook(lambda m, i, o: taps.update(hs=[h.detach() for h in o.hidden_states], pf=o.projector_features.detach()))
        _tap_head(head, taps, "pred")
        with (contextlib.nullcontext() if grad else torch.no_grad()):
            loss, metrics = rfp(vla, _Ddp(head), pp, dict(batch, actions=actions), None, "cpu", True, True, False, Np, False, cfg.pro,
                                types.SimpleNamespace(phase="Inference"))
            if grad:
                loss.backward()
        return taps, metrics, (vla, head, pp, vit_grads)

    taps0, _, _ = one_pass(torch.zeros(batch["actions"].shape), False)
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, taps0["pred"].shape, generator=g) * 2 - 1
    actions = VG.bf16(taps0["pred"] + sign * (0.1 + 0.4 * torch.rand(taps0["pred"].shape, generator=g)))
    return (actions,) + one_pass(actions, True)


def forward_record(cfg, taps):
    """The forward taps every fixture keeps: projector input / output, multimodal mask, actions, the regroup as row indices."""
    out = dict(vis=taps["vis"].numpy(), patches=taps["patches"].numpy(), mm_mask=taps["mm_mask"].to(torch.uint8).numpy(),
               pred=taps["pred"].numpy(), n_states=np.array(len(taps["hs"])))
    assert torch.equal(taps["pf"], taps["patches"]) and len(taps["hs"]) == cfg.llm.n_layers + 1
    # the regroup as row indices: each regrouped state is one row of the hidden states (index ops only, exact copies)
    hs, mlhs = taps["hs"], taps["mlhs"]
    B = hs[0].shape[0]
    eq = torch.stack([(hs[-1][b][None, :, :] == mlhs[b, -1][:, None, :]).all(-1) for b in range(B)])    # [B, Np+64, S]
    assert (eq.sum(-1) == 1).all(), "every regrouped state must match exactly one hidden-state row"
    rows = eq.float().argmax(-1)
    assert torch.equal(VG.regroup_from_rows(hs, rows), mlhs)
    out["rows"] = rows.to(torch.int16).numpy()
    return out


def named_gradients(vla, head, pp, vit_grads):
    """Every gradient of the run under the reference's state-dict names (ViTs in timm layout)."""
    named = {}
    for pre, fn in zip(("vision_backbone.featurizer.", "vision_backbone.fused_featurizer."), vit_grads):
        named.update({pre + k: v for k, v in fn().items()})
    for mod, pre in ((vla.projector, "projector."), (vla.language_model.model, "language_model.model."), (head, "head."), (pp, "proprio.")):
        named.update({pre + k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    named["action_queries.weight"] = vla.action_queries.weight.grad
    return named


def run_case(name, R, rfp):
    cfg, W, batch, (pids, ppx, pprop) = VG.case(name)
    actions, taps, metrics, (vla, head, pp, vit_grads) = train_run(R, rfp, cfg, W, batch, CASE_SEEDS[name])
    out = dict(digest=np.array(VG.digest(cfg, W, batch, (pids, ppx, pprop))), actions=actions.numpy(),
               input_ids=batch["input_ids"].numpy(), labels=batch["labels"].numpy(), attention_mask=batch["attention_mask"].numpy(),
               metrics=np.array([metrics["loss_value"], metrics["curr_action_l1_loss"], metrics["next_actions_l1_loss"]], np.float64))
    out.update(forward_record(cfg, taps))
    hs = taps["hs"]
    # gradients under the reference's state-dict names
    named = named_gradients(vla, head, pp, vit_grads)
    keep = lambda k: k.startswith(("head.", "proprio.", "projector.", "action_queries")) or ".layers.0." in k or ".blocks.0." in k
    for k, v in named.items():
        out["gn." + k] = np.array(v.double().norm().item())
        if keep(k):
            out["g." + k] = (v if v.numel() <= FULL else v[:ROWS]).numpy()
    out["grow.language_model.model.embed_tokens.weight"] = named["language_model.model.embed_tokens.weight"].norm(dim=1).numpy()
    # one batch-1 predict_action call (phase Inference, modeling_prismatic.py:892-972)
    vla, head, pp, _ = build_reference(R, cfg, W)
    taps = {}
    _tap_head(head, taps, "normalized")
    # the prepared batch: ids + placeholders + stop id, extended mask, fake labels (what the forward then runs on)
    prep_in, prep_lab = vla._prepare_input_for_action_prediction, vla._prepare_labels_for_action_prediction

    def prepare_input(*a):
        out = prep_in(*a)
        taps.update(p_ids=out[0], p_am=out[1])
        return out

    def prepare_labels(*a):
        out = prep_lab(*a)
        taps.update(p_labels=out.clone())
        return out
    vla._prepare_input_for_action_prediction, vla._prepare_labels_for_action_prediction = prepare_input, prepare_labels
    vla.language_model.register_forward_pre_hook(lambda m, a, k: taps.update(p_mm_mask=k["attention_mask"].detach()), with_kwargs=True)
    with torch.no_grad():
        act, hid = vla.predict_action(input_ids=pids, unnorm_key="golden", proprio=pprop, proprio_projector=pp, action_head=head,
                                      pixel_values=ppx, attention_mask=torch.ones_like(pids, dtype=torch.bool))
    out.update({"p.actions": np.asarray(act, np.float64), "p.hidden": hid.numpy(), "p.normalized": taps["normalized"].numpy(),
                "p.input_ids": taps["p_ids"].numpy(), "p.attention_mask": taps["p_am"].numpy(), "p.labels": taps["p_labels"].numpy(),
                "p.mm_mask": taps["p_mm_mask"].to(torch.uint8).numpy()})
    return out, {f"hs.{i}": h.numpy() for i, h in enumerate(hs)}


def adapted_modules(vla):
    """peft's target_modules="all-linear" on the built VLM: every nn.Linear but get_output_embeddings(), under the reference's
    module names (the ViT stand-ins' HF q / k / v map to timm's one fused attn.qkv)."""
    out_emb, names = vla.get_output_embeddings(), []
    for n, m in vla.named_modules():
        if not isinstance(m, nn.Linear) or m is out_emb:
            continue
        for pre in ("vision_backbone.featurizer.", "vision_backbone.fused_featurizer."):
            if n.startswith(pre):
                n = pre + vla.get_submodule(pre[:-1]).timm_modules[n[len(pre):]]
        if n not in names:
            names.append(n)
    return names


def run_lora_case(name, R, rfp):
    """The reference's run with W_eff = W + 2 B A in every adapted Linear; adapter gradients from its fp32 weight gradients."""
    cfg, W, batch, pred_in, r, AB = VG.lora_case(name)
    We = VG.effective_weights(W, AB)
    actions, taps, metrics, (vla, head, pp, vit_grads) = train_run(R, rfp, cfg, We, batch, LORA_SEEDS[name])
    mods = adapted_modules(vla)
    assert mods == [m for m, _ in VG.lora_targets(cfg, W)], "the adapted set differs from tests/vla_golden.lora_targets"
    out = dict(digest=np.array(VG.lora_digest(cfg, W, batch, pred_in, AB)), actions=actions.numpy(),
               metrics=np.array([metrics["loss_value"], metrics["curr_action_l1_loss"], metrics["next_actions_l1_loss"]], np.float64))
    out.update(forward_record(cfg, taps))
    del out["vis"]
    named = named_gradients(vla, head, pp, vit_grads)
    dead = [m for m in mods if m + ".weight" not in named]             # no forward reaches them (the ViTs' last block)
    assert all(".blocks." in m for m in dead), dead
    for m in mods:
        if m in dead:
            continue
        A, B = (t.double() for t in AB[m])
        dW = named[m + ".weight"].double()
        for which, g in (("A", VG.LORA_SCALE * B.t() @ dW), ("B", VG.LORA_SCALE * dW @ A.t())):
            k = VG.lora_key(m, which)
            out["gn." + k] = np.array(g.norm().item())
            out["g." + k] = g[VG.lora_rows(g.shape[0])].float().numpy()
    # the parameters that train outside the adapters: the action head, the proprio projector (modules of their own) and the
    # action queries (finetune.py:841-843)
    for k, v in named.items():
        if k.startswith(("head.", "proprio.", "action_queries")):
            out["gn." + k] = np.array(v.double().norm().item())
            out["g." + k] = (v if v.numel() <= FULL else v[:ROWS]).numpy()
    for m in VG.MERGED:                                                 # what merge_and_unload writes (fp32 here)
        lo = VG.merged_rows(cfg, m)
        w = dict(VG.lora_targets(cfg, We))[m]
        out["merged." + m] = w[lo:lo + VG.MERGED_ROWS].numpy()
    out["lora_modules"], out["lora_dead"] = np.array(mods), np.array(dead)
    out["trainable"] = np.array([f"base_model.model.{m}.lora_{w}.default.weight" for m in mods for w in "AB"]
                                + ["base_model.model.action_queries.weight"])
    return out, {f"hs.{i}": h.numpy() for i, h in enumerate(taps["hs"])}


def save(path, arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), a.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--only", nargs="*", default=list(VG.CASES) + list(VG.LORA_CASES))
    args = ap.parse_args()
    torch.set_num_threads(1)                  # one summation order: the same fixture on every run
    R = import_reference(args.ref)
    rfp = extract_run_forward_pass(args.ref, R)
    R["modeling_prismatic"].torch = R["action_heads"].torch = F32      # the fp32 run (module docstring)
    for name in args.only:
        out, hs = (run_lora_case if name in VG.LORA_CASES else run_case)(name, R, rfp)
        save(os.path.join(VG.GOLDEN, f"vla_{name}.npz"), out)
        save(os.path.join(VG.GOLDEN, f"vla_{name}_hs.npz"), hs)
        print(name, [os.path.getsize(os.path.join(VG.GOLDEN, f"vla_{name}{s}.npz")) for s in ("", "_hs")], "bytes;",
              "loss_value / curr / next", out["metrics"].tolist())


if __name__ == "__main__":
    main()
