"""The LoRA trainer against the reference's OWN run (tests/golden/vla_lora_*.npz, tools/make_golden_vla.py): peft's Linear computes
y = W x + b + 2 B(A x), in exact arithmetic the plain Linear with W_eff = W + 2 B A, so the reference's run_forward_pass on W_eff gives
the forward, and its fp32 weight gradient the adapter gradients (dA = 2 B^T dW_eff, dB = 2 dW_eff A^T).  tests/test_lora_gpu.py and
tests/test_layer_gradients_gpu.py compare the trainer with oracle.lora_linear, our own restatement; a misreading both share (the
scale, the adapted set, gate / up or q / k / v blocks of B_blk and A_cat, rank padding) passes those and fails here.

Budgets of tests/test_vla_golden_gpu.py: |native - reference fp32| <= factor x |oracle(emu) - reference fp32| + floor, where oracle(emu)
is the bf16-emulating oracle in the native build's form (LORA_FUSED) on the same weights, adapters and batch.  Each check is also fed
one deliberately wrong result (rolled by one row, a halved scale, exchanged gate / up gradients, a zeroed q|k|v pair) and must fail."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from oracle import vla_oracle as O  # noqa: E402
from test_engine_gpu import budget, budget_family  # noqa: E402
from test_vla_golden_gpu import _dev, _forward_checks, _grad_checks, _metric_checks  # noqa: E402
import vla_golden as VG  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
CASES = list(VG.LORA_CASES)
PRE = "base_model.model."


def _load(name):
    """Engine weights from the reference-layout state dict (geometry read off it), the case's adapters and the fixture."""
    from vla_adapter_amd import checkpoints as CK
    cfg0, W, batch, r, AB, z = VG.lora_fixture(name)
    sd = {k: v.to(BF) for k, v in VG.reference_state_dict(W, cfg0).items()}
    cfg = CK.infer_config(sd)
    cfg.n_img, cfg.pro = cfg0.n_img, cfg0.pro                      # not held by a state dict
    assert cfg == cfg0, (cfg, cfg0)
    Wd = _dev(CK.split_reference_state_dict(sd, cfg, head=W["head"], proprio=W["proprio"]))
    return cfg, W, Wd, batch, r, AB, z


def _oracle_emu(cfg, W, batch, AB):
    """The bf16-emulating oracle with the adapters in the native build's form (low-rank branch inside the base accumulator)."""
    OW = VG.oracle_weights(W, requires_grad=True)
    O.LORA.clear()
    leaves = VG.oracle_lora(OW, AB, requires_grad=True)
    O.LORA_FUSED = True
    try:
        out = O.vla_forward(batch, OW, VG.oracle_cfg(cfg), emu=True)
        out["loss"].backward()
    finally:
        O.LORA.clear()
        O.LORA_FUSED = False
    return out, OW, leaves


def _module(l, p):
    return f"{l.name}.{p}"[len(PRE):]


def _native_adapter_grads(lo):
    """{peft key: gradient} without padding; every padded entry (rank padding, the ViT MLP's width padding) has NO gradient."""
    out = {}
    for l in lo.L.values():
        for p, _ in l.projs:
            gA, gB = lo.P.g(f"{l.name}.{p}.lora_A"), lo.P.g(f"{l.name}.{p}.lora_B")
            assert not gA[l.r:].any() and not gA[:, l.k_real:].any(), f"{l.name}.{p}: gradient on A's padding"
            assert not gB[:, l.r:].any() and not gB[l.n_real:].any(), f"{l.name}.{p}: gradient on B's padding"
            out[VG.lora_key(_module(l, p), "A")] = gA[:l.r, :l.k_real].float().cpu()
            out[VG.lora_key(_module(l, p), "B")] = gB[:l.n_real, :l.r].float().cpu()
    return out


def _paddings_are_zero(lo):
    for l in lo.L.values():
        for p, _ in l.projs:
            A, Bm = lo.P.view(f"{l.name}.{p}.lora_A"), lo.P.view(f"{l.name}.{p}.lora_B")
            assert not A[l.r:].any() and not A[:, l.k_real:].any() and not Bm[:, l.r:].any() and not Bm[l.n_real:].any(), \
                f"{l.name}.{p}: a padded adapter entry holds a value"


def _adapter_checks(native, leaves, z, what, roll=False):
    """Kept rows of every live dA / dB element by element (the A's and the B's each a family), the norm of every one; B = 0 cases
    carry dA = 0 exactly (checked by the caller).  roll: the native rows rolled by one (slices only)."""
    dead = set(z["lora_dead"].tolist())
    fam, norms = {"A": [], "B": []}, []
    for mod, (a, b) in leaves.items():
        if mod in dead:
            continue
        for which, e in (("A", a.grad), ("B", b.grad)):
            k = VG.lora_key(mod, which)
            t = z["g." + k]
            if not t.any():
                continue
            g = native[k]
            rows = VG.lora_rows(g.shape[0])
            fam[which].append((k, torch.roll(g[rows], 1, 0) if roll else g[rows], e[rows], t))
            norms.append((k, g.double().norm().reshape(1), e.double().norm().reshape(1), z["gn." + k].reshape(1)))
    assert fam["B"], "every live adapter has a dB"
    gmax = max(t.norm().item() for v in fam.values() for _, _, _, t in v)
    for which, items in fam.items():
        if items:
            budget_family(items, f"{what}: d{which} (kept rows)", each=3.0, total=1.5, floor=5e-3, absfloor=1e-3 * gmax)
    if not roll:
        # the kept rows sit 0.1 - 0.35 (relative) from the fp32 run on both sides (bf16 through the LLM and the head): a single norm
        # is one realisation of that noise - measured on the MI355X 1.4e-2 where the emulation landed at 2.2e-3 (fused1,
        # fused_featurizer qkv dA) - hence the 2e-2 floor of test_vla_golden_gpu's head norms
        budget_family(norms, f"{what}: adapter gradient norms", each=3.0, total=1.5, floor=2e-2)


def _trained_checks(eng, OW, z, what):
    """The gradients of what trains beside the adapters: action head, proprio projector (bounds of test_vla_golden_gpu's adapter
    step: the head's bf16 noise), action queries."""
    head, prop = eng.head.named_views(eng.head.P.grad), eng.head.proprio_views(eng.head.P.grad)
    names = [k for k in VG.norm_keys(z) if k.startswith(("head.", "proprio."))]
    assert names and all((k[5:] in head) if k.startswith("head.") else (k[8:] in prop) for k in names)
    native_of = lambda k: head[k[5:]] if k.startswith("head.") else prop[k[8:]]
    # a gradient three orders of magnitude below the family's largest is a near-cancelling sum on the absolute noise floor: fused2's
    # block-0 gating factor is -2.3e-5 in the reference run, +3.6e-5 and -7.4e-5 in the oracle's two bf16 LoRA forms, and the
    # emulation's own distance moves between 0.2 and 2.2 with the CPU thread count.  Those are held to that floor instead.
    gn = {k: float(z["gn." + k]) for k in names}
    tiny = [k for k in names if gn[k] < 1e-3 * max(gn.values())]
    for k in tiny:
        d = abs(native_of(k).double().norm().item() - gn[k])
        print(f"{what} {k}: |norm - reference| {d:.2e} (reference {gn[k]:.2e}; floor {1e-3 * max(gn.values()):.2e})")
        assert d <= 1e-3 * max(gn.values()), (k, d)
    _grad_checks(native_of, OW, z, [k for k in names if k not in tiny], what, total=2.0, each=4.0, norm_floor=2e-2)
    aq = eng.head.P.g("action_queries")
    budget(aq, OW["action_queries"].grad, z["g.action_queries.weight"], f"{what}: action_queries gradient", factor=2.5)
    with pytest.raises(AssertionError):
        budget(torch.roll(aq, 1, 0), OW["action_queries"].grad, z["g.action_queries.weight"], f"{what}: action_queries rolled (must fail)",
               factor=2.5)


def _step_checks(cfg, eng, lo, pred, loss3, emu, OW, leaves, batch, AB, z, what):
    _metric_checks(loss3, pred, emu, batch, z, what)
    native = _native_adapter_grads(lo)
    _adapter_checks(native, leaves, z, what)
    for mod, (A, B) in AB.items():
        if not B.any() and mod not in set(z["lora_dead"].tolist()):
            assert not native[VG.lora_key(mod, "A")].any(), f"{what}: {mod}: B = 0, yet dA = 2 dt^T x is not exactly zero"
    _trained_checks(eng, OW, z, what)
    return native


def _merged_reference_rows(cfg, merged, mod):
    """A reference Linear's rows out of merged_weights() (engine names: fused q|k|v, gate / up interleaved in 16-row groups)."""
    c = cfg.llm
    H, KV, dh, I = c.heads, c.kv_heads, c.dh, c.inter
    if mod.startswith("projector."):
        return merged["proj." + mod.split(".")[1]]
    if mod.startswith("vision_backbone."):
        j = 0 if ".featurizer." in mod else 1
        i, n = mod.split(".blocks.")[1].split(".", 1)
        w = merged[f"vit{j}.{i}.{ {'attn.qkv': 'qkv', 'attn.proj': 'proj', 'mlp.fc1': 'fc1', 'mlp.fc2': 'fc2'}[n] }"]
        return w[:cfg.vit[j].mlp] if n == "mlp.fc1" else w
    i, n = mod.split(".layers.")[1].split(".", 1)
    qkv = {"self_attn.q_proj": (0, H * dh), "self_attn.k_proj": (H * dh, (H + KV) * dh), "self_attn.v_proj": ((H + KV) * dh, (H + 2 * KV) * dh)}
    if n in qkv:
        return merged[f"llm.{i}.qkv"][qkv[n][0]:qkv[n][1]]
    if n in ("mlp.gate_proj", "mlp.up_proj"):
        gu = merged[f"llm.{i}.gu"]
        return gu.view(I // 16, 2, 16, gu.shape[1])[:, int(n == "mlp.up_proj")].reshape(I, gu.shape[1])
    return merged[f"llm.{i}.{ {'self_attn.o_proj': 'o', 'mlp.down_proj': 'down'}[n] }"]


@pytest.mark.parametrize("name", CASES)
def test_lora_step_matches_the_reference_run(name):
    """LoRAFinetune on the case's weights with its adapters loaded (load_lora_state_dict): the adapted set and the trainable set,
    merged_weights() against the reference's W_eff, one eager step and one captured step against the reference run (forward values,
    loss and metrics, every adapter gradient, the head's, the proprio projector's and the action queries'), and after an update:
    every other VLM tensor unchanged, paddings still zero."""
    from vla_adapter_amd import checkpoints as CK, engine as E
    from vla_adapter_amd.lora_finetune import LoRAFinetune
    cfg, W, Wd, batch, r, AB, z = _load(name)
    eng = E.VLAEngine(cfg, Wd, DEV)
    lo = LoRAFinetune(eng, rank=r, seed=0)
    # --- the adapted set, one to one: every Linear of the VLM but lm_head, less what no forward reaches (the ViTs' last block,
    # behind the featurizer's output: the engine does not build it; the reference's adapter there keeps its initial value)
    sd = lo.lora_state_dict()
    mods = [k[len(PRE):-len(".lora_A.weight")] for k in sd if k.endswith(".lora_A.weight")]
    dead = set(z["lora_dead"].tolist())
    live = [m for m in z["lora_modules"].tolist() if m not in dead]
    assert len(set(mods)) == len(mods) and sorted(mods) == sorted(live), sorted(set(mods) ^ set(live))
    assert set(sd) == {VG.lora_key(m, w) for m in live for w in "AB"}
    trainable = {k.replace(".default.", ".") for k in z["trainable"].tolist() if not any(f".{d}.lora_" in k for d in dead)}
    assert trainable == set(sd) | {PRE + "action_queries.weight"}
    lo.load_lora_state_dict({VG.lora_key(m, w): t for m, (A, B) in AB.items() for w, t in (("A", A), ("B", B))})
    _paddings_are_zero(lo)
    assert all(torch.equal(sd2.cpu().float(), AB[k[len(PRE):-len(".lora_A.weight")]][0]) for k, sd2 in lo.lora_state_dict().items()
               if k.endswith(".lora_A.weight"))
    # --- merge_and_unload: W + 2 B A, one bf16 rounding of the fp32 sum per element
    merged = lo.merged_weights()
    for mod in VG.MERGED:
        lo_ = VG.merged_rows(cfg, mod)
        got = _merged_reference_rows(cfg, merged, mod)[lo_:lo_ + VG.MERGED_ROWS].cpu()
        ex = VG.half_ulp_excess(got, z["merged." + mod])
        print(f"{name} merged_weights {mod}: max |merged - W_eff| / half a bf16 ulp = {ex:.3f} (bound 1)")
        assert ex <= 1.0, (mod, ex)
        assert VG.half_ulp_excess(torch.roll(got, 1, 0), z["merged." + mod]) > 1.0, "merged rows rolled by one (must fail)"
    emu, OW, leaves = _oracle_emu(cfg, W, batch, AB)
    bd = _dev(batch)
    # --- one eager step
    pred = lo.forward(bd, None)
    torch.cuda.synchronize()
    _forward_checks(cfg, eng, pred, emu, z, f"{name} LoRA eager step")
    pred = pred.clone()
    loss3 = lo.backward(pred, bd["actions"])
    torch.cuda.synchronize()
    native = _step_checks(cfg, eng, lo, pred, loss3, emu, OW, leaves, batch, AB, z, f"{name} LoRA eager step")
    # the same checks on deliberately wrong gradients: rolled rows, the scale 1 (halves dA and dB), gate / up exchanged, a q|k|v pair's
    # dA zeroed
    with pytest.raises(AssertionError):
        _adapter_checks(native, leaves, z, f"{name}: rolled by one row (must fail)", roll=True)
    with pytest.raises(AssertionError):
        _adapter_checks({k: 0.5 * v for k, v in native.items()}, leaves, z, f"{name}: scale 1 (must fail)")
    g, u = (VG.lora_key(f"language_model.model.layers.1.mlp.{n}", "B") for n in ("gate_proj", "up_proj"))
    with pytest.raises(AssertionError):
        _adapter_checks(dict(native, **{g: native[u], u: native[g]}), leaves, z, f"{name}: gate / up dB exchanged (must fail)")
    if AB["language_model.model.layers.0.self_attn.k_proj"][1].any():
        k = VG.lora_key("language_model.model.layers.0.self_attn.k_proj", "A")
        with pytest.raises(AssertionError):
            _adapter_checks(dict(native, **{k: torch.zeros_like(native[k])}), leaves, z, f"{name}: k_proj dA zeroed (must fail)")
    # --- one captured step (lr 0: AdamW leaves every parameter as it is, so the replay runs on the same weights)
    state = [t.clone() for t in (lo.P.data, eng.head.P.data)]
    lo.capture(bd, None)
    loss3 = lo.train_step_graphed(0.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, (lo.P.data, eng.head.P.data))), "lr 0 must leave the parameters"
    pred = lo._pred
    _forward_checks(cfg, eng, pred, emu, z, f"{name} LoRA captured step")
    _step_checks(cfg, eng, lo, pred, loss3, emu, OW, leaves, batch, AB, z, f"{name} LoRA captured step")
    # --- an update moves the adapters, the head and the action queries, nothing else of the VLM
    before = CK.engine_vlm_state_dict(eng)
    lo.optimizer_step(1e-3)
    torch.cuda.synchronize()
    after = CK.engine_vlm_state_dict(eng)
    frozen = [k for k in before if k != "action_queries.weight"]
    changed = [k for k in frozen if not torch.equal(before[k], after[k])]
    assert not changed, f"frozen VLM tensors changed under LoRA: {changed[:5]}"
    assert not torch.equal(before["action_queries.weight"], after["action_queries.weight"]), "the action queries train"
    assert not torch.equal(state[0], lo.P.data) and not torch.equal(state[1], eng.head.P.data), "adapters and head train"
    _paddings_are_zero(lo)
