"""The native engine against the reference's OWN run of the multimodal glue (tests/golden/vla_*.npz, tools/make_golden_vla.py): the
reference's run_forward_pass / predict_action in fp32 on seeded weights.  Every other model-level GPU test compares the engine
with oracle/vla_oracle.py; a misreading the engine and the oracle share (patch placement, channel order of a second image, the
regroup's off-by-one, predict_action's slice) passes those and fails here.

Budget rule of tests/test_engine_gpu.py: |native - reference fp32| <= factor x |oracle(emu) - reference fp32| + floor, where
oracle(emu) is the bf16-emulating oracle on the same weights and batch.  Gradients are kept as 8-row slices for the larger
matrices (and as norms for every tensor): single slices carry more rounding noise than whole tensors, hence each = 3 and a
5e-3 floor in the gradient families (the head's gradients need more; the bounds below say what was measured).  Every test also feeds its
checker one deliberately shifted result (states rolled by one token position) and requires it to fail."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from oracle import vla_oracle as O  # noqa: E402
from test_engine_gpu import budget, budget_family  # noqa: E402
import vla_golden as VG  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
CASES = list(VG.CASES)


def _dev(x):
    if isinstance(x, dict):
        return {k: _dev(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_dev(v) for v in x]
    return x.to(DEV)


def _load(name):
    """Engine weights from the reference-layout state dict, geometry read off it (checkpoints.infer_config)."""
    from vla_adapter_amd import checkpoints as CK
    cfg0, W, batch, pred_in, z = VG.fixture(name)
    sd = {k: v.to(BF) for k, v in VG.reference_state_dict(W, cfg0).items()}
    cfg = CK.infer_config(sd)
    cfg.n_img, cfg.pro = cfg0.n_img, cfg0.pro                      # not held by a state dict
    assert cfg == cfg0, (cfg, cfg0)
    Wd = _dev(CK.split_reference_state_dict(sd, cfg, head=W["head"], proprio=W["proprio"]))
    return cfg, W, Wd, batch, pred_in, z


def _oracle_emu(cfg, W, batch):
    OW = VG.oracle_weights(W, requires_grad=True)
    out = O.vla_forward(batch, OW, VG.oracle_cfg(cfg), emu=True)
    out["loss"].backward()
    return out, OW


def _forward_checks(cfg, eng, pred, emu, z, what):
    """Patches, every hidden state (valid positions), the head's regrouped states, actions; the rolled regroup must fail."""
    hs, valid = VG.hidden_states(z), z["mm_mask"].bool()
    Np, n, nb = cfg.n_patches, cfg.llm.n_layers, cfg.num_blocks
    HS = [eng.llm.HS[i].float().cpu() for i in range(n + 1)]
    budget(HS[0][:, 1:Np + 1], emu["patches"], z["patches"], f"{what}: projected patches")
    for i in range(n + 1):
        budget(HS[i][valid], emu["hidden_states"][i].detach()[valid], hs[i][valid], f"{what}: hidden_states[{i}]")
    # the regroup as the head reads it: task rows HS[i+1][:, :Np] in place, the 64 gathered action-query rows in h_adp[i]
    reg = torch.stack([torch.cat([HS[i + 1][:, :Np], eng.head.h_adp[i][:, :O.NUM_TOKENS].float().cpu()], dim=1) for i in range(nb)], 1)
    reg_t, reg_e = VG.regroup_from_rows(hs, z["rows"])[:, 1:nb + 1], emu["mlhs"].detach()[:, 1:nb + 1]
    budget(reg, reg_e, reg_t, f"{what}: regrouped multi-layer states")
    with pytest.raises(AssertionError):
        budget(torch.roll(reg, 1, dims=2), reg_e, reg_t, f"{what}: regrouped states rolled by one position (must fail)")
    budget(pred, emu["pred"], z["pred"], f"{what}: actions")


def _metric_checks(loss3, pred, emu, batch, z, what):
    """loss_value and the two L1 metrics.  A mean of |pred - target| moves by at most the mean of |pred - pred_ref| (triangle
    inequality), and pred itself is held to the budget: that bound, not a ratio of two scalars whose errors may cancel."""
    p, t = pred.float().cpu(), z["pred"]
    m = O.l1_metrics(emu["pred"].detach(), batch["actions"])
    e = [emu["loss"].item(), m["curr_action_l1_loss"].item(), m["next_actions_l1_loss"].item()]
    bounds = [(p - t).abs().mean().item(), (p[:, 0] - t[:, 0]).abs().mean().item(), (p[:, 1:] - t[:, 1:]).abs().mean().item()]
    for got, ee, ref, bd, k in zip(loss3.float().cpu().tolist(), e, z["metrics"].tolist(), bounds,
                                   ("loss_value", "curr_action_l1_loss", "next_actions_l1_loss")):
        print(f"{what} {k}: native {got:.6f}  oracle(emu) {ee:.6f}  reference {ref:.6f}  bound {bd:.2e}")
        assert abs(got - ref) <= bd + 1e-6 * abs(ref), (k, got, ref, bd)


def _grad_checks(native_of, OW, z, names, what, total=1.5, each=3.0, norm_floor=5e-3):
    """Kept slices element by element (families of matrices and of vectors) and the norm of every listed gradient."""
    items, norms = [], []
    for k in names:
        g = native_of(k)
        e = VG.oracle_grad(OW, k)
        g = g.float().cpu().reshape(e.shape)
        if "g." + k in z:
            t = z["g." + k]
            items.append((k, g[:t.shape[0]], e[:t.shape[0]], t))
        norms.append((k, g.double().norm().reshape(1), e.double().norm().reshape(1), z["gn." + k].reshape(1)))
    gmax = max(t.norm().item() for _, _, _, t in items)
    mats, vecs = [i for i in items if i[3].dim() >= 2], [i for i in items if i[3].dim() < 2]
    budget_family(mats, f"{what}: weight-matrix gradients (8-row slices)", each=each, total=total, floor=5e-3, absfloor=1e-3 * gmax)
    budget_family(vecs, f"{what}: bias / norm / gate gradients", each=each, total=total, floor=5e-3, absfloor=1e-3 * gmax)
    budget_family(norms, f"{what}: gradient norms", each=each, total=total, floor=norm_floor)


@pytest.mark.parametrize("name", CASES)
def test_adapter_step_matches_the_reference_run(name):
    """Adapter-only step (VLAEngine.forward + loss_and_backward): forward values, loss and L1 metrics, and the gradients of the
    action head, the proprio projector and the action queries (through the frozen LLM)."""
    from vla_adapter_amd import engine as E
    cfg, W, Wd, batch, _, z = _load(name)
    eng = E.VLAEngine(cfg, Wd, DEV)
    bd = _dev(batch)
    pred = eng.forward(bd, None)
    loss3 = eng.loss_and_backward(pred, bd["actions"])
    torch.cuda.synchronize()
    emu, OW = _oracle_emu(cfg, W, batch)
    _forward_checks(cfg, eng, pred, emu, z, f"{name} adapter step")
    _metric_checks(loss3, pred, emu, batch, z, f"{name} adapter step")
    head, prop = eng.head.named_views(eng.head.P.grad), eng.head.proprio_views(eng.head.P.grad)
    names = [k for k in VG.norm_keys(z) if k.startswith(("head.", "proprio."))]
    assert names and all((k[5:] in head) if k.startswith("head.") else (k[8:] in prop) for k in names)
    # the head's bf16 gradients sit 0.15 - 0.4 (relative) from the fp32 run at this width (ReLU patterns flip between two bf16
    # evaluations): single realisations of that noise.  Measured on the MI355X over the three fixtures: aggregate ratios 0.2 - 1.7,
    # single slices up to x2.4, single norms up to 1.6e-2 where the emulation happened to land at 2e-3.  Hence total 2, each 4 (the
    # per-tensor factor of test_oracle_golden.py for the reference's own bf16 run) and a 2e-2 floor on norms.
    _grad_checks(lambda k: head[k[5:]] if k.startswith("head.") else prop[k[8:]], OW, z, names, f"{name} adapter step", total=2.0,
                 each=4.0, norm_floor=2e-2)
    # through the whole head backward, so it carries the head's noise: ratios measured 0.35 (siglip), 1.39 (fused2), 1.97 (fused1)
    budget(eng.head.P.g("action_queries"), OW["action_queries"].grad, z["g.action_queries.weight"], f"{name}: action_queries gradient",
           factor=2.5)


@pytest.mark.parametrize("name", CASES)
def test_full_finetune_step_matches_the_reference_run(name):
    """Full fine-tune (trainers.FullFinetune): forward values and the gradients of every VLM parameter the reference run has -
    ViT block 0 of each backbone, the projector, LLM layer 0 element by element, every tensor's norm, and the embedding table's
    row norms (which rows the splice feeds)."""
    from vla_adapter_amd import engine as E
    from vla_adapter_amd.full_finetune import FullFinetune
    cfg, W, Wd, batch, _, z = _load(name)
    eng = E.VLAEngine(cfg, Wd, DEV)
    ft = FullFinetune(eng)
    bd = _dev(batch)
    pred = ft.forward(bd, None)
    loss3 = ft.backward(pred, bd["actions"])
    torch.cuda.synchronize()
    emu, OW = _oracle_emu(cfg, W, batch)
    _forward_checks(cfg, eng, pred, emu, z, f"{name} full fine-tune")
    _metric_checks(loss3, pred, emu, batch, z, f"{name} full fine-tune")
    got = ft.reference_named_gradients()
    names = [k for k in VG.norm_keys(z) if k.startswith(("vision_backbone.", "projector.", "language_model."))]
    assert set(names) <= set(got), sorted(set(names) - set(got))[:5]
    emb = "language_model.model.embed_tokens.weight"
    _grad_checks(lambda k: got[k], OW, z, [k for k in names if k != emb], f"{name} full fine-tune")
    budget(got[emb].float().cpu().norm(dim=1), OW["llm"]["embed_tokens.weight"].grad.norm(dim=1), z["grow." + emb],
           f"{name}: embedding-table gradient row norms", factor=1.5)
    assert torch.equal(got[emb].float().cpu().abs().sum(1) > 0, z["grow." + emb] > 0), "the rows of the spliced tokens get a gradient"


@pytest.mark.parametrize("name", CASES)
def test_predict_action_matches_the_reference(name, monkeypatch):
    """The public twins (modeling_prismatic.OpenVLAForActionPrediction.predict_action with L1RegressionActionHead and
    ProprioProjector) against the reference's predict_action: un-normalised actions and actions_hidden_states, on three calls -
    the eager path (VLA_PREDICT_EAGER, a model of its own), the first graphed call (capture, then a replay) and a second replay.
    The prepared batch itself (placeholders, stop id, fake labels) is compared exactly in test_oracle_golden.py."""
    from vla_adapter_amd.action_heads import L1RegressionActionHead
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    from vla_adapter_amd.projectors import ProprioProjector
    cfg, W, Wd, batch, (ids, px, proprio), z = _load(name)
    D = cfg.llm.d
    am = torch.ones_like(ids, dtype=torch.bool)
    pids, pam, plab = OpenVLAForActionPrediction.prepare_inference_inputs(ids, am)
    assert torch.equal(pids, z["p.input_ids"]) and torch.equal(pam.bool(), z["p.attention_mask"].bool()) and torch.equal(plab, z["p.labels"])

    def model():
        vla = OpenVLAForActionPrediction(cfg, Wd, DEV, norm_stats=VG.NORM_STATS)
        head = L1RegressionActionHead(input_dim=D, hidden_dim=D, action_dim=cfg.action_dim, num_task_tokens=cfg.n_patches,
                                      use_pro_version=cfg.pro, device=DEV, num_blocks=cfg.num_blocks)
        head.load_state_dict(Wd["head"], Wd["proprio"])
        pp = ProprioProjector(D, cfg.proprio_dim, DEV)
        pp.load_state_dict(Wd["proprio"])

        def call():
            act, hid = vla.predict_action(input_ids=ids, unnorm_key="golden", proprio=proprio, proprio_projector=pp, action_head=head,
                                          pixel_values=px.to(BF), attention_mask=am)
            torch.cuda.synchronize()
            return torch.from_numpy(np.asarray(act, np.float64)), hid.float().cpu().clone()
        return vla, call

    runs = {}
    with monkeypatch.context() as m:
        m.setenv("VLA_PREDICT_EAGER", "1")
        vla_e, call_e = model()
        runs["eager"] = call_e()
        assert not getattr(vla_e.engine, "_predict_graphs", None), "the eager call must not capture graphs"
    vla, call = model()
    runs["graphed"], runs["replay"] = call(), call()
    assert len(vla.engine._predict_graphs) == 1
    act_e, _, hid_e = O.predict_action_batch1(ids, am, px, torch.from_numpy(proprio), VG.oracle_weights(W), VG.oracle_cfg(cfg),
                                              VG.NORM_STATS["golden"]["action"], emu=True)
    for tag, (act, hid) in runs.items():
        # batch 1: 56 numbers, one realisation of the rounding noise (measured up to x1.35 on the SigLIP case)
        budget(act, torch.from_numpy(act_e), z["p.actions"], f"{name} predict_action ({tag}): un-normalised actions", factor=1.6)
        budget(hid, hid_e, z["p.hidden"], f"{name} predict_action ({tag}): actions_hidden_states")
        with pytest.raises(AssertionError):
            budget(torch.roll(hid, 1, dims=2), hid_e, z["p.hidden"], f"{name}: actions_hidden_states rolled by one position (must fail)")
