"""VLAEngine.generate / OpenVLAForActionPrediction.generate_actions: greedy action-token decoding with a key/value cache, end to end.

Per case (a ragged batch at the real vocabulary, the fused two-image configuration at batch 3 and at batch 1):
 1. exact - every token is the rule's argmax (lowest index among equals, NaN first) of that step's stored logits; the captured and the
    eager run and a second call give the same tokens;
 2. teacher-forced - prompt + the device's own tokens through the oracle composed as tests/test_token_ce_gpu.py composes it (uncached,
    whole sequence), bf16-emulating and fp32: the step logits pass budget() with its default factor, the project's criterion for these
    very logits;
 3. against the oracle's OWN greedy decode (uncached, on the CPU): a step is decisive when the oracle's top-1 exceeds its top-2 by more
    than twice the largest |device - oracle| logit difference measured at that step in (2); a row is compared up to its first step
    that is not, the tokens of every compared step must be equal, and at least half of all B x T steps must be compared.  The weights
    are made on the CPU, so the seeds could be chosen from the oracle's margins alone before any device ran (see SEEDS);
 4. the public path - generate_actions equals a numpy restatement of ActionTokenizer.decode_token_ids_to_actions and
    openvla.py:99-105 on the returned tokens, bit for bit in float64, with a statistics entry that has a mask;
 5. isolation - predict_actions gives the same bits before and after a generate_actions on the same model."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

from oracle import vla_oracle as O  # noqa: E402
from test_engine_gpu import budget, cpu_f32  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
# (weights seed, inputs seed) per case.  Random weights leave the two largest of V bf16 logits a few ulps apart at most steps (the top
# logit is near 3, its ulp 2^-6), so a row usually meets an indecisive step early: of the seeds 61, 63, .. 119 (and 21 .. 51) most
# compare a fifth to a half of the steps.  These were chosen on the CPU, before the first device run, from the oracle's margins alone:
# the share of steps up to each row's first one whose margin is not above 2 % of the top logit (five ulps; the device's logits were
# expected within two of the oracle's) is 91 %, 99 % and 100 %.
SEEDS = {"vocab": (63, 64), "fused3": (71, 72), "fused1": (41, 42)}
CASES = {"vocab": ([20, 13], 16), "fused3": ([20, 17, 25], 56), "fused1": ([20], 56)}       # prompt lengths (ragged), T


def make_case(name):
    """(cfg, weights on the CPU, prompts, pixel_values on the CPU, T)."""
    from vla_adapter_amd import engine as E, synthetic as S
    lens, T = CASES[name]
    if name == "vocab":                  # the test-local LLM of tests/test_token_ce_gpu.py: the real vocabulary on two layers
        cfg = E.tiny_config()
        cfg.llm = E.LLMCfg(256, 2, 4, 2, 64, 512, 1e-6, 1e6, 151936)
    else:
        cfg = E.tiny_fused_config()
    ws, bs = SEEDS[name]
    W = S.make_weights(cfg, "cpu", seed=ws, std=0.05)
    g = torch.Generator().manual_seed(bs)
    hi = min(151386, cfg.llm.vocab - 300)
    prompts = [torch.randint(0, hi, (n,), generator=g).tolist() for n in lens]
    img = cfg.vit[0].img
    px = torch.randn(len(lens), 3 * len(cfg.vit) * cfg.n_img, img, img, generator=g).clamp_(-3, 3)
    return cfg, W, prompts, px, T


class Oracle:
    """The uncached forward of _oracle_ce (tests/test_token_ce_gpu.py) on prompt + tokens: vision and projector once, then the Qwen2
    stack over the whole right-padded sequence and the tied lm_head on the rows that predict a token."""

    def __init__(self, cfg, W, px, emu):
        self.cfg, self.emu = cfg, emu
        vit, proj, self.llm = [cpu_f32(s) for s in W["vit"]], cpu_f32(W["proj"]), cpu_f32(W["llm"])
        px, nbk, feats = px.float(), len(cfg.vit), []
        for im in range(cfg.n_img):
            ch = px[:, im * 3 * nbk:(im + 1) * 3 * nbk]
            feats.append(torch.cat([O.vit_forward(ch[:, 3 * j:3 * j + 3], vit[j], cfg.vit[j].as_oracle(), emu) for j in range(nbk)], dim=2))
        self.patches = O.projector(torch.cat(feats, dim=1), proj, cfg.fused, emu)

    def step_logits(self, rows, n_last):
        """rows: per sample the ids so far (prompt + tokens) -> the logits of each sample's last n_last rows, [B, n_last, V]."""
        B, Lm, Np = len(rows), max(len(r) for r in rows), self.patches.shape[1]
        ids = torch.zeros(B, Lm, dtype=torch.int64)
        am = torch.zeros(B, Lm, dtype=torch.bool)
        for b, r in enumerate(rows):
            ids[b, :len(r)] = torch.tensor(r)
            am[b, :len(r)] = True
        emb = self.llm["embed_tokens.weight"][ids]
        mm = torch.cat([emb[:, :1], self.patches, emb[:, 1:]], dim=1)
        mask = torch.cat([am[:, :1], torch.ones(B, Np, dtype=torch.bool), am[:, 1:]], dim=1)
        hs = O.qwen2_forward(mm, mask, self.llm, self.cfg.llm.as_oracle(), self.emu)[-1]
        last = torch.stack([hs[b, Np + len(r) - n_last:Np + len(r)] for b, r in enumerate(rows)])
        return O.linear(last, self.llm["embed_tokens.weight"], None, self.emu)

    def greedy(self, prompts, T):
        """The oracle's own greedy decode -> (tokens [B, T], top-1 minus top-2 of every step [B, T])."""
        rows = [list(p) for p in prompts]
        toks, margin = torch.zeros(len(rows), T, dtype=torch.int64), torch.zeros(len(rows), T)
        for t in range(T):
            top = self.step_logits(rows, 1)[:, 0].float().topk(2, dim=-1)
            toks[:, t], margin[:, t] = top.indices[:, 0], top.values[:, 0] - top.values[:, 1]
            for b, r in enumerate(rows):
                r.append(int(toks[b, t]))
        return toks, margin


def rule_argmax(row):
    nan = torch.isnan(row).nonzero()
    return int(nan[0]) if nan.numel() else int((row == row.max()).nonzero()[0])


NORM_STATS = {"libero": {"action": {"q01": np.linspace(-0.9, -0.3, 7).tolist(), "q99": np.linspace(0.4, 1.3, 7).tolist(),
                                    "mask": [True] * 6 + [False]},
                         "proprio": {"q01": [-1.0] * 8, "q99": [1.0] * 8}}}
_RUNS = {}


def run_case(name):
    """The device runs of one case, made once: eager with logits, captured twice, and the model they ran on."""
    if name in _RUNS:
        return _RUNS[name]
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    cfg, W, prompts, px, T = make_case(name)
    model = OpenVLAForActionPrediction(cfg, W, DEV, norm_stats=NORM_STATS)
    tok = model.input_stage().decode_prompt(prompts, cfg.n_patches)
    batch = dict(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"], pixel_values=px.to(DEV).to(BF), pos=tok["pos"], last_row=tok["last_row"])
    assert tok["input_ids"].shape[1] % 32 == 0
    old = os.environ.get("VLA_PREDICT_EAGER")
    os.environ["VLA_PREDICT_EAGER"] = "1"
    try:
        eager, logits = model.engine.generate(batch, T, return_logits=True)
    finally:
        os.environ.pop("VLA_PREDICT_EAGER") if old is None else os.environ.__setitem__("VLA_PREDICT_EAGER", old)
    first = model.engine.generate(batch, T).cpu()
    second = model.engine.generate(batch, T).cpu()
    torch.cuda.synchronize()
    _RUNS[name] = dict(cfg=cfg, W=W, prompts=prompts, px=px, T=T, model=model, batch=batch, eager=eager.cpu(), logits=logits.float().cpu(),
                       first=first, second=second)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_tokens_are_the_argmax_of_the_stored_logits_eager_captured_and_again(name):
    r = run_case(name)
    B, T = r["eager"].shape
    assert (B, T) == (len(r["prompts"]), r["T"]) and r["logits"].shape == (B, T, r["cfg"].llm.vocab)
    for b in range(B):
        for t in range(T):
            assert int(r["eager"][b, t]) == rule_argmax(r["logits"][b, t]), f"sample {b} step {t}"
    assert torch.equal(r["first"], r["eager"]), "captured and eager tokens differ"
    assert torch.equal(r["second"], r["first"]), "a second call gives other tokens"


@pytest.mark.parametrize("name", list(CASES))
def test_step_logits_against_the_oracle_teacher_forced_and_its_own_greedy_decode(name):
    r = run_case(name)
    prompts, T, dev_tok, dev_logits = r["prompts"], r["T"], r["eager"], r["logits"]
    B = len(prompts)
    px = r["batch"]["pixel_values"].float().cpu()                                  # the bf16 pixels the device saw
    ora = {emu: Oracle(r["cfg"], r["W"], px, emu) for emu in (True, False)}
    # (2) teacher-forced on the device's own tokens: the row of the last prompt id predicts token 0, token t - 1 predicts token t
    rows = [list(p) + dev_tok[b, :T - 1].tolist() for b, p in enumerate(prompts)]
    tf = {emu: ora[emu].step_logits(rows, T).float() for emu in (True, False)}
    budget(dev_logits, tf[True], tf[False], f"generate [{name}]: step logits, teacher-forced")
    # (3) the oracle's own greedy decode
    otok, margin = ora[True].greedy(prompts, T)
    err = (dev_logits - tf[True]).abs().amax(dim=-1)                               # largest |device - oracle| logit difference per step
    compared = 0
    for b in range(B):
        for t in range(T):
            if not margin[b, t] > 2 * err[b, t]:
                break                                                              # first step that is not decisive: the row ends here
            assert int(dev_tok[b, t]) == int(otok[b, t]), f"sample {b} step {t}: device {int(dev_tok[b, t])}, oracle {int(otok[b, t])} on a decisive step"
            compared += 1
    print(f"generate [{name}]: {compared} of {B * T} steps compared ({compared / (B * T):.0%}); every one equal")
    assert 2 * compared >= B * T, f"only {compared} of {B * T} steps were decisive up to each row's first indecisive one"


def numpy_actions(tokens, stats, Da, tokenizer_len=151643, n_bins=256):
    """ActionTokenizer.decode_token_ids_to_actions (action_tokenizer.py:76-95) and openvla.py:99-105, restated."""
    bins = np.linspace(-1.0, 1.0, n_bins)
    centers = (bins[:-1] + bins[1:]) / 2.0
    d = np.clip(tokenizer_len - tokens - 1, a_min=0, a_max=centers.shape[0] - 1)
    a = centers[d].reshape(tokens.shape[0], -1, Da)
    mask = np.asarray(stats.get("mask", np.ones_like(stats["q01"], dtype=bool)))
    high, low = np.array(stats["q99"]), np.array(stats["q01"])
    return np.where(mask, 0.5 * (a + 1) * (high - low) + low, a)


@pytest.mark.parametrize("name", ["vocab", "fused3"])
def test_generate_actions_is_the_reference_rule_on_the_returned_tokens(name):
    r = run_case(name)
    model, Da = r["model"], r["cfg"].action_dim
    T = r["T"] - r["T"] % Da                                                       # (16 -> 14: two actions)
    px = r["batch"]["pixel_values"]
    actions, tokens = model.generate_actions(r["prompts"], pixel_values=px, max_new_tokens=T, return_tokens=True)
    tokens = tokens.cpu().numpy()
    assert actions.dtype == np.float64 and actions.shape == (len(r["prompts"]), T // Da, Da)
    want = numpy_actions(tokens, NORM_STATS["libero"]["action"], Da)
    assert np.array_equal(actions.view(np.int64), want.view(np.int64)), "generate_actions differs from the numpy rule in some bit"
    assert np.array_equal(tokens, r["eager"][:, :T].numpy()), "a shorter generation is a prefix of the longer one"
    dev_actions = model.generate_actions(r["prompts"], pixel_values=px, max_new_tokens=T, return_tensors=True)
    assert dev_actions.is_cuda and np.array_equal(dev_actions.cpu().numpy().view(np.int64), want.view(np.int64))
    # tokens the model never learned to keep inside the action range still decode (the clip), and real action ids decode to their bins
    ids = np.array([[151643 - 1 - k for k in (0, 1, 100, 254, 255)] + [0, 151935]])
    assert np.array_equal(model.input_stage().decode_token_ids_to_actions(torch.from_numpy(ids)).cpu().numpy().view(np.int64),
                          numpy_actions(ids, {"q01": [0.0] * 7, "q99": [0.0] * 7, "mask": [False] * 7}, 7)[0].view(np.int64))


def test_generate_actions_leaves_predict_actions_bits_alone():
    r = run_case("fused3")
    model, px = r["model"], r["batch"]["pixel_values"]
    g = torch.Generator().manual_seed(5)
    proprio = (torch.rand(len(r["prompts"]), r["cfg"].proprio_dim, generator=g) * 2 - 1).to(DEV)
    call = lambda: model.predict_actions(r["prompts"], pixel_values=px, proprio=proprio, proprio_normalized=True, return_tensors=True)
    a0, h0 = (t.clone() for t in call())                                           # captures the predict graphs
    a1, h1 = (t.clone() for t in call())                                           # a replay
    model.generate_actions(r["prompts"], pixel_values=px)
    a2, h2 = (t.clone() for t in call())
    torch.cuda.synchronize()
    assert torch.equal(a0.view(torch.int64), a1.view(torch.int64)) and torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    assert torch.equal(a2.view(torch.int64), a1.view(torch.int64)), "predict_actions changed its actions after a generate_actions"
    assert torch.equal(h2.view(torch.int16), h1.view(torch.int16)), "predict_actions changed its hidden states after a generate_actions"
    assert model.engine.generate(r["batch"], r["T"]).cpu().equal(r["first"]), "and generation is unchanged by the predict in between"
