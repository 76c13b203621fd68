"""VLAEngine.generate(sample=, return_logprobs=) / generate_actions(do_sample=...): sampled action-token decoding end to end, on the tiny
configuration with B = 3 ragged prompts and T = 14.

 1. the default call is unchanged: the tokens are the argmax of the eager run's stored logits, before and after the sampled calls, and
    the greedy cache entry is the one it was;
 2. return_logprobs without sampling: the greedy tokens bit for bit, and log_softmax of the eager path's return_logits at them;
 3. sampled: captured equals eager, the same seed gives the same tokens and log-probabilities, another seed other tokens, other
    settings no new capture; every step's token is the numpy rule's (tests/sample_rule_np.py) on the eager run's own logits of that
    step - teacher-forced per step, so an early difference cannot cascade - wherever the rule's draw is decisive (margin above 1e-3),
    and at least 90 % of the B x T draws must be;
 4. the public path: shapes, dtypes and tuple order of (actions, tokens, logprobs), host and device forms.
Log-probabilities are held to four times torch's own float32 log_softmax error against float64 on the same logits (the bound of
tests/test_sample_kernels_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from tests import sample_rule_np as R

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
LENS, T = [20, 13, 25], 14
SAMPLE = dict(temperature=0.8, top_k=50, top_p=0.95, seed=11)
STREAMS = [5, 0, 1 << 35]
NORM_STATS = {"libero": {"action": {"q01": np.linspace(-0.9, -0.3, 7).tolist(), "q99": np.linspace(0.4, 1.3, 7).tolist(), "mask": [True] * 6 + [False]}}}
_RUN = {}


def eagerly(fn):
    old = os.environ.get("VLA_PREDICT_EAGER")
    os.environ["VLA_PREDICT_EAGER"] = "1"
    try:
        return fn()
    finally:
        os.environ.pop("VLA_PREDICT_EAGER") if old is None else os.environ.__setitem__("VLA_PREDICT_EAGER", old)


def run():
    """Every device run of this module, made once, in the order a server would meet them."""
    if _RUN:
        return _RUN
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    cfg = E.tiny_config()
    W = S.make_weights(cfg, "cpu", seed=63, std=0.05)
    g = torch.Generator().manual_seed(64)
    prompts = [torch.randint(0, cfg.llm.vocab - 300, (n,), generator=g).tolist() for n in LENS]
    img = cfg.vit[0].img
    px = torch.randn(len(LENS), 3 * len(cfg.vit) * cfg.n_img, img, img, generator=g).clamp_(-3, 3).to(DEV).to(BF)
    model = OpenVLAForActionPrediction(cfg, W, DEV, norm_stats=NORM_STATS)
    eng = model.engine
    tok = model.input_stage().decode_prompt(prompts, cfg.n_patches)
    batch = dict(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"], pixel_values=px, pos=tok["pos"], last_row=tok["last_row"])
    r = _RUN
    r.update(cfg=cfg, model=model, eng=eng, prompts=prompts, px=px, batch=batch)
    r["greedy_eager"], r["greedy_logits"] = (t.cpu() for t in eagerly(lambda: eng.generate(batch, T, return_logits=True)))
    r["greedy"] = eng.generate(batch, T).cpu()
    r["keys_after_greedy"] = sorted(map(repr, eng._generate_sets))
    r["greedy_entry"] = next(v for k, v in eng._generate_sets.items() if "sample" not in k and not k[5])
    r["greedy_lp_tok"], r["greedy_lp"] = (t.cpu() for t in eng.generate(batch, T, return_logprobs=True))
    sample = dict(SAMPLE, streams=STREAMS)
    r["cap"] = tuple(t.cpu() for t in eng.generate(batch, T, sample=sample, return_logprobs=True))
    r["keys_after_sampled"] = sorted(map(repr, eng._generate_sets))
    r["cap_again"] = tuple(t.cpu() for t in eng.generate(batch, T, sample=sample, return_logprobs=True))
    r["cap_tokens_only"] = eng.generate(batch, T, sample=sample).cpu()
    r["other_seed"] = eng.generate(batch, T, sample=dict(sample, seed=12)).cpu()
    r["other_streams"] = eng.generate(batch, T, sample=dict(SAMPLE)).cpu()
    r["other_settings"] = tuple(t.cpu() for t in eng.generate(batch, T, sample=dict(sample, temperature=1.7, top_k=0, top_p=0.8), return_logprobs=True))
    r["keys_after_settings"] = sorted(map(repr, eng._generate_sets))
    r["eager"] = tuple(t.cpu() for t in eagerly(lambda: eng.generate(batch, T, return_logits=True, sample=sample, return_logprobs=True)))
    r["greedy_after"] = eng.generate(batch, T).cpu()
    r["keys_at_end"] = sorted(map(repr, eng._generate_sets))
    torch.cuda.synchronize()
    return r


def rule_argmax(row):
    nan = torch.isnan(row).nonzero()
    return int(nan[0]) if nan.numel() else int((row == row.max()).nonzero()[0])


def log_softmax_error(logits):
    """torch's float32 log_softmax against float64 on these logits: the largest absolute difference."""
    return float((torch.log_softmax(logits.float(), -1).double() - torch.log_softmax(logits.double(), -1)).abs().max())


def test_the_default_call_is_unchanged():
    r = run()
    B = len(LENS)
    assert r["greedy"].shape == (B, T) and r["greedy"].dtype == torch.int64
    for b in range(B):
        for t in range(T):
            assert int(r["greedy"][b, t]) == rule_argmax(r["greedy_logits"][b, t].float()), f"sample {b} step {t}"
    assert torch.equal(r["greedy"], r["greedy_eager"]) and torch.equal(r["greedy_after"], r["greedy"])
    eng = r["eng"]
    greedy_keys = [k for k in eng._generate_sets if "sample" not in k and not k[5]]
    assert len(greedy_keys) == 1 and len(greedy_keys[0]) == 6, "the greedy key is the six-field key it was"
    assert eng._generate_sets[greedy_keys[0]] is r["greedy_entry"], "the greedy entry was captured again"
    assert "logits" not in r["greedy_entry"]["state"] and "sparams" not in r["greedy_entry"]["state"], "the greedy state holds no sampler buffers"
    assert len(r["keys_after_greedy"]) == 2 and len(r["keys_at_end"]) == 4      # greedy and sampled, eager and captured


def test_greedy_logprobs_are_the_log_softmax_of_the_logits():
    r = run()
    assert torch.equal(r["greedy_lp_tok"], r["greedy"]), "return_logprobs changed a greedy token"
    lp = r["greedy_lp"]
    assert lp.dtype == torch.float32 and lp.shape == r["greedy"].shape
    want = torch.log_softmax(r["greedy_logits"].double(), -1).gather(-1, r["greedy"][..., None])[..., 0]
    err, bound = float((lp.double() - want).abs().max()), 4 * log_softmax_error(r["greedy_logits"])
    print(f"greedy log-probs: {err:.3e} from float64 (bound {bound:.3e})")
    assert err <= bound


def test_sampled_runs_repeat_follow_the_seed_and_never_capture_again():
    r = run()
    tok, lp = r["cap"]
    assert torch.equal(r["cap_again"][0], tok) and torch.equal(r["cap_again"][1].view(torch.int32), lp.view(torch.int32)), "the same seed, other draws"
    assert torch.equal(r["cap_tokens_only"], tok)
    etok, elogits, elp = r["eager"]
    assert torch.equal(etok, tok) and torch.equal(elp.view(torch.int32), lp.view(torch.int32)), "captured and eager differ"
    assert not torch.equal(r["other_seed"], tok) and not torch.equal(r["other_streams"], tok) and not torch.equal(r["other_settings"][0], tok)
    assert not torch.equal(tok, r["greedy"])
    assert r["keys_after_settings"] == r["keys_after_sampled"] and len(r["keys_after_sampled"]) == 3, "a new setting or seed captured again"
    assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())


def test_every_sampled_step_is_the_rule_on_that_steps_logits():
    r = run()
    etok, elogits, elp = r["eager"]
    B = len(LENS)
    decisive = 0
    worst = 0.0
    kept_all = torch.zeros(elogits.shape, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            l = elogits[b, t].float().numpy()
            w = R.step(l, SAMPLE["temperature"], SAMPLE["top_k"], SAMPLE["top_p"], seed=SAMPLE["seed"], stream=STREAMS[b], t=t)
            tok = int(etok[b, t])
            assert w["kept"][tok], f"sample {b} step {t}: a removed token was drawn"
            kept_all[b, t] = torch.from_numpy(w["kept"])
            z = R.scale(l, SAMPLE["temperature"])
            worst = max(worst, abs(float(elp[b, t]) - float(z[tok] - R.logsumexp(z[w["kept"]]))))
            if w["margin"] > 1e-3:
                decisive += 1
                assert tok == w["token"], f"sample {b} step {t}: device {tok}, rule {w['token']} on a decisive draw"
    warped = (elogits.float() / np.float32(SAMPLE["temperature"])).masked_fill(~kept_all, float("-inf"))
    diff = torch.log_softmax(warped, -1).double() - torch.log_softmax(warped.double(), -1)
    bound = 4 * float(diff[kept_all].abs().max())               # torch's float32 log_softmax of the warped scores against float64
    print(f"sampled: {decisive} of {B * T} draws decisive, every one equal; log-probs {worst:.3e} from the rule (bound {bound:.3e})")
    assert decisive >= 0.9 * B * T
    assert worst <= bound


def test_the_public_path_returns_actions_tokens_logprobs_in_that_order():
    r = run()
    model, px, Da = r["model"], r["px"], r["cfg"].action_dim
    kw = dict(pixel_values=px, max_new_tokens=T, do_sample=True, sample_streams=STREAMS, **SAMPLE)
    actions, tokens, logprobs = model.generate_actions(r["prompts"], return_tokens=True, return_logprobs=True, **kw)
    assert isinstance(actions, np.ndarray) and actions.dtype == np.float64 and actions.shape == (len(LENS), T // Da, Da)
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (len(LENS), T) and torch.equal(tokens.cpu(), r["cap"][0])
    assert isinstance(logprobs, np.ndarray) and logprobs.dtype == np.float32 and np.array_equal(logprobs, r["cap"][1].numpy())
    a2, lp2 = model.generate_actions(r["prompts"], return_logprobs=True, **kw)
    assert np.array_equal(a2, actions) and np.array_equal(lp2, logprobs)
    da, dt, dl = model.generate_actions(r["prompts"], return_tokens=True, return_logprobs=True, return_tensors=True, **kw)
    assert da.is_cuda and dt.is_cuda and dl.is_cuda and dl.dtype == torch.float32 and da.dtype == torch.float64
    assert np.array_equal(da.cpu().numpy(), actions) and np.array_equal(dl.cpu().numpy(), logprobs)
    ga, gl = model.generate_actions(r["prompts"], pixel_values=px, max_new_tokens=T, return_logprobs=True)
    assert np.array_equal(gl, r["greedy_lp"].numpy()) and np.array_equal(ga, model.generate_actions(r["prompts"], pixel_values=px, max_new_tokens=T))
    assert sorted(map(repr, r["eng"]._generate_sets)) == r["keys_at_end"], "the public path captured again"
