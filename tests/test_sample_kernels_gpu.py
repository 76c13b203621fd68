"""vla_sample_tokens (include/vla_sample.h) against the float64 rule of tests/sample_rule_np.py, row by row.

Shapes: B in {1, 5, 64} at V in {1016, 1000} and B = 2 at the real vocabulary; the logits rows stand in a buffer whose row stride is
larger than V, NaN behind every row.  Per shape and setting the rule is computed once (RULE) and shared.

Tolerance of the probabilities and log-probabilities: torch's own float32 softmax / log_softmax of the warped scores, measured against
float64 on the same inputs (all settings of a shape pooled), times four - the device and torch are two float32 evaluations in
different orders.  Every case prints what it measured in front of its assertion.

The kept set must be the rule's exactly (a removed token's probability is exactly 0), so the inputs must not sit on a top-p boundary:
every row's cumulative probability is farther than 1e-5 from 1 - top_p (asserted).  The bound comes from the device's arithmetic, not
from its results: a token's mass is expf (within 2 ulp, 2.4e-7 relative) truncated to 2^-40, summed exactly as integers, so a
cumulative share is within about 5e-7 of the float64 one; 1e-5 leaves a factor of twenty.  (With 64 rows and two top-p settings a
wider margin leaves almost no generator seed: the cumulative shares step by about 1e-3, so one row in twenty sits within 1e-4.)  A
draw is compared where it is decisive: the rule's best z + g exceeds the second best by more than 1e-3 (float32 evaluates z + g to
about 1e-5); every decisive row must match and at least 90 % of a case's rows must be decisive.  The generator seed of host_logits was
chosen with the rule alone, before any device ran, so that both preconditions hold for every shape and setting."""
import numpy as np
import pytest
import torch

from tests import sample_rule_np as R
from tests.test_sample_cpu import DIST_SEED, DIST_STEPS, DIST_STREAMS, DIST_V, chi2_quantile, chi_square, dist_logits

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
SHAPES = [(B, V) for V in (1016, 1000) for B in (1, 5, 64)] + [(2, 151936)]
SETTINGS = [(0.7, 50, 0.9), (1.0, 0, 0.95), (1.6, 5, 1.0), (1.0, 0, 1.0)]     # (temperature, top_k, top_p)
SEED, STEP = 20240917, 3
IDS = [f"B{B}-V{V}" for B, V in SHAPES]


def host_logits(B, V):
    g = torch.Generator().manual_seed(500000 + 1000 * B + V % 997)      # (chosen with the rule alone: see the module docstring)
    return (4.0 * torch.randn(B, V, generator=g)).to(BF)


def strided(host, pad=24):
    """The rows of `host` in a device buffer with a row stride above the width and NaN behind every row."""
    B, V = host.shape
    buf = torch.full((B, V + pad), float("nan"), dtype=host.dtype, device=DEV)
    buf[:, :V] = host.to(DEV)
    return buf[:, :V]


def streams_of(B):
    return [(7 * b + 3) % 101 + (1 << 33) * (b % 2) for b in range(B)]


def device_step(logits, *, temperature=1.0, top_k=0, top_p=1.0, seed=SEED, greedy=False, streams=None, step=STEP, T=8, probs=True):
    from vla_adapter_amd import ops
    B, V = logits.shape
    blk = ops.sample_params(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, greedy=greedy).to(DEV)
    st = None if streams is None else torch.tensor(streams, dtype=torch.int64, device=DEV)
    lp = torch.full((B, T), -7.0, device=DEV)
    pr = strided(torch.full((B, V), -7.0)) if probs else None
    ids = ops.sample_tokens(logits, blk, torch.tensor([step], dtype=torch.int32, device=DEV), streams=st, logprob_out=lp, probs_out=pr)
    torch.cuda.synchronize()
    assert bool((lp[:, [c for c in range(T) if c != step]] == -7.0).all()), "only column t of logprob_out is written"
    return ids.cpu().numpy(), lp[:, step].cpu().numpy(), None if pr is None else pr.cpu().numpy()


RULE, TORCH_ERR = {}, {}


def rule(B, V, setting):
    key = (B, V, setting)
    if key not in RULE:
        l = host_logits(B, V).float().numpy()
        T_, k, p = setting
        RULE[key] = [R.step(l[b], T_, k, p, seed=SEED, stream=streams_of(B)[b], t=STEP) for b in range(B)]
    return RULE[key]


def torch_error(B, V):
    """(probabilities, log-probabilities): the largest |float32 - float64| of torch's softmax / log_softmax over the warped scores of
    every setting of this shape - kept tokens only for the logarithm."""
    if (B, V) not in TORCH_ERR:
        l = host_logits(B, V).float().numpy()
        ep = el = 0.0
        for s in SETTINGS:
            kept = np.stack([r["kept"] for r in rule(B, V, s)])
            z = torch.from_numpy(np.stack([R.scale(l[b], s[0]) for b in range(B)])).masked_fill(torch.from_numpy(~kept), float("-inf"))
            p64, l64 = torch.softmax(z, -1), torch.log_softmax(z, -1)
            p32, l32 = torch.softmax(z.float(), -1).double(), torch.log_softmax(z.float(), -1).double()
            ep = max(ep, float((p32 - p64).abs().max()))
            el = max(el, float((l32 - l64)[torch.from_numpy(kept)].abs().max()))
        TORCH_ERR[(B, V)] = (ep, el)
    return TORCH_ERR[(B, V)]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
@pytest.mark.parametrize("B,V", SHAPES, ids=IDS)
def test_probabilities_logprobs_and_tokens_against_the_rule(B, V, setting):
    want = rule(B, V, setting)
    assert min(r["gap"] for r in want) > 1e-5, "an input row sits on the top-p boundary: choose another generator seed"
    decisive = np.array([r["margin"] > 1e-3 for r in want])
    assert decisive.mean() >= 0.9, "fewer than 90 % of the rows are decisive under the rule: choose other seeds"
    ep, el = torch_error(B, V)
    ids, lp, pr = device_step(strided(host_logits(B, V)), temperature=setting[0], top_k=setting[1], top_p=setting[2], streams=streams_of(B))
    kept = np.stack([r["kept"] for r in want])
    assert np.array_equal(pr != 0, kept) and (pr[~kept] == 0).all(), "the kept set differs from the rule's"
    dp = float(np.abs(pr - np.stack([r["probs"] for r in want])).max())
    # the log-probability of the device's own token under the rule (equal to the rule's wherever the tokens agree)
    z = [R.scale(host_logits(B, V).float().numpy()[b], setting[0]) for b in range(B)]
    ref_lp = np.array([z[b][ids[b]] - R.logsumexp(z[b][kept[b]]) for b in range(B)])
    dl = float(np.abs(lp - ref_lp).max())
    print(f"sample [{B} x {V}, T {setting[0]} k {setting[1]} p {setting[2]}]: probs {dp:.3e} (torch {ep:.3e}, bound {4 * ep:.3e}); "
          f"logprob {dl:.3e} (torch {el:.3e}, bound {4 * el:.3e}); decisive {int(decisive.sum())} of {B}")
    assert kept[np.arange(B), ids].all(), "a removed token was drawn"
    assert dp <= 4 * ep and dl <= 4 * el
    tok = np.array([r["token"] for r in want])
    assert np.array_equal(ids[decisive], tok[decisive]), f"decisive rows {np.flatnonzero(decisive & (ids != tok)).tolist()} differ from the rule"


@pytest.mark.parametrize("B,V", SHAPES, ids=IDS)
def test_top_k_one_draws_a_largest_logit(B, V):
    l = host_logits(B, V)
    ids, lp, pr = device_step(strided(l), temperature=0.9, top_k=1, top_p=0.8, streams=streams_of(B))
    lf = l.float().numpy()
    assert np.array_equal(lf[np.arange(B), ids], lf.max(axis=1)), "compared by value: two equal largest bf16 logits do occur"
    ties = (lf == lf.max(axis=1, keepdims=True)).sum(axis=1)
    assert np.array_equal((pr != 0).sum(axis=1), ties) and np.allclose(lp, -np.log(ties), rtol=0, atol=1e-6)
    if B == 5:                                                   # a three-way tie: every one of them is kept and one is drawn
        l2 = l.clone()
        l2[:, [11, 500, 999]] = float(l.float().max()) + 1.0
        ids2, lp2, pr2 = device_step(strided(l2), top_k=1, streams=streams_of(B))
        assert set(ids2.tolist()) <= {11, 500, 999} and np.array_equal(np.flatnonzero(pr2[0]), [11, 500, 999]) and np.allclose(lp2, -np.log(3.0), atol=1e-6)


@pytest.mark.parametrize("B,V", SHAPES, ids=IDS)
def test_greedy_is_the_lm_head_argmax_with_its_log_softmax(B, V):
    from vla_adapter_amd import ops
    g = torch.Generator().manual_seed(B + V)
    x, W = torch.randn(B, 64, generator=g).to(BF).to(DEV), (0.3 * torch.randn(V, 64, generator=g)).to(BF).to(DEV)
    W[min(V - 1, 777)] = W[5]                                    # two equal columns: equal logits in every row
    logits = strided(torch.zeros(B, V, dtype=BF))
    ref = ops.decode_lm_head_argmax(x, W, ops.decode_argmax_workspace(B, V, DEV), logits_out=logits).cpu().numpy()
    ids, lp, pr = device_step(logits, greedy=True, temperature=0.5, top_k=3, top_p=0.5)       # (greedy reads none of the three)
    assert np.array_equal(ids, ref), "greedy ids differ from vla_decode_lm_head_argmax's"
    l64 = torch.log_softmax(logits.double().cpu(), -1)
    l32 = torch.log_softmax(logits.float().cpu(), -1).double()
    el, ep = float((l32 - l64).abs().max()), float((torch.softmax(logits.float().cpu(), -1).double() - l64.exp()).abs().max())
    dl = float(np.abs(lp - l64[torch.arange(B), torch.from_numpy(ids)].numpy()).max())
    dp = float(np.abs(pr - l64.exp().numpy()).max())
    print(f"greedy [{B} x {V}]: logprob {dl:.3e} (torch {el:.3e}), probs {dp:.3e} (torch {ep:.3e})")
    assert dl <= 4 * el and dp <= 4 * ep


def test_a_non_finite_row_takes_the_greedy_token_and_a_nan_logprob():
    B, V = 5, 1000
    l = host_logits(B, V)
    bad = l.clone()
    bad[1, 700] = float("nan")
    bad[1, 900] = float("nan")
    bad[3, 123] = float("inf")
    bad[4] = float("-inf")
    for kw in (dict(temperature=0.7, top_k=50, top_p=0.9), dict(greedy=True)):
        ids0, lp0, pr0 = device_step(strided(l), **kw)
        ids1, lp1, pr1 = device_step(strided(bad), **kw)
        assert ids1[1] == 700 and ids1[3] == 123 and ids1[4] == 0, "the first NaN, the +inf, the lowest id of an all -inf row"
        assert np.isnan(lp1[[1, 3, 4]]).all() and np.isnan(pr1[[1, 3, 4]]).all()
        for b in (0, 2):
            assert ids1[b] == ids0[b] and lp1[b].tobytes() == lp0[b].tobytes() and pr1[b].tobytes() == pr0[b].tobytes(), "a neighbour changed"
    # -inf logits beside finite ones are ordinary: probability 0, never drawn
    some = l.clone()
    some[:, ::2] = float("-inf")
    ids, lp, pr = device_step(strided(some), streams=streams_of(B))
    assert (ids % 2 == 1).all() and np.isfinite(lp).all() and (pr[:, ::2] == 0).all() and np.allclose(pr.sum(axis=1), 1.0, atol=1e-5)


def test_two_launches_give_equal_bits_and_seed_stream_and_step_move_the_draw():
    B, V = 64, 1016
    logits = strided(host_logits(B, V))
    kw = dict(temperature=1.3, top_k=200, top_p=0.97, streams=streams_of(B))
    a, b = device_step(logits, **kw), device_step(logits, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert not np.array_equal(device_step(logits, **dict(kw, seed=SEED + 1))[0], a[0]), "another seed draws the same tokens"
    assert not np.array_equal(device_step(logits, **dict(kw, step=STEP + 1))[0], a[0]), "another step draws the same tokens"
    assert not np.array_equal(device_step(logits, **dict(kw, streams=None))[0], a[0]), "other streams draw the same tokens"
    # the noise belongs to (seed, stream, step, token): a row draws the same token alone, in another batch position, in another batch
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(0)).tolist()
    moved = device_step(strided(host_logits(B, V)[perm]), **dict(kw, streams=[streams_of(B)[i] for i in perm]))
    assert np.array_equal(moved[0], a[0][perm]) and moved[1].tobytes() == a[1][perm].tobytes()
    one = device_step(strided(host_logits(B, V)[9:10]), **dict(kw, streams=streams_of(B)[9:10]))
    assert one[0][0] == a[0][9] and one[1][0] == a[1][9]
    # streams NULL means stream b
    assert np.array_equal(device_step(logits, **dict(kw, streams=None))[0], device_step(logits, **dict(kw, streams=list(range(B))))[0])


@pytest.mark.parametrize("first", [False, True], ids=["step", "behind-the-prefill"])
def test_the_advance_is_the_one_of_the_greedy_decoder(first):
    from vla_adapter_amd import ops
    B, V, D, T = 5, 1000, 64, 6
    host = host_logits(B, V)
    host[0, 950] = 30.0                                                         # row 0 draws an id behind the embedding table
    logits = strided(host)
    g = torch.Generator().manual_seed(9)
    embed = strided(torch.randn(900, D, generator=g).to(BF), pad=8)             # fewer rows than V: the id is clamped into the table
    blk = ops.sample_params(temperature=1.5, top_k=0, top_p=1.0, seed=SEED).to(DEV)
    out_ids = torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    logprobs = torch.full((B, T), -7.0, device=DEV)
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    pos = torch.tensor([3, 4, 5, 6, 7], dtype=torch.int32, device=DEV)
    pos_from = torch.tensor([30, 40, 50, 60, 70], dtype=torch.int32, device=DEV) if first else None
    x_next = strided(torch.zeros(B, D, dtype=BF), pad=8)
    ids = ops.sample_tokens(logits, blk, step, logprob_out=logprobs, advance=(out_ids, step, pos, embed, x_next), pos_from=pos_from)
    torch.cuda.synchronize()
    t = 0 if first else 2
    free = device_step(logits, temperature=1.5, step=t, T=T, probs=False)       # the same draw without an advance: streams NULL, step t
    assert np.array_equal(ids.cpu().numpy(), free[0]) and np.array_equal(logprobs[:, t].cpu().numpy(), free[1])
    assert step.item() == t + 1 and pos.tolist() == ([31, 41, 51, 61, 71] if first else [4, 5, 6, 7, 8])
    assert torch.equal(out_ids[:, t], ids) and bool((out_ids[:, [c for c in range(T) if c != t]] == -7).all())
    assert bool((logprobs[:, [c for c in range(T) if c != t]] == -7.0).all())
    assert torch.equal(x_next.view(torch.int16), embed[ids.clamp(max=899)].view(torch.int16))
    assert bool((ids > 899).any()), "the case must exercise the clamp"
    # a step index at or behind T writes no column and still advances the counters
    step.fill_(T)
    before = out_ids.clone()
    ops.sample_tokens(logits, blk, step, logprob_out=logprobs, advance=(out_ids, step, pos, embed, x_next))
    torch.cuda.synchronize()
    assert torch.equal(out_ids, before) and step.item() == T + 1


def test_draws_follow_the_softmax_on_the_device():
    """The CPU distribution test on the device: the same logits, seed, streams and steps, the same threshold - and the same tokens
    wherever the rule's draw is decisive."""
    from vla_adapter_amd import ops
    l = dist_logits()
    logits = strided(torch.from_numpy(l).to(BF).repeat(DIST_STREAMS, 1))
    blk = ops.sample_params(seed=DIST_SEED).to(DEV)
    out_ids = torch.zeros(DIST_STREAMS, DIST_STEPS, dtype=torch.int64, device=DEV)
    step, pos = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(DIST_STREAMS, dtype=torch.int32, device=DEV)
    embed, x_next = torch.zeros(DIST_V, 8, dtype=BF, device=DEV), torch.zeros(DIST_STREAMS, 8, dtype=BF, device=DEV)
    for _ in range(DIST_STEPS):
        ops.sample_tokens(logits, blk, step, advance=(out_ids, step, pos, embed, x_next))
    torch.cuda.synchronize()
    tokens = out_ids.cpu().numpy()
    assert step.item() == DIST_STEPS and pos.tolist() == [DIST_STEPS] * DIST_STREAMS
    stat, bound = chi_square(tokens, l), chi2_quantile(DIST_V - 1, 1e-6)
    print(f"device chi-square of {tokens.size} draws over {DIST_V} tokens: {stat:.2f} (bound {bound:.2f})")
    assert stat < bound
    want = [[R.step(l, seed=DIST_SEED, stream=s, t=t) for t in range(DIST_STEPS)] for s in range(DIST_STREAMS)]
    decisive = np.array([[r["margin"] > 1e-3 for r in row] for row in want])
    rule_tok = np.array([[r["token"] for r in row] for row in want])
    assert decisive.mean() >= 0.9 and np.array_equal(tokens[decisive], rule_tok[decisive])
