"""The kernels of include/vla_decode.h one by one (the cached single-token step of VLAEngine.generate): prompt assembly, RoPE and append,
single-query attention over the cache, and the fused lm_head argmax with its advance.

Criteria: what is a copy or a rotation is compared bit for bit (the prompt rows, the appended cache row against ops.rope_half_ at that
position, the one-key attention against the v row, the chosen id against the rule's argmax of the stored logits); what accumulates is
held to the project's own budgets - the attention rows to tests/accuracy.assert_row_budget with the attention constants against
oracle.attention (bf16-emulating) and float64, the stored logits to assert_contract with the GEMM constants."""
import math

import pytest
import torch

from oracle import vla_oracle as O
from tests import accuracy as A
from tests.arena import assert_bits_equal, bits
from vla_adapter_amd import ops

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
TILE, WAVES = 64, 4                     # csrc/decode.hip: ATT_TILE keys per wave tile, tile t -> wave t % 4 (one round: 256 keys)
SLAB = 128                              # csrc/decode.hip: LM_SLAB rows of W per workgroup


def gen(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def rule_argmax(row: torch.Tensor) -> int:
    """torch.argmax's order on the CPU, spelled out: the first NaN if there is one, else the lowest index of the maximum."""
    row = row.float().cpu()
    nan = torch.isnan(row).nonzero()
    if nan.numel():
        return int(nan[0])
    return int((row == row.max()).nonzero()[0])


# ================================================================================================================ prompt assembly
def test_prompt_rows_positions_and_padding():
    prompts = [[5, 6, 7], list(range(100, 133)), [9], list(range(40))]
    flat = torch.tensor([t for r in prompts for t in r], dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 3, 36, 37, 77], dtype=torch.int32, device=DEV)
    L, Np, pad = 64, 16, 1023
    ids, am, pos, last_row, ok = ops.decode_prompt(flat, off, L, Np, pad_id=pad)
    for b, r in enumerate(prompts):
        assert ids[b].tolist() == r + [pad] * (L - len(r))
        assert am[b].tolist() == [1] * len(r) + [0] * (L - len(r))
    assert pos.tolist() == [Np + len(r) - 1 for r in prompts]
    assert last_row.tolist() == [b * (Np + L) + Np + len(r) - 1 for b, r in enumerate(prompts)]
    assert ok.tolist() == [1, 1, 1, 1]
    # an empty row and one that does not fit: the row of the one-id prompt [pad], reported by row_ok alone
    off2 = torch.tensor([0, 0, 77, 77], dtype=torch.int32, device=DEV)
    ids, am, pos, last_row, ok = ops.decode_prompt(flat, off2, L, Np, pad_id=pad)
    assert ok.tolist() == [0, 0, 0] and pos.tolist() == [Np] * 3 and bool((ids == pad).all()) and am.sum(1).tolist() == [1, 1, 1]


# ================================================================================================================ RoPE and append
@pytest.mark.parametrize("Hq, Hkv, dh", [(4, 2, 64), (14, 2, 64), (12, 2, 128)])
def test_rope_append_writes_the_rotated_row_and_nothing_else(Hq, Hkv, dh):
    B, S_cap = 3, 288
    pos = [0, 65, S_cap - 1]
    qkv0 = gen(B, (Hq + 2 * Hkv) * dh, seed=1).to(DEV)
    cos, sin = ops.rope_half_tables(S_cap, dh, 1e6, DEV)
    kvw = Hkv * dh
    K = torch.full((B, S_cap, kvw), float("nan"), dtype=BF, device=DEV)
    V = torch.full((B, S_cap, kvw), float("nan"), dtype=BF, device=DEV)
    K0, V0 = K.clone(), V.clone()
    qkv = qkv0.clone()
    ops.decode_rope_append_(qkv, cos, sin, torch.tensor(pos, dtype=torch.int32, device=DEV), K, V, Hq, Hkv, dh)
    # the full-sequence rotation of the same values standing at row pos[b] of a [B * S_cap]-row tensor
    ref = torch.zeros(B * S_cap, (Hq + Hkv) * dh, dtype=BF, device=DEV)
    rows = [b * S_cap + p for b, p in enumerate(pos)]
    ref[rows] = qkv0[:, :(Hq + Hkv) * dh]
    ops.rope_half_(ref[:, :Hq * dh], cos, sin, S_cap, Hq, dh)
    ops.rope_half_(ref[:, Hq * dh:], cos, sin, S_cap, Hkv, dh)
    torch.cuda.synchronize()
    assert_bits_equal(qkv[:, :Hq * dh], ref[rows][:, :Hq * dh], "rotated q")
    assert_bits_equal(qkv[:, Hq * dh:], qkv0[:, Hq * dh:], "the k and v columns of qkv stay")
    for b, p in enumerate(pos):
        assert_bits_equal(K[b, p], ref[rows[b], Hq * dh:], f"appended k row of sample {b}")
        assert_bits_equal(V[b, p], qkv0[b, (Hq + Hkv) * dh:], f"appended v row of sample {b}")
        K0[b, p], V0[b, p] = K[b, p], V[b, p]
    assert_bits_equal(K, K0, "every other byte of the k cache")
    assert_bits_equal(V, V0, "every other byte of the v cache")


def test_rope_append_skips_a_position_outside_the_cache():
    B, Hq, Hkv, dh, S_cap = 2, 4, 2, 64, 32
    qkv = gen(B, (Hq + 2 * Hkv) * dh, seed=2).to(DEV)
    q0 = qkv.clone()
    cos, sin = ops.rope_half_tables(S_cap, dh, 1e6, DEV)
    K = torch.full((B, S_cap, Hkv * dh), float("nan"), dtype=BF, device=DEV)
    V = K.clone()
    K0 = K.clone()
    ops.decode_rope_append_(qkv, cos, sin, torch.tensor([S_cap, -1], dtype=torch.int32, device=DEV), K, V, Hq, Hkv, dh)
    torch.cuda.synchronize()
    assert_bits_equal(qkv, q0, "qkv")
    assert_bits_equal(K, K0, "k cache")
    assert_bits_equal(V, K0, "v cache")


# ================================================================================================================ attention
POSITIONS = [0, TILE - 1, TILE, TILE + 1, TILE * WAVES - 1, TILE * WAVES, TILE * WAVES + 1, 287]


@pytest.mark.parametrize("Hq, Hkv, dh", [(4, 2, 64), (14, 2, 64), (12, 2, 128)])
def test_single_query_attention_over_the_cache(Hq, Hkv, dh):
    B, S_cap = 3, 288
    assert POSITIONS[-1] == S_cap - 1
    kvw = Hkv * dh
    Kc, Vc = gen(B, S_cap, kvw, seed=3), gen(B, S_cap, kvw, seed=4)
    worst = 0.0
    for c in range(0, len(POSITIONS) + 1, B):
        pos = (POSITIONS + [1])[c:c + B]
        q = gen(B, Hq * dh, seed=5 + c)
        K, V = Kc.clone(), Vc.clone()
        for b, p in enumerate(pos):                   # behind pos[b]: poison that must not reach the output
            K[b, p + 1:] = float("nan")
            V[b, p + 1:] = float("nan")
        out = ops.decode_attn(q.to(DEV), K.to(DEV), V.to(DEV), torch.tensor(pos, dtype=torch.int32, device=DEV), Hq, Hkv, dh)
        torch.cuda.synchronize()
        out = out.cpu().view(B, Hq, dh)
        assert bool(torch.isfinite(out.float()).all()), f"pos {pos}: a key behind pos[b] reached the output"
        for b, p in enumerate(pos):
            qb = q[b].view(1, Hq, 1, dh)
            kb = Kc[b, :p + 1].view(1, p + 1, Hkv, dh).transpose(1, 2)
            vb = Vc[b, :p + 1].view(1, p + 1, Hkv, dh).transpose(1, 2)
            emu = O.attention(qb.float(), kb.float(), vb.float(), False, emu=True)[0, :, 0]
            t64 = O.attention(qb.double(), kb.double(), vb.double(), False, emu=False)[0, :, 0]
            worst = max(worst, A.assert_row_budget(out[b], emu, t64, 1, A.ATTN_FACTOR, A.ATTN_FLOOR, name=f"decode_attn pos {p}"))
            if p == 0:                                # one key: the output is that v row, bit for bit
                want = Vc[b, 0].view(Hkv, 1, dh).expand(Hkv, Hq // Hkv, dh).reshape(Hq, dh)
                assert_bits_equal(out[b], want, "one key")
    print(f"decode_attn ({Hq}, {Hkv}, {dh}): worst row at {worst:.2f} of its budget")


# ================================================================================================================ lm_head argmax
_OPERANDS = {}


def lm_operands(B, D, V):
    """x [B, D] and W [V, D] of one shape, made once (the largest W is 272 MB) and never written by a test: cases plant into copies of
    single rows."""
    if (B, D, V) not in _OPERANDS:
        g = torch.Generator(device=DEV).manual_seed(B * 7 + D)
        W = (torch.randn(V, D, device=DEV, generator=g) * 0.05).to(BF)
        x = torch.randn(B, D, device=DEV, generator=g).to(BF)
        _OPERANDS[(B, D, V)] = (x, W)
    return _OPERANDS[(B, D, V)]


SHAPES = [(1, 64, 1016), (5, 256, 4104), (2, 896, 151936)]


def run_argmax(x, W):
    B, V = x.shape[0], W.shape[0]
    logits = torch.full((B, V), float("nan"), dtype=BF, device=DEV)
    ids = ops.decode_lm_head_argmax(x, W, ops.decode_argmax_workspace(B, V, DEV), logits_out=logits)
    torch.cuda.synchronize()
    return ids.cpu(), logits.cpu()


@pytest.mark.parametrize("B, D, V", SHAPES)
def test_argmax_of_random_rows_and_the_stored_logits(B, D, V):
    x, W = lm_operands(B, D, V)
    ids, logits = run_argmax(x, W)
    for b in range(B):
        assert int(ids[b]) == rule_argmax(logits[b]), f"row {b}: the id is not the rule's argmax of the logits that were compared"
    truth = x.cpu().double() @ W.cpu().double().t()
    frac = A.assert_contract(logits, truth, acc_floor=A.acc_floor(x, W), max_frac=A.GEMM_MAX_FRAC, name=f"lm_head logits {B}x{D}x{V}")
    print(f"lm_head logits ({B}, {D}, {V}): {frac:.3%} of the elements differ from RN(truth)")
    # without logits_out: the same ids
    ids2 = ops.decode_lm_head_argmax(x, W, ops.decode_argmax_workspace(B, V, DEV)).cpu()
    assert ids2.tolist() == ids.tolist()


def planted(case, B, D, V):
    """(W with planted rows, expected id of sample 0 or of all samples)."""
    x, W = lm_operands(B, D, V)
    big = (x[0].float() * (64.0 / x[0].float().pow(2).sum())).to(BF)             # logit of sample 0 about 64; the random ones: 0.05 sqrt(D) N(0, 1)
    last_slab = (V - 1) // SLAB * SLAB
    rows = {"first": [0], "last": [V - 1], "last_slab": [min(last_slab + 3, V - 2)], "tie": [40, 41, V - 2]}.get(case)
    W = W.clone()
    if case == "nan":
        W[7] = float("nan")
        W[V - 5] = float("nan")
        return x, W, 7, True
    for r in rows:
        W[r] = big
    return x, W, rows[0], False


@pytest.mark.parametrize("case", ["first", "last", "last_slab", "tie", "nan"])
@pytest.mark.parametrize("B, D, V", SHAPES)
def test_argmax_planted_winners(B, D, V, case):
    x, W, want, every_row = planted(case, B, D, V)
    ids, logits = run_argmax(x, W)
    assert int(ids[0]) == want, f"{case}: sample 0 chose {int(ids[0])}, planted {want}"
    if case == "tie":
        assert bits(logits[0, 40:42]).tolist() == [int(bits(logits[0, V - 2:V - 1])[0])] * 2, "identical rows of W give identical logits"
    for b in range(B):
        assert int(ids[b]) == rule_argmax(logits[b])
        if every_row:
            assert int(ids[b]) == want


def test_advance_writes_the_token_its_embedding_and_the_counters():
    B, D, V, T = 5, 256, 4104, 4
    x, W = lm_operands(B, D, V)
    ws = ops.decode_argmax_workspace(B, V, DEV)
    want = ops.decode_lm_head_argmax(x, W, ws).cpu()
    embed = gen(V, D, seed=9).to(DEV)
    out_ids = torch.full((B, T), -7, dtype=torch.int64, device=DEV)
    step = torch.tensor([2], dtype=torch.int32, device=DEV)
    pos = torch.arange(10, 10 + B, dtype=torch.int32, device=DEV)
    x_next = torch.full((B, D), float("nan"), dtype=BF, device=DEV)
    ops.decode_lm_head_argmax(x, W, ws, advance=(out_ids, step, pos, embed, x_next))
    torch.cuda.synchronize()
    assert out_ids[:, 2].cpu().tolist() == want.tolist() and bool((out_ids[:, [0, 1, 3]] == -7).all())
    assert_bits_equal(x_next, embed[want.to(DEV)], "x_next")
    assert step.item() == 3 and pos.cpu().tolist() == list(range(11, 11 + B))
    # the first advance of a generation: counts from 0 whatever the counter holds, positions from pos_from
    pos_from = torch.arange(100, 100 + B, dtype=torch.int32, device=DEV)
    ops.decode_lm_head_argmax(x, W, ws, advance=(out_ids, step, pos, embed, x_next), pos_from=pos_from)
    torch.cuda.synchronize()
    assert out_ids[:, 0].cpu().tolist() == want.tolist() and step.item() == 1 and pos.cpu().tolist() == list(range(101, 101 + B))
    # a counter at T: no token is written, nothing behind out_ids is touched
    step.fill_(T)
    before = out_ids.clone()
    ops.decode_lm_head_argmax(x, W, ws, advance=(out_ids, step, pos, embed, x_next))
    torch.cuda.synchronize()
    assert bool((out_ids == before).all()) and step.item() == T + 1
