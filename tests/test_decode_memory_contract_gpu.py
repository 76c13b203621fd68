"""The memory contract of the entry points of include/vla_decode.h, by the procedure of tests/test_memory_contract_gpu.py: every entry
point runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum
alignment its host check accepts, with row strides larger than the width and a sample stride that is no multiple of the row stride;
the outputs must be bit-equal, the inputs unchanged and nothing written outside the declared extents.  The caches are outputs whose
declared extent is the whole [B, S_cap, Hkv dh] view: the rows an append does not own must keep their poison."""
import torch

from tests.test_memory_contract_gpu import BF, F32, I32, I64, U8, call, case_for, contract, gen, ld_of, st2, st3
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {"vla_decode_argmax_slabs": "host arithmetic only: it takes no pointer"}

case = case_for(COVERED)


@case("vla_decode_prompt")
def test_decode_prompt_contract():
    prompts = [[5, 6, 7], list(range(100, 133)), [9]]
    flat = torch.tensor([t for r in prompts for t in r], dtype=I64)
    off = torch.tensor([0, 3, 36, 37], dtype=I32)
    B, L, Np = 3, 40, 16

    def body(mk):
        f = mk.inp(flat, align=8, poison=77, name="prompt_flat")
        o = mk.inp(off, align=4, poison=1, name="prompt_off")
        ids = mk.out((B, L), I64, align=8, poison=-3, name="ids")
        am = mk.out((B, L), U8, align=1, name="attention_mask")
        pos, last = mk.out((B,), I32, align=4, poison=-9, name="pos"), mk.out((B,), I32, align=4, poison=-9, name="last_row")
        ok = mk.out((B,), U8, align=1, name="row_ok")
        call("vla_decode_prompt", f, o, flat.numel(), ids, am, pos, last, ok, B, L, Np, 1023)
        return dict(ids=ids, am=am, pos=pos, last=last, ok=ok)

    rc, _ = contract(body)
    assert rc["pos"].cpu().tolist() == [Np + len(r) - 1 for r in prompts]


def _cache(mk, B, S_cap, kvw, name, init=None):
    """One layer's cache as an output arena: row stride above the width, sample stride no multiple of it."""
    return mk.out((B, S_cap, kvw), BF, strides=st3(B, S_cap, kvw), align=16, init=init, name=name)


@case("vla_decode_rope_append")
def test_decode_rope_append_contract():
    B, Hq, Hkv, dh, S_cap = 3, 4, 2, 64, 40
    W, kvw = (Hq + 2 * Hkv) * dh, Hkv * dh
    cos, sin = ops.rope_half_tables(S_cap, dh, 1e6, "cpu")
    pos = torch.tensor([0, 17, S_cap - 1], dtype=I32)

    def body(mk):
        qkv = mk.out(strides=st2(B, W), align=2, init=gen(B, W, seed=1), name="qkv", cld=W)
        c, s = mk.inp(cos, align=4, name="cos"), mk.inp(sin, align=4, name="sin")
        p = mk.inp(pos, align=4, poison=S_cap - 2, name="pos")
        K, V = _cache(mk, B, S_cap, kvw, "k_cache"), _cache(mk, B, S_cap, kvw, "v_cache")
        call("vla_decode_rope_append", qkv, c, s, p, K, V, B, Hq, Hkv, dh, qkv.stride(0), S_cap, K.stride(0), K.stride(1))
        return dict(qkv=qkv, K=K, V=V)

    rc, _ = contract(body)
    K = rc["K"].float().cpu()
    written = torch.zeros(B, S_cap, dtype=torch.bool)
    written[torch.arange(B), pos.long()] = True
    assert bool(torch.isfinite(K[written]).all()) and bool(torch.isnan(K[~written]).all()), "exactly row pos[b] of every sample is written"


@case("vla_decode_attn")
def test_decode_attn_contract():
    B, Hq, Hkv, dh, S_cap = 3, 14, 2, 64, 80
    kvw = Hkv * dh
    pos = torch.tensor([0, 64, 70], dtype=I32)
    Kd, Vd = gen(B, S_cap, kvw, seed=2), gen(B, S_cap, kvw, seed=3)
    for b in range(B):                                     # behind pos[b]: poison, as in the arena's gaps
        Kd[b, int(pos[b]) + 1:] = float("nan")
        Vd[b, int(pos[b]) + 1:] = float("nan")

    def body(mk):
        q = mk.inp(gen(B, Hq * dh, seed=4), strides=st2(B, Hq * dh), align=2, name="q")
        K = mk.inp(Kd, strides=st3(B, S_cap, kvw), align=16, name="k_cache")
        V = mk.inp(Vd, strides=st3(B, S_cap, kvw), align=16, name="v_cache")
        p = mk.inp(pos, align=4, poison=S_cap - 1, name="pos")
        out = mk.out((B, Hq * dh), BF, strides=st2(B, Hq * dh), align=2, name="out")
        call("vla_decode_attn", q, K, V, p, out, B, Hq, Hkv, dh, q.stride(0), out.stride(0), S_cap, K.stride(0), K.stride(1), float(dh ** -0.5))
        return dict(out=out)

    rc, _ = contract(body)
    assert bool(torch.isfinite(rc["out"].float()).all())


@case("vla_decode_lm_head_argmax")
def test_decode_lm_head_argmax_contract():
    B, D, V, T = 3, 64, 1016, 4
    n_slab = ops._lib().vla_decode_argmax_slabs(V)
    xd, Wd, Ed = gen(B, D, seed=5), gen(V, D, seed=6, scale=0.05), gen(V, D, seed=7)

    def body(mk):
        x = mk.inp(xd, strides=(ld_of(D), 1), align=16, name="x")
        W = mk.inp(Wd, strides=(ld_of(D), 1), align=16, name="W")
        E = mk.inp(Ed, strides=(ld_of(D), 1), align=16, name="embed")
        pv, pi = mk.out((B, n_slab), F32, align=4, name="part_val"), mk.out((B, n_slab), I32, align=4, poison=-1, name="part_idx")
        ids = mk.out((B,), I64, align=8, poison=-5, name="id")
        logits = mk.out((B, V), BF, strides=(V + 3, 1), align=2, name="logits_out")
        out_ids = mk.out(dtype=I64, align=8, poison=-3, init=torch.full((B, T), -7, dtype=I64), name="out_ids")
        step = mk.out(dtype=I32, align=4, poison=2, init=torch.tensor([1], dtype=I32), name="step")
        pos = mk.out(dtype=I32, align=4, poison=9, init=torch.tensor([3, 4, 5], dtype=I32), name="pos")
        xn = mk.out((B, D), BF, strides=(ld_of(D), 1), align=16, name="x_next")
        call("vla_decode_lm_head_argmax", x, x.stride(0), W, W.stride(0), B, D, V, pv, pi, ids, logits, logits.stride(0), out_ids, T, step, pos,
             None, E, V, E.stride(0), xn, xn.stride(0))
        return dict(ids=ids, logits=logits, out_ids=out_ids, step=step, pos=pos, x_next=xn, pv=pv, pi=pi)

    rc, _ = contract(body)
    assert rc["step"].item() == 2 and rc["pos"].cpu().tolist() == [4, 5, 6]
    assert rc["out_ids"][:, 1].cpu().tolist() == rc["ids"].cpu().tolist() and bool((rc["out_ids"][:, [0, 2, 3]] == -7).all())
