"""The memory contract of the entry point of include/vla_sample.h, by the procedure of tests/test_memory_contract_gpu.py: it runs on
compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum alignment its host
check accepts, the logits and the probabilities with a row stride larger than V (and odd, so that rows start on 2-B boundaries); the
outputs must be bit-equal, the inputs unchanged and nothing written outside the declared extents - with logprob_out / probs_out NULL
and not NULL, with and without the advance, and on a non-finite row."""
import pytest
import torch

from tests.test_memory_contract_gpu import BF, F32, I32, I64, call, case_for, contract, gen, ld_of
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {}

case = case_for(COVERED)

B, V, D, T = 3, 1016, 64, 4


def _logits(nan_row=None):
    l = gen(B, V, seed=11, scale=4.0)
    if nan_row is not None:
        l[nan_row, 321] = float("nan")
    return l


def _params(**kw):
    return ops.sample_params(**kw)


@case("vla_sample_tokens")
@pytest.mark.parametrize("outputs", ["none", "logprobs", "probs", "both"])
def test_sample_tokens_contract(outputs):
    logits, blk = _logits(), _params(temperature=0.8, top_k=40, top_p=0.9, seed=5)
    streams = torch.tensor([4, 1 << 40, 9], dtype=I64)

    def body(mk):
        l = mk.inp(logits, strides=(V + 3, 1), align=2, name="logits")
        p = mk.inp(blk, align=8, name="params")
        s = mk.inp(streams, align=8, poison=77, name="streams")
        step = mk.inp(torch.tensor([2], dtype=I32), align=4, poison=1, name="step")
        ids = mk.out((B,), I64, align=8, poison=-5, name="id")
        lp = mk.out((B, T), F32, align=4, name="logprob_out") if outputs in ("logprobs", "both") else None
        pr = mk.out((B, V), F32, strides=(V + 5, 1), align=4, name="probs_out") if outputs in ("probs", "both") else None
        call("vla_sample_tokens", l, l.stride(0), B, V, p, s, ids, lp, pr, pr.stride(0) if pr is not None else 0, None, T, step, None, None,
             None, 0, 0, None, 0, 0)
        out = dict(ids=ids)
        if lp is not None:
            out["logprobs"] = lp
        if pr is not None:
            out["probs"] = pr
        return out

    rc, _ = contract(body)
    assert bool(((rc["ids"] >= 0) & (rc["ids"] < V)).all())
    if "logprobs" in rc:
        lp = rc["logprobs"]
        assert bool(torch.isfinite(lp[:, 2]).all()) and bool(torch.isnan(lp[:, [0, 1, 3]]).all()), "exactly column t is written"
    if "probs" in rc:
        kept = (rc["probs"] != 0).sum(dim=1)
        assert bool(torch.isfinite(rc["probs"]).all()) and bool(((kept >= 1) & (kept < V)).all())


@case("vla_sample_tokens")
@pytest.mark.parametrize("first", [False, True])
def test_sample_tokens_advance_contract(first):
    logits, blk = _logits(nan_row=1), _params(temperature=1.2, top_k=0, top_p=0.95, seed=6)
    Ed = gen(V, D, seed=7)

    def body(mk):
        l = mk.inp(logits, strides=(V + 3, 1), align=2, name="logits")
        p = mk.inp(blk, align=8, name="params")
        E = mk.inp(Ed, strides=(ld_of(D), 1), align=16, name="embed")
        pf = mk.inp(torch.tensor([30, 40, 50], dtype=I32), align=4, poison=9, name="pos_from") if first else None
        ids = mk.out((B,), I64, align=8, poison=-5, name="id")
        lp = mk.out((B, T), F32, align=4, name="logprob_out")
        pr = mk.out((B, V), F32, strides=(V + 5, 1), align=4, name="probs_out")
        out_ids = mk.out(dtype=I64, align=8, poison=-3, init=torch.full((B, T), -7, dtype=I64), name="out_ids")
        step = mk.out(dtype=I32, align=4, poison=2, init=torch.tensor([1], dtype=I32), name="step")
        pos = mk.out(dtype=I32, align=4, poison=9, init=torch.tensor([3, 4, 5], dtype=I32), name="pos")
        xn = mk.out((B, D), BF, strides=(ld_of(D), 1), align=16, name="x_next")
        call("vla_sample_tokens", l, l.stride(0), B, V, p, None, ids, lp, pr, pr.stride(0), out_ids, T, step, pos, pf, E, V, E.stride(0), xn,
             xn.stride(0), D)
        return dict(ids=ids, logprobs=lp, probs=pr, out_ids=out_ids, step=step, pos=pos, x_next=xn)

    rc, _ = contract(body)
    t = 0 if first else 1
    assert rc["step"].item() == t + 1 and rc["pos"].cpu().tolist() == ([31, 41, 51] if first else [4, 5, 6])
    assert rc["out_ids"][:, t].cpu().tolist() == rc["ids"].cpu().tolist() and bool((rc["out_ids"][:, [c for c in range(T) if c != t]] == -7).all())
    assert rc["ids"][1].item() == 321 and bool(torch.isnan(rc["logprobs"][1, t])) and bool(torch.isnan(rc["probs"][1]).all()), "the NaN row"
    assert bool(torch.isfinite(rc["logprobs"][[0, 2], t]).all()) and bool(torch.isfinite(rc["probs"][[0, 2]]).all())
    assert torch.equal(rc["x_next"].view(torch.int16), Ed.to(rc["x_next"].device)[rc["ids"]].view(torch.int16))
