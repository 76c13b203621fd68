"""The memory contract of the serving entry points (include/vla_serve.h), by the procedure of tests/test_memory_contract_gpu.py: each
runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum alignment
its host check accepts - strided where the entry point takes a stride; outputs must be bit-equal, inputs unchanged, and nothing written
outside the declared extent.  COVERED / EXEMPT: tests/test_abi_families.py checks on the CPU that they cover the "serve" family of native.FAMILIES."""
import pytest
import torch

from tests.arena import assert_bits_equal
from tests.test_memory_contract_gpu import BF, DEV, F32, F64, I32, I64, U8, call, case_for, contract, gen, ld_of

COVERED = {}
EXEMPT = {}                      # every serving entry point has a device footprint


case = case_for(COVERED)


@case("vla_serve_tokens")
def test_serve_tokens_contract():
    """Three good rows, one that does not fit and an empty one; L = 80 leaves room for prompts of up to 15 ids."""
    L, nt = 80, 64
    lens = [4, 15, 1, 16, 0]
    B = len(lens)
    flat = torch.arange(100, 100 + sum(lens), dtype=I64)
    off = torch.tensor([sum(lens[:i]) for i in range(B + 1)], dtype=I32)

    def body(mk):
        pf, po = mk.inp(flat, align=8, poison=55, name="prompt ids"), mk.inp(off, align=4, poison=1, name="prompt offsets")
        ids, lab = mk.out((B, L), I64, align=8, poison=7, name="input ids"), mk.out((B, L), I64, align=8, poison=7, name="labels")
        am = mk.out((B, L), U8, align=1, name="attention mask")
        hid, ok = mk.out((B,), I32, align=4, poison=77, name="hid_row"), mk.out((B,), U8, align=1, name="row_ok")
        call("vla_serve_tokens", pf, po, flat.numel(), ids, lab, am, hid, ok, B, L, nt, 1, 2, 151387, 1023, -100)
        return {"input_ids": ids, "labels": lab, "attention_mask": am, "hid_row": hid, "row_ok": ok}

    rc, _ = contract(body)
    assert rc["row_ok"].tolist() == [1, 1, 1, 0, 0] and rc["hid_row"].tolist() == [3, 14, 0, 0, 0]
    assert torch.equal(rc["input_ids"][3], rc["input_ids"][4]) and int(rc["input_ids"][3, 0]) == 1023 and int(rc["input_ids"][3, 65]) == 2
    assert rc["attention_mask"].sum(1).tolist() == [4 + 65, 15 + 65, 66, 66, 66]


@case("vla_normalize_proprio_serve")
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_normalize_proprio_serve_contract(dtype):
    D = 8
    x = gen(5, D, seed=300, scale=2.0, dtype=dtype)
    low, high = -gen(D, seed=301, dtype=F64).abs() - 0.1, gen(D, seed=302, dtype=F64).abs() + 0.1
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 0, 1], dtype=U8)

    def body(mk):
        y = mk.out((5, D), F32, align=4)
        call("vla_normalize_proprio_serve", mk.inp(x, align=x.element_size(), name="x"), int(dtype == F64), y, 5 * D, D,
             mk.inp(low, align=8, name="low"), mk.inp(high, align=8, name="high"), mk.inp(mask, align=1, poison=0, name="mask"))
        return {"normalised": y}

    rc, _ = contract(body)
    assert torch.isfinite(rc["normalised"]).all() and rc["normalised"].abs().max() <= 1


@case("vla_unnormalize_actions")
def test_unnormalize_actions_contract():
    """pred and out with row strides larger than the row; one row not ok."""
    B, chunk, Da = 3, 8, 7
    row = chunk * Da
    pred = gen(B, row, seed=310)
    low, high = -gen(Da, seed=311, dtype=F64).abs() - 0.1, gen(Da, seed=312, dtype=F64).abs() + 0.1
    mask = torch.tensor([1, 1, 1, 1, 1, 1, 0], dtype=U8)
    ok = torch.tensor([1, 0, 1], dtype=U8)

    def body(mk):
        p = mk.inp(pred, (row + 3, 1), align=2, name="pred")
        out = mk.out((B, row), F64, (row + 5, 1), align=8, name="actions")
        call("vla_unnormalize_actions", p, out, B, row, Da, p.stride(0), out.stride(0), mk.inp(low, align=8, name="low"),
             mk.inp(high, align=8, name="high"), mk.inp(mask, align=1, poison=0, name="mask"), mk.inp(ok, align=1, poison=0, name="row_ok"))
        return {"actions": out}

    rc, _ = contract(body)
    assert torch.isnan(rc["actions"][1]).all() and torch.isfinite(rc["actions"][[0, 2]]).all()


@case("vla_serve_gather_hidden")
def test_serve_gather_hidden_contract():
    """hs: one hidden state inside a larger buffer - row stride above the width, batch stride no multiple of the row stride."""
    B, S, D, T, Np = 3, 40, 72, 8, 5
    hs = gen(B, S, D, seed=320)
    hid = torch.tensor([0, 26, 11], dtype=I32)               # rows 5.., 31.. (26 + 5 + 8 = 39 <= S), 16..
    ld = ld_of(D)

    def body(mk):
        h = mk.inp(hs, (S * ld + 8, ld, 1), align=16, name="hidden state")
        out = mk.out((B, T, D), BF, align=16, name="gathered")
        call("vla_serve_gather_hidden", h, mk.inp(hid, align=4, poison=S, name="hid_row"), out, B, S, Np, T, D, h.stride(0), h.stride(1))
        return {"gathered": out}

    rc, _ = contract(body)
    for b, r in enumerate(hid.tolist()):
        assert_bits_equal(rc["gathered"][b], hs[b, Np + r:Np + r + T].to(DEV), f"sample {b}")
