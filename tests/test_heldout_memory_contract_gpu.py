"""The memory contract of the held-out validation entry points (include/vla_heldout.h), by the procedure of
tests/test_memory_contract_gpu.py: each runs on compact operands and then with every device operand a view inside a poisoned arena
(tests/arena.py) at the minimum alignment its host check accepts - acc at 8 bytes, valid at 1; outputs must be bit-equal, inputs
unchanged, and nothing written outside the declared extent.  The index tables' arenas are poisoned with in-range values that would
change the result, pred / target with NaN and valid with 1, so a read one element past an operand shows.
COVERED / EXEMPT: tests/test_abi_families.py checks on the CPU that they cover the "heldout" family of native.FAMILIES."""
import numpy as np
import pytest
import torch

from tests.test_heldout_cpu import make_pair, make_store
from tests.test_memory_contract_gpu import F64, I32, I64, U8, call, case_for, contract, gen
from vla_adapter_amd import heldout as HO

COVERED = {}
EXEMPT = {}                      # both entry points have a device footprint


case = case_for(COVERED)


@case("vla_heldout_sweep")
@pytest.mark.parametrize("B, j", [(6, 0), (70, 0)], ids=["one-wave", "two-waves"])
@pytest.mark.parametrize("source", ["store", "mix"])
def test_heldout_sweep_contract(source, B, j):
    """Batch 0 of rank 1 of 2: at B = 6 windows 6 .. 11 (partly valid: the store holds 8, the mix 10), at B = 70 every sample is invalid
    and the scan runs across two waves.  The store passes dataset_off NULL."""
    if source == "store":
        _, s = make_store("cpu")
        ds_off, D = None, 1
    else:
        _, s = make_pair("cpu")
        ds_off, D = s.dataset_off_host, s.D
    val, eo, po = s.val_off_host, s.episode_off, s.prompt_off
    E, Pmax = s.E, s.Pmax

    def body(mk):
        vo, e_off = mk.inp(val, align=8, poison=3, name="val_off"), mk.inp(eo, align=8, poison=2, name="episode_off")
        p_off = mk.inp(po, align=4, poison=1, name="prompt_off")
        d_off = mk.inp(ds_off, align=4, poison=1, name="dataset_off") if ds_off is not None else None
        ds, ep = mk.out((B,), I32, align=4, poison=77, name="ds"), mk.out((B,), I32, align=4, poison=77, name="ep")
        row, off = mk.out((B,), I64, align=8, poison=7, name="row"), mk.out((B + 1,), I32, align=4, poison=77, name="out_off")
        valid = mk.out((B,), U8, align=1, poison=9, name="valid")
        call("vla_heldout_sweep", vo, e_off, p_off, d_off, E, D, 1, 2, j, 1, B, Pmax, ds, ep, row, off, valid)
        return {"ds": ds, "ep": ep, "row": row, "out_off": off, "valid": valid}

    rc, _ = contract(body)
    want = HO.sweep_windows(val.tolist(), None if ds_off is None else ds_off.tolist(), B, 1, 2, j, 1)
    lens = po.diff().tolist()
    assert rc["valid"].tolist() == [ok for ok, _, _, _ in want] and rc["ds"].tolist() == [d for _, d, _, _ in want]
    assert rc["ep"].tolist() == [e for _, _, e, _ in want] and rc["row"].tolist() == [int(eo[e]) + t for _, _, e, t in want]
    assert rc["out_off"].tolist() == [sum(lens[e] for _, _, e, _ in want[:b]) for b in range(B + 1)]
    assert sum(rc["valid"].tolist()) == ((2 if source == "store" else 4) if B == 6 else 0)


@case("vla_heldout_l1_accumulate")
@pytest.mark.parametrize("B, C, A, D", [(6, 8, 7, 1), (70, 8, 7, 2), (5, 25, 14, 3)])
def test_heldout_l1_accumulate_contract(B, C, A, D):
    """acc / cnt start from values of their own (accumulators); every third row is invalid and holds NaN; ds carries one index below 0
    and one past D - 1; D == 1 passes ds NULL.  (5, 25, 14, 3): 350 cells, six workgroups of cells."""
    pred, tgt = gen(B, C, A, seed=400 + B), gen(B, C, A, seed=500 + B)
    valid = torch.tensor([0 if b % 3 == 2 else 1 for b in range(B)], dtype=U8)
    pred[valid == 0] = float("nan")
    ds = None
    if D > 1:
        ds = torch.tensor([b % D for b in range(B)], dtype=I32)
        ds[0], ds[1] = -3, D + 4
    acc0 = torch.rand(D, C, A, generator=torch.Generator().manual_seed(B), dtype=F64)
    cnt0 = torch.arange(D, dtype=I64) * 5 + 1

    def body(mk):
        p, t = mk.inp(pred, align=2, name="pred"), mk.inp(tgt, align=2, name="target")
        d = mk.inp(ds, align=4, poison=0, name="ds") if ds is not None else None
        v = mk.inp(valid, align=1, poison=1, name="valid")
        acc, cnt = mk.out(init=acc0, align=8, name="acc"), mk.out(init=cnt0, align=8, poison=11, name="cnt")
        call("vla_heldout_l1_accumulate", p, t, d, v, B, C, A, D, acc, cnt)
        return {"acc": acc, "cnt": cnt}

    rc, _ = contract(body)
    acc, cnt = HO.l1_accumulate_reference(pred.float().numpy(), tgt.float().numpy(), None if ds is None else ds.tolist(), valid.tolist(), D,
                                          acc0.numpy(), cnt0.numpy())
    assert np.array_equal(rc["acc"].cpu().numpy().view(np.int64), acc.view(np.int64)) and rc["cnt"].tolist() == cnt.tolist()
    assert bool(torch.isfinite(rc["acc"]).all())
