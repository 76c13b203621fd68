"""The memory contract of the mixture entry points (include/vla_mixture.h), by the procedure of tests/test_memory_contract_gpu.py: each
runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum alignment
its host check accepts; outputs must be bit-equal, inputs unchanged, and nothing written outside the declared extent.  The index
tables' arenas are poisoned with in-range values that would change the result, so a read one element past a table shows.
COVERED / EXEMPT: tests/test_abi_families.py checks on the CPU that they cover the "mixture" family of native.FAMILIES."""
import pytest
import torch

from tests.test_memory_contract_gpu import DEV, F32, I32, I64, U8, call, case_for, contract, gen
from tests.test_mixture_cpu import PERIOD, make_mix
from vla_adapter_amd import mixture as MX
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {}                      # both entry points have a device footprint


case = case_for(COVERED)


@case("vla_mixture_sample")
@pytest.mark.parametrize("B", [6, 70], ids=["one-wave", "two-waves"])
def test_mixture_sample_contract(B):
    """Step 2 of rank 1 of 2: at B = 6 positions 30 .. 35 (the end of period 1 and the start of period 2), at B = 70 more than four
    periods and a scan across two waves."""
    tables, m = make_mix("cpu")
    valid, ds_off, q_off = m.valid_off_host, m.dataset_off_host, m.quota_off_host
    eo, po = m.episode_off, m.prompt_off
    E, D, Pmax = m.E, m.D, m.Pmax

    def body(mk):
        vo, e_off = mk.inp(valid, align=8, poison=3, name="valid_off"), mk.inp(eo, align=8, poison=2, name="episode_off")
        p_off = mk.inp(po, align=4, poison=1, name="prompt_off")
        d_off, quota = mk.inp(ds_off, align=4, poison=1, name="dataset_off"), mk.inp(q_off, align=8, poison=5, name="quota_off")
        ds, ep = mk.out((B,), I32, align=4, poison=77, name="ds"), mk.out((B,), I32, align=4, poison=77, name="ep")
        row, off = mk.out((B,), I64, align=8, poison=7, name="row"), mk.out((B + 1,), I32, align=4, poison=77, name="out_off")
        call("vla_mixture_sample", vo, e_off, p_off, d_off, quota, E, D, 9, 1, 2, 2, B, Pmax, ds, ep, row, off)
        return {"ds": ds, "ep": ep, "row": row, "out_off": off}

    rc, _ = contract(body)
    want = MX.sample_windows(valid.tolist(), ds_off.tolist(), q_off.tolist(), B, 9, 1, 2, 2)
    assert rc["ds"].tolist() == [d for d, _, _ in want]
    assert rc["ep"].tolist() == [e for _, e, _ in want]
    assert rc["row"].tolist() == [int(eo[e]) + t for _, e, t in want]
    lens = po.diff().tolist()
    assert rc["out_off"].tolist() == [sum(lens[e] for _, e, _ in want[:b]) for b in range(B + 1)]
    assert PERIOD * 4 < 70 and len({d for d, _, _ in want}) == 3


@case("vla_normalize_bounds_rows")
@pytest.mark.parametrize("tables", ["mask-and-zero", "neither"])
def test_normalize_bounds_rows_contract(tables):
    """R = 5 rows of 8 x 7 elements over three statistics sets; sel holds one value below 0 and one past n_sets - 1 (inside the arena):
    those rows come back as the clamped set's rows, and every row equals the single-set kernel on that row with that set."""
    R, chunk, D, n_sets = 5, 8, 7, 3
    x = gen(R, chunk, D, seed=300, dtype=F32) * 2
    low, high = -gen(n_sets, D, seed=301, dtype=F32).abs() - 0.1, gen(n_sets, D, seed=302, dtype=F32).abs() + 0.1
    sel = torch.tensor([2, -4, 1, 7, 0], dtype=I32)
    clamped = [2, 0, 1, 2, 0]
    mask = torch.tensor([[1] * 7, [1, 1, 0, 1, 1, 1, 0], [1] * 6 + [0]], dtype=U8) if tables == "mask-and-zero" else None
    zero = torch.tensor([[0] * 7, [0] * 7, [0, 0, 0, 1, 0, 0, 0]], dtype=U8) if tables == "mask-and-zero" else None

    def body(mk):
        xi, y = mk.inp(x, align=4, name="x"), mk.out((R, chunk, D), F32, align=4, name="y")
        lo, hi = mk.inp(low, align=4, name="low"), mk.inp(high, align=4, name="high")
        s = mk.inp(sel, align=4, poison=1, name="sel")
        mi = mk.inp(mask, align=1, poison=0, name="mask") if mask is not None else None
        zi = mk.inp(zero, align=1, poison=1, name="zero mask") if zero is not None else None
        call("vla_normalize_bounds_rows", xi, y, R, chunk * D, D, s, n_sets, lo, hi, mi, zi)
        return {"normalised": y}

    rc, _ = contract(body)
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    for r, s in enumerate(clamped):
        want = ops.normalize_bounds(x[r].to(DEV).contiguous(), dv(low[s]), dv(high[s]), dv(None if mask is None else mask[s]),
                                    dv(None if zero is None else zero[s]))
        assert torch.equal(rc["normalised"][r].view(torch.int32), want.view(torch.int32)), f"row {r}: set {s}"
    if tables == "mask-and-zero":
        assert (rc["normalised"][0][:, 3] == 0).all() and torch.equal(rc["normalised"][2][:, 2].cpu(), x[2][:, 2]), "zeroed / unmasked columns"
