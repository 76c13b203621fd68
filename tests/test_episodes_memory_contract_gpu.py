"""The memory contract of the episode entry points (include/vla_episodes.h), by the procedure of tests/test_memory_contract_gpu.py: each
runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum alignment
its host check accepts; outputs must be bit-equal, inputs unchanged, and nothing written outside the declared extent.  The gather runs
on both arms: 16-byte chunks (384-byte rows, frames 16-B aligned) and bytes (150-byte rows; and 384-byte rows at a 1-B aligned base).
COVERED / EXEMPT: tests/test_abi_families.py checks on the CPU that they cover the "episodes" family of native.FAMILIES."""
import pytest
import torch

from tests.arena import assert_bits_equal
from tests.test_episodes_cpu import CHUNK, LENGTHS, make_tables
from tests.test_memory_contract_gpu import DEV, F32, I32, I64, U8, call, case_for, contract
from vla_adapter_amd import episodes as EP

COVERED = {}
EXEMPT = {}                      # both entry points have a device footprint


case = case_for(COVERED)


@case("vla_episode_sample")
@pytest.mark.parametrize("B", [6, 70], ids=["one-wave", "two-waves"])
def test_episode_sample_contract(B):
    """Step 2 of rank 1 of 2: at B = 6 positions 30 .. 35 (epoch 1 and 2 of the 16 windows), at B = 70 a scan across two waves."""
    d = make_tables()
    E, Pmax = len(LENGTHS), 11
    valid = EP.valid_offsets(d["episode_off"], CHUNK)

    def body(mk):
        vo, eo = mk.inp(valid, align=8, poison=3, name="valid_off"), mk.inp(d["episode_off"], align=8, poison=2, name="episode_off")
        po = mk.inp(d["prompt_off"], align=4, poison=1, name="prompt_off")
        ep, row = mk.out((B,), I32, align=4, poison=77, name="ep"), mk.out((B,), I64, align=8, poison=7, name="row")
        off = mk.out((B + 1,), I32, align=4, poison=77, name="out_off")
        call("vla_episode_sample", vo, eo, po, E, 9, 1, 2, 2, B, Pmax, ep, row, off)
        return {"ep": ep, "row": row, "out_off": off}

    rc, _ = contract(body)
    want = EP.sample_windows(valid.tolist(), B, 9, 1, 2, 2)
    assert rc["ep"].tolist() == [e for e, _ in want]
    assert rc["row"].tolist() == [int(d["episode_off"][e]) + t for e, t in want]
    lens = d["prompt_off"].diff().tolist()
    assert rc["out_off"].tolist() == [sum(lens[e] for e, _ in want[:b]) for b in range(B + 1)]


@case("vla_episode_gather")
@pytest.mark.parametrize("hw, align", [(8, 16), (5, 1), (8, 1)], ids=["chunks-of-16", "bytes-odd-row", "bytes-misaligned"])
def test_episode_gather_contract(hw, align):
    d = make_tables(hw=hw)
    E, T, A, Pd, Pmax = len(LENGTHS), sum(LENGTHS), 7, 8, 11
    valid = EP.valid_offsets(d["episode_off"], CHUNK).tolist()
    want = EP.sample_windows(valid, 6, 4, 0, 1, 1)                        # positions 6 .. 11
    eo, lens = d["episode_off"].tolist(), d["prompt_off"].diff().tolist()
    B = len(want)
    ep_t = torch.tensor([e for e, _ in want], dtype=I32)
    row_t = torch.tensor([eo[e] + t for e, t in want], dtype=I64)
    off_t = torch.tensor([sum(lens[e] for e, _ in want[:b]) for b in range(B + 1)], dtype=I32)
    row_bytes = 2 * hw * hw * 3

    def body(mk):
        fr = mk.inp(d["frames_u8"].view(T, row_bytes), align=align, name="frames")
        act, pr = mk.inp(d["actions_raw"], align=4, name="actions"), mk.inp(d["proprio_raw"], align=4, name="proprio")
        e_off, pf = mk.inp(d["episode_off"], align=8, poison=2, name="episode_off"), mk.inp(d["prompt_flat"], align=8, poison=55, name="prompt_flat")
        po = mk.inp(d["prompt_off"], align=4, poison=1, name="prompt_off")
        ep, row = mk.inp(ep_t, align=4, poison=0, name="ep"), mk.inp(row_t, align=8, poison=0, name="row")
        off = mk.inp(off_t, align=4, poison=1, name="out_off")
        ofr = mk.out((B, row_bytes), U8, align=align, name="out_frames")
        oact, opr = mk.out((B, CHUNK, A), F32, align=4, name="out_actions"), mk.out((B, Pd), F32, align=4, name="out_proprio")
        opf = mk.out((B * Pmax,), I64, align=8, poison=7, name="out_prompt")
        call("vla_episode_gather", fr, act, pr, e_off, pf, po, ep, row, off, ofr, oact, opr, opf, B, E, T, row_bytes, CHUNK, A, Pd,
             d["prompt_flat"].numel(), Pmax)
        return {"frames_u8": ofr, "actions_raw": oact, "proprio_raw": opr, "prompt_flat": opf}

    rc, _ = contract(body)
    rows = row_t.tolist()
    assert_bits_equal(rc["frames_u8"], d["frames_u8"].view(T, row_bytes)[rows].to(DEV), "frames")
    assert_bits_equal(rc["proprio_raw"], d["proprio_raw"][rows].to(DEV), "proprio")
    win = torch.tensor([EP.window_rows(r, eo[e + 1], CHUNK) for r, (e, _) in zip(rows, want)])
    assert_bits_equal(rc["actions_raw"], d["actions_raw"][win].to(DEV), "actions")
    flat = [t for e, _ in want for t in d["prompt_flat"][d["prompt_off"][e]:d["prompt_off"][e + 1]].tolist()]
    assert rc["prompt_flat"].tolist() == flat + [0] * (B * Pmax - len(flat))
