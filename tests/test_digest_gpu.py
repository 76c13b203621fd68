"""The state digest kernel (csrc/digest.hip, include/vla_digest.h) against the numpy rule of tests/digest_rule_np.py, bit for bit: the
sizes around a chunk and a 16-byte group, more than one workgroup (65539) and more than the grid's cap of workgroups (2^22 + 5), views
starting 0, 1, 3 and 8 words into a buffer (16-byte loads / word by word), two salts, a second call into ``out=``; and its memory contract
on poisoned arenas by the procedure of tests/test_memory_contract_gpu.py - nothing outside ``out`` and the scratch is written, no
input changes, a read past the view would meet a NaN.  The header's third entry, vla_token_ce_metrics_ordered, against the atomic
form on the same operands, against its fixed summation order restated in numpy (bit for bit, run after run), and its memory contract.
COVERED / EXEMPT: tests/test_abi_families.py checks on the CPU that they cover the "digest" family of native.FAMILIES."""
import numpy as np
import pytest
import torch

from tests import digest_rule_np as R
from tests.test_memory_contract_gpu import F32, I32, I64, U8, call, case_for, contract, gen, st2
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {"vla_state_digest_slots": "host only: returns a constant"}
SIZES = [1, 3, 4, 5, 7, 8, 9, 65539, 2 ** 22 + 5]
SALTS = (0, 0xDEADBEEFCAFEF00D)


case = case_for(COVERED)


_WORDS = {}


def host_words(n):
    """Random 16-bit patterns (NaNs, infinities and denormals of bf16 included), made once per size."""
    if n not in _WORDS:
        _WORDS[n] = np.random.default_rng(1000 + n).integers(0, 1 << 16, size=n, dtype=np.uint16)
    return _WORDS[n]


def device_view(w: np.ndarray, offset: int) -> torch.Tensor:
    """The words as a bf16 view starting `offset` words into a larger device buffer (torch allocations are 16-byte aligned)."""
    buf = torch.full((w.size + offset + 8,), 0x7FC0, dtype=torch.int16, device="cuda")
    view = buf[offset:offset + w.size]
    view.copy_(torch.from_numpy(w.view(np.int16)))
    assert (view.data_ptr() - buf.data_ptr()) == 2 * offset and buf.data_ptr() % 16 == 0
    return view.view(torch.bfloat16)


@case("vla_state_digest")
@pytest.mark.parametrize("offset", [0, 1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_kernel_equals_the_rule(n, offset):
    w = host_words(n)
    t = device_view(w, offset)
    got = [ops.state_digest(t, salt) for salt in SALTS]
    assert all(g.dtype == torch.int64 and tuple(g.shape) == (1,) and g.is_cuda for g in got)
    for g, salt in zip(got, SALTS):
        want = R.digest(w, salt)
        assert ops.digest_value(g) == want, f"n={n} offset={offset} salt={salt:#x}: {ops.digest_value(g):#018x} != {want:#018x}"
    assert ops.digest_value(got[0]) != ops.digest_value(got[1])


@case("vla_state_digest")
@pytest.mark.parametrize("n", [9, 65539])
def test_a_second_call_into_out_and_other_16_bit_dtypes(n):
    w = host_words(n)
    t = device_view(w, 0)
    out = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    r = ops.state_digest(t, 5, out=out[1:2])
    assert r.data_ptr() == out[1:2].data_ptr()
    first = out.tolist()
    assert first[0] == first[2] == -7 and first[1] & R.M64 == R.digest(w, 5)
    ops.state_digest(t, 6, out=out[1:2])                       # the same destination again: overwritten, not accumulated
    assert out[1].item() & R.M64 == R.digest(w, 6)
    for dt in (torch.int16, torch.float16):
        assert ops.digest_value(ops.state_digest(t.view(dt))) == R.digest(w)
    one = torch.empty(1, dtype=torch.int64, device="cuda")      # one scratch slot: a single workgroup walks everything
    assert ops.digest_value(ops.state_digest(t, 5, scratch=one)) == R.digest(w, 5)


@case("vla_state_digest")
def test_the_wrapper_refuses_an_empty_view():
    with pytest.raises(ValueError, match="empty view"):
        ops.state_digest(torch.empty(0, dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(AssertionError, match="16-bit"):
        ops.state_digest(torch.zeros(4, dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError, match="16-bit"):
        ops.state_digest(torch.zeros(4, 4, dtype=torch.bfloat16, device="cuda")[:, :2])


@case("vla_state_digest")
@pytest.mark.parametrize("align", [2, 8, 16])
@pytest.mark.parametrize("n", [5, 8, 1027, 65539])
def test_state_digest_contract(n, align):
    """x at exactly `align` bytes inside a NaN-poisoned arena (16: the vector path and its tail; 2 and 8: word by word), out and the
    scratch in poisoned arenas of their own at 8 bytes."""
    w = host_words(n)
    x = torch.from_numpy(w.view(np.int16).copy()).view(torch.bfloat16)
    slots = ops._lib().vla_state_digest_slots()

    def body(mk):
        xv = mk.inp(x, align=align, name="x")
        out = mk.out((1,), I64, align=8, poison=77, name="out")
        scratch = mk.out((slots,), I64, align=8, poison=5, name="scratch")
        call("vla_state_digest", xv, n, 3, scratch, slots, out)
        return {"out": out}

    rc, _ = contract(body)
    assert rc["out"].item() & R.M64 == R.digest(w, 3)


# ---------------------------------------------------------------------------------------------------------------- the ordered token-CE sum
def ordered_sum_np(terms: np.ndarray, valid: np.ndarray) -> np.float32:
    """include/vla_digest.h, vla_token_ce_metrics_ordered: thread t adds the valid rows t, t + 256, ... in ascending order, the lanes of
    a wave by the xor butterfly 32, 16, .. 1, the four waves in index order - every addition rounded to f32."""
    part = np.zeros(256, dtype=np.float32)
    for r in range(terms.size):
        if valid[r]:
            part[r % 256] = np.float32(part[r % 256] + terms[r])
    waves = []
    for w in range(4):
        v = part[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[np.arange(64) ^ o]).astype(np.float32)
        waves.append(v[0])
    return np.float32(np.float32(np.float32(waves[0] + waves[1]) + waves[2]) + waves[3])


@case("vla_token_ce_metrics_ordered")
@pytest.mark.parametrize("rows, V", [(3, 11), (70, 2059), (600, 523)])
def test_the_ordered_token_ce_sum(rows, V):
    """Against vla_token_ce_metrics on the same operands: the same counters, argmax ids and count, per-row terms whose fixed-order sum
    (restated above) IS the reported sum, bit for bit, in every repetition; the atomic form's sum agrees within the rounding of its
    `valid` additions.  600 rows: more than two passes of the 256 threads; every seventh row is ignored."""
    g = torch.Generator().manual_seed(rows)
    logits = gen(rows, -(-V // 8) * 8, seed=rows + 1, scale=3.0).cuda()[:, :V]          # (the row stride is a multiple of 8)
    tgt = torch.randint(0, V, (rows,), generator=g)
    tgt[::7] = -100
    cls = torch.randint(0, 3, (rows,), generator=g).to(U8).cuda()
    tgt = tgt.cuda()
    valid = (tgt >= 0).cpu().numpy()

    def run(ordered):
        sums, cnt = torch.zeros(2, device="cuda"), torch.zeros(6, dtype=I64, device="cuda")
        pred = torch.full((rows,), 7, dtype=I32, device="cuda")
        terms = torch.full((rows,), float("nan"), device="cuda") if ordered else None
        ops.token_ce_metrics(logits, tgt, cls, sums, cnt, pred, V + 1, 8, terms=terms)
        return sums.cpu(), cnt.cpu(), pred.cpu(), None if terms is None else terms.cpu()
    s0, c0, p0, _ = run(False)
    s1, c1, p1, t1 = run(True)
    assert torch.equal(c0, c1) and torch.equal(p0, p1) and s1[1].item() == s0[1].item() == valid.sum()
    assert bool(torch.isfinite(t1).all()) and bool((t1[torch.from_numpy(~valid)] == 0).all()), "every slot of terms is written; ignored rows hold 0"
    want = ordered_sum_np(t1.numpy(), valid)
    assert s1[0].item() == float(want), f"{s1[0].item()!r} != {float(want)!r}"
    total = float(t1.double().sum())
    assert abs(s0[0].item() - total) <= valid.sum() * 2.0 ** -24 * abs(total) and abs(s1[0].item() - total) <= valid.sum() * 2.0 ** -24 * abs(total)
    for _ in range(3):
        s2, _, _, t2 = run(True)
        assert torch.equal(s2, s1) and torch.equal(t2, t1), "the same bits in every run"


@case("vla_token_ce_metrics_ordered")
@pytest.mark.parametrize("V", [11, 2059])
def test_token_ce_metrics_ordered_contract(V):
    """The operands of tests/test_memory_contract_gpu.py::test_token_ce, plus the terms at 4 bytes: written whole, nothing around them."""
    rows = 3
    tgt = torch.tensor([V - 2, -100, 3], dtype=I64)

    def body(mk):
        lg = mk.inp(gen(rows, V, seed=190, scale=3.0), st2(rows, V), name="logits", cld=-(-V // 8) * 8)
        t = mk.inp(tgt, align=8, poison=1, name="targets")
        cls = mk.inp(torch.tensor([1, 2, 0], dtype=U8), align=1, poison=1, name="row class")
        sums = mk.out(init=torch.zeros(2), align=4, name="sums")
        cnt = mk.out(init=torch.zeros(6, dtype=I64), align=8, poison=5, name="counters")
        pred = mk.out((rows,), I32, align=4, poison=7, name="pred ids")
        terms = mk.out((rows,), F32, align=4, name="terms")
        call("vla_token_ce_metrics_ordered", lg, lg.stride(0), t, cls, rows, V, sums, cnt, pred, V + 1, 8, terms)
        return {"sums": sums, "counters": cnt, "pred": pred, "terms": terms}

    rc, _ = contract(body)
    assert rc["sums"][1].item() == 2 and rc["terms"][1].item() == 0 and bool(torch.isfinite(rc["terms"]).all())
    assert rc["sums"][0].item() == float(np.float32(rc["terms"][0].item()) + np.float32(rc["terms"][2].item()))
