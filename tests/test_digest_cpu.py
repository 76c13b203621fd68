"""CPU checks of the state digest (include/vla_digest.h): the ordered token-CE sum's signature beside
vla_token_ce_metrics', the entry points' and the host wrapper's refusals, and the rule itself in numpy (tests/digest_rule_np.py) -
vectorised form against plain Python integers, sensitivity to a swap, to a +1 / -1 pair and to an appended zero word, independence of
the summation order, independence of where the view lies."""
import numpy as np
import pytest

from tests import digest_rule_np as R

SIZES = [1, 3, 4, 5, 7, 8, 9, 65539]


def words(n, seed=0):
    return np.random.default_rng(seed).integers(0, 1 << 16, size=n, dtype=np.uint16)


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def test_the_ordered_sum_takes_token_ce_metrics_operands_and_the_per_row_terms():
    from vla_adapter_amd import native
    assert native.family("digest").protos["vla_token_ce_metrics_ordered"][0][:-1] == native.family("native").protos["vla_token_ce_metrics"][0]


def test_host_checks_refuse_bad_arguments(lib):
    """The entry points' own argument checks answer before anything is launched (no device needed)."""
    P = 64
    dg = lambda **kw: lib.vla_state_digest(None, kw.get("x", P), kw.get("n", 8), 0, kw.get("scratch", P), kw.get("slots", 4), kw.get("out", P))
    assert dg(n=0) == -1 and b"n >= 1" in lib.vla_last_error()
    assert dg(n=-5) == -1
    assert dg(x=None) == -1 and b"null" in lib.vla_last_error()
    assert dg(out=None) == -1 and b"null" in lib.vla_last_error()
    assert dg(x=65) == -1 and b"2-byte" in lib.vla_last_error()
    assert dg(out=68) == -1 and b"8-byte" in lib.vla_last_error()
    assert dg(scratch=68) == -1 and b"8-byte" in lib.vla_last_error()
    assert dg(scratch=None, slots=4) == -1 and b"null scratch" in lib.vla_last_error()
    assert dg(slots=-1) == -1
    assert lib.vla_state_digest_slots() >= 1
    assert lib.vla_token_ce_metrics_ordered(None, P, 16, P, P, 3, 11, P, P, None, 12, 8, None) == -1 and b"terms" in lib.vla_last_error()
    assert lib.vla_token_ce_metrics_ordered(None, P, 16, P, P, 0, 11, P, P, None, 12, 8, P) == -1


def test_the_wrapper_refuses_an_empty_or_wide_operand():
    """ops.state_digest looks at its operand before it loads the library or touches a device."""
    import torch
    from vla_adapter_amd import ops
    with pytest.raises(AssertionError, match="16-bit"):
        ops.state_digest(torch.zeros(4, dtype=torch.bfloat16))          # not on the device
    assert ops.digest_value(-1) == 2 ** 64 - 1 and ops.digest_value(torch.tensor([-2])) == 2 ** 64 - 2 and ops.digest_value(5) == 5


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_the_chunks_are_little_endian_and_zero_padded():
    q = R.chunks(np.array([0x1111, 0x2222, 0x3333, 0x4444, 0xABCD], dtype=np.uint16))
    assert q.tolist() == [0x4444333322221111, 0xABCD] and q.dtype == np.uint64
    assert R.chunks(np.array([1], dtype=np.int16)).tolist() == [1]
    assert R.chunks(np.array([-1], dtype=np.int16)).tolist() == [0xFFFF], "the bits count, not the dtype"


def test_the_weights_are_the_documented_mixer():
    for salt in (0, 7, 2 ** 64 - 1):
        w = R.weights(5, salt)
        for c in range(5):
            z = (c + R.GOLDEN * (((salt & R.M64) + 1))) & R.M64
            z = ((z ^ z >> 30) * R.MUL1) & R.M64
            z = ((z ^ z >> 27) * R.MUL2) & R.M64
            z ^= z >> 31
            assert int(w[c]) == z | 1 and int(w[c]) & 1
    assert len(set(R.weights(4096).tolist())) == 4096


@pytest.mark.parametrize("salt", [0, 12345])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 1027])
def test_numpy_equals_python_integers(n, salt):
    w = words(n, seed=n)
    assert R.digest(w, salt) == R.digest_python(w, salt)


def test_one_word_by_hand():
    """n = 1, word 0: q_0 = 0, so the digest is the first weight plus the length constant."""
    assert R.digest(np.zeros(1, dtype=np.uint16)) == (int(R.weights(1)[0]) + R.LENGTH) & R.M64
    assert R.digest(np.array([2], dtype=np.uint16)) == (3 * int(R.weights(1)[0]) + R.LENGTH) & R.M64


def test_an_empty_view_is_refused():
    with pytest.raises(ValueError, match="empty"):
        R.digest(np.zeros(0, dtype=np.uint16))


@pytest.mark.parametrize("n", SIZES + [2 ** 22 + 5])
def test_summation_order_does_not_show(n):
    """Reversed, shuffled and in blocks of 256 terms summed first: a wrapping sum has one value."""
    w = words(n, seed=n + 1)
    t = R.terms(w, 3)
    want = R.digest(w, 3)
    tail = (n * R.LENGTH) & R.M64
    rng = np.random.default_rng(n)
    for order in (t[::-1], rng.permutation(t)):
        assert (int(np.add.reduce(order, dtype=np.uint64)) + tail) & R.M64 == want
    pad = np.concatenate([t, np.zeros(-t.size % 256, dtype=np.uint64)]).reshape(-1, 256)
    partial = np.add.reduce(pad, axis=1, dtype=np.uint64)
    assert (int(np.add.reduce(partial[::-1], dtype=np.uint64)) + tail) & R.M64 == want
    py = 0
    for v in t[:1000].tolist():
        py = (py + v) & R.M64
    assert py == int(np.add.reduce(t[:1000], dtype=np.uint64))


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 3] + [2 ** 22 + 5])
def test_a_swap_a_plus_minus_pair_and_an_appended_zero_change_it(n):
    """What a plain sum of bit patterns (ddp.params_checksum) cannot see."""
    w = words(n, seed=n + 2)
    w[0], w[n - 1] = 0x0102, 0x0304                      # unequal, away from the wrap-around of a +1 / -1
    base = R.digest(w)
    for i, j in {(0, n - 1), (0, 1), (n - 2, n - 1), (n // 2, n - 1)}:
        if i != j and w[i] != w[j]:
            s = w.copy()
            s[i], s[j] = w[j], w[i]
            assert R.digest(s) != base, f"swap of words {i} and {j}"
            assert int(s.astype(np.uint64).sum()) == int(w.astype(np.uint64).sum()), "the plain sum is blind to it"
    for i, j in {(0, n - 1), (0, 1), (n // 2, n - 1)}:
        if i != j:
            s = w.copy()
            s[i] += 1
            s[j] -= 1
            assert R.digest(s) != base, f"+1 at {i}, -1 at {j}"
            assert int(s.astype(np.uint64).sum()) == int(w.astype(np.uint64).sum())
    assert R.digest(np.concatenate([w, np.zeros(1, dtype=np.uint16)])) != base, "an appended zero word (same chunks when n % 4 != 0)"
    assert R.digest(w, 1) != base, "another salt"


def test_a_swap_inside_one_chunk_changes_it():
    w = np.array([5, 9, 9, 9, 1], dtype=np.uint16)
    s = w.copy()
    s[0], s[1] = w[1], w[0]
    assert R.digest(s) != R.digest(w)


def test_the_digest_does_not_depend_on_where_the_view_lies():
    """The chunk index counts from the view's first word: the same words at offsets 0, 1 and 3 of a larger buffer."""
    w = words(1001, seed=9)
    for off in (0, 1, 3):
        buf = words(1001 + 8, seed=10)
        buf[off:off + 1001] = w
        assert R.digest(buf[off:off + 1001]) == R.digest(w)
