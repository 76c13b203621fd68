"""The vectorised restatement of the sampling rules (tests/episode_rule_np.py) against the scalar rules of episodes.py, mixture.py and
heldout.py, which stay the specification: every position where that is cheap, seeded positions at the extents of a real dataset - 10^5
to 10^6 windows, stream positions 10^13 along, window counts beyond 2^32 and up to 2^62 - and the bijection on whole domains of that
size.  tests/test_episodes_scale_gpu.py then holds the kernels against the vector rule at every position of whole epochs."""
import numpy as np
import pytest
import torch

from tests import episode_rule_np as R
from tests.test_episodes_cpu import CHUNK, LENGTHS
from tests.test_heldout_cpu import make_pair, make_store
from tests.test_mixture_cpu import make_mix
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import heldout as HO
from vla_adapter_amd import mixture as MX

P9 = 4 ** 9                                                 # 262 144: the Feistel domain is exactly N, no walking
SCALE_N = (P9, P9 + 1, 2 * P9 - 3, 1_500_007)               # P9 + 1: the domain is 4 N, the longest walks
KEYS = (0, 2 ** 64 - 1, EP.epoch_key(0, 0), EP.epoch_key(0, 3), EP.epoch_key(12345, 0), EP.epoch_key(12345, 3))
WIDE_N = (2 ** 32 + 1, 2 ** 40 + 12345, 2 ** 62 + 1)


# ---------------------------------------------------------------------------------------------------------------- tables of real extent
def scale_tables(N: int, episodes: int = 3000, short: float = 0.05, seed: int = 0, chunk: int = CHUNK) -> dict:
    """The offset tables of a store of ``episodes`` episodes that yield exactly N windows: about ``short`` of them - the first and the
    last among them - are shorter than the chunk and yield none (the binary search steps over them), the others share the N windows
    out by a seeded multinomial draw.  Prompts of 0 .. 11 ids.  Nothing but tables: int64 episode_off / valid_off, int32 prompt_off."""
    rng = np.random.default_rng(seed)
    is_short = rng.random(episodes) < short
    is_short[[0, -1]] = True
    n_long = int((~is_short).sum())
    windows = np.zeros(episodes, dtype=np.int64)
    windows[~is_short] = rng.multinomial(N - n_long, np.full(n_long, 1.0 / n_long)) + 1
    lengths = np.where(is_short, rng.integers(1, chunk, episodes), windows + chunk - 1)
    episode_off = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64)
    valid_off = EP.valid_offsets(episode_off, chunk)
    assert int(valid_off[-1]) == N and int((valid_off.diff() == 0).sum()) == int(is_short.sum()) >= 0.03 * episodes
    prompt_off = torch.tensor(np.concatenate([[0], np.cumsum(rng.integers(0, 12, episodes))]), dtype=torch.int32)
    return dict(episode_off=episode_off, valid_off=valid_off, prompt_off=prompt_off, Pmax=int(prompt_off.diff().max()))


def wide_tables(N: int, chunk: int = CHUNK) -> dict:
    """Three episodes that yield N windows in all, N beyond 32 bits: N // 3, 5 and the rest.  Offset tables only - nothing of that size
    is ever allocated - with episode_off consistent with them (an episode of n windows has n + chunk - 1 rows)."""
    windows = [N // 3, 5, N - N // 3 - 5]
    valid = np.cumsum([0] + windows, dtype=object)
    eo = np.cumsum([0] + [w + chunk - 1 for w in windows], dtype=object)
    episode_off = torch.tensor([int(x) for x in eo], dtype=torch.int64)
    valid_off = torch.tensor([int(x) for x in valid], dtype=torch.int64)
    assert EP.valid_offsets(episode_off, chunk).tolist() == valid_off.tolist() and int(valid_off[-1]) == N
    return dict(episode_off=episode_off, valid_off=valid_off, prompt_off=torch.tensor([0, 4, 4, 13], dtype=torch.int32), Pmax=9)


def scalar_window(pos: int, valid_off, seed: int):
    N = int(valid_off[-1])
    return EP.locate(EP.permute_index(pos % N, N, EP.epoch_key(seed, pos // N)), valid_off)


def unpermute_index(y: int, N: int, key: int) -> int:
    """The index permute_index sends to y: the Feistel rounds undone in reverse order, (L, R) -> (R ^ F(L), L), walked back along the
    same cycle.  With it a test can choose, by the rule alone, the batch that draws a given window."""
    if N == 1:
        return 0
    half = max(((N - 1).bit_length() + 1) // 2, 1)
    mask = (1 << half) - 1
    x = y
    while True:
        l, r = x >> half, x & mask
        for rnd in (3, 2, 1, 0):
            l, r = r ^ (EP.splitmix64_key(EP.splitmix64_key(key, rnd), l) & mask), l
        x = (l << half) | r
        if x < N:
            return x


def seeded_positions(n: int, hi: int, seed: int) -> list:
    """n seeded positions inside [0, hi) plus the first and the last, as Python ints (hi may lie beyond 2^63)."""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2 ** 63, n, dtype=np.uint64).tolist()
    return [0, hi - 1] + [w % hi for w in words]


def pairs(e, t) -> list:
    return list(zip(e.tolist(), t.tolist()))


# ---------------------------------------------------------------------------------------------------------------- every position
def test_the_pieces_equal_the_scalar_pieces():
    seeds = [0, 1, 2 ** 64 - 1, 0x9E3779B97F4A7C15, 12345]
    idx = [0, 1, 2, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    for s in seeds:
        assert R.splitmix64_key(s, idx).tolist() == [EP.splitmix64_key(s, i) for i in idx]
        assert R.epoch_key(s, idx).tolist() == [EP.epoch_key(s, i) for i in idx]
        assert R.period_key(s, idx).tolist() == [MX.period_key(s, i) for i in idx]
    values = [0, 1, 2, 3, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, 2 ** 62, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    assert R.bit_length(R.u64(values)).tolist() == [v.bit_length() for v in values]
    for half in (1, 2, 9, 16, 31, 32):
        x = [0, 1, 4 ** half - 1, (4 ** half - 1) // 3]
        got = R.feistel4(R.u64(x), R.u64(KEYS[3]), R.u64(half))
        assert got.tolist() == [EP._feistel4(v, KEYS[3], half) for v in x]
    with pytest.raises(ValueError):
        R.permute_index([5], 5, 0)


@pytest.mark.parametrize("key", KEYS[:4])
def test_permute_index_equals_the_scalar_rule_on_every_position_up_to_70(key):
    for N in range(1, 71):
        got = R.permute_index(np.arange(N, dtype=np.uint64), N, key)
        assert got.tolist() == [EP.permute_index(i, N, key) for i in range(N)], N
    # every N at once, each element with its own N and key: the form the mixture rule uses
    i = np.concatenate([np.arange(N, dtype=np.uint64) for N in range(1, 71)])
    n = np.concatenate([np.full(N, N, dtype=np.uint64) for N in range(1, 71)])
    k = R.splitmix64_key(key, n)
    assert R.permute_index(i, n, k).tolist() == [EP.permute_index(int(a), int(b), int(c)) for a, b, c in zip(i, n, k)]


@pytest.mark.parametrize("N", [2, 3, 37, 1000, P9 + 1, 2 ** 32 + 1, 2 ** 62 + 1])
def test_unpermute_index_undoes_permute_index(N):
    for key in KEYS[:3]:
        for y in {0, 1, N // 2, N - 1}:
            i = unpermute_index(y, N, key)
            assert 0 <= i < N and EP.permute_index(i, N, key) == y


def test_locate_equals_the_binary_search_on_tables_with_empty_episodes():
    for tab in ([0, 0, 0, 1, 3, 16], [0, 2, 2, 15, 16, 16, 16, 16], [0, 0, 0, 0, 0, 0, 5, 8], [0, 1], [0, 0, 7, 7, 7, 9, 9]):
        j = np.arange(tab[-1], dtype=np.uint64)
        assert pairs(*R.locate(j, tab)) == [EP.locate(int(x), tab) for x in j], tab


@pytest.mark.parametrize("world", [1, 2, 3])
def test_the_toy_store_on_every_position_of_five_epochs(world):
    valid = EP.valid_offsets(torch.tensor(np.cumsum([0] + LENGTHS)), CHUNK).tolist()
    B, seed, steps = 6, 21, -(-5 * 16 // (6 * world))
    want = [w for step in range(steps) for rank in range(world) for w in EP.sample_windows(valid, B, seed, rank, world, step)]
    assert pairs(*R.windows_at(np.arange(len(want)), valid, seed)) == want
    for step in (0, 4):
        for rank in range(world):
            assert pairs(*R.sample_windows(valid, B, seed, rank, world, step)) == EP.sample_windows(valid, B, seed, rank, world, step)
    _, s = make_store()
    got = R.windows_at(np.arange(16 * 7), s.valid_off_host, 13)
    assert pairs(*got) == [w for step in range(16) for w in EP.sample_windows(s.valid_off_host.tolist(), 7, 13, 0, 1, step)]


def test_the_toy_mix_on_every_position_of_forty_periods():
    for m in (make_mix()[1], make_pair()[1], make_mix(balance_weights=False, period=37)[1]):
        tabs = m.valid_off_host.tolist(), m.dataset_off_host.tolist(), m.quota_off_host.tolist()
        n = 40 * m.Q
        d, c, e, t = R.mixture_at(np.arange(n), *tabs, seed=7)
        assert list(zip(d.tolist(), c.tolist(), e.tolist(), t.tolist())) == [MX.sample_window(pos, *tabs, seed=7) for pos in range(n)]


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("world", [1, 2])
def test_the_toy_sweeps_on_every_batch(world, stride):
    for s, ds_off in ((make_store()[1], None), (make_pair()[1], make_pair()[1].dataset_off_host.tolist())):
        val = s.val_off_host.tolist()
        for rank in range(world):
            for j in range(HO.sweep_batches(s.Nv, stride, 6, rank, world) + 1):          # and the empty batch behind the last
                got = R.sweep_windows(val, ds_off, 6, rank, world, j, stride)
                assert list(zip(*(x.tolist() for x in got))) == HO.sweep_windows(val, ds_off, 6, rank, world, j, stride)


# ---------------------------------------------------------------------------------------------------------------- real extents
@pytest.mark.parametrize("N", SCALE_N)
def test_permute_index_equals_the_scalar_rule_at_seeded_positions(N):
    pos = seeded_positions(200, N, seed=N)
    for key in KEYS:
        assert R.permute_index(pos, N, key).tolist() == [EP.permute_index(i, N, key) for i in pos], key


@pytest.mark.parametrize("key", range(len(KEYS)))
@pytest.mark.parametrize("N", SCALE_N)
def test_permute_index_is_a_bijection_at_scale(N, key):
    """The sorted image of [0, N) is [0, N).  Largest number of Feistel passes any index took (the cycle walk), over the six keys:
    N = 262 144: 1 (the domain is N); N = 262 145: 52; N = 524 285: 20; N = 1 500 007: 38."""
    stats = {}
    i = np.arange(N, dtype=np.uint64)
    image = R.permute_index(i, N, KEYS[key], stats)
    image.sort()
    assert np.array_equal(image, i)
    print(f"N = {N}, key {key}: at most {stats['passes']} Feistel passes")
    assert (stats["passes"] == 1) == (N == P9), "no walk where the domain is exactly N, some walk everywhere else"


@pytest.mark.parametrize("rank", [0, 7])
def test_positions_far_along_the_stream(rank):
    """step = 10^9 of 8 ranks at B = 1024: position 8.2 10^12, epoch 3.1 10^7 of N = 4^9 + 1, on a 3000-episode table."""
    tab = scale_tables(P9 + 1)
    valid, B, world, step, seed = tab["valid_off"].tolist(), 1024, 8, 10 ** 9, 5
    assert EP.sample_position(B, rank, world, step, 0) // (P9 + 1) > 3 * 10 ** 7
    assert pairs(*R.sample_windows(valid, B, seed, rank, world, step)) == EP.sample_windows(valid, B, seed, rank, world, step)


@pytest.mark.parametrize("N", WIDE_N)
def test_windows_counted_beyond_32_bits(N):
    """Python integers are the truth: 200 positions up to 2^63 - 1 of a three-episode table of N windows; and the three wide tables'
    batches at step 0 and 10^9."""
    tab = wide_tables(N)
    valid = tab["valid_off"].tolist()
    for seed in (0, 12345):
        pos = seeded_positions(200, 2 ** 63, seed=seed + 1)
        got = R.windows_at(R.u64(pos), valid, seed)
        assert pairs(*got) == [scalar_window(p, valid, seed) for p in pos]
        assert max(got[1].tolist()) >= 2 ** 31, "steps inside an episode beyond 31 bits are among them"
    for step in (0, 10 ** 9):
        assert pairs(*R.sample_windows(valid, 64, 3, 5, 8, step)) == EP.sample_windows(valid, 64, 3, 5, 8, step)


def wide_mix_tables(chunk: int = CHUNK) -> dict:
    """Two datasets back to back: three episodes of 2^40 + 12 345 windows in all, then one episode of 1000; quotas 11 and 5 of a
    period of 16."""
    big = wide_tables(2 ** 40 + 12345, chunk)
    eo, valid = big["episode_off"].tolist(), big["valid_off"].tolist()
    return dict(episode_off=torch.tensor(eo + [eo[-1] + 1000 + chunk - 1], dtype=torch.int64),
                valid_off=torch.tensor(valid + [valid[-1] + 1000], dtype=torch.int64),
                prompt_off=torch.tensor([0, 4, 4, 13, 20], dtype=torch.int32), Pmax=9,
                dataset_off=torch.tensor([0, 3, 4], dtype=torch.int32), quota_off=torch.tensor([0, 11, 16], dtype=torch.int64))


def test_a_mixture_with_a_dataset_counted_beyond_32_bits():
    tab = wide_mix_tables()
    tabs = tab["valid_off"].tolist(), tab["dataset_off"].tolist(), tab["quota_off"].tolist()
    pos = seeded_positions(200, 2 ** 63, seed=9)
    d, c, e, t = R.mixture_at(R.u64(pos), *tabs, seed=4)
    assert list(zip(d.tolist(), c.tolist(), e.tolist(), t.tolist())) == [MX.sample_window(p, *tabs, seed=4) for p in pos]
    assert set(d.tolist()) == {0, 1}


def test_a_sweep_beyond_32_bits():
    val = wide_tables(2 ** 40 + 12345)["valid_off"].tolist()
    for rank, world, j, stride in ((3, 8, 5_000_000, 7), (4, 8, 2 ** 27 + 1, 1), (0, 1, 2 ** 40, 1)):
        got = R.sweep_windows(val, [0, 1, 3], 64, rank, world, j, stride)
        assert list(zip(*(x.tolist() for x in got))) == HO.sweep_windows(val, [0, 1, 3], 64, rank, world, j, stride)


def test_the_narrowed_rule_differs_exactly_where_the_window_index_passes_32_bits():
    """``width=32`` is what the GPU file's self-tests feed their comparisons: it changes a sample if and only if its window index does
    not fit 32 bits."""
    tab = wide_tables(2 ** 40 + 12345)
    valid = tab["valid_off"].tolist()
    pos = R.positions(1024, 5, 8, 10 ** 9)
    N = 2 ** 40 + 12345
    j = [EP.permute_index(int(p) % N, N, EP.epoch_key(3, int(p) // N)) for p in pos]
    full, narrow = R.windows_at(pos, valid, 3), R.windows_at(pos, valid, 3, width=32)
    differ = (full[0] != narrow[0]) | (full[1] != narrow[1])
    assert differ.tolist() == [x >= 2 ** 32 for x in j] and differ.sum() >= 1000
    small = scale_tables(P9 + 1)["valid_off"]
    assert pairs(*R.windows_at(pos, small, 3, width=32)) == pairs(*R.windows_at(pos, small, 3))
