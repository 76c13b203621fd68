"""The episode data path at a real dataset's extents (csrc/episodes.hip, csrc/mixture.hip, csrc/heldout.hip, csrc/permute.h).

The three samplers read nothing but offset tables, so they are held against the vectorised rule (tests/episode_rule_np.py, itself pinned
to the scalar rules by tests/test_episodes_scale_cpu.py) at EVERY position of whole epochs of 2.6 10^5 to 5.2 10^5 windows over 3000
episodes, and against the scalar Python rule on tables whose window counts pass 2^32, 2^40 and 2^62.  The gather is run on one 4.04 GiB
frame table - the smallest in which whole 224 x 224 x 3 x 2 rows lie past 2^32 bytes - in which every row carries its own number, on
each of its copy arms, directly and through EpisodeStore, the held-out sweep and EpisodeMix.  Every comparison is exact (integers and
bytes), and each has a self-test that feeds it what a 32-bit kernel would have produced and requires it to fail."""
import numpy as np
import pytest
import torch

from tests import episode_rule_np as R
from tests.test_episodes_cpu import CHUNK, largest_step
from tests.test_episodes_gpu import indexed_batch
from tests.test_episodes_scale_cpu import P9, WIDE_N, scale_tables, unpermute_index, wide_mix_tables, wide_tables
from tests.test_mixture_cpu import WEIGHTS
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import heldout as HO
from vla_adapter_amd import mixture as MX

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, WORLD = 1024, 8
GIB = 1 << 30


def compare(got: dict, want: dict) -> None:
    """Every array of ``want`` equals its namesake in ``got``, as integers, everywhere."""
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.flatnonzero((g != w).reshape(-1))
        assert bad.size == 0, f"{k}: {bad.size} of {g.size} differ, the first at {bad[0]}: {g.reshape(-1)[bad[0]]} for {w.reshape(-1)[bad[0]]}"


def on_device(tab: dict, *keys):
    return [tab[k].to(DEV) if tab.get(k) is not None else None for k in keys]


def host(bufs: dict) -> dict:
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def index_buffers(batches: int, **extra) -> dict:
    """[batches, B] / [batches, B + 1] buffers: the samplers write into row slices, a whole epoch is collected without a clone."""
    e = torch.empty
    out = dict(ep=e(batches, B, dtype=torch.int32, device=DEV), row=e(batches, B, dtype=torch.int64, device=DEV),
               out_off=e(batches, B + 1, dtype=torch.int32, device=DEV))
    out.update({k: e(batches, B, dtype=dt, device=DEV) for k, dt in extra.items()})
    return out


def window_starts(episode_off, off_table) -> np.ndarray:
    """The first row of every window the table ``off_table`` counts, in window order (ascending)."""
    eo, tab = R._table(episode_off), R._table(off_table)
    return np.repeat(eo[:-1] - tab[:-1], np.diff(tab)) + np.arange(tab[-1], dtype=np.int64)


def rule_outputs(tab: dict, e, t, **extra) -> dict:
    row, off = R.batch_outputs(e, t, tab["episode_off"], tab["prompt_off"], B, tab["Pmax"])
    out = dict(ep=e.astype(np.int32).reshape(-1, B), row=row.reshape(-1, B), out_off=off)
    out.update({k: v.reshape(-1, B) for k, v in extra.items()})
    return out


# ---------------------------------------------------------------------------------------------------------------- the store's sampler
def run_episode_sampler(tab: dict, seed: int, batches: int, rank: int = 0, world: int = WORLD, step: int = 0) -> dict:
    """``batches`` consecutive batches starting with that of (rank, step), the ranks of a step in turn."""
    from vla_adapter_amd import ops
    v, eo, po = on_device(tab, "valid_off", "episode_off", "prompt_off")
    o = index_buffers(batches)
    for g in range(batches):
        s, r = divmod(rank + g, world)
        ops.episode_sample(v, eo, po, seed, r, world, step + s, tab["Pmax"], o["ep"][g], o["row"][g], o["out_off"][g])
    return host(o)


def episode_rule(tab: dict, seed: int, batches: int, rank: int = 0, world: int = WORLD, step: int = 0, width: int = 64) -> dict:
    e, t = R.windows_at(R.positions(B, rank, world, step, batches), tab["valid_off"], seed, width=width)
    return rule_outputs(tab, e, t)


@pytest.mark.parametrize("N", [P9, P9 + 1, 2 * P9 - 3])
def test_one_whole_epoch_of_the_store_at_every_position(N):
    """3000 episodes (about 5 % without a window) that yield N windows, B = 1024 on 8 ranks: every step of epoch 0 and one more, so
    that the batches behind position N are drawn with epoch 1's own key."""
    tab, seed = scale_tables(N), 21
    batches = (-(-N // (B * WORLD)) + 1) * WORLD
    got = run_episode_sampler(tab, seed, batches)
    compare(got, episode_rule(tab, seed, batches))
    # on the kernel's outputs alone: epoch 0 visits every window exactly once
    rows = got["row"].reshape(-1)
    assert np.array_equal(np.sort(rows[:N]), window_starts(tab["episode_off"], tab["valid_off"]))
    # the positions behind N are the first of epoch 1, drawn with that epoch's key
    tail = np.arange(rows.size - N, dtype=np.uint64)
    e, t = R.locate(R.permute_index(tail, N, EP.epoch_key(seed, 1)), tab["valid_off"])
    assert tail.size >= B and np.array_equal(rows[N:], R._table(tab["episode_off"])[e] + t)
    assert not np.array_equal(rows[N:], rows[:tail.size]), "epoch 1 is another order"
    if N % B:
        g = N // B
        assert g * B < N < (g + 1) * B and g < batches, "one batch holds the end of epoch 0 and the start of epoch 1"


# ---------------------------------------------------------------------------------------------------------------- the mixture's sampler
def concat_tables(parts) -> dict:
    """Datasets back to back, as EpisodeMix lays them out: both offset tables shifted, dataset_off over the episodes."""
    eo, valid, po, ds = [0], [0], [0], [0]
    for p in parts:
        eo += [x + eo[-1] for x in p["episode_off"].tolist()[1:]]
        valid += [x + valid[-1] for x in p["valid_off"].tolist()[1:]]
        po += [x + po[-1] for x in p["prompt_off"].tolist()[1:]]
        ds.append(len(eo) - 1)
    return dict(episode_off=torch.tensor(eo, dtype=torch.int64), valid_off=torch.tensor(valid, dtype=torch.int64),
                prompt_off=torch.tensor(po, dtype=torch.int32), dataset_off=torch.tensor(ds, dtype=torch.int32),
                Pmax=max(p["Pmax"] for p in parts))


def run_mixture_sampler(tab: dict, seed: int, batches: int, rank: int = 0, world: int = WORLD, step: int = 0) -> dict:
    from vla_adapter_amd import ops
    v, eo, po, ds_off, q_off = on_device(tab, "valid_off", "episode_off", "prompt_off", "dataset_off", "quota_off")
    o = index_buffers(batches, ds=torch.int32)
    for g in range(batches):
        s, r = divmod(rank + g, world)
        ops.mixture_sample(v, eo, po, ds_off, q_off, seed, r, world, step + s, tab["Pmax"], o["ds"][g], o["ep"][g], o["row"][g], o["out_off"][g])
    return host(o)


def mixture_rule(tab: dict, seed: int, batches: int, rank: int = 0, world: int = WORLD, step: int = 0, width: int = 64):
    d, c, e, t = R.mixture_at(R.positions(B, rank, world, step, batches), tab["valid_off"], tab["dataset_off"], tab["quota_off"], seed, width=width)
    return rule_outputs(tab, e, t, ds=d.astype(np.int32)), c


def test_the_mixture_at_every_position_until_the_largest_dataset_completes_an_epoch():
    """Three datasets of 4^9 + 1, 100 003 and 17 training windows, the default period of 65 536 slots, make_mix's weights (1, 1, 0.5).
    The weights are not multiplied by the transition counts here (balance_weights=False: quotas 26 215 / 26 214 / 13 107): balanced,
    the 17-window dataset would hold the floor quota of one slot per period and pass an epoch only every 17 periods, while the
    largest needs 10 periods for its first - 'the smallest many epochs, the largest just over one' cannot hold together.  Ten
    periods: 1.000 epochs of dataset 0, 2.6 of dataset 1 and 7710 of dataset 2."""
    parts = [scale_tables(P9 + 1, 3000, seed=0), scale_tables(100_003, 1200, seed=1), scale_tables(17, 4, seed=2)]
    tab = concat_tables(parts)
    windows = [int(p["valid_off"][-1]) for p in parts]
    transitions = [int(p["episode_off"][-1]) for p in parts]
    quota = MX.quotas(MX.probabilities(WEIGHTS, transitions, balance_weights=False), MX.DEFAULT_PERIOD)
    assert quota == [26215, 26214, 13107] and windows == [P9 + 1, 100_003, 17]
    tab["quota_off"] = torch.tensor(np.cumsum([0] + quota), dtype=torch.int64)
    periods = -(-windows[0] // quota[0])
    batches, seed = periods * MX.DEFAULT_PERIOD // B, 11
    assert periods == 10 and batches == 640
    got = run_mixture_sampler(tab, seed, batches)
    want, c = mixture_rule(tab, seed, batches)
    compare(got, want)
    # per dataset, on the kernel's rows: the draws of each of its completed epochs cover its windows exactly once
    starts = window_starts(tab["episode_off"], tab["valid_off"])
    ds, rows, first = got["ds"].reshape(-1), got["row"].reshape(-1), np.cumsum([0] + windows)
    for d, n in enumerate(windows):
        mine = ds == d
        assert int(mine.sum()) == periods * quota[d]
        order = np.argsort(c[mine], kind="stable")
        assert np.array_equal(c[mine][order], np.arange(periods * quota[d], dtype=np.uint64)), "its ordinals: each once, none skipped"
        full = periods * quota[d] // n
        assert full >= (1, 2, 7000)[d]
        epochs = np.sort(rows[mine][order][:full * n].reshape(full, n), axis=1)
        assert np.array_equal(epochs, np.broadcast_to(starts[first[d]:first[d + 1]], (full, n))), d


# ---------------------------------------------------------------------------------------------------------------- the held-out sweep
def run_sweep(tab: dict, jobs, stride: int, slots: int) -> dict:
    """jobs: (rank, world, j, slot) - batch j of ``rank`` goes to row ``slot`` of the buffers."""
    from vla_adapter_amd import ops
    v, eo, po, ds_off = on_device(tab, "val_off", "episode_off", "prompt_off", "dataset_off")
    o = index_buffers(slots, ds=torch.int32, valid=torch.uint8)
    for rank, world, j, g in jobs:
        ops.heldout_sweep(v, eo, po, ds_off, rank, world, j, stride, tab["Pmax"], o["ds"][g], o["ep"][g], o["row"][g], o["out_off"][g], o["valid"][g])
    return host(o)


def sweep_rule(tab: dict, w, width: int = 64) -> dict:
    ok, d, e, t = R.sweep_at(w, tab["val_off"], tab.get("dataset_off"), width=width)
    return rule_outputs(tab, e, t, ds=d.astype(np.int32), valid=ok.astype(np.uint8))


@pytest.mark.parametrize("world", [1, 8])
@pytest.mark.parametrize("stride", [1, 7])
def test_the_held_out_sweep_names_every_strided_held_out_window_once_and_no_other(stride, world):
    """The 3000-episode store as two datasets of 1800 and 1200 episodes, the last 11.5 % of each held out: about 31 000 held-out
    windows.  Every batch of every rank against the rule, the flags of the last, partly empty batch among them."""
    tab = scale_tables(P9)
    E, ds_off = 3000, [0, 1800, 3000]
    held = torch.zeros(E, dtype=torch.bool)
    for d in range(2):
        held[ds_off[d + 1] - EP.holdout_count(ds_off[d + 1] - ds_off[d], 0.115):ds_off[d + 1]] = True
    train_off, tab["val_off"] = EP.split_offsets(tab["episode_off"], CHUNK, held)
    tab["dataset_off"] = torch.tensor(ds_off, dtype=torch.int32)
    Nv = int(tab["val_off"][-1])
    assert 28_000 <= Nv <= 34_000 and Nv + int(train_off[-1]) == P9
    total = -(-(-(-Nv // stride)) // B)
    jobs = [(rank, world, j, j * world + rank) for rank in range(world) for j in range(HO.sweep_batches(Nv, stride, B, rank, world))]
    assert sorted(g for *_, g in jobs) == list(range(total)), "the ranks' batches are the sweep's batches, each once"
    got = run_sweep(tab, jobs, stride, total)
    compare(got, sweep_rule(tab, np.arange(total * B, dtype=np.uint64) * np.uint64(stride)))
    # on the kernel's outputs alone
    ok, rows, eps = got["valid"].reshape(-1) != 0, got["row"].reshape(-1), got["ep"].reshape(-1)
    assert 0 < int(got["valid"][-1].sum()) < B and bool(got["valid"][:-1].all()), "only the last batch is partly empty"
    assert np.array_equal(rows[ok], window_starts(tab["episode_off"], tab["val_off"])[::stride]), "every window with w % stride == 0, once, in order"
    assert bool(held.numpy()[eps].all()) and not np.isin(rows, window_starts(tab["episode_off"], train_off)).any(), "no training window, valid or not"
    assert set(got["ds"].reshape(-1)[ok].tolist()) == {0, 1}


# ---------------------------------------------------------------------------------------------------------------- tables beyond 32 bits
WIDE_RANK = 5
# the seeds of the two 2^40 cases are the first for which the RULE puts every window index of the batch of (rank 5, step 10^9) beyond
# 2^32 (255 of 256 are, so most seeds leave a few below): the self-test can then require that every sample differs
WIDE_SEED = {WIDE_N[0]: 3, WIDE_N[1]: 64, WIDE_N[2]: 3}
WIDE_MIX_SEED = 9


def wide_batches(N: int):
    """(rank, step) of the batches drawn on the table of N windows: rank 5 of step 0, of step 10^9 and of the largest step the entry
    point accepts (positions up to 2^63 - 1), and the batch of epoch 0 that draws the table's LAST window, N - 1 - found by undoing the
    permutation.  On N = 2^32 + 1 that is the only window whose index does not fit 32 bits."""
    top = unpermute_index(N - 1, N, EP.epoch_key(WIDE_SEED[N], 0)) // B
    return [(WIDE_RANK, 0), (WIDE_RANK, 10 ** 9), (WIDE_RANK, largest_step(B, WIDE_RANK, WORLD)), (top % WORLD, top // WORLD)]


def wide_steps():
    return (0, 10 ** 9, largest_step(B, WIDE_RANK, WORLD))


@pytest.fixture(scope="module")
def wide_episode_runs():
    """N -> (tables, {(rank, step): the kernel's batch}) for the three synthetic three-episode tables; one launch each."""
    out = {}
    for N in WIDE_N:
        tab = wide_tables(N)
        out[N] = tab, {(rank, step): run_episode_sampler(tab, WIDE_SEED[N], 1, rank, WORLD, step) for rank, step in wide_batches(N)}
    return out


@pytest.fixture(scope="module")
def wide_mixture_runs():
    tab = wide_mix_tables()
    return tab, {step: run_mixture_sampler(tab, WIDE_MIX_SEED, 1, WIDE_RANK, WORLD, step) for step in wide_steps()}


WIDE_SWEEPS = ((3, 8, 5_000_000, 7), (4, 8, 2 ** 27 + 1, 1))         # (rank, world, batch j, stride): windows near 2.9 10^11; the batch that holds Nv


@pytest.fixture(scope="module")
def wide_sweep_runs():
    tab = wide_tables(2 ** 40 + 12345)
    tab["val_off"], tab["dataset_off"] = tab["valid_off"], torch.tensor([0, 1, 3], dtype=torch.int32)
    return tab, [run_sweep(tab, [(rank, world, j, 0)], stride, 1) for rank, world, j, stride in WIDE_SWEEPS]


@pytest.mark.parametrize("N", WIDE_N)
def test_the_sampler_on_tables_counted_beyond_32_bits(wide_episode_runs, N):
    """The batches of wide_batches against the scalar Python rule: Python integers are the truth here."""
    tab, runs = wide_episode_runs[N]
    valid, eo = tab["valid_off"].tolist(), tab["episode_off"].tolist()
    for (rank, step), got in runs.items():
        w = EP.sample_windows(valid, B, WIDE_SEED[N], rank, WORLD, step)
        assert got["ep"][0].tolist() == [e for e, _ in w] and got["row"][0].tolist() == [eo[e] + t for e, t in w], (rank, step)
        compare(got, episode_rule(tab, WIDE_SEED[N], 1, rank, WORLD, step))
        assert max(t for _, t in w) >= 2 ** 31, "steps inside an episode that do not fit 31 bits are among them"
    assert (2, N - 1 - valid[2]) in w, "the last batch draws the table's last window"


def test_the_mixture_sampler_with_a_dataset_of_2_to_the_40_windows(wide_mixture_runs):
    tab, runs = wide_mixture_runs
    tabs = tab["valid_off"].tolist(), tab["dataset_off"].tolist(), tab["quota_off"].tolist()
    eo = tab["episode_off"].tolist()
    for step, got in runs.items():
        w = MX.sample_windows(*tabs, B, WIDE_MIX_SEED, WIDE_RANK, WORLD, step)
        assert got["ds"][0].tolist() == [d for d, _, _ in w] and got["ep"][0].tolist() == [e for _, e, _ in w], step
        assert got["row"][0].tolist() == [eo[e] + t for _, e, t in w], step
        compare(got, mixture_rule(tab, WIDE_MIX_SEED, 1, WIDE_RANK, WORLD, step)[0])
        assert {d for d, _, _ in w} == {0, 1}


def test_the_sweep_on_windows_beyond_32_bits(wide_sweep_runs):
    """batch_j * stride reaches windows near 2.9 10^11; the second case is the batch in which the table of 2^40 + 12 345 windows ends:
    57 valid samples, the rest flagged and on window 0."""
    tab, runs = wide_sweep_runs
    val, eo = tab["val_off"].tolist(), tab["episode_off"].tolist()
    for (rank, world, j, stride), got in zip(WIDE_SWEEPS, runs):
        w = HO.sweep_windows(val, [0, 1, 3], B, rank, world, j, stride)
        assert got["valid"][0].tolist() == [ok for ok, *_ in w] and got["ds"][0].tolist() == [d for _, d, _, _ in w]
        assert got["ep"][0].tolist() == [e for _, _, e, _ in w] and got["row"][0].tolist() == [eo[e] + t for _, _, e, t in w]
        first = (j * world + rank) * B
        compare(got, sweep_rule(tab, (np.uint64(first) + np.arange(B, dtype=np.uint64)) * np.uint64(stride)))
    assert int(runs[1]["valid"].sum()) == 57 and int(runs[0]["valid"].sum()) == B


def differing(got: dict, want: dict) -> np.ndarray:
    return ((got["ep"] != want["ep"]) | (got["row"] != want["row"])).reshape(-1)


def test_self_test_a_32_bit_window_index_turns_every_comparison_red(wide_episode_runs, wide_mixture_runs, wide_sweep_runs):
    """The comparisons above are fed the rule with the window index cut to 32 bits - what a kernel with an ``int`` or ``unsigned`` j
    would give - and must fail on every wide table; without this they prove nothing about width.  On the tables of 2^40 + 12 345
    windows the samples that differ are exactly those whose window index does not fit 32 bits, and - at the step and seed chosen
    so, by the rule - that is every sample of the batch."""
    for N in WIDE_N:
        tab, runs = wide_episode_runs[N]
        for (rank, step), got in runs.items():
            pos = R.positions(B, rank, WORLD, step)
            j = R.permute_index(pos % np.uint64(N), N, R.epoch_key(WIDE_SEED[N], pos // np.uint64(N)))
            narrow = episode_rule(tab, WIDE_SEED[N], 1, rank, WORLD, step, width=32)
            assert np.array_equal(differing(got, narrow), j >= 2 ** 32), "exactly the samples whose window index does not fit 32 bits"
            if N > 2 ** 32 + 1 or (rank, step) == wide_batches(N)[-1]:
                assert bool((j >= 2 ** 32).any())
                with pytest.raises(AssertionError):
                    compare(got, narrow)
            if N == WIDE_N[1] and step == 10 ** 9:
                assert bool((j >= 2 ** 32).all()), "the seed was chosen so"
                assert differing(got, narrow).all(), "every sample differs"
    step = 10 ** 9
    # the mixture: dataset 1 lies behind the 2^40 windows of dataset 0, so its window indices are all wide; dataset 0 as above
    tab, runs = wide_mixture_runs
    for s, got in runs.items():
        narrow = mixture_rule(tab, WIDE_MIX_SEED, 1, WIDE_RANK, WORLD, s, width=32)[0]
        with pytest.raises(AssertionError):
            compare(got, narrow)
        if s == step:
            assert differing(got, narrow).all(), "every sample differs"
    # the sweep: every window of the first case lies beyond 2^32, so every sample differs; in the second the 57 valid ones do
    tab, runs = wide_sweep_runs
    for (rank, world, j, stride), got, n in zip(WIDE_SWEEPS, runs, (B, 57)):
        first = (j * world + rank) * B
        narrow = sweep_rule(tab, (np.uint64(first) + np.arange(B, dtype=np.uint64)) * np.uint64(stride), width=32)
        with pytest.raises(AssertionError):
            compare(got, narrow)
        assert differing(got, narrow)[:n].all()


# ---------------------------------------------------------------------------------------------------------------- the gather past 2^32 bytes
FRAME = (2, 224, 224, 3)                                    # 301 056 bytes per transition: two 224 x 224 RGB images
ROW_BYTES = 2 * 224 * 224 * 3
ROWS = 14_400                                               # 4 335 206 400 bytes: the smallest table of whole episodes with rows past 2^32
TOTAL = ROWS * ROW_BYTES
EPISODE_ROWS = 150
# name -> (byte offset into the buffer, rows, frame shape): one view per copy arm of vla_episode_gather
VIEWS = {"aligned": (0, ROWS, FRAME),                       # 16-byte arm
         "offset-1": (1, ROWS - 1, FRAME),                  # rows divisible by 16 on a misaligned base: byte arm
         "odd-rows": (0, 28_600, (1, 223, 225, 3))}         # 150 525-byte rows: byte arm
NEED = int(8.5 * GIB)                                       # the buffer, the mix assembled from it, and the batches


class FrameTable:
    """One flat uint8 device buffer of TOTAL seeded random bytes, allocated when first asked for.  ``view(name)`` is one of VIEWS with
    the first 8 bytes of every row overwritten by the row's own number (little-endian int64): a row that turns up anywhere in an output
    is then identified by name.  Stamping one view spoils the stamps of the others, so the view last stamped is remembered."""

    def __init__(self):
        self.buf, self.stamped = None, None

    def get(self) -> torch.Tensor:
        if self.buf is None:
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            if free < NEED:
                pytest.fail(f"the frame table needs {NEED / GIB:.1f} GiB of free device memory (a 4.04 GiB table and, for the mix, its copy); "
                            f"{free / GIB:.1f} GiB are free.  This is a failure, not a skip: the cases past 2^32 bytes did not run.")
            self.buf = torch.empty(TOTAL, dtype=torch.uint8, device=DEV)
            g = torch.Generator(device=DEV).manual_seed(7)
            for lo in range(0, TOTAL, GIB):
                self.buf[lo:lo + GIB].random_(0, 256, generator=g)
            self.stamped = None
        return self.buf

    def view(self, name: str) -> torch.Tensor:
        off, T, shape = VIEWS[name]
        n = T * int(np.prod(shape))
        v = self.get()[off:off + n].view((T,) + shape)
        if self.stamped != name:
            v.view(T, -1)[:, :8] = torch.arange(T, dtype=torch.int64, device=DEV).view(torch.uint8).view(T, 8)
            self.stamped = name
        return v

    def release(self) -> None:
        self.buf, self.stamped = None, None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def table():
    t = FrameTable()
    yield t
    t.release()


def stamps(frames: torch.Tensor) -> list:
    """The row number every frame of a batch carries."""
    n = frames.shape[0]
    return frames.reshape(n, -1)[:, :8].contiguous().view(torch.int64).view(n).tolist()


def frame_check(out_frames: torch.Tensor, frames: torch.Tensor, rows) -> list:
    """Per sample: the output frame carries the number of rows[b] and equals frames[rows[b]] byte for byte."""
    got = stamps(out_frames)
    return [got[b] == int(r) and bool(torch.equal(out_frames[b], frames[int(r)])) for b, r in enumerate(rows)]


def small_tables(T: int, seed: int, first_row: int = 0) -> dict:
    """Everything of an episode file but the frames, on the host: episodes of 150 rows (the last one shorter where T is no multiple),
    float32 actions [T, 7] and proprio [T, 8], one prompt of 0 .. 11 ids per episode."""
    g = torch.Generator().manual_seed(seed)
    eo = list(range(0, T, EPISODE_ROWS)) + [T]
    lens = torch.randint(0, 12, (len(eo) - 1,), generator=g)
    return dict(actions_raw=torch.randn(T, 7, generator=g) * 2, proprio_raw=torch.randn(T, 8, generator=g) * 2,
                episode_off=torch.tensor(eo, dtype=torch.int64), prompt_flat=torch.randint(1, 1000, (int(lens.sum()),), generator=g, dtype=torch.int64),
                prompt_off=torch.tensor(np.cumsum([0] + lens.tolist()), dtype=torch.int32))


def boundary_rows(name: str) -> list:
    """The rows either side of 2^31 and of 2^32 bytes - the last row that starts below the boundary and the first that starts at or
    above it -, row 0, the last row, and the last valid window start of the last episode (its action window ends on the episode's
    last row; the one of row T - 1 is clamped there eight times)."""
    off, T, shape = VIEWS[name]
    rb = int(np.prod(shape))
    k31, k32 = (2 ** 31 - off - 1) // rb, (2 ** 32 - off - 1) // rb
    assert off + k31 * rb < 2 ** 31 <= off + (k31 + 1) * rb and off + k32 * rb < 2 ** 32 <= off + (k32 + 1) * rb and k32 + 1 < T - CHUNK
    return [0, k31, k31 + 1, k32, k32 + 1, T - 1, T - CHUNK]


def gather(frames, tabs_dev: dict, rows, Pmax: int) -> dict:
    """ops.episode_gather of the given rows into fresh buffers (ep and out_off follow from the rows and the tables)."""
    from vla_adapter_amd import ops
    eo, po = tabs_dev["episode_off"].tolist(), tabs_dev["prompt_off"].tolist()
    n = len(rows)
    ep = [int(np.searchsorted(eo, r, side="right")) - 1 for r in rows]
    off = np.cumsum([0] + [po[e + 1] - po[e] for e in ep])
    e = torch.empty
    out = dict(frames_u8=e((n,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=DEV), actions_raw=e(n, CHUNK, 7, dtype=torch.float32, device=DEV),
               proprio_raw=e(n, 8, dtype=torch.float32, device=DEV), prompt_flat=e(n * Pmax, dtype=torch.int64, device=DEV),
               prompt_off=torch.tensor(off, dtype=torch.int32, device=DEV))
    ops.episode_gather(frames, tabs_dev["actions_raw"], tabs_dev["proprio_raw"], tabs_dev["episode_off"], tabs_dev["prompt_flat"], tabs_dev["prompt_off"],
                       torch.tensor(ep, dtype=torch.int32, device=DEV), torch.tensor(rows, dtype=torch.int64, device=DEV), out["prompt_off"],
                       out["frames_u8"], out["actions_raw"], out["proprio_raw"], out["prompt_flat"], Pmax)
    return out, ep


def assert_small_outputs_equal(got: dict, tabs: dict, windows) -> None:
    """actions, proprio and both prompt tensors against the toy tests' torch-indexed reference (tests/test_episodes_gpu.py)."""
    want = indexed_batch(dict(tabs, frames_u8=torch.zeros(tabs["actions_raw"].shape[0], 1, dtype=torch.uint8)), windows)
    for k in ("actions_raw", "proprio_raw", "prompt_flat", "prompt_off"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k


@pytest.mark.parametrize("name", list(VIEWS))
def test_gather_of_rows_either_side_of_2_to_the_31_and_2_to_the_32_bytes(table, name):
    off, T, shape = VIEWS[name]
    frames = table.view(name)
    rb = frames[0].numel()
    wide = rb % 16 == 0 and frames.data_ptr() % 16 == 0
    assert wide == (name == "aligned") and frames.data_ptr() == table.get().data_ptr() + off and frames.is_contiguous()
    tabs = small_tables(T, seed=len(name))
    tabs_dev = {k: v.to(DEV) for k, v in tabs.items()}
    rows = boundary_rows(name)
    if name == "aligned":
        assert rows == [0, 7133, 7134, 14266, 14267, 14399, 14392]
    got, ep = gather(frames, tabs_dev, rows, int(tabs["prompt_off"].diff().max()))
    assert stamps(got["frames_u8"]) == rows, "every output frame carries the number of the row asked for"
    assert all(frame_check(got["frames_u8"], frames, rows)), "and equals it byte for byte"
    eo = tabs["episode_off"].tolist()
    assert_small_outputs_equal(got, tabs, [(e, r - eo[e]) for e, r in zip(ep, rows)])
    last = tabs["actions_raw"][T - 1].to(DEV)
    assert torch.equal(got["actions_raw"][-1, -1], last) and not torch.equal(got["actions_raw"][-1, -2], last), "the window ends on the episode's last row"
    assert torch.equal(got["actions_raw"][-2], last.expand(CHUNK, -1)), "the goal step repeats"


def test_self_test_a_32_bit_byte_offset_turns_the_frame_check_red_past_2_to_the_32(table):
    """The batch a kernel with a 32-bit ``row * row_bytes`` would have produced, built with torch from byte offset (row row_bytes) mod
    2^32 - inside the table, nothing is read out of bounds: the frame check fails on every row that starts past 2^32 and on no other."""
    frames, buf = table.view("aligned"), table.get()
    rows = boundary_rows("aligned")
    wrapped = [(r * ROW_BYTES) % 2 ** 32 for r in rows]
    assert all(0 <= o and o + ROW_BYTES <= TOTAL for o in wrapped)
    fake = torch.stack([buf[o:o + ROW_BYTES].view(FRAME) for o in wrapped])
    past = [r * ROW_BYTES >= 2 ** 32 for r in rows]
    assert past == [False, False, False, False, True, True, True]
    assert [not ok for ok in frame_check(fake, frames, rows)] == past
    assert all(frame_check(torch.stack([frames[r] for r in rows]), frames, rows)), "and passes on the right batch"


@pytest.mark.parametrize("name", ["aligned", "offset-1"])
def test_store_and_held_out_sweep_on_the_4_gib_table(table, name):
    """EpisodeStore.from_dict on tables that already live on the device, holdout 0.1: 96 episodes, the last 10 - rows 12 900 and up,
    straddling 2^32 bytes - held out.  sample() draws training batches, ops.heldout_sweep + ops.episode_gather (HeldOutSweep.draw's two
    launches) the sweep's; every gathered frame carries the number of the row the rule names.  The store must not copy the frames.
    Once on the aligned view (16-byte arm, whose uint4 index stays below 2^32 at this size) and once on the view off by one byte (byte
    arm: the element index itself passes 2^32)."""
    from vla_adapter_amd import ops
    frames = table.view(name)
    tabs = small_tables(frames.shape[0], seed=3)
    before = torch.cuda.memory_allocated()
    st = EP.EpisodeStore.from_dict(dict({k: v.to(DEV) for k, v in tabs.items()}, frames_u8=frames, dataset_name="big"), DEV, chunk=CHUNK, holdout=0.1)
    assert st.frames_u8.data_ptr() == frames.data_ptr(), "the store copied frames that were already on the device"
    assert torch.cuda.memory_allocated() - before < GIB
    assert st.heldout["big"]["episodes"] == [86, 96] and int(tabs["episode_off"][86]) == 12_900 and st.Nv == frames.shape[0] - 12_900 - 10 * (CHUNK - 1)
    eo, n, seen = R._table(tabs["episode_off"]), 64, []
    for rank, world, step in ((0, 1, 0), (1, 2, 3), (7, 8, 10 ** 9)):
        b = st.sample(n, 5, rank, world, step)
        e, t = R.windows_at(R.positions(n, rank, world, step), st.valid_off_host, 5)
        rows = (eo[e] + t).tolist()
        assert stamps(b["frames_u8"]) == rows and all(frame_check(b["frames_u8"], frames, rows)), (rank, world, step)
        assert_small_outputs_equal(b, tabs, list(zip(e.tolist(), t.tolist())))
        seen += rows
    assert max(seen) < 12_900 and min(seen) * ROW_BYTES < 2 ** 31 < max(seen) * ROW_BYTES, "training rows only, either side of 2^31 bytes"
    # the sweep: its own buffers, the gather HeldOutSweep itself runs
    e_ = torch.empty
    idx = dict(ds=e_(n, dtype=torch.int32, device=DEV), ep=e_(n, dtype=torch.int32, device=DEV), row=e_(n, dtype=torch.int64, device=DEV),
               prompt_off=e_(n + 1, dtype=torch.int32, device=DEV), valid=e_(n, dtype=torch.uint8, device=DEV))
    raw = dict(frames_u8=e_((n,) + FRAME, dtype=torch.uint8, device=DEV), actions_raw=e_(n, CHUNK, st.A, dtype=torch.float32, device=DEV),
               proprio_raw=e_(n, st.Pd, dtype=torch.float32, device=DEV), prompt_flat=e_(n * st.Pmax, dtype=torch.int64, device=DEV))
    named = []
    for j in range(HO.sweep_batches(st.Nv, 1, n, 0, 1)):
        ops.heldout_sweep(st.val_off, st.episode_off, st.prompt_off, None, 0, 1, j, 1, st.Pmax, idx["ds"], idx["ep"], idx["row"], idx["prompt_off"], idx["valid"])
        ops.episode_gather(st.frames_u8, st.actions_raw, st.proprio_raw, st.episode_off, st.prompt_flat, st.prompt_off, idx["ep"], idx["row"],
                           idx["prompt_off"], raw["frames_u8"], raw["actions_raw"], raw["proprio_raw"], raw["prompt_flat"], st.Pmax)
        ok, _, e, t = R.sweep_windows(st.val_off_host, None, n, 0, 1, j)
        rows = (eo[e] + t).tolist()
        assert idx["valid"].tolist() == ok.tolist() and stamps(raw["frames_u8"]) == rows and all(frame_check(raw["frames_u8"], frames, rows)), j
        assert_small_outputs_equal(dict(raw, prompt_off=idx["prompt_off"]), tabs, list(zip(e.tolist(), t.tolist())))
        named += [r for r, v in zip(rows, ok.tolist()) if v]
    assert named == window_starts(tabs["episode_off"], st.val_off_host).tolist() and len(named) == st.Nv
    assert min(named) == 12_900 and min(named) * ROW_BYTES < 2 ** 32 < max(named) * ROW_BYTES, "held-out rows only, either side of 2^32 bytes"
    del st, b, raw, idx
    torch.cuda.empty_cache()


def test_a_mix_of_two_datasets_whose_second_lies_past_2_to_the_31_and_2_to_the_32_bytes(table):
    """EpisodeMix.from_dicts of the two halves of the table, 7200 rows each: the mix assembles its own 4.04 GiB frame table (the one time
    two of them are live), the sources are released, and a batch of 512 carries the numbers of the rows the rule names - the second
    dataset's are rows 7200 and up of the mix - and the rule's dataset_index."""
    frames = table.view("aligned")
    half = ROWS // 2
    parts = [small_tables(half, seed=11), small_tables(half, seed=12)]
    base = torch.cuda.memory_allocated()
    free, _ = torch.cuda.mem_get_info()
    if free < TOTAL + GIB // 2:
        pytest.fail(f"assembling the mix needs a second table of {TOTAL / GIB:.2f} GiB; {free / GIB:.1f} GiB of device memory are free")
    entries = [(dict({k: v.to(DEV) for k, v in p.items()}, frames_u8=frames[d * half:(d + 1) * half], dataset_name=f"half_{d}"), 1.0) for d, p in enumerate(parts)]
    m = MX.EpisodeMix.from_dicts(entries, DEV, chunk=CHUNK)
    del entries, frames
    table.release()
    assert m.frames_u8.shape[0] == ROWS and m.quota == [32768, 32768] and m.dataset_off_host.tolist() == [0, 48, 96]
    assert torch.cuda.memory_allocated() - base < GIB, "the source table is released: the mix's own table took its place"
    eo, n, seen = R._table(m.episode_off), 512, []
    both = dict(actions_raw=torch.cat([p["actions_raw"] for p in parts]), proprio_raw=torch.cat([p["proprio_raw"] for p in parts]),
                episode_off=m.episode_off.cpu(), prompt_flat=torch.cat([p["prompt_flat"] for p in parts]), prompt_off=m.prompt_off.cpu())
    for rank, world, step in ((0, 1, 0), (3, 8, 10 ** 9)):
        b = m.sample(n, 13, rank, world, step)
        d, _, e, t = R.mixture_at(R.positions(n, rank, world, step), m.valid_off_host, m.dataset_off_host, m.quota_off_host, 13)
        rows = (eo[e] + t).tolist()
        assert b["dataset_index"].tolist() == d.tolist() == [int(r >= half) for r in rows]
        assert stamps(b["frames_u8"]) == rows and all(frame_check(b["frames_u8"], m.frames_u8, rows)), (rank, world, step)
        assert_small_outputs_equal(b, both, list(zip(e.tolist(), t.tolist())))
        seen += rows
    assert min(seen) * ROW_BYTES < 2 ** 31 and any(2 ** 31 <= r * ROW_BYTES < 2 ** 32 for r in seen) and max(seen) * ROW_BYTES >= 2 ** 32
    del m, b
    torch.cuda.empty_cache()
