"""The sampling rules of the episode data path restated on whole numpy arrays of positions: episodes.py (splitmix64_key, _feistel4,
permute_index, locate, sample_windows), mixture.py (sample_window) and heldout.py (sweep_windows).  Product code keeps its scalar
rules, which stay the specification; this file exists so that the tests can evaluate 10^5 to 10^6 positions - a whole epoch of a
dataset of real size - and is itself tested against the scalar rules (tests/test_episodes_scale_cpu.py).

Everything runs in numpy uint64, whose array arithmetic wraps modulo 2^64 like the kernels' u64.  The offset tables are int64 and the
window index is cast to int64 before ``searchsorted`` (it stays below 2^63): numpy compares uint64 against int64 in float64, which is
not exact above 2^53.

``width`` is for the tests' self-tests only: the result a kernel that kept the window index in ``width`` bits would give.
"""
import numpy as np

from vla_adapter_amd.episodes import EPISODE_STREAM
from vla_adapter_amd.mixture import MIX_STREAM

U = np.uint64
_M64 = (1 << 64) - 1


def u64(x) -> np.ndarray:
    """x (a Python int of any size below 2^64, a list of them, or an array) as a uint64 array of at least one dimension."""
    if isinstance(x, np.ndarray):
        return np.atleast_1d(x.astype(np.uint64, copy=False))
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & _M64 for v in x], dtype=np.uint64)
    return np.array([int(x) & _M64], dtype=np.uint64)


def splitmix64_key(seed, idx) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = u64(seed) + u64(idx) * U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def epoch_key(seed: int, epoch) -> np.ndarray:
    return splitmix64_key((int(seed) & _M64) ^ EPISODE_STREAM, epoch)


def period_key(seed: int, period) -> np.ndarray:
    return splitmix64_key((int(seed) & _M64) ^ MIX_STREAM, period)


def bit_length(v: np.ndarray) -> np.ndarray:
    """int.bit_length of every element of a uint64 array, in integer arithmetic (log2 in float64 is off by one next to 2^53 and up)."""
    v = v.copy()
    bits = np.zeros(v.shape, dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (v >> U(s)) != 0
        bits += np.where(big, U(s), U(0))
        v = np.where(big, v >> U(s), v)
    return bits + (v != 0).astype(np.uint64)


def feistel4(x: np.ndarray, key: np.ndarray, half: np.ndarray) -> np.ndarray:
    mask = (U(1) << half) - U(1)
    l, r = x >> half, x & mask
    for rnd in range(4):
        l, r = r, l ^ (splitmix64_key(splitmix64_key(key, rnd), r) & mask)
    return (l << half) | r


def permute_index(i, N, key, stats: dict = None) -> np.ndarray:
    """permute_index of episodes.py for arrays: i, N and key broadcast against each other (a mixture draws every sample from its own
    dataset and epoch: its own N and key).  ``stats["passes"]`` receives the largest number of Feistel passes any element took."""
    i, N, key = np.broadcast_arrays(u64(i), u64(N), u64(key))
    if bool((i >= N).any()):
        raise ValueError("permute_index: an index outside [0, N)")
    half = np.maximum((bit_length(N - U(1)) + U(1)) // U(2), U(1))
    y = np.where(N > 1, i, U(0))
    idx = np.flatnonzero(N > 1)
    passes = 0
    while idx.size:
        y[idx] = feistel4(y[idx], key[idx], half[idx])
        passes += 1
        idx = idx[y[idx] >= N[idx]]
    if stats is not None:
        stats["passes"] = max(stats.get("passes", 0), passes)
    return y


def _table(t) -> np.ndarray:
    return np.asarray(t.tolist() if hasattr(t, "tolist") else t, dtype=np.int64)


def _narrow(j: np.ndarray, width: int) -> np.ndarray:
    return j if width >= 64 else j & U((1 << width) - 1)


def locate(j, valid_off):
    """(episode, step inside it) of every window index: the largest e below E with valid_off[e] <= j, as ``searchsorted``."""
    tab = _table(valid_off)
    j = u64(j).astype(np.int64)
    e = np.clip(np.searchsorted(tab, j, side="right") - 1, 0, tab.size - 2)
    return e, j - tab[e]


def positions(B: int, rank: int, world: int, step: int, batches: int = 1) -> np.ndarray:
    """The stream positions of ``batches`` consecutive batches starting with the batch of (rank, step): the ranks' batches of one step
    are consecutive, so these are the batches of (rank, step), (rank + 1, step), ... in order."""
    first = (int(step) * int(world) + int(rank)) * int(B)
    if first + batches * B > _M64:
        raise ValueError("positions beyond 2^64")
    return U(first) + np.arange(batches * B, dtype=np.uint64)


def windows_at(pos, valid_off, seed: int, stats: dict = None, width: int = 64):
    """sample_windows of episodes.py at arbitrary stream positions -> (episode [n], step inside it [n]) as int64 arrays."""
    tab = _table(valid_off)
    N = U(int(tab[-1]))
    pos = u64(pos)
    j = permute_index(pos % N, N, epoch_key(seed, pos // N), stats)
    return locate(_narrow(j, width), tab)


def sample_windows(valid_off, B: int, seed: int, rank: int, world: int, step: int, width: int = 64):
    return windows_at(positions(B, rank, world, step), valid_off, seed, width=width)


def mixture_at(pos, valid_off, dataset_off, quota_off, seed: int, stats: dict = None, width: int = 64):
    """sample_window of mixture.py at arbitrary stream positions -> (dataset, ordinal in the dataset's own stream, global episode, step
    inside it); the ordinal is uint64, the others int64."""
    tab, ds_off, q_off = _table(valid_off), _table(dataset_off), _table(quota_off)
    D, Q = ds_off.size - 1, U(int(q_off[-1]))
    pos = u64(pos)
    k, s = pos // Q, pos % Q
    s2 = permute_index(s, Q, period_key(seed, k)).astype(np.int64)
    d = np.clip(np.searchsorted(q_off, s2, side="right") - 1, 0, D - 1)
    with np.errstate(over="ignore"):
        c = k * (q_off[d + 1] - q_off[d]).astype(np.uint64) + (s2 - q_off[d]).astype(np.uint64)
    v0 = tab[ds_off[d]]
    N_d = (tab[ds_off[d + 1]] - v0).astype(np.uint64)
    key = splitmix64_key(epoch_key(seed, c // N_d), (d + 1).astype(np.uint64))
    j = v0.astype(np.uint64) + permute_index(c % N_d, N_d, key, stats)
    e, t = locate(_narrow(j, width), tab)
    return d, c, e, t


def sweep_at(w, val_off, dataset_off=None, width: int = 64):
    """sweep_windows of heldout.py for arbitrary window indices w -> (valid, dataset, global episode, step inside it), int64 arrays."""
    tab = _table(val_off)
    w = _narrow(u64(w), width).astype(np.int64)
    ok = w < tab[-1]
    e, t = locate(np.where(ok, w, 0).astype(np.uint64), tab)
    d = np.zeros(e.shape, dtype=np.int64)
    if dataset_off is not None:
        ds_off = _table(dataset_off)
        d = np.clip(np.searchsorted(ds_off[:-1], e, side="right") - 1, 0, ds_off.size - 2)
    return ok.astype(np.int64), d, e, t


def sweep_windows(val_off, dataset_off, B: int, rank: int, world: int, j: int, stride: int = 1, batches: int = 1, width: int = 64):
    """The windows of ``batches`` consecutive global batches starting with batch j of ``rank`` (global batch j world + rank)."""
    first = (int(j) * int(world) + int(rank)) * int(B)
    if (first + batches * B) * int(stride) >= 1 << 63:
        raise ValueError("window indices beyond 2^63")
    return sweep_at((U(first) + np.arange(batches * B, dtype=np.uint64)) * U(int(stride)), val_off, dataset_off, width)


def batch_outputs(e: np.ndarray, t: np.ndarray, episode_off, prompt_off, B: int, Pmax: int):
    """What the three samplers write for windows (e, t) taken B at a time: row int64 [n] and out_off int32 [n / B, B + 1] - the first row
    of every window and, per batch, the running sum of the prompt lengths clamped to Pmax."""
    eo, po = _table(episode_off), _table(prompt_off)
    lens = np.clip(po[1:] - po[:-1], 0, Pmax)[e].reshape(-1, B)
    off = np.concatenate([np.zeros((lens.shape[0], 1), dtype=np.int64), np.cumsum(lens, axis=1)], axis=1)
    return eo[e] + t, off.astype(np.int32)
