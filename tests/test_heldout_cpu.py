"""CPU checks of validation on held-out episodes (vla_adapter_amd/heldout.py, include/vla_heldout.h): the entry points' own
refusals, the split rule and its refusals, training epochs that never touch a held-out episode, the ordered sweep in plain Python - every strided held-out window exactly once over ranks and batches, for a store
and a mix -, the flags, the report's derivation from hand-made sums, and the two-rank merge on gloo."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_episodes_cpu import CHUNK, make_tables
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import heldout as HO
from vla_adapter_amd import mixture as MX

LENGTHS = [9, 1, 20, 8, 7, 12, 10]          # the issue's store: 2, 0, 13, 1, 0, 5 and 3 windows at chunk 8
PROMPTS = (3, 0, 11, 5, 7, 2, 6)
F = 0.4                                     # holds the last 3 episodes out
TRAIN_OFF = [0, 2, 2, 15, 16, 16, 16, 16]
VAL_OFF = [0, 0, 0, 0, 0, 0, 5, 8]
# a second dataset whose LAST episode is too short for a window: 5 episodes, f = 0.4 holds [3, 5) out - 2 and 0 windows
LENGTHS_B = [10, 8, 3, 9, 5]
PROMPTS_B = (4, 9, 1, 2, 8)


def make_store(device="cpu", holdout=F, **kw):
    t = make_tables(lengths=LENGTHS, prompt_lens=PROMPTS, dataset_name="suite_a", **kw)
    return t, EP.EpisodeStore.from_dict(t, device, chunk=CHUNK, holdout=holdout)


def make_pair_tables(**kw):
    a = make_tables(lengths=LENGTHS, prompt_lens=PROMPTS, seed=0, dataset_name="suite_a", **kw)
    b = make_tables(lengths=LENGTHS_B, prompt_lens=PROMPTS_B, seed=1, dataset_name="suite_b", **kw)
    A = b["actions_raw"].shape[1]
    b["action_mask"] = torch.tensor([True] * (A - 1) + [False])
    b["actions_raw"] = b["actions_raw"] * 0.5 + 1.0
    return [a, b]


def make_pair(device="cpu", holdout=F, **kw):
    tables = make_pair_tables(**kw)
    return tables, MX.EpisodeMix.from_dicts([(tables[0], 1.0), (tables[1], 1.0)], device, chunk=CHUNK, period=16, holdout=holdout)


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def test_host_checks_refuse_bad_arguments(lib):
    """The entry points' own argument checks answer before anything is launched (no device needed)."""
    P = 8
    sweep = lambda **kw: lib.vla_heldout_sweep(None, P, P, P, kw.get("ds_off", P), 7, kw.get("D", 2), kw.get("rank", 0), kw.get("world", 1), kw.get("j", 0),
                                               kw.get("stride", 1), kw.get("B", 4), 4, P, P, P, P, kw.get("valid", P))
    assert sweep(B=0) == -1 and b"1 <= B <= 1024" in lib.vla_last_error()
    assert sweep(B=1025) == -1
    assert sweep(D=8) == -1 and b"D <= E" in lib.vla_last_error()
    assert sweep(rank=2, world=2) == -1 and b"rank < world" in lib.vla_last_error()
    assert sweep(stride=0) == -1 and b"stride" in lib.vla_last_error()
    assert sweep(ds_off=None) == -1 and b"dataset_off" in lib.vla_last_error()
    assert sweep(valid=None) == -1 and b"null" in lib.vla_last_error()
    assert sweep(j=2 ** 61, stride=8) == -1 and b"overflows" in lib.vla_last_error()
    assert lib.vla_heldout_l1_accumulate(None, P, P, None, P, 0, 8, 7, 1, P, P) == -1 and b">= 1" in lib.vla_last_error()
    assert lib.vla_heldout_l1_accumulate(None, P, P, None, None, 4, 8, 7, 1, P, P) == -1 and b"null" in lib.vla_last_error()


# ---------------------------------------------------------------------------------------------------------------- the split rule
def test_the_example_gives_the_two_tables():
    _, s = make_store()
    assert EP.holdout_count(7, F) == 3
    assert s.valid_off.tolist() == s.valid_off_host.tolist() == TRAIN_OFF and s.val_off.tolist() == s.val_off_host.tolist() == VAL_OFF
    assert s.valid_off.dtype == s.val_off.dtype == torch.int64 and (s.N, s.Nv, s.E) == (16, 8, 7)
    assert s.heldout == {"suite_a": dict(episodes=[4, 7], num_episodes=3, train_windows=16, heldout_windows=8)}
    assert [EP.locate(j, VAL_OFF)[0] for j in range(8)] == [5, 5, 5, 5, 5, 6, 6, 6]
    assert [EP.locate(j, VAL_OFF)[1] for j in range(8)] == [0, 1, 2, 3, 4, 0, 1, 2]
    both = [a + b for a, b in zip(TRAIN_OFF, VAL_OFF)]
    assert both == EP.valid_offsets(s.episode_off.cpu(), CHUNK).tolist(), "the two tables are complementary: nothing is lost or doubled"


@pytest.mark.parametrize("E, f, H", [(7, 0.4, 3), (7, 0.05, 1), (2, 0.9, 1), (20, 0.05, 1)])
def test_holdout_counts(E, f, H):
    assert EP.holdout_count(E, f) == H == min(E - 1, max(1, math.floor(f * E + 0.5)))


@pytest.mark.parametrize("f", [0.0, 1.0, -0.1, 1.5, float("nan"), "0.4", True])
def test_a_fraction_outside_the_open_interval_is_refused(f):
    with pytest.raises(ValueError, match=r"suite_a: holdout must be a fraction inside \(0, 1\)"):
        make_store(holdout=f)
    with pytest.raises(ValueError, match=r"suite_a: holdout must be a fraction inside \(0, 1\)"):
        make_pair(holdout=f)


def test_every_other_refusal_names_the_dataset_and_what_is_wrong():
    one = make_tables(lengths=[30], prompt_lens=(4,), dataset_name="lonely")
    with pytest.raises(ValueError, match="lonely: holdout needs at least 2 episodes"):
        EP.EpisodeStore.from_dict(one, "cpu", chunk=CHUNK, holdout=0.5)
    no_train = make_tables(lengths=[3, 5, 20], prompt_lens=(1, 2, 3), dataset_name="short_heads")
    with pytest.raises(ValueError, match="short_heads: holdout leaves no training window"):
        EP.EpisodeStore.from_dict(no_train, "cpu", chunk=CHUNK, holdout=0.3)
    no_val = make_tables(lengths=[20, 12, 5], prompt_lens=(1, 2, 3), dataset_name="short_tail")
    with pytest.raises(ValueError, match="short_tail: holdout leaves no held-out window"):
        EP.EpisodeStore.from_dict(no_val, "cpu", chunk=CHUNK, holdout=0.3)
    assert EP.EpisodeStore.from_dict(no_val, "cpu", chunk=CHUNK, holdout=0.6).Nv == 5, "two held-out episodes: the middle one has windows"
    ok = make_tables(lengths=LENGTHS, prompt_lens=PROMPTS, dataset_name="suite_a")
    for bad, what in ((one, "lonely: holdout needs at least 2"), (no_train, "short_heads: holdout leaves no training"), (no_val, "short_tail: holdout leaves no held-out")):
        with pytest.raises(ValueError, match=what):
            MX.EpisodeMix.from_dicts([(ok, 1.0), (bad, 1.0)], "cpu", chunk=CHUNK, period=16, holdout=0.3)


def test_without_holdout_nothing_changes():
    t, s = make_store(holdout=None)
    assert s.valid_off.tolist() == EP.valid_offsets(t["episode_off"], CHUNK).tolist() and s.val_off is None and s.heldout is None and s.N == 24
    tables, m = make_pair(holdout=None)
    assert m.valid_off.tolist() == EP.valid_offsets(m.episode_off.cpu(), CHUNK).tolist() and m.val_off is None and m.heldout is None
    assert m.windows == [24, 6]


def test_statistics_and_balance_stay_over_all_episodes():
    _, a = make_store(holdout=None)
    _, b = make_store()
    assert a.statistics() == b.statistics() and b.statistics()["suite_a"]["num_trajectories"] == 7
    _, m0 = make_pair(holdout=None)
    _, m1 = make_pair()
    assert m0.statistics() == m1.statistics() and m0.p.tolist() == m1.p.tolist() and m0.quota == m1.quota and m0.transitions == m1.transitions
    assert m1.windows == [16, 4] and m1.mixture_info()["windows"] == [16, 4], "N_d follows from the training table"


# ---------------------------------------------------------------------------------------------------------------- exactly once and never
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("B", [2, 5])
def test_a_training_epoch_visits_every_training_window_once_and_no_held_out_episode(world, B):
    """N * world * B positions are world * B whole epochs: every training window that many times, across all ranks and steps."""
    _, s = make_store()
    seen = {}
    steps = s.N                                     # steps * world * B positions in all
    for step in range(steps):
        for rank in range(world):
            for e, t in EP.sample_windows(TRAIN_OFF, B, 13, rank, world, step):
                assert e <= 3, "an episode of the training side"
                assert 0 <= t < TRAIN_OFF[e + 1] - TRAIN_OFF[e]
                seen[(e, t)] = seen.get((e, t), 0) + 1
    assert len(seen) == 16 and set(seen.values()) == {world * B}
    first = [w for step in range(-(-16 // (world * B))) for rank in range(world) for w in EP.sample_windows(TRAIN_OFF, B, 13, rank, world, step)][:16]
    assert len(set(first)) == 16, "the first epoch: 16 positions, 16 different windows"


def _union(val_off, ds_off, B, world, stride):
    Nv = int(val_off[-1])
    got = []
    for rank in range(world):
        n = HO.sweep_batches(Nv, stride, B, rank, world)
        for j in range(n):
            ws = HO.sweep_windows(val_off, ds_off, B, rank, world, j, stride)
            assert any(ok for ok, _, _, _ in ws), "a batch without a valid sample is not run"
            got += [(d, e, t) for ok, d, e, t in ws if ok]
            for ok, d, e, t in ws:
                if not ok:
                    assert (e, t) == EP.locate(0, val_off), "an invalid sample takes window 0 of the held-out set"
        assert not any(ok for ok, _, _, _ in HO.sweep_windows(val_off, ds_off, B, rank, world, n, stride)), "the batch behind the last is empty"
    return got


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("stride", [1, 3])
def test_the_sweep_visits_every_strided_window_exactly_once(world, stride):
    got = _union(VAL_OFF, None, 6, world, stride)
    want = [(0,) + EP.locate(w, VAL_OFF) for w in range(0, 8, stride)]
    assert sorted(got) == sorted(want) and len(set(got)) == len(got) == -(-8 // stride)
    assert {e for _, e, _ in got} <= {5, 6}, "held-out episodes only (episode 4 is held out and yields no window)"


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("stride", [1, 3])
def test_the_sweep_of_a_mix_names_the_dataset_of_every_window(world, stride):
    """Two datasets back to back: suite_a holds episodes [4, 7) out (0, 5 and 3 windows), suite_b [10, 12) (2 and 0 windows: its last
    episode, the last of the table, yields none).  Window 8 is the first of suite_b, right behind the boundary."""
    _, m = make_pair()
    val, ds_off = m.val_off_host.tolist(), m.dataset_off_host.tolist()
    assert ds_off == [0, 7, 12] and val == [0, 0, 0, 0, 0, 0, 5, 8, 8, 8, 8, 10, 10] and m.Nv == 10
    assert m.valid_off.tolist() == [0, 2, 2, 15, 16, 16, 16, 16, 19, 20, 20, 20, 20]
    got = _union(val, ds_off, 6, world, stride)
    want = []
    for w in range(0, 10, stride):
        e, t = EP.locate(w, val)
        want.append((0 if e < 7 else 1, e, t))
    assert sorted(got) == sorted(want) and len(set(got)) == len(got)
    if stride == 1:
        assert (0, 6, 2) in got and (1, 10, 0) in got and (1, 10, 1) in got and not [g for g in got if g[1] in (4, 11)]
    assert m.heldout == {"suite_a": dict(episodes=[4, 7], num_episodes=3, train_windows=16, heldout_windows=8),
                         "suite_b": dict(episodes=[10, 12], num_episodes=2, train_windows=4, heldout_windows=2)}


def test_sweep_batches():
    assert [HO.sweep_batches(8, 1, 6, r, 2) for r in range(2)] == [1, 1] and HO.sweep_batches(8, 1, 6, 0, 1) == 2
    assert [HO.sweep_batches(8, 3, 6, r, 2) for r in range(2)] == [1, 0] and HO.sweep_batches(8, 1, 4, 0, 1) == 2
    assert [HO.sweep_batches(100, 1, 4, r, 3) for r in range(3)] == [9, 8, 8]


def test_mix_training_never_draws_a_held_out_episode():
    _, m = make_pair()
    valid, ds_off, q_off = m.valid_off_host.tolist(), m.dataset_off_host.tolist(), m.quota_off_host.tolist()
    seen = set()
    for pos in range(16 * 20):
        d, _, e, t = MX.sample_window(pos, valid, ds_off, q_off, seed=3)
        assert (e <= 3) if d == 0 else (7 <= e <= 9), (d, e)
        seen.add((e, t))
    assert len(seen) == 20, "all 16 + 4 training windows"


# ---------------------------------------------------------------------------------------------------------------- flags
def _cfg(*extra):
    from vla_adapter_amd import finetune as F_
    return F_.parse_args(["--use_proprio", "True", "--use_fz", "True", *extra])


def test_the_flags():
    from vla_adapter_amd import finetune as F_
    assert _cfg().val_episode_fraction is None and _cfg().val_window_stride == 1
    for src in (("--episode_file", "a.pt"), ("--episode_mix", "a.pt=1.0,b.pt")):
        ok = _cfg(*src, "--max_seq_len", "96", "--use_val_set", "True", "--val_episode_fraction", "0.25", "--val_window_stride", "4", "--val_freq", "5",
                  "--val_time_limit", "9")
        assert ok.val_episode_fraction == 0.25 and ok.val_window_stride == 4
        F_.check_supported(ok, ok._explicit)
        cfg = _cfg(*src, "--max_seq_len", "96", "--val_episode_fraction", "0.25")
        with pytest.raises(ValueError, match="--val_episode_fraction without --use_val_set"):
            F_.check_supported(cfg, cfg._explicit)
        cfg = _cfg(*src, "--max_seq_len", "96", "--use_val_set", "True", "--val_episode_fraction", "0.25", "--val_batch_file", "v.pt")
        with pytest.raises(ValueError, match="two validation sources"):
            F_.check_supported(cfg, cfg._explicit)
        with pytest.raises(ValueError, match="two validation sources"):
            F_.check_supported(ok, ok._explicit, val_batches=True)
        for bad in ("0", "1", "1.5"):
            cfg = _cfg(*src, "--max_seq_len", "96", "--use_val_set", "True", "--val_episode_fraction", bad)
            with pytest.raises(ValueError, match=r"--val_episode_fraction must lie inside \(0, 1\)"):
                F_.check_supported(cfg, cfg._explicit)
        cfg = _cfg(*src, "--max_seq_len", "96", "--use_val_set", "True", "--val_episode_fraction", "0.25", "--val_window_stride", "0")
        with pytest.raises(ValueError, match="--val_window_stride"):
            F_.check_supported(cfg, cfg._explicit)
        ok = _cfg(*src, "--max_seq_len", "96", "--use_val_set", "True", "--val_batch_file", "v.pt")       # unchanged: still accepted
        F_.check_supported(ok, ok._explicit)
    cfg = _cfg("--batch_file", "b.pt", "--use_val_set", "True", "--val_episode_fraction", "0.25")
    with pytest.raises(ValueError, match="--val_episode_fraction holds episodes out of --episode_file / --episode_mix"):
        F_.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_file", "a.pt", "--max_seq_len", "96", "--use_val_set", "True", "--val_episode_fraction", "0.25", "--objective", "token_ce", "--use_fz", "False")
    with pytest.raises(NotImplementedError, match="token_ce"):
        F_.check_supported(cfg, cfg._explicit)


def test_the_two_pinned_refusals_stay_without_the_flag():
    from vla_adapter_amd import finetune as F_
    for flag in ("episode_file", "episode_mix"):
        cfg = _cfg(f"--{flag}", "a.pt", "--max_seq_len", "96", "--use_val_set", "True")
        with pytest.raises(NotImplementedError, match=rf"--use_val_set with --{flag}: no validation split is cut from the episodes \(ValidationPass takes "
                                                      r"collated batches\); pass held-out batches with --val_batch_file") as ei:
            F_.check_supported(cfg, cfg._explicit)
        assert "--val_episode_fraction" in str(ei.value), "the closing sentence names the flag"


# ---------------------------------------------------------------------------------------------------------------- the reference rule
def test_l1_accumulate_reference_by_hand():
    """B = 3, C = 2, A = 2, D = 2; row 1 is invalid and holds NaN, row 2's dataset index is clamped from 5 to 1."""
    pred = np.array([[[1, 2], [3, 4]], [[np.nan, np.inf], [0, 0]], [[0.5, -1], [2, 2]]], dtype=np.float32)
    tgt = np.array([[[0, 0], [0, 8]], [[0, 0], [0, 0]], [[1, 1], [0, 4]]], dtype=np.float32)
    acc0 = np.arange(8, dtype=np.float64).reshape(2, 2, 2)
    acc, cnt = HO.l1_accumulate_reference(pred, tgt, [0, 0, 5], [1, 0, 1], 2, acc0, np.array([10, 20]))
    assert acc.tolist() == [[[0 + 1, 1 + 2], [2 + 3, 3 + 4]], [[4 + 0.5, 5 + 2], [6 + 2, 7 + 2]]] and cnt.tolist() == [11, 21]
    assert acc0[0, 0, 0] == 0, "the inputs are left as they are"
    acc, cnt = HO.l1_accumulate_reference(pred, tgt, None, [0, 0, 0], 2, acc0, np.array([10, 20]))
    assert np.array_equal(acc, acc0) and cnt.tolist() == [10, 20], "no valid row: nothing changes"
    acc, cnt = HO.l1_accumulate_reference(pred, tgt, None, [1, 0, 1], 1, np.zeros((1, 2, 2)), np.zeros(1, dtype=np.int64))
    assert acc.tolist() == [[[1.5, 4], [5, 6]]] and cnt.tolist() == [2]


# ---------------------------------------------------------------------------------------------------------------- the report
def test_the_report_is_derived_from_the_sums():
    """D = 2, C = 3, A = 2: dataset 0 counted 4 samples, dataset 1 counted 1; dataset 1 has a mask that leaves column 1 raw."""
    acc = np.array([[[4.0, 8.0], [2.0, 2.0], [0.0, 4.0]], [[1.0, 3.0], [0.5, 0.5], [2.0, 1.0]]])
    cnt = np.array([4, 1])
    st = [dict(q01=[-1.0, 0.0], q99=[3.0, 10.0]), dict(q01=[0.0, -2.0], q99=[0.5, 2.0], mask=[True, False])]
    r = HO.report(acc, cnt, ("a", "b"), st, step=6, batches=2, windows=[4, 3])
    tot = acc[0] + acc[1]
    assert r["step"] == 6 and r["val_batches_count"] == 2 and r["val_samples_count"] == 5 and r["val_windows_total"] == 7
    assert r["loss_value"] == r["loss"] == tot.sum() / (5 * 3 * 2) == 28.0 / 30
    assert r["curr_action_l1_loss"] == tot[0].sum() / (5 * 2) == 1.6 and r["next_actions_l1_loss"] == tot[1:].sum() / (5 * 2 * 2) == 0.6
    assert r["l1_by_chunk_step"] == [16.0 / 10, 5.0 / 10, 7.0 / 10] and r["l1_by_action_dim"] == [9.5 / 15, 18.5 / 15]
    a, b = r["per_dataset"]["a"], r["per_dataset"]["b"]
    assert list(r["per_dataset"]) == ["a", "b"]
    assert a["loss_value"] == a["loss"] == 20.0 / 24 and a["curr_action_l1_loss"] == 12.0 / 8 and a["next_actions_l1_loss"] == 8.0 / 16
    assert a["val_samples_count"] == 4 and a["val_windows_total"] == 4 and b["val_samples_count"] == 1 and b["val_windows_total"] == 3
    assert a["l1_by_chunk_step"] == [1.5, 0.5, 0.5] and a["l1_by_action_dim"] == [0.5, 14.0 / 12]
    assert a["l1_by_action_dim_raw"] == [0.5 * ((3.0 + 1.0 + 1e-8) / 2), 14.0 / 12 * ((10.0 + 1e-8) / 2)]
    assert b["l1_by_action_dim"] == [3.5 / 3, 4.5 / 3] and b["l1_by_action_dim_raw"] == [3.5 / 3 * ((0.5 + 1e-8) / 2), 4.5 / 3], "an unmasked column keeps its units"
    assert b["loss_value"] == 8.0 / 6
    # the overall line is the count-weighted combination of the datasets' lines
    assert math.isclose(r["loss_value"], (4 * a["loss_value"] + 1 * b["loss_value"]) / 5, rel_tol=1e-15)
    import json
    assert json.loads(json.dumps(r)) == r
    # C == 1: next_actions_l1_loss is 0.0, as vla_l1_loss has it; a dataset nothing was counted for reports None, not NaN
    r1 = HO.report(np.array([[[2.0, 4.0]], [[0.0, 0.0]]]), np.array([2, 0]), ("a", "b"), None, 1, 1, [2, 5])
    assert r1["next_actions_l1_loss"] == 0.0 and r1["loss_value"] == 1.5 and r1["per_dataset"]["a"]["l1_by_action_dim_raw"] == [1.0, 2.0]
    assert r1["per_dataset"]["b"]["loss_value"] is None and r1["per_dataset"]["b"]["val_samples_count"] == 0
    assert json.loads(json.dumps(r1)) == r1


# ---------------------------------------------------------------------------------------------------------------- the merge
def _merge_worker(rank, world, port, q):
    from vla_adapter_amd import ddp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    ddp.init_process_group_from_env("gloo")
    g = torch.Generator().manual_seed(50 + rank)
    acc = torch.rand(2, 3, 4, generator=g, dtype=torch.float64)
    cnt = torch.tensor([3 + rank, 2 ** 40 + 7 * rank], dtype=torch.int64)
    acc2, cnt2 = HO.all_reduce_sums(acc, cnt)
    q.put((rank, acc2.numpy().copy(), cnt2.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_both_end_with_the_sum():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (a, c) for r, a, c in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    want = sum(torch.rand(2, 3, 4, generator=torch.Generator().manual_seed(50 + r), dtype=torch.float64) for r in range(2)).numpy()
    for r in range(2):
        assert np.array_equal(got[r][0], want) and got[r][0].dtype == np.float64
        assert got[r][1].tolist() == [7, 2 ** 41 + 7] and got[r][1].dtype == np.int64
    a = torch.ones(1, 1, 1, dtype=torch.float64)
    assert HO.all_reduce_sums(a, torch.ones(1, dtype=torch.int64))[0] is a, "one rank: nothing is exchanged"
