"""CPU checks of training on a weighted mixture of episode datasets (vla_adapter_amd/mixture.py, include/vla_mixture.h): the quotas, the
sampling rule in plain Python - exact quotas per period, every ordinal once, every window of a dataset once per N_d ordinals, ranks without gap or overlap - the
per-dataset statistics, the reference's dataset_len, and the refusals that need no device."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_episodes_cpu import CHUNK, LENGTHS, make_tables
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import mixture as MX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("suite_a", "suite_b", "suite_c")
MIX_LENGTHS = (LENGTHS, [12, 8], [30])      # 16, 6 and 23 windows at chunk 8; 45, 20 and 30 transitions
WEIGHTS = (1.0, 1.0, 0.5)                   # balanced: p = (45, 20, 15) / 80
PERIOD = 16
QUOTA = [9, 4, 3]
WINDOWS = [16, 6, 23]
CONSTANT_COLUMN = 3                         # of dataset 2's actions: min == max


def make_mix_tables(**kw):
    """The issue's three datasets as episode-file dicts: dataset 1 with an action_mask that has one False column, dataset 2 with one
    constant action column.  kw goes to every make_tables (n_img, hw, A, Pd)."""
    a = make_tables(lengths=MIX_LENGTHS[0], prompt_lens=(3, 0, 11, 5, 7), seed=0, dataset_name=NAMES[0], **kw)
    A = a["actions_raw"].shape[1]
    b = make_tables(lengths=MIX_LENGTHS[1], prompt_lens=(4, 9), seed=1, dataset_name=NAMES[1],
                    action_mask=torch.tensor([True] * (A - 1) + [False]), **kw)
    c = make_tables(lengths=MIX_LENGTHS[2], prompt_lens=(6,), seed=2, dataset_name=NAMES[2], **kw)
    b["actions_raw"] = b["actions_raw"] * 0.5 + 1.0        # every dataset its own range: the wrong statistics row shows
    c["actions_raw"] = c["actions_raw"] * 3.0 - 2.0
    c["proprio_raw"] = c["proprio_raw"] * 0.25 + 4.0
    c["actions_raw"][:, CONSTANT_COLUMN] = 0.75
    return [a, b, c]


def make_mix(device="cpu", period=PERIOD, weights=WEIGHTS, balance_weights=True, **kw):
    tables = make_mix_tables(**kw)
    return tables, MX.EpisodeMix.from_dicts(list(zip(tables, weights)), device, chunk=CHUNK, period=period, balance_weights=balance_weights)


def host_tables(mix):
    return mix.valid_off_host.tolist(), mix.dataset_off_host.tolist(), mix.quota_off_host.tolist()


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


@pytest.fixture(scope="module")
def mix():
    return make_mix()


def test_host_checks_refuse_bad_arguments(lib):
    """The entry points' own argument checks answer before anything is launched (no device needed)."""
    P = 8
    assert lib.vla_mixture_sample(None, P, P, P, P, P, 8, 3, 0, 0, 1, 0, 0, 4, P, P, P, P) == -1 and b"1 <= B <= 1024" in lib.vla_last_error()
    assert lib.vla_mixture_sample(None, P, P, P, P, P, 8, 3, 0, 0, 1, 0, 1025, 4, P, P, P, P) == -1
    assert lib.vla_mixture_sample(None, P, P, P, P, P, 8, 9, 0, 0, 1, 0, 4, 4, P, P, P, P) == -1 and b"D <= E" in lib.vla_last_error()
    assert lib.vla_mixture_sample(None, P, P, P, P, P, 8, 3, 0, 2, 2, 0, 4, 4, P, P, P, P) == -1 and b"rank < world" in lib.vla_last_error()
    assert lib.vla_mixture_sample(None, P, P, P, None, P, 8, 3, 0, 0, 1, 0, 4, 4, P, P, P, P) == -1 and b"null" in lib.vla_last_error()
    assert lib.vla_normalize_bounds_rows(None, P, P, 5, 55, 7, P, 3, P, P, None, None) == -1 and b"multiple of Dim" in lib.vla_last_error()
    assert lib.vla_normalize_bounds_rows(None, P, P, 5, 56, 7, None, 3, P, P, None, None) == -1 and b"null" in lib.vla_last_error()
    assert lib.vla_normalize_bounds_rows(None, P, P, 5, 56, 7, P, 0, P, P, None, None) == -1


@pytest.mark.parametrize("B, rank, world", [(4, 0, 1), (4, 2, 3), (2, 1, 2), (1024, 7, 8), (1000, 5, 2 ** 20)])
def test_sample_refuses_a_stream_position_beyond_63_bits(lib, mix, B, rank, world):
    """As tests/test_episodes_cpu.py has it for vla_episode_sample: the largest step is accepted by the position check (and stopped by
    the next one, B * Pmax, violated on purpose: nothing is launched), the step behind it is refused by name."""
    from tests.test_episodes_cpu import largest_step
    P, step = 8, largest_step(B, rank, world)
    call = lambda s: lib.vla_mixture_sample(None, P, P, P, P, P, 8, 3, 0, rank, world, s, B, 2 ** 31 - 1, P, P, P, P)
    assert call(step) == -1 and b"B * Pmax" in lib.vla_last_error(), "accepted by the position check"
    assert call(step + 1) == -1 and b"stream position overflows 63 bits" in lib.vla_last_error()
    assert call(2 ** 63 - 1) == -1 and b"stream position overflows 63 bits" in lib.vla_last_error()
    _, m = mix
    with pytest.raises(ValueError, match="stream position overflows 63 bits"):
        m.sample_indices(B, 0, rank, world, step + 1)


def test_the_feistel_network_is_stated_once():
    """episodes.hip and mixture.hip include csrc/permute.h; neither restates the bijection."""
    csrc = os.path.join(ROOT, "vla_adapter_amd", "csrc")
    assert "u64 feistel4(" in open(os.path.join(csrc, "permute.h")).read()
    for f in ("episodes.hip", "mixture.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "permute.h"' in txt and "u64 feistel4(" not in txt and "u64 permute_index(" not in txt, f
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "mixture.hip" in mk and "permute.h" in mk and "vla_mixture.h" in mk


def test_the_streams_differ():
    """MIX_STREAM is none of the other stream constants (the augmentation keys its draws with the bare seed: 0), and the kernel file
    restates the Python constants: its own, and EPISODE_STREAM in the csrc/windows.h it includes (the one place all three pickers take
    it from)."""
    csrc = os.path.join(ROOT, "vla_adapter_amd", "csrc")
    collate = int(re.search(r"COLLATE_STREAM = (0x[0-9A-Fa-f]+)ull", open(os.path.join(csrc, "collate.hip")).read()).group(1), 16)
    assert len({MX.MIX_STREAM, EP.EPISODE_STREAM, collate, 0}) == 4
    txt = open(os.path.join(csrc, "mixture.hip")).read()
    assert '#include "windows.h"' in txt
    txt += open(os.path.join(csrc, "windows.h")).read()
    assert f"MIX_STREAM = 0x{MX.MIX_STREAM:X}ull" in txt and f"EPISODE_STREAM = 0x{EP.EPISODE_STREAM:X}ull" in txt


# ---------------------------------------------------------------------------------------------------------------- quotas
def test_the_example_gives_9_4_3():
    p = MX.probabilities(WEIGHTS, [45, 20, 30], True)
    assert p.tolist() == [45 / 80, 20 / 80, 15 / 80] and MX.quotas(p, PERIOD) == QUOTA
    assert MX.probabilities(WEIGHTS, [45, 20, 30], False).tolist() == [0.4, 0.4, 0.2]


@pytest.mark.parametrize("Q", [3, 7, 16, 100, 65536])
def test_quotas_sum_to_the_period_and_stay_within_one_of_the_share(Q):
    rng = np.random.default_rng(Q)
    cases = [np.array([1 / 3, 1 / 3, 1 / 3]), np.array([0.5, 0.25, 0.25]), np.array([0.999, 0.0005, 0.0005]), np.array([1.0])]
    cases += [rng.dirichlet(np.ones(D)) for D in (2, 3, 3, 3) for _ in range(5)]
    for p in cases:
        q = MX.quotas(p, Q)
        assert sum(q) == Q and min(q) >= 1 and len(q) == p.size, (p, q)
        if (p * Q >= 1).all():
            assert all(abs(qd - pd * Q) < 1 for qd, pd in zip(q, p)), (p, q)


def test_more_datasets_than_slots_are_refused():
    with pytest.raises(ValueError, match="period"):
        MX.quotas(np.full(4, 0.25), 3)
    assert MX.quotas(np.full(4, 0.25), 4) == [1, 1, 1, 1]
    with pytest.raises(ValueError, match="period"):
        make_mix(period=2)


# ---------------------------------------------------------------------------------------------------------------- the sampling rule
def test_forty_periods_of_the_rule(mix):
    _, m = mix
    valid, ds_off, q_off = host_tables(m)
    assert m.quota == QUOTA and m.windows == WINDOWS and q_off == [0, 9, 13, 16] and ds_off == [0, 5, 7, 8]
    periods = 40
    ordinals, visits = [[] for _ in NAMES], [{} for _ in NAMES]
    for k in range(periods):
        count = [0, 0, 0]
        for s in range(PERIOD):
            d, c, e, t = MX.sample_window(k * PERIOD + s, valid, ds_off, q_off, seed=7)
            count[d] += 1
            ordinals[d].append(c)
            assert ds_off[d] <= e < ds_off[d + 1], "an episode of the drawn dataset"
            assert 0 <= t < valid[e + 1] - valid[e], "a window start the episode yields"
            visits[d][(e, t)] = visits[d].get((e, t), 0) + 1
        assert count == QUOTA, f"period {k} gives every dataset exactly its quota"
    for d in range(3):
        n = periods * QUOTA[d]
        assert sorted(ordinals[d]) == list(range(n)), "the ordinals of a dataset's own stream: each once, none skipped"
        assert len(visits[d]) == WINDOWS[d], "every window of the dataset is visited"
        assert set(visits[d].values()) <= {n // WINDOWS[d], -(-n // WINDOWS[d])}, "floor or ceil of draws / windows: whole epochs"


def test_the_order_is_shuffled_keyed_and_repeatable(mix):
    _, m = mix
    tabs = host_tables(m)
    run = lambda seed: [MX.sample_window(pos, *tabs, seed=seed)[:1] + MX.sample_window(pos, *tabs, seed=seed)[2:] for pos in range(64)]
    assert run(3) == run(3) and run(3) != run(4)
    ds = [w[0] for w in run(3)]
    assert ds[:PERIOD] != sorted(ds[:PERIOD]) and ds[:PERIOD] != ds[PERIOD:2 * PERIOD], "slots are shuffled, every period anew"


def test_two_ranks_share_the_positions_without_gap_or_overlap(mix):
    _, m = mix
    tabs = host_tables(m)
    B, seed = 5, 11
    one = [w for step in range(8) for w in MX.sample_windows(*tabs, B, seed, 0, 1, step)]
    two = [w for step in range(4) for rank in range(2) for w in MX.sample_windows(*tabs, B, seed, rank, 2, step)]
    assert one == two == [MX.sample_window(pos, *tabs, seed=seed)[:1] + MX.sample_window(pos, *tabs, seed=seed)[2:] for pos in range(40)]
    pos = sorted(EP.sample_position(B, rank, 2, step, b) for step in range(4) for rank in range(2) for b in range(B))
    assert pos == list(range(40))


def test_a_mix_of_one_dataset_is_allowed():
    t = make_tables(dataset_name="only")
    m = MX.EpisodeMix.from_dicts([(t, 2.0)], "cpu", chunk=CHUNK, period=16)
    assert m.quota == [16] and m.p.tolist() == [1.0] and m.mixture_info()["dataset_len"] is None
    tabs = host_tables(m)
    seen = [MX.sample_window(pos, *tabs, seed=0) for pos in range(32)]
    assert sorted(c for _, c, _, _ in seen) == list(range(32)) and len({(e, t) for _, _, e, t in seen[:16]}) == 16


# ---------------------------------------------------------------------------------------------------------------- the mix on the host
def test_statistics_are_each_datasets_own(mix):
    tables, m = mix
    st = m.statistics()
    assert list(st) == list(NAMES)
    for name, t in zip(NAMES, tables):
        mask = torch.as_tensor(t["action_mask"]).tolist() if "action_mask" in t else None
        want = EP.dataset_statistics(t["actions_raw"].numpy(), t["proprio_raw"].numpy(), t["episode_off"].numel() - 1, mask)
        assert st[name] == want, name
    assert "mask" not in st[NAMES[0]]["action"] and st[NAMES[1]]["action"]["mask"] == [True] * 6 + [False]
    a = st[NAMES[2]]["action"]
    assert a["min"][CONSTANT_COLUMN] == a["max"][CONSTANT_COLUMN] == 0.75
    assert json.loads(json.dumps(st)) == st
    assert [st[n]["num_transitions"] for n in NAMES] == [45, 20, 30] and [st[n]["num_trajectories"] for n in NAMES] == [5, 2, 1]


def test_tables_lie_back_to_back(mix):
    tables, m = mix
    assert (m.D, m.E, m.T, m.A, m.Pd, m.Pmax, m.Q) == (3, 8, 95, 7, 8, 11, 16)
    assert m.episode_off.tolist() == np.cumsum([0] + LENGTHS + [12, 8] + [30]).tolist()
    assert m.valid_off.tolist() == [0, 0, 0, 1, 3, 16, 21, 22, 45]
    assert torch.equal(m.actions_raw, torch.cat([t["actions_raw"] for t in tables]))
    assert torch.equal(m.frames_u8, torch.cat([t["frames_u8"] for t in tables]))
    assert m.prompt_off.tolist() == [0, 3, 3, 14, 19, 26, 30, 39, 45] and m.prompt_off.dtype == torch.int32
    assert m.dataset_off.dtype == torch.int32 and m.quota_off.dtype == torch.int64


def test_dataset_len_follows_the_reference(mix):
    """rlds/dataset.py:512-522: int(max over the datasets with weight 1.0 of num_transitions / p)."""
    _, m = mix
    info = m.mixture_info()
    p = np.array(WEIGHTS) * np.array([45, 20, 30])
    p = p / p.sum()
    assert info["dataset_len"] == int((np.array([45, 20, 30]) / p)[[0, 1]].max()) == 80
    assert info["datasets"] == list(NAMES) and info["quota"] == QUOTA and info["period"] == PERIOD and info["p"] == p.tolist()
    assert json.loads(json.dumps(info)) == info
    _, flat = make_mix(balance_weights=False)
    assert flat.p.tolist() == [0.4, 0.4, 0.2] and flat.mixture_info()["dataset_len"] == int(45 / 0.4)
    assert MX.DEFAULT_PERIOD == 65536


def test_paths_name_their_datasets_by_stem(tmp_path):
    tables = make_mix_tables()
    del tables[2]["dataset_name"]
    paths = []
    for t, stem in zip(tables, ("a", "b", "third_suite")):
        torch.save(t, tmp_path / f"{stem}.pt")
        paths.append(str(tmp_path / f"{stem}.pt"))
    m = MX.EpisodeMix.load(list(zip(paths, WEIGHTS)), "cpu", chunk=CHUNK, period=PERIOD)
    assert m.names == (NAMES[0], NAMES[1], "third_suite") and m.quota == QUOTA
    assert torch.equal(m.proprio_raw, torch.cat([t["proprio_raw"] for t in tables]))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _spoiled(spoil, weights=WEIGHTS):
    tables = make_mix_tables()
    spoil(tables)
    return MX.EpisodeMix.from_dicts(list(zip(tables, weights)), "cpu", chunk=CHUNK, period=PERIOD)


@pytest.mark.parametrize("key, spoil", [
    ("dataset_name", lambda t: t[1].__setitem__("dataset_name", NAMES[0])),
    ("frames_u8", lambda t: t[1].__setitem__("frames_u8", t[1]["frames_u8"][:, :, :4])),
    ("frames_u8", lambda t: t[2].__setitem__("frames_u8", t[2]["frames_u8"][:, :1])),
    ("actions_raw", lambda t: t[2].__setitem__("actions_raw", t[2]["actions_raw"][:, :6])),
    ("proprio_raw", lambda t: t[1].__setitem__("proprio_raw", t[1]["proprio_raw"][:, :7])),
    ("no valid window", lambda t: t[1].__setitem__("episode_off", torch.tensor([0, 6, 13, 20]))),
    ("episode_off", lambda t: t[1].__setitem__("episode_off", torch.tensor([0, 6, 13, 20]))),
    ("prompt_off", lambda t: t[2]["prompt_off"].__setitem__(-1, 99)),
])
def test_datasets_that_do_not_fit_are_refused_by_key(key, spoil):
    if "episode_off" in key or "window" in key:       # three episodes need three prompts
        inner = spoil
        spoil = lambda t: (inner(t), t[1].__setitem__("prompt_off", torch.tensor([0, 4, 9, 13], dtype=torch.int32)))
    with pytest.raises(ValueError, match=key):
        _spoiled(spoil)


@pytest.mark.parametrize("w", [0.0, -1.0, float("nan"), float("inf"), "1.0"])
def test_bad_weights_are_refused(w):
    with pytest.raises(ValueError, match=rf"{NAMES[1]}: weight"):
        _spoiled(lambda t: None, weights=(1.0, w, 0.5))


def test_concat_shards_still_refuses_mixed_names():
    a, b, _ = make_mix_tables()
    del b["action_mask"]
    with pytest.raises(ValueError, match="dataset_name"):
        EP.concat_shards([a, b])


def _cfg(*extra):
    from vla_adapter_amd import finetune as F
    return F.parse_args(["--use_proprio", "True", "--use_fz", "True", *extra])


def test_episode_mix_is_a_fifth_batch_source():
    from vla_adapter_amd import finetune as F
    ok = _cfg("--episode_mix", "a.pt=1.0,b.pt=0.5,c.pt", "--max_seq_len", "96")
    F.check_supported(ok, ok._explicit)
    assert ok.episode_mix_balance is True and _cfg("--episode_mix", "a.pt", "--episode_mix_balance", "False").episode_mix_balance is False
    ok = _cfg("--episode_mix", "a.pt", "--max_seq_len", "96", "--image_aug", "False")           # raw frames: --image_aug is honoured
    F.check_supported(ok, ok._explicit)
    for other in ("batch_file", "frame_batch_file", "raw_batch_file", "episode_file"):
        cfg = _cfg("--episode_mix", "a.pt", "--max_seq_len", "96", f"--{other}", "x.pt", "--dataset_statistics_file", "s.json")
        with pytest.raises(ValueError, match=rf"--{other} and --episode_mix are 2 batch sources: pass one"):
            F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_mix", "a.pt")
    with pytest.raises(ValueError, match=r"need --max_seq_len .*--episode_mix"):
        F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_mix", "a.pt", "--max_seq_len", "96", "--batch_size", "2048")
    with pytest.raises(ValueError, match=r"--episode_mix .*--batch_size"):
        F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_mix", "a.pt", "--max_seq_len", "96", "--use_val_set", "True")
    with pytest.raises(NotImplementedError, match="--use_val_set with --episode_mix"):
        F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_mix", "a.pt=heavy", "--max_seq_len", "96")
    with pytest.raises(ValueError, match=r"--episode_mix: the weight of 'a.pt'"):
        F.check_supported(cfg, cfg._explicit)


def test_parse_mix():
    assert MX.parse_mix("a.pt=1.0, dir/b=0.5,c.pt") == [("a.pt", 1.0), ("dir/b", 0.5), ("c.pt", 1.0)]
    assert MX.parse_mix("x=y.pt=2") == [("x=y.pt", 2.0)]
    for bad in ("", ",", "=1.0"):
        with pytest.raises(ValueError, match="--episode_mix"):
            MX.parse_mix(bad)


def test_statistics_file_needs_every_name(mix):
    from vla_adapter_amd import finetune as F
    _, m = mix
    st = dict(m.statistics())
    act, pr = F.mixture_stats(st, m.names)
    assert [a is st[n]["action"] for a, n in zip(act, NAMES)] == [True] * 3 and [p is st[n]["proprio"] for p, n in zip(pr, NAMES)] == [True] * 3
    del st[NAMES[1]]
    with pytest.raises(KeyError, match=NAMES[1]):
        F.mixture_stats(st, m.names)


def test_sample_refuses_bad_arguments_before_the_device(mix):
    _, m = mix
    for args in ((0, 0, 0, 1, 0), (1025, 0, 0, 1, 0), (4, 0, 2, 2, 0), (4, 0, 0, 1, -1)):
        with pytest.raises(ValueError, match="sample"):
            m.sample_indices(*args)
    assert math.isclose(sum(m.p), 1.0)
