"""CPU checks of training from device-resident episodes (vla_adapter_amd/episodes.py, include/vla_episodes.h): the sampling rule in plain
Python - bijection, exactly-once epochs, the reference's action windows - the statistics against numpy, and the refusals that need no
device."""
import os
import re

import numpy as np
import pytest
import torch

from vla_adapter_amd import episodes as EP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 7, 8, 9, 20]                 # episodes of the issue's store: 0, 0, 1, 2 and 13 windows at chunk 8
CHUNK = 8


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def make_tables(lengths=LENGTHS, prompt_lens=(3, 0, 11, 5, 7), n_img=2, hw=8, A=7, Pd=8, seed=0, **extra):
    """An episode file's dict: every value distinct enough that a wrong row shows."""
    g = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    d = dict(frames_u8=torch.randint(0, 256, (T, n_img, hw, hw, 3), generator=g, dtype=torch.uint8),
             actions_raw=torch.randn(T, A, generator=g) * 2, proprio_raw=torch.randn(T, Pd, generator=g) * 2,
             episode_off=torch.tensor(np.cumsum([0] + list(lengths)), dtype=torch.int64),
             prompt_flat=torch.randint(1, 1000, (sum(prompt_lens),), generator=g, dtype=torch.int64),
             prompt_off=torch.tensor(np.cumsum([0] + list(prompt_lens)), dtype=torch.int32))
    d.update(extra)
    return d


def largest_step(B, rank, world):
    """The largest step whose batch ends at a position below 2^63, in Python integers."""
    step = (2 ** 63 - 1 - (B - 1) - rank * B) // (world * B)
    assert EP.sample_position(B, rank, world, step, B - 1) <= 2 ** 63 - 1 < EP.sample_position(B, rank, world, step + 1, B - 1)
    return step


@pytest.mark.parametrize("B, rank, world", [(4, 0, 1), (4, 2, 3), (2, 1, 2), (1024, 7, 8), (1000, 5, 2 ** 20)])
def test_sample_refuses_a_stream_position_beyond_63_bits(lib, B, rank, world):
    """The largest step whose last sample stands below 2^63 passes the position check - the call is then stopped by the NEXT check, B *
    Pmax, which this test violates on purpose so that nothing is launched - and the step behind it is refused by name.  The Python
    rule refuses the same arguments."""
    P, step = 8, largest_step(B, rank, world)
    call = lambda s: lib.vla_episode_sample(None, P, P, P, 5, 0, rank, world, s, B, 2 ** 31 - 1, P, P, P)
    assert call(step) == -1 and b"B * Pmax" in lib.vla_last_error(), "accepted by the position check"
    assert call(step + 1) == -1 and b"stream position overflows 63 bits" in lib.vla_last_error()
    assert call(2 ** 63 - 1) == -1 and b"stream position overflows 63 bits" in lib.vla_last_error()
    EP.check_position(B, rank, world, step)
    with pytest.raises(ValueError, match="stream position overflows 63 bits"):
        EP.check_position(B, rank, world, step + 1)
    assert lib.vla_episode_sample(None, P, P, P, 5, 0, 2 ** 62, 2 ** 62 + 1, 0, B, 2 ** 31 - 1, P, P, P) == -1
    assert b"stream position overflows 63 bits" in lib.vla_last_error(), "a rank term that overflows on its own"


def test_the_store_refuses_the_overflowing_step_before_the_device():
    st = EP.EpisodeStore.from_dict(make_tables(), "cpu", chunk=CHUNK)
    with pytest.raises(ValueError, match="stream position overflows 63 bits"):
        st.sample_indices(4, 0, 2, 3, largest_step(4, 2, 3) + 1)


def test_the_window_tail_and_the_tables_are_stated_once():
    """csrc/windows.h alone defines clampll, last_not_above, EPISODE_STREAM and the scan of the prompt lengths; the three picker files
    include it, call emit_windows and restate none of them.  The package states the raw-batch buffers and MAX_BATCH once."""
    csrc, pkg = os.path.join(ROOT, "vla_adapter_amd", "csrc"), os.path.join(ROOT, "vla_adapter_amd")
    stated = ("long long clampll(", "int last_not_above(", "EPISODE_STREAM =", "scan[b] += v;")
    head = open(os.path.join(csrc, "windows.h")).read()
    assert all(head.count(s) == 1 for s in stated) and head.count("__forceinline__ void emit_windows(") == 1
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            txt = open(os.path.join(csrc, f)).read()
            assert not any(s in txt for s in stated), f
            assert txt.count("emit_windows(") == ('#include "windows.h"' in txt) == (f in ("episodes.hip", "mixture.hip", "heldout.hip")), f
    assert "windows.h" in open(os.path.join(csrc, "Makefile")).read()
    py = "".join(open(os.path.join(pkg, f)).read() for f in sorted(os.listdir(pkg)) if f.endswith(".py"))
    assert py.count("def _buffers") == 1 and len(re.findall(r"^MAX_BATCH = ", py, re.M)) == 1


# ---------------------------------------------------------------------------------------------------------------- the sampling rule
def test_splitmix64_key_restates_the_header():
    """The constants of csrc/common.h's splitmix64_key, and two values of the public splitmix64 sequence (seed 0: the first outputs of
    the generator are the finaliser of 1 and 2 golden-ratio steps)."""
    txt = open(os.path.join(ROOT, "vla_adapter_amd", "csrc", "common.h")).read()
    body = txt[txt.index("splitmix64_key(unsigned long long seed"):]
    body = body[:body.index("}")]
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", ">> 30", ">> 27", ">> 31"):
        assert const in body
    assert EP.splitmix64_key(0, 1) == 0xE220A8397B1DCDAF and EP.splitmix64_key(0, 2) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 16, 17, 37, 1000])
def test_permute_index_is_a_bijection(N):
    for key in (0, EP.epoch_key(0, 0), EP.epoch_key(12345, 3), (1 << 64) - 1):
        assert sorted(EP.permute_index(i, N, key) for i in range(N)) == list(range(N)), (N, key)
    if N == 1:
        assert EP.permute_index(0, 1, 99) == 0
    with pytest.raises(ValueError):
        EP.permute_index(N, N, 0)


def test_two_epochs_and_two_seeds_give_different_orders():
    order = lambda seed, epoch: [EP.permute_index(i, 37, EP.epoch_key(seed, epoch)) for i in range(37)]
    assert order(3, 0) != order(3, 1) and order(3, 0) != order(4, 0)
    assert order(3, 0) == order(3, 0) and order(3, 0) != list(range(37)), "keyed, repeatable, and a shuffle"


def test_one_epoch_covers_every_window_exactly_once_across_ranks_and_steps():
    """N = 37, B = 4, 2 ranks: positions 0 .. 39 are steps 0 .. 4; the 37 of epoch 0 cover the windows once, the last batch (rank 1 of
    step 4) takes its last three from epoch 1."""
    N, B, world, seed = 37, 4, 2, 11
    seen, tail = [], []
    for step in range(5):
        for rank in range(world):
            for b in range(B):
                pos = EP.sample_position(B, rank, world, step, b)
                j = EP.permute_index(pos % N, N, EP.epoch_key(seed, pos // N))
                (seen if pos // N == 0 else tail).append((pos, j, rank, step))
    assert sorted(p for p, *_ in seen + tail) == list(range(40)), "the ranks' batches tile the positions without gap or overlap"
    assert sorted(j for _, j, *_ in seen) == list(range(N)), "epoch 0 visits every window exactly once"
    assert len(tail) == 3 and all(r == 1 and s == 4 for _, _, r, s in tail), "the last batch straddles the epochs"
    assert [j for _, j, *_ in tail] == [EP.permute_index(i, N, EP.epoch_key(seed, 1)) for i in range(3)]
    # the same through sample_windows on a one-episode table
    valid = [0, N]
    got = [w for step in range(5) for rank in range(world) for w in EP.sample_windows(valid, B, seed, rank, world, step)]
    assert sorted(t for _, t in got[:N]) == list(range(N)) and all(e == 0 for e, _ in got)


def chunk_act_obs_numpy(traj_len, window_size=1, future_action_window_size=CHUNK - 1):
    """traj_transforms.py:24-43 in numpy -> (observation indices [n, window], action indices [n, window + future]), n = effective_traj_len."""
    eff = max(traj_len - future_action_window_size, 0)
    chunk_idx = np.arange(-window_size + 1, 1)[None, :] + np.arange(eff)[:, None]
    act_idx = np.arange(-window_size + 1, 1 + future_action_window_size)[None, :] + np.arange(eff)[:, None]
    goal = np.full((eff, 1), traj_len - 1)
    return np.maximum(chunk_idx, 0), np.minimum(np.maximum(act_idx, 0), goal)


def test_windows_match_chunk_act_obs():
    """Every window index j -> locate -> (episode, t); the observation row and the clamped action rows equal the reference's gather
    indices of that episode, episode by episode, in order."""
    eo = np.cumsum([0] + LENGTHS)
    valid = EP.valid_offsets(torch.tensor(eo), CHUNK).tolist()
    assert np.diff(valid).tolist() == [0, 0, 1, 2, 13]
    want = []
    for e, n in enumerate(LENGTHS):
        obs, act = chunk_act_obs_numpy(n)
        assert obs.shape[0] == valid[e + 1] - valid[e]
        want += [(e, int(eo[e] + o[0]), (eo[e] + a).tolist()) for o, a in zip(obs, act)]
    got = []
    for j in range(valid[-1]):
        e, t = EP.locate(j, valid)
        got.append((e, int(eo[e] + t), EP.window_rows(int(eo[e] + t), int(eo[e + 1]), CHUNK)))
    assert got == want
    # the clamp binds only for a start the sampler never draws: the last row of the 9-step episode repeats its goal step
    assert EP.window_rows(int(eo[4]) - 1, int(eo[4]), CHUNK) == [int(eo[4]) - 1] * CHUNK


# ---------------------------------------------------------------------------------------------------------------- the store on the host
def test_statistics_match_numpy_with_a_constant_column():
    d = make_tables(dataset_name="toy", action_mask=torch.tensor([True] * 6 + [False]))
    d["actions_raw"][:, 2] = 0.25
    st = EP.EpisodeStore.from_dict(d, "cpu", chunk=CHUNK).statistics()
    assert list(st) == ["toy"] and sorted(st["toy"]) == ["action", "num_trajectories", "num_transitions", "proprio"]
    assert st["toy"]["num_transitions"] == sum(LENGTHS) and st["toy"]["num_trajectories"] == len(LENGTHS)
    for part, x in (("action", d["actions_raw"].numpy()), ("proprio", d["proprio_raw"].numpy())):
        want = dict(mean=x.mean(0), std=x.std(0), max=x.max(0), min=x.min(0), q01=np.quantile(x, 0.01, axis=0), q99=np.quantile(x, 0.99, axis=0))
        assert sorted(k for k in st["toy"][part] if k != "mask") == sorted(want)
        for k, v in want.items():
            assert st["toy"][part][k] == v.tolist(), (part, k)
    a = st["toy"]["action"]
    assert a["min"][2] == a["max"][2] == 0.25 and a["mask"] == [True] * 6 + [False] and "mask" not in st["toy"]["proprio"]
    import json
    assert json.loads(json.dumps(st)) == st, "plain lists and numbers: what dataset_statistics.json holds"
    # no name in the file: the caller's, else a default
    assert list(EP.EpisodeStore.from_dict(make_tables(), "cpu", dataset_name="mine").statistics()) == ["mine"]


def test_store_tables_and_shards(tmp_path):
    d = make_tables()
    st = EP.EpisodeStore.from_dict(d, "cpu", chunk=CHUNK)
    assert st.valid_off.tolist() == [0, 0, 0, 1, 3, 16] and st.N == 16 and (st.E, st.T, st.A, st.Pd, st.Pmax) == (5, 45, 7, 8, 11)
    assert st.row_bytes == 2 * 8 * 8 * 3
    # a directory of two shards equals the one file
    cut, pcut = int(d["episode_off"][3]), int(d["prompt_off"][3])
    a = dict(frames_u8=d["frames_u8"][:cut], actions_raw=d["actions_raw"][:cut], proprio_raw=d["proprio_raw"][:cut],
             episode_off=d["episode_off"][:4].clone(), prompt_flat=d["prompt_flat"][:pcut], prompt_off=d["prompt_off"][:4].clone())
    b = dict(frames_u8=d["frames_u8"][cut:], actions_raw=d["actions_raw"][cut:], proprio_raw=d["proprio_raw"][cut:],
             episode_off=d["episode_off"][3:] - cut, prompt_flat=d["prompt_flat"][pcut:], prompt_off=d["prompt_off"][3:] - pcut)
    (tmp_path / "demos").mkdir()
    torch.save({k: v.clone() for k, v in a.items()}, tmp_path / "demos" / "shard_000.pt")
    torch.save({k: v.clone() for k, v in b.items()}, tmp_path / "demos" / "shard_001.pt")
    two = EP.EpisodeStore.load(tmp_path / "demos", "cpu", chunk=CHUNK)
    for k in ("frames_u8", "actions_raw", "proprio_raw", "episode_off", "prompt_flat", "prompt_off", "valid_off"):
        assert torch.equal(getattr(two, k), getattr(st, k)) and getattr(two, k).dtype == getattr(st, k).dtype, k
    assert two.statistics() == st.statistics()
    with pytest.raises(FileNotFoundError):
        (tmp_path / "empty").mkdir()
        EP.EpisodeStore.load(tmp_path / "empty", "cpu")


@pytest.mark.parametrize("key, spoil", [
    ("episode_off", lambda d: d["episode_off"].__setitem__(0, 1)),                      # first offset not 0
    ("episode_off", lambda d: d["episode_off"].__setitem__(-1, 44)),                    # last offset not T
    ("episode_off", lambda d: d["episode_off"].__setitem__(2, 20)),                     # a step back
    ("episode_off", lambda d: d.__setitem__("episode_off", d["episode_off"].to(torch.int32))),
    ("prompt_off", lambda d: d["prompt_off"].__setitem__(-1, 99)),                      # past the flat table
    ("prompt_off", lambda d: d["prompt_off"].__setitem__(1, 20)),                       # a step back behind it
    ("prompt_off", lambda d: d.__setitem__("prompt_off", d["prompt_off"][:-1])),        # not one prompt per episode
    ("actions_raw", lambda d: d.__setitem__("actions_raw", d["actions_raw"][:-1])),     # shapes disagree
    ("proprio_raw", lambda d: d.__setitem__("proprio_raw", d["proprio_raw"].double())),
    ("frames_u8", lambda d: d.__setitem__("frames_u8", d["frames_u8"][..., :2])),
    ("prompt_flat", lambda d: d.pop("prompt_flat")),
    ("action_mask", lambda d: d.__setitem__("action_mask", torch.ones(6, dtype=torch.bool))),
])
def test_malformed_tables_are_refused_by_key(key, spoil):
    d = make_tables()
    spoil(d)
    with pytest.raises(ValueError, match=key):
        EP.EpisodeStore.from_dict(d, "cpu", chunk=CHUNK)


def test_a_store_without_a_valid_window_is_refused():
    with pytest.raises(ValueError, match="no valid window"):
        EP.EpisodeStore.from_dict(make_tables(lengths=[1, 7, 3], prompt_lens=(2, 2, 2)), "cpu", chunk=CHUNK)
    assert EP.EpisodeStore.from_dict(make_tables(lengths=[1, 7, 3], prompt_lens=(2, 2, 2)), "cpu", chunk=7).N == 1


# ---------------------------------------------------------------------------------------------------------------- finetune's refusals
def _cfg(*extra):
    from vla_adapter_amd import finetune as F
    return F.parse_args(["--use_proprio", "True", "--use_fz", "True", *extra])


def test_episode_file_is_a_fourth_batch_source():
    from vla_adapter_amd import finetune as F
    ok = _cfg("--episode_file", "demos", "--max_seq_len", "96")
    F.check_supported(ok, ok._explicit)
    ok = _cfg("--episode_file", "demos", "--max_seq_len", "96", "--image_aug", "False")       # raw frames: --image_aug is honoured
    F.check_supported(ok, ok._explicit)
    for other in ("batch_file", "frame_batch_file", "raw_batch_file"):
        cfg = _cfg("--episode_file", "demos", "--max_seq_len", "96", f"--{other}", "x.pt", "--dataset_statistics_file", "s.json")
        with pytest.raises(ValueError, match=rf"--{other} and --episode_file are 2 batch sources: pass one"):
            F.check_supported(cfg, cfg._explicit)


def test_episode_file_needs_max_seq_len():
    from vla_adapter_amd import finetune as F
    cfg = _cfg("--episode_file", "demos")
    with pytest.raises(ValueError, match=r"raw batches with prompt offsets on the device need --max_seq_len \(the natural length would be read back\)"):
        F.check_supported(cfg, cfg._explicit)


def test_episode_file_refuses_validation_without_held_out_batches():
    from vla_adapter_amd import finetune as F
    cfg = _cfg("--episode_file", "demos", "--max_seq_len", "96", "--use_val_set", "True")
    with pytest.raises(NotImplementedError, match="--use_val_set with --episode_file"):
        F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_file", "demos", "--max_seq_len", "96", "--use_val_set", "True", "--val_batch_file", "val.pt")
    F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--episode_file", "demos", "--max_seq_len", "96", "--batch_size", "2048")
    with pytest.raises(ValueError, match="batch_size"):
        F.check_supported(cfg, cfg._explicit)
