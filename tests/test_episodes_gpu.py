"""Training from device-resident episodes on the device (csrc/episodes.hip, episodes.EpisodeStore): the sampler against the Python rule,
the gather against torch indexing of the store on both copy arms, the clamps, the raw batch through collate(), and a fine-tune fed
from --episode_file against the same run fed the store's batches through --raw_batch_file."""
import json

import pytest
import torch

from tests.test_episodes_cpu import CHUNK, LENGTHS, make_tables
from vla_adapter_amd import episodes as EP

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_WINDOWS = 16


@pytest.fixture(scope="module", params=[8, 5], ids=["rows-of-384-B", "rows-of-150-B"])
def store(request):
    """E = 5 episodes of 1, 7, 8, 9 and 20 steps, prompts of 3, 0, 11, 5 and 7 ids, two views: 384-byte rows move in 16-byte chunks,
    150-byte rows byte by byte.  (tables on the host, the store) - left unchanged."""
    d = make_tables(hw=request.param, dataset_name="toy")
    return d, EP.EpisodeStore.from_dict(d, DEV, chunk=CHUNK)


def indexed_batch(d, windows):
    """The raw batch of (episode, t) windows by torch indexing of the host tables: the five outputs of the gather."""
    eo, po = d["episode_off"].tolist(), d["prompt_off"].tolist()
    rows = [eo[e] + t for e, t in windows]
    B, Pmax = len(windows), int(d["prompt_off"].diff().max())
    flat = [x for e, _ in windows for x in d["prompt_flat"][po[e]:po[e + 1]].tolist()]
    off = [0]
    for e, _ in windows:
        off.append(off[-1] + po[e + 1] - po[e])
    win = torch.tensor([EP.window_rows(r, eo[e + 1], CHUNK) for r, (e, _) in zip(rows, windows)])
    return dict(frames_u8=d["frames_u8"][rows], actions_raw=d["actions_raw"][win], proprio_raw=d["proprio_raw"][rows],
                prompt_flat=torch.tensor(flat + [0] * (B * Pmax - len(flat)), dtype=torch.int64), prompt_off=torch.tensor(off, dtype=torch.int32))


def assert_batch_equal(got, want):
    for k in EP.RAW_BATCH_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu().view(torch.uint8), want[k].contiguous().view(torch.uint8)), k      # bit for bit


@pytest.mark.parametrize("B", [6, 1, 64, 65])
@pytest.mark.parametrize("world", [1, 2])
def test_sampler_equals_the_python_rule(store, world, B):
    """B = 6, steps 0 .. 5: 36 (72) positions over N = 16 windows cross epoch boundaries inside a batch.  B = 1, 64 and 65: one thread
    of one wave, a full wave, and one thread into the second wave - the scan of the prompt lengths at a wave boundary (B = 1 runs the
    16 steps that epoch 0 takes)."""
    d, st = store
    assert st.N == N_WINDOWS
    valid, eo, lens = st.valid_off_host.tolist(), d["episode_off"].tolist(), d["prompt_off"].diff().tolist()
    got, want = [], []
    for step in range(max(6, -(-N_WINDOWS // (B * world)))):
        for rank in range(world):
            ep, row, off = st.sample_indices(B, 21, rank, world, step)
            got.append((ep.tolist(), row.tolist(), off.tolist()))
            w = EP.sample_windows(valid, B, 21, rank, world, step)
            want.append(([e for e, _ in w], [eo[e] + t for e, t in w], [sum(lens[e] for e, _ in w[:b]) for b in range(B + 1)]))
    assert got == want
    firsts = [r for _, rows, _ in got for r in rows][:N_WINDOWS]
    assert len(set(firsts)) == N_WINDOWS, "epoch 0 visits every window once"


def test_gather_equals_torch_indexing(store):
    d, st = store
    valid = st.valid_off_host.tolist()
    for step, world, rank in ((0, 1, 0), (2, 1, 0), (3, 2, 1)):
        got = st.sample(6, 21, rank, world, step)
        assert got["dataset_name"] == "toy" and all(got[k].is_cuda for k in EP.RAW_BATCH_KEYS)
        assert_batch_equal(got, indexed_batch(d, EP.sample_windows(valid, 6, 21, rank, world, step)))
    # one window per sample (B = 16 = N): every window of the store, and the empty prompt among them
    got = st.sample(16, 5, 0, 1, 0)
    w = EP.sample_windows(valid, 16, 5, 0, 1, 0)
    assert sorted(w) == [(2, 0), (3, 0), (3, 1)] + [(4, t) for t in range(13)]
    assert_batch_equal(got, indexed_batch(d, w))


def test_gather_clamps_bad_indices_into_the_store(store):
    """Episode indices below 0 and past E - 1, rows before and behind their episode: the gather returns the nearest in-range row of the
    clamped episode (and windows that run to the goal step repeat it) - nothing outside the store is read."""
    from vla_adapter_amd import ops
    d, st = store
    eo = d["episode_off"].tolist()
    bad_ep = [-3, 99, 2, 4, 3, 0]
    bad_row = [10 ** 9, -5, eo[3] - 1, eo[5] + 40, eo[3], -(10 ** 12)]
    o = st._buffers(6)
    o["ep"].copy_(torch.tensor(bad_ep, dtype=torch.int32))
    o["row"].copy_(torch.tensor(bad_row, dtype=torch.int64))
    lens = d["prompt_off"].diff().tolist()
    eps = [min(max(e, 0), st.E - 1) for e in bad_ep]
    o["prompt_off"].copy_(torch.tensor([sum(lens[e] for e in eps[:b]) for b in range(7)], dtype=torch.int32))
    ops.episode_gather(st.frames_u8, st.actions_raw, st.proprio_raw, st.episode_off, st.prompt_flat, st.prompt_off, o["ep"], o["row"], o["prompt_off"],
                       o["frames_u8"], o["actions_raw"], o["proprio_raw"], o["prompt_flat"], st.Pmax)
    windows = [(e, min(max(r, eo[e]), eo[e + 1] - 1) - eo[e]) for e, r in zip(eps, bad_row)]
    assert windows == [(0, 0), (4, 0), (2, 7), (4, 19), (3, 0), (0, 0)]
    assert_batch_equal({k: o[k] for k in EP.RAW_BATCH_KEYS}, indexed_batch(d, windows))
    assert torch.equal(o["actions_raw"][2].cpu(), d["actions_raw"][eo[3] - 1].expand(CHUNK, -1)), "the goal step repeats"


def test_sample_allocates_nothing_and_never_synchronises_after_the_first_call(store):
    _, st = store
    ptrs = {k: v.data_ptr() for k, v in st.sample(6, 1, 0, 1, 0).items() if isinstance(v, torch.Tensor)}
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        again = st.sample(6, 1, 0, 1, 2)               # a read-back or a synchronising call inside raises here
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        print("torch.cuda.set_sync_debug_mode is not honoured by this build: the no-sync check did not run")
    assert after == before, "sample() allocated device memory on a batch size it had served before"
    assert {k: v.data_ptr() for k, v in again.items() if isinstance(v, torch.Tensor)} == ptrs


def test_sampled_batch_through_collate_equals_the_indexed_batch(store):
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    d, st = store
    stage = GPUInputStage(DEV, backbones=("siglip",), image_size=d["frames_u8"].shape[2])
    stats = st.statistics()["toy"]
    want_raw = indexed_batch(d, EP.sample_windows(st.valid_off_host.tolist(), 6, 21, 0, 1, 1))

    def collate(b):
        return stage.collate(b["frames_u8"].to(DEV), (b["prompt_flat"].to(DEV), b["prompt_off"].to(DEV)), b["actions_raw"].to(DEV), b["proprio_raw"].to(DEV),
                             action_stats=stats["action"], proprio_stats=stats["proprio"], L=80, seed=21, rank=0, step=1,
                             augment=ImageAugment(seed=21, rank=0, step=1))
    got, want = collate(st.sample(6, 21, 0, 1, 1)), collate(want_raw)
    assert set(got) == set(want) == {"pixel_values", "input_ids", "labels", "attention_mask", "actions", "proprio"}
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["actions"]).all()) and float(got["actions"].abs().max()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- end to end
def _tiny_episode_file(tmp_path, mcfg):
    img = mcfg.vit[0].img
    g = torch.Generator().manual_seed(3)
    d = make_tables(prompt_lens=(10, 0, 27, 5, 24), n_img=1, hw=4, A=mcfg.action_dim, Pd=mcfg.proprio_dim, dataset_name="toy")
    d["frames_u8"] = torch.randint(0, 256, (sum(LENGTHS), 1, img, img, 3), generator=g, dtype=torch.uint8)
    d["prompt_flat"] = d["prompt_flat"] % 700
    torch.save(d, tmp_path / "episodes.pt")
    return d, tmp_path / "episodes.pt"


def test_finetune_from_episodes_equals_finetune_from_their_raw_batches(tmp_path):
    """Adapter-only on the tiny config, 3 steps at batch 4 with augmentation on: --episode_file against --raw_batch_file on the three raw
    batches the store draws (statistics from the store, written to a file); the loss logs are bit-identical, a second run repeats
    them, and the checkpoint carries the store's statistics."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny"]()
    assert mcfg.chunk == CHUNK
    d, f = _tiny_episode_file(tmp_path, mcfg)
    st = EP.EpisodeStore.load(f, DEV, chunk=mcfg.chunk)
    (tmp_path / "raw").mkdir()
    for step in range(3):
        b = st.sample(4, 5, 0, 1, step)
        torch.save({k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}, tmp_path / "raw" / f"batch_{step:03d}.pt")
    (tmp_path / "stats.json").write_text(json.dumps(st.statistics()))
    args = lambda tmp: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "2", "--learning_rate", "1e-3",
                        "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                        "--run_root_dir", str(tmp), "--max_seq_len", "96", "--seed", "5"]
    losses = lambda out: [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in out["log"]]
    a = F.finetune(F.parse_args(args(tmp_path / "a") + ["--episode_file", str(f)]))
    b = F.finetune(F.parse_args(args(tmp_path / "b") + ["--raw_batch_file", str(tmp_path / "raw"), "--dataset_statistics_file", str(tmp_path / "stats.json")]))
    a2 = F.finetune(F.parse_args(args(tmp_path / "a2") + ["--episode_file", str(f)]))
    assert len(a["log"]) == 3 and all(x == x and abs(x) < float("inf") for l in losses(a) for x in l)
    assert losses(a) == losses(b), "the episode-fed run equals the run fed the same raw batches from files"
    assert losses(a) == losses(a2), "a second run repeats the log"
    saved = list((tmp_path / "a").rglob("dataset_statistics.json"))
    assert saved and all(json.load(open(p)) == st.statistics() for p in saved)
    assert json.load(open(saved[0]))["toy"]["num_trajectories"] == len(LENGTHS)


def test_lora_finetune_from_episodes_is_finite(tmp_path):
    from vla_adapter_amd import engine as E, finetune as F
    _, f = _tiny_episode_file(tmp_path, E.NAMED_CONFIGS["tiny"]())
    out = F.finetune(F.parse_args(["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "1", "--learning_rate", "1e-3",
                                   "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_lora", "True",
                                   "--run_root_dir", str(tmp_path / "l"), "--max_seq_len", "96", "--seed", "5", "--episode_file", str(f)]))
    assert len(out["log"]) == 2 and all(x == x and abs(x) < float("inf") for l in out["log"] for x in (l["loss_value"], l["curr_action_l1_loss"]))
