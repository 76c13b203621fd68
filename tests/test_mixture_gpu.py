"""Training on a weighted mixture of episode datasets on the device (csrc/mixture.hip, mixture.EpisodeMix): the sampler against the Python
rule, the per-row normaliser against the single-set kernel, the mixed raw batch through collate() against the indexed rows collated with
each sample's own dataset's statistics, and a fine-tune fed from --episode_mix against the same run fed the mix's batches through
--raw_batch_file."""
import json

import pytest
import torch

from tests.test_episodes_cpu import CHUNK
from tests.test_episodes_gpu import assert_batch_equal, indexed_batch
from tests.test_mixture_cpu import NAMES, PERIOD, QUOTA, WEIGHTS, make_mix, make_mix_tables
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import mixture as MX

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def mix():
    """The issue's three datasets (16, 6 and 23 windows; quotas 9, 4, 3 of a period of 16) -> (tables on the host, the mix, the tables
    back to back as one episode dict) - left unchanged."""
    tables, m = make_mix(DEV)
    bare = [{k: v for k, v in t.items() if k not in ("dataset_name", "action_mask")} for t in tables]
    return tables, m, EP.concat_shards(bare)


def host(m):
    return m.valid_off_host.tolist(), m.dataset_off_host.tolist(), m.quota_off_host.tolist()


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("B", [6, 70, 1, 64, 65])
def test_sampler_equals_the_python_rule(mix, B, world):
    """Steps 0 .. 7: at B = 6 the batches straddle the periods of 16; B = 70 spans two waves and more than four periods in one batch;
    dataset 1 (6 windows, 4 draws per period) crosses several of its own epochs.  B = 1, 64 and 65: one thread of one wave, a full
    wave, and one thread into the second wave - the scan of the prompt lengths at a wave boundary (B = 1 runs the 16 steps of a whole
    period)."""
    _, m, all_ = mix
    assert m.quota == QUOTA
    eo, lens = all_["episode_off"].tolist(), all_["prompt_off"].diff().tolist()
    got, want = [], []
    for step in range(max(8, -(-PERIOD // (B * world)))):
        for rank in range(world):
            ds, ep, row, off = m.sample_indices(B, 21, rank, world, step)
            got.append((ds.tolist(), ep.tolist(), row.tolist(), off.tolist()))
            w = MX.sample_windows(*host(m), B, 21, rank, world, step)
            want.append(([d for d, _, _ in w], [e for _, e, _ in w], [eo[e] + t for _, e, t in w],
                         [sum(lens[e] for _, e, _ in w[:b]) for b in range(B + 1)]))
    assert got == want
    ds_all = [d for g in got for d in g[0]]
    whole = len(ds_all) // PERIOD * PERIOD
    assert [ds_all[:whole].count(d) for d in range(3)] == [q * whole // PERIOD for q in QUOTA], "every whole period gives each dataset its quota"


def test_normalize_rows_equals_the_single_set_kernel(mix):
    """R = 5 rows over all three sets - one with a mask, one with a min == max column: actions [5, 8, 7] and proprio [5, 8]."""
    from vla_adapter_amd.input_stage import GPUInputStage
    tables, m, _ = mix
    stage = GPUInputStage(DEV, backbones=("siglip",), image_size=8)
    st = m.statistics()
    sel = [2, 0, 1, 2, 1]
    sel_t = torch.tensor(sel, dtype=torch.int32, device=DEV)
    for part, x in (("action", torch.stack([tables[s]["actions_raw"][3 * r:3 * r + CHUNK] for r, s in enumerate(sel)])),
                    ("proprio", torch.stack([tables[s]["proprio_raw"][2 * r] for r, s in enumerate(sel)]))):
        assert tuple(x.shape) == ((5, 8, 7) if part == "action" else (5, 8))
        entries = tuple(st[n][part] for n in NAMES)
        got = stage.normalize_rows(x, entries, sel_t)
        assert got.shape == x.shape and got.dtype == torch.float32
        for r, s in enumerate(sel):
            assert torch.equal(got[r], stage.normalize(x[r], entries[s])), (part, r, s)
        assert stage.normalize_rows(x, entries, sel_t).data_ptr() != got.data_ptr() and len([k for k in stage._stats if k[-1] == "rows"]) == (1 if part == "action" else 2)
    a = stage.normalize_rows(torch.stack([tables[2]["actions_raw"][:CHUNK]] * 2), tuple(st[n]["action"] for n in NAMES), torch.tensor([2, 1], dtype=torch.int32, device=DEV))
    assert (a[0, :, 3] == 0).all() and (a[1, :, 3] != 0).all(), "the constant column of dataset 2 is zeroed for its own rows only"
    assert torch.equal(a[1, :, 6].cpu(), tables[2]["actions_raw"][:CHUNK, 6]), "dataset 1 leaves its unmasked column as it is"
    with pytest.raises(ValueError, match="stats_index"):
        stage.collate(tables[0]["frames_u8"][:2], [[1, 2], [3]], tables[0]["actions_raw"][:16].view(2, 8, 7), action_stats=[st[NAMES[0]]["action"]], L=80)


def test_gather_of_the_mix_equals_torch_indexing(mix):
    _, m, all_ = mix
    for step, world, rank in ((0, 1, 0), (3, 2, 1)):
        got = m.sample(6, 21, rank, world, step)
        w = MX.sample_windows(*host(m), 6, 21, rank, world, step)
        assert got["dataset_names"] == NAMES and got["dataset_index"].tolist() == [d for d, _, _ in w] and got["dataset_index"].is_cuda
        assert_batch_equal(got, indexed_batch(all_, [(e, t) for _, e, t in w]))


def test_mixed_batch_through_collate_equals_each_samples_own_statistics(mix):
    """collate() of the sampled batch with the three entries and dataset_index, against the indexed rows collated once per dataset with
    that dataset's single entry (today's path): sample b must equal row b of its own dataset's collate.  Augmentation on, equal
    seed words, so the pixels and the filler ids are keyed alike."""
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    tables, m, all_ = mix
    stage = GPUInputStage(DEV, backbones=("siglip",), image_size=all_["frames_u8"].shape[2])
    st = m.statistics()
    B, seed, step = 16, 21, 1
    w = MX.sample_windows(*host(m), B, seed, 0, 1, step)
    ds = [d for d, _, _ in w]
    assert sorted(set(ds)) == [0, 1, 2]
    raw = indexed_batch(all_, [(e, t) for _, e, t in w])

    def collate(b, action_stats, proprio_stats, **kw):
        return stage.collate(b["frames_u8"].to(DEV), (b["prompt_flat"].to(DEV), b["prompt_off"].to(DEV)), b["actions_raw"].to(DEV), b["proprio_raw"].to(DEV),
                             action_stats=action_stats, proprio_stats=proprio_stats, L=80, seed=seed, rank=0, step=step,
                             augment=ImageAugment(seed=seed, rank=0, step=step), **kw)
    sampled = m.sample(B, seed, 0, 1, step)
    got = collate(sampled, tuple(st[n]["action"] for n in NAMES), tuple(st[n]["proprio"] for n in NAMES), stats_index=sampled["dataset_index"])
    own = [collate(raw, st[n]["action"], st[n]["proprio"]) for n in NAMES]
    assert set(got) == set(own[0]) == {"pixel_values", "input_ids", "labels", "attention_mask", "actions", "proprio"}
    for k in got:
        for b, d in enumerate(ds):
            assert torch.equal(got[k][b], own[d][k][b]), (k, b, d)
    assert not torch.equal(own[0]["actions"], own[2]["actions"]) and not torch.equal(own[0]["input_ids"], own[2]["input_ids"]), "the statistics matter"
    assert bool(torch.isfinite(got["actions"]).all())


def test_sample_allocates_nothing_and_never_synchronises_after_the_first_call(mix):
    _, m, _ = mix
    ptrs = {k: v.data_ptr() for k, v in m.sample(6, 1, 0, 1, 0).items() if isinstance(v, torch.Tensor)}
    assert len(ptrs) == len(EP.RAW_BATCH_KEYS) + 1
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
        again = m.sample(6, 1, 0, 1, 2)               # a read-back or a synchronising call inside raises here
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        print("torch.cuda.set_sync_debug_mode is not honoured by this build: the no-sync check did not run")
    assert after == before, "sample() allocated device memory on a batch size it had served before"
    assert {k: v.data_ptr() for k, v in again.items() if isinstance(v, torch.Tensor)} == ptrs


# ---------------------------------------------------------------------------------------------------------------- end to end
def _tiny_mix_files(tmp_path, mcfg):
    img = mcfg.vit[0].img
    g = torch.Generator().manual_seed(3)
    tables = make_mix_tables(n_img=1, hw=4, A=mcfg.action_dim, Pd=mcfg.proprio_dim)
    paths = []
    for t, name in zip(tables, NAMES):
        t["frames_u8"] = torch.randint(0, 256, (t["actions_raw"].shape[0], 1, img, img, 3), generator=g, dtype=torch.uint8)
        t["prompt_flat"] = t["prompt_flat"] % 700
        torch.save(t, tmp_path / f"{name}.pt")
        paths.append(str(tmp_path / f"{name}.pt"))
    return paths, ",".join(f"{p}={w}" for p, w in zip(paths, WEIGHTS))


def test_finetune_from_a_mix_equals_finetune_from_its_raw_batches(tmp_path):
    """Adapter-only on the tiny config, 3 logged steps at batch 4 with augmentation on: --episode_mix against --raw_batch_file on the raw
    batches the mix draws (dataset_index and dataset_names in the files, the mix's statistics in a file); the loss logs are
    bit-identical, a second run repeats them, and the checkpoint's statistics hold all three datasets."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny"]()
    assert mcfg.chunk == CHUNK
    paths, spec = _tiny_mix_files(tmp_path, mcfg)
    m = MX.EpisodeMix.load(list(zip(paths, WEIGHTS)), DEV, chunk=mcfg.chunk)
    assert m.Q == MX.DEFAULT_PERIOD and m.names == NAMES
    (tmp_path / "raw").mkdir()
    seen = set()
    for step in range(3):
        b = m.sample(4, 5, 0, 1, step)
        seen |= set(b["dataset_index"].tolist())
        torch.save({k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()}, tmp_path / "raw" / f"batch_{step:03d}.pt")
    assert len(seen) >= 2, "the three batches mix datasets"
    (tmp_path / "stats.json").write_text(json.dumps(m.statistics()))
    args = lambda tmp: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "2", "--learning_rate", "1e-3",
                        "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                        "--run_root_dir", str(tmp), "--max_seq_len", "96", "--seed", "5"]
    losses = lambda out: [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in out["log"]]
    a = F.finetune(F.parse_args(args(tmp_path / "a") + ["--episode_mix", spec]))
    b = F.finetune(F.parse_args(args(tmp_path / "b") + ["--raw_batch_file", str(tmp_path / "raw"), "--dataset_statistics_file", str(tmp_path / "stats.json")]))
    a2 = F.finetune(F.parse_args(args(tmp_path / "a2") + ["--episode_mix", spec]))
    assert len(a["log"]) == 3 and all(x == x and abs(x) < float("inf") for l in losses(a) for x in l)
    assert losses(a) == losses(b), "the mix-fed run equals the run fed the same raw batches from files"
    assert losses(a) == losses(a2), "a second run repeats the log"
    assert a["mixture"] == m.mixture_info() and a["mixture"]["datasets"] == list(NAMES) and "mixture" not in b
    saved = list((tmp_path / "a").rglob("dataset_statistics.json"))
    assert saved and all(json.load(open(p)) == m.statistics() for p in saved)
    assert sorted(json.load(open(saved[0]))) == sorted(NAMES)
    # a statistics file that lacks a dataset of the mix is refused by name
    st = m.statistics()
    (tmp_path / "short.json").write_text(json.dumps({n: st[n] for n in NAMES[:2]}))
    cfg = F.parse_args(args(tmp_path / "c") + ["--episode_mix", spec, "--dataset_statistics_file", str(tmp_path / "short.json")])
    mcfg.n_img, mcfg.pro = 1, True
    with pytest.raises(KeyError, match=NAMES[2]):
        next(F.batch_stream(cfg, mcfg, DEV, 0))


def test_lora_finetune_from_a_mix_is_finite(tmp_path):
    from vla_adapter_amd import engine as E, finetune as F
    _, spec = _tiny_mix_files(tmp_path, E.NAMED_CONFIGS["tiny"]())
    out = F.finetune(F.parse_args(["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "1", "--learning_rate", "1e-3",
                                   "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_lora", "True",
                                   "--run_root_dir", str(tmp_path / "l"), "--max_seq_len", "96", "--seed", "5", "--episode_mix", spec]))
    assert len(out["log"]) == 2 and all(x == x and abs(x) < float("inf") for l in out["log"] for x in (l["loss_value"], l["curr_action_l1_loss"]))
