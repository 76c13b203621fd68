"""Validation on held-out episodes on the device (csrc/heldout.hip, heldout.HeldOutSweep): both kernels against their Python rules bit
for bit, a full sweep against the existing validation forward on the same windows, fine-tunes whose training is untouched by the
sweeps and by the held-out episodes, a mixture whose per-dataset numbers are those of each dataset alone, the time limit, two ranks
sharing one sweep, and a second sweep that needs no new device memory and no host wait."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_episodes_cpu import CHUNK, make_tables
from tests.test_episodes_gpu import indexed_batch
from tests.test_heldout_cpu import F as FRACTION, LENGTHS, LENGTHS_B, make_pair, make_store
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import heldout as HO
from vla_adapter_amd import mixture as MX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
L = 96
LONG = [20, 130, 130]                      # f = 0.67 holds the last 2 episodes out: 246 held-out windows, 13 to train on
ENTRY_KEYS = {"step", "loss_value", "loss", "curr_action_l1_loss", "next_actions_l1_loss", "val_batches_count", "val_samples_count",
              "val_windows_total", "l1_by_chunk_step", "l1_by_action_dim", "per_dataset"}
DATASET_KEYS = (ENTRY_KEYS - {"step", "val_batches_count", "per_dataset"}) | {"l1_by_action_dim_raw"}


# ---------------------------------------------------------------------------------------------------------------- 1: the sweep kernel
def _sources():
    _, s = make_store(DEV)
    _, m = make_pair(DEV)
    long_ = EP.EpisodeStore.from_dict(make_tables(lengths=LONG, prompt_lens=(3, 9, 4), dataset_name="long"), DEV, chunk=CHUNK, holdout=0.67)
    return {"store": s, "mix": m, "long": long_}


@pytest.fixture(scope="module")
def sources():
    return _sources()


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("B", [6, 70, 1, 64, 65])
def test_sweep_kernel_equals_the_python_rule(sources, B, world, stride):
    """Batches j = 0 .. 3 of every rank.  The issue's store (8 held-out windows, dataset_off NULL) and the two-dataset mix (10, the
    last episode without a window) give a full batch at B = 6, j = 0, partly valid ones and wholly invalid ones; the long store (246)
    fills a whole batch of 70 - a scan across two waves - even at stride 3, before its partly valid and its empty ones.  B = 1, 64 and
    65: one thread of one wave, a full wave, and one thread into the second wave (batches of one are whole or empty, never part:
    j = 0 .. 11 runs past the 8 and the 10 windows)."""
    from vla_adapter_amd import ops
    assert sources["long"].Nv == 246 and sources["store"].Nv == 8 and sources["mix"].Nv == 10
    kinds = set()
    for name, s in sources.items():
        mixed = name == "mix"
        val, ds_off = s.val_off_host.tolist(), (s.dataset_off_host.tolist() if mixed else None)
        eo, lens = s.episode_off.tolist(), s.prompt_off.diff().tolist()
        e = torch.empty
        ds, ep, valid = e(B, dtype=torch.int32, device=DEV), e(B, dtype=torch.int32, device=DEV), e(B, dtype=torch.uint8, device=DEV)
        row, off = e(B, dtype=torch.int64, device=DEV), e(B + 1, dtype=torch.int32, device=DEV)
        for rank in range(world):
            for j in range(4 if B > 1 else 12):
                for t in (ds, ep, valid, row, off):
                    t.fill_(99)
                ops.heldout_sweep(s.val_off, s.episode_off, s.prompt_off, s.dataset_off if mixed else None, rank, world, j, stride, s.Pmax,
                                  ds, ep, row, off, valid)
                w = HO.sweep_windows(val, ds_off, B, rank, world, j, stride)
                got = (valid.tolist(), ds.tolist(), ep.tolist(), row.tolist(), off.tolist())
                want = ([ok for ok, _, _, _ in w], [d for _, d, _, _ in w], [x for _, _, x, _ in w], [eo[x] + t for _, _, x, t in w],
                        [sum(lens[x] for _, _, x, _ in w[:b]) for b in range(B + 1)])
                assert got == want, (name, rank, j)
                n = sum(want[0])
                kinds.add((name, "full" if n == B else "empty" if n == 0 else "part"))
    if B == 1:
        assert ("long", "full") in kinds and {k for _, k in kinds} == {"full", "empty"}
    else:
        assert ("long", "full") in kinds and {k for _, k in kinds} == {"full", "part", "empty"} and ("mix", "part") in kinds
    if B == 6 and stride == 1 and world == 1:
        assert ("store", "full") in kinds and ("mix", "full") in kinds


def test_sweep_and_mixture_sampler_agree_on_the_same_window(sources):
    """Two kernels through one tail (csrc/windows.h): over the mix's TRAINING table, window w of vla_heldout_sweep and the draw of
    vla_mixture_sample at a position whose rule (MX.sample_window, on the CPU) lands on the same (episode, step) write the same ep, row
    and prompt_off, bit for bit - for every one of the 20 training windows, each pair two launches of one workgroup of B = 1.  One sweep
    batch over all 20 windows then repeats every pair's row and prompt length inside a scan over 20 threads."""
    from vla_adapter_amd import ops
    m = sources["mix"]
    valid, ds_off, q_off = m.valid_off_host.tolist(), m.dataset_off_host.tolist(), m.quota_off_host.tolist()
    N = m.N
    assert N == 20 and m.windows == [16, 4]
    position = {}                                                        # (e, t) -> the first position that draws it
    for pos in range(64 * 16):
        _, _, e, t = MX.sample_window(pos, valid, ds_off, q_off, 21)
        position.setdefault((e, t), pos)
        if len(position) == N:
            break
    assert len(position) == N, "64 periods draw every training window"
    e_ = torch.empty
    new = lambda n: dict(ds=e_(n, dtype=torch.int32, device=DEV), ep=e_(n, dtype=torch.int32, device=DEV), row=e_(n, dtype=torch.int64, device=DEV),
                         off=e_(n + 1, dtype=torch.int32, device=DEV), valid=e_(n, dtype=torch.uint8, device=DEV))
    a, b, pairs = new(1), new(1), []
    for w in range(N):
        for o in (a, b):
            for t in o.values():
                t.fill_(99)
        ops.heldout_sweep(m.valid_off, m.episode_off, m.prompt_off, m.dataset_off, 0, 1, w, 1, m.Pmax, a["ds"], a["ep"], a["row"], a["off"], a["valid"])
        pos = position[EP.locate(w, valid)]
        ops.mixture_sample(m.valid_off, m.episode_off, m.prompt_off, m.dataset_off, m.quota_off, 21, 0, 1, pos, m.Pmax, b["ds"], b["ep"], b["row"], b["off"])
        got = {k: a[k].tolist() for k in ("ds", "ep", "row", "off")}
        assert got == {k: b[k].tolist() for k in ("ds", "ep", "row", "off")} and a["valid"].tolist() == [1], (w, pos)
        assert (got["ep"][0], got["row"][0] - int(m.episode_off[got["ep"][0]])) == EP.locate(w, valid) and got["off"][0] == 0
        pairs.append((got["ep"][0], got["row"][0], got["off"][1]))
    c = new(N)
    ops.heldout_sweep(m.valid_off, m.episode_off, m.prompt_off, m.dataset_off, 0, 1, 0, 1, m.Pmax, c["ds"], c["ep"], c["row"], c["off"], c["valid"])
    assert list(zip(c["ep"].tolist(), c["row"].tolist(), c["off"].diff().tolist())) == pairs and c["off"][0].item() == 0


# ---------------------------------------------------------------------------------------------------------------- 2: the accumulation
def _bf16(*shape, seed):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.7).to(torch.bfloat16)


@pytest.mark.parametrize("B, C, A, D", [(6, 8, 7, 1), (70, 8, 7, 2), (5, 25, 14, 3)])
def test_accumulate_equals_the_reference(B, C, A, D):
    """Two calls in a row on different batches, against two applications of the rule; ds carries indices below 0 and past D - 1; the
    invalid rows of pred then get NaN and Inf and the sums must not move; a batch without a valid row changes nothing."""
    from vla_adapter_amd import ops
    pred, tgt = [_bf16(B, C, A, seed=10 * B + k) for k in range(2)], [_bf16(B, C, A, seed=10 * B + 5 + k) for k in range(2)]
    valid = torch.tensor([0 if b % 4 == 1 else 1 for b in range(B)], dtype=torch.uint8)
    ds = None
    if D > 1:
        ds = torch.tensor([(b * 7) % D for b in range(B)], dtype=torch.int32)
        ds[2], ds[3] = -5, D + 2
    dv = lambda t: None if t is None else t.to(DEV)
    acc0 = torch.rand(D, C, A, generator=torch.Generator().manual_seed(B), dtype=torch.float64)
    cnt0 = torch.arange(D, dtype=torch.int64) + 3

    def run(preds):
        acc, cnt = acc0.to(DEV), cnt0.to(DEV)
        for p, t in zip(preds, tgt):
            ops.heldout_l1_accumulate(dv(p), dv(t), dv(ds), dv(valid), acc, cnt)
        return acc.cpu().numpy(), cnt.cpu().numpy()

    acc, cnt = run(pred)
    want_a, want_c = acc0.numpy(), cnt0.numpy()
    for p, t in zip(pred, tgt):
        want_a, want_c = HO.l1_accumulate_reference(p.float().numpy(), t.float().numpy(), None if ds is None else ds.tolist(), valid.tolist(), D, want_a, want_c)
    assert np.array_equal(acc.view(np.int64), want_a.view(np.int64)), "bit for bit"
    assert cnt.tolist() == want_c.tolist() and int(cnt.sum() - cnt0.sum()) == 2 * int(valid.sum())
    if D > 1:
        assert want_c[0] > cnt0[0] and want_c[D - 1] > cnt0[D - 1], "the clamped rows are counted at both ends"
    poisoned = [p.clone() for p in pred]
    for p in poisoned:
        p[valid == 0] = float("nan")
        p[1, 0, 0] = float("inf")                    # row 1 is invalid
    acc2, cnt2 = run(poisoned)
    assert np.isfinite(acc2).all() and np.array_equal(acc2.view(np.int64), acc.view(np.int64)) and cnt2.tolist() == cnt.tolist()
    a, c = acc0.to(DEV), cnt0.to(DEV)
    ops.heldout_l1_accumulate(dv(poisoned[0]), dv(tgt[0]), dv(ds), torch.zeros(B, dtype=torch.uint8, device=DEV), a, c)
    assert torch.equal(a.cpu(), acc0) and torch.equal(c.cpu(), cnt0), "all rows invalid: acc and cnt unchanged"


# ---------------------------------------------------------------------------------------------------------------- the tiny model
def _mcfg():
    from vla_adapter_amd import engine as E
    mcfg = E.NAMED_CONFIGS["tiny"]()
    mcfg.n_img, mcfg.pro = 1, True
    assert mcfg.chunk == CHUNK
    return mcfg


def _tiny_tables(lengths, prompts, name, seed, scale=1.0, shift=0.0, mask=False):
    mcfg = _mcfg()
    img = mcfg.vit[0].img
    d = make_tables(lengths=lengths, prompt_lens=prompts, n_img=1, hw=4, A=mcfg.action_dim, Pd=mcfg.proprio_dim, seed=seed, dataset_name=name)
    d["frames_u8"] = torch.randint(0, 256, (sum(lengths), 1, img, img, 3), generator=torch.Generator().manual_seed(seed + 3), dtype=torch.uint8)
    d["prompt_flat"] = d["prompt_flat"] % 700
    d["actions_raw"] = d["actions_raw"] * scale + shift
    if mask:
        d["action_mask"] = torch.tensor([True] * (mcfg.action_dim - 1) + [False])
    return d


TINY_PROMPTS = (10, 0, 27, 5, 24, 7, 12)


def _tables_a():
    return _tiny_tables(LENGTHS, TINY_PROMPTS, "suite_a", 0)


def _tables_b():
    return _tiny_tables(LENGTHS_B, (4, 9, 1, 2, 8), "suite_b", 1, scale=0.5, shift=1.0, mask=True)


def _cfg(B=4, stride=1, graph="false", phase="Training", extra=()):
    from vla_adapter_amd import finetune as F
    return F.parse_args(["--tiny", "true", "--backbone", "tiny", "--batch_size", str(B), "--use_proprio", "True", "--use_fz", "True", "--max_seq_len", str(L),
                         "--seed", "5", "--phase", phase, "--use_graph", graph, "--episode_file", "unused", "--use_val_set", "True",
                         "--val_episode_fraction", str(FRACTION), "--val_window_stride", str(stride), *extra])


class Rig:
    """One tiny engine (random weights) and what a stand-alone HeldOutSweep needs beside it."""

    def __init__(self, graph=False):
        from vla_adapter_amd import engine as E, synthetic as S
        from vla_adapter_amd.input_stage import GPUInputStage, backbone_norms
        self.mcfg, self.graph = _mcfg(), graph
        self.eng = E.VLAEngine(self.mcfg, S.make_weights(self.mcfg, DEV, seed=0), DEV)
        self.stage = GPUInputStage(DEV, backbones=backbone_norms(self.mcfg), image_size=self.mcfg.vit[0].img)
        self.captured = False

    def collate(self, raw, stats, j, seed=5, index=None):
        dv = lambda t: t.to(DEV)
        return self.stage.collate(dv(raw["frames_u8"]), (dv(raw["prompt_flat"]), dv(raw["prompt_off"])), dv(raw["actions_raw"]), dv(raw["proprio_raw"]),
                                  action_stats=stats[0], proprio_stats=stats[1], L=L, seed=(seed ^ HO.HELDOUT_STREAM), rank=0, step=j, augment=None,
                                  stats_index=index)

    def sweeper(self, store, cfg, norm_stats=None):
        st = norm_stats or store.statistics()
        first = next(iter(st.values()))
        static = self.collate(store.sample(cfg.batch_size, 5, 0, 1, 0), (first["action"], first["proprio"]), 0)
        if self.graph and not self.captured:      # as finetune() does: the training step is captured before the first sweep
            noise = torch.zeros(self.mcfg.chunk, self.mcfg.action_dim * self.mcfg.llm.d, device=DEV, dtype=torch.bfloat16)
            self.eng.capture({k: v.clone() for k, v in static.items()}, noise, conservative_rows=True)
            self.captured = True
        return HO.HeldOutSweep(cfg, self.mcfg, DEV, 0, 1, self.eng, store, st, static, L, self.graph)


# ---------------------------------------------------------------------------------------------------------------- 3: a full sweep
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_a_full_sweep_equals_the_existing_validation_forward(graph):
    """B = 4 on the issue's split: its 8 held-out windows fill two whole batches.  The test gathers the same windows by torch indexing,
    collates them with the sweep's seed word and runs model.val_forward with the same noise; vla_l1_loss sums the same non-negative
    f32 terms in f32 (n - 1 additions and one division: relative error below (n + 2) 2^-24 with n = B C A terms, whatever the order),
    the sweep in f64.  Then stride 3: one batch with 3 valid rows and one padded row - the result is the numpy mean over the 3 valid
    windows, not the padded batch's mean."""
    from vla_adapter_amd import finetune as F
    rig = Rig(graph)
    tables = _tables_a()
    store = EP.EpisodeStore.from_dict(tables, DEV, chunk=CHUNK, holdout=FRACTION)
    assert store.Nv == 8 and store.N == 16
    st = store.statistics()["suite_a"]
    cfg = _cfg(graph="true" if graph else "false")
    got = rig.sweeper(store, cfg).sweep(6)
    assert set(got) == ENTRY_KEYS and got["val_batches_count"] == 2 and got["val_samples_count"] == 8 == got["val_windows_total"] and got["step"] == 6
    eng, val = rig.eng, store.val_off_host.tolist()
    eng.begin_validation()
    vals = []
    for j in range(2):
        w = HO.sweep_windows(val, None, 4, 0, 1, j, 1)
        b = rig.collate(indexed_batch(tables, [(e, t) for _, _, e, t in w]), (st["action"], st["proprio"]), j)
        vals.append(eng.val_forward(b, F.validation_noise(cfg, rig.mcfg, 0, 6, j).to(DEV)).tolist())
    eng.end_validation()
    want = [sum(v[k] for v in vals) / 2 for k in range(3)]
    B, C, A = 4, rig.mcfg.chunk, rig.mcfg.action_dim
    bound = (B * C * A + 2) * 2.0 ** -24
    for k, name in enumerate(("loss_value", "curr_action_l1_loss", "next_actions_l1_loss")):
        print(name, got[name], want[k], abs(got[name] - want[k]) / want[k], "bound", bound)
        assert abs(got[name] - want[k]) <= bound * abs(want[k]), (name, got[name], want[k])
    assert got["loss"] == got["loss_value"] and len({v[0] for v in vals}) == 2
    assert math.isclose(sum(got["l1_by_chunk_step"]) / C, got["loss_value"], rel_tol=1e-12) and got["l1_by_chunk_step"][0] == got["curr_action_l1_loss"]
    assert math.isclose(sum(got["l1_by_action_dim"]) / A, got["loss_value"], rel_tol=1e-12)
    assert set(got["per_dataset"]) == {"suite_a"} and set(got["per_dataset"]["suite_a"]) == DATASET_KEYS
    # a partly filled batch: windows 0, 3, 6 and one padded row
    rig2 = Rig(True) if graph else rig        # the captured validation graphs hold the first sweeper's static batch: one sweeper per model
    part = rig2.sweeper(store, _cfg(stride=3, graph="true" if graph else "false")).sweep(6)
    w = HO.sweep_windows(val, None, 4, 0, 1, 0, 3)
    assert [ok for ok, _, _, _ in w] == [1, 1, 1, 0] and part["val_samples_count"] == 3 and part["val_batches_count"] == 1 and part["val_windows_total"] == 8
    b = rig.collate(indexed_batch(tables, [(e, t) for _, _, e, t in w]), (st["action"], st["proprio"]), 0)
    eng.begin_validation()
    padded = eng.val_forward(b, F.validation_noise(cfg, rig.mcfg, 0, 6, 0).to(DEV)).tolist()
    err = (eng.val_pred.float() - eng._to_bf16(b["actions"]).float()).abs().cpu().numpy().astype(np.float64)
    eng.end_validation()
    for name, m in (("loss_value", err[:3].mean()), ("curr_action_l1_loss", err[:3, 0].mean()), ("next_actions_l1_loss", err[:3, 1:].mean())):
        assert abs(part[name] - m) <= (1e-12 if not graph else bound) * m, (name, part[name], m)
    assert abs(err.mean() - padded[0]) <= bound * padded[0] and abs(part["loss_value"] - padded[0]) > 1e-4 * padded[0], "the padded row would have moved the mean"


# ---------------------------------------------------------------------------------------------------------------- 4: finetune()
def _ft_args(tmp, graph, mode, extra):
    """(--conservative_rows: the prompts of the training episodes differ in length, so the action block moves from batch to batch.)"""
    modes = {"adapter": ["--use_fz", "True"], "lora": ["--use_lora", "True", "--lora_rank", "8"]}
    return (["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "4", "--learning_rate", "1e-3", "--wandb_log_freq", "1",
             "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_graph", graph, "--max_seq_len", str(L), "--seed", "5",
             "--run_root_dir", str(tmp), "--run_id_override", "r", "--conservative_rows", "true"] + modes[mode] + list(extra))


@pytest.mark.parametrize("mode, graph", [("adapter", "true"), ("adapter", "false"), ("lora", "true")])
def test_sweeps_and_held_out_episodes_leave_training_as_it_is(tmp_path, mode, graph):
    """--episode_file --use_val_set True --val_episode_fraction 0.4 --val_freq 2 against (b) the same run with --val_freq beyond
    max_steps - the sweeps disturb neither the training buffers nor any random stream - and (c) a run without validation on a file
    that holds the four training episodes only, with the full store's statistics: the held-out episodes are never trained on.
    Per-step losses and every tensor of the final checkpoint are bit-identical."""
    from tests.test_validation_gpu import _ckpt
    from vla_adapter_amd import finetune as F
    d = _tables_a()
    torch.save(d, tmp_path / "episodes.pt")
    full = EP.EpisodeStore.from_dict(d, "cpu", chunk=CHUNK, holdout=FRACTION)
    (tmp_path / "stats.json").write_text(json.dumps(full.statistics()))
    n_ep, rows, ids = 4, int(d["episode_off"][4]), int(d["prompt_off"][4])
    train_only = dict(d, frames_u8=d["frames_u8"][:rows], actions_raw=d["actions_raw"][:rows], proprio_raw=d["proprio_raw"][:rows],
                      episode_off=d["episode_off"][:n_ep + 1], prompt_flat=d["prompt_flat"][:ids], prompt_off=d["prompt_off"][:n_ep + 1])
    torch.save({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in train_only.items()}, tmp_path / "train_only.pt")
    held = ["--episode_file", str(tmp_path / "episodes.pt"), "--use_val_set", "True", "--val_episode_fraction", str(FRACTION)]
    a = F.finetune(F.parse_args(_ft_args(tmp_path / "a", graph, mode, held + ["--val_freq", "2"])))
    b = F.finetune(F.parse_args(_ft_args(tmp_path / "b", graph, mode, held + ["--val_freq", "1000"])))
    c = F.finetune(F.parse_args(_ft_args(tmp_path / "c", graph, mode, ["--episode_file", str(tmp_path / "train_only.pt"), "--dataset_statistics_file",
                                                                      str(tmp_path / "stats.json")])))
    assert len(a["log"]) == 5 and a["log"] == b["log"] == c["log"] and b["val_log"] == [] == c["val_log"]
    assert len({l["loss_value"] for l in a["log"]}) == 5
    ca, cb, cc = (_ckpt(str(tmp_path / x / "r--4_chkpt")) for x in "abc")
    assert set(ca) == set(cb) == set(cc)
    assert all(torch.equal(ca[k], cb[k]) and torch.equal(ca[k], cc[k]) for k in ca), [k for k in ca if not (torch.equal(ca[k], cb[k]) and torch.equal(ca[k], cc[k]))][:5]
    assert [v["step"] for v in a["val_log"]] == [2, 4]
    for v in a["val_log"]:
        assert set(v) == ENTRY_KEYS and set(v["per_dataset"]["suite_a"]) == DATASET_KEYS
        assert v["val_samples_count"] == math.ceil(full.Nv / 1) == 8 and v["val_windows_total"] == 8 and v["val_batches_count"] == 2
        assert all(x == x and 0 < x < float("inf") for x in [v["loss_value"], v["curr_action_l1_loss"], v["next_actions_l1_loss"]] + v["l1_by_chunk_step"] + v["l1_by_action_dim"])
        assert len(v["l1_by_chunk_step"]) == CHUNK and len(v["l1_by_action_dim"]) == 7 and json.loads(json.dumps(v)) == v
    assert a["val_log"][0]["loss_value"] != a["val_log"][1]["loss_value"], "the model moved between the sweeps"
    assert a["heldout"]["datasets"] == full.heldout and a["heldout"]["fraction"] == FRACTION and a["heldout"]["stride"] == 1 and "heldout" not in c
    saved = json.load(open(next((tmp_path / "a").rglob("dataset_statistics.json"))))
    assert saved == full.statistics() and saved["suite_a"]["num_trajectories"] == 7, "the statistics stay over all episodes"


# ---------------------------------------------------------------------------------------------------------------- 5: a mixture
def test_a_mix_reports_every_dataset_as_if_it_were_swept_alone(tmp_path):
    """Phase Inference (no input perturbation: a row's prediction depends on its window alone).  The mix's sweep visits suite_a's 8 and
    suite_b's 2 held-out windows; every dataset's line equals, bit for bit, the sweep of a store of that dataset alone with its own
    statistics - the acc rows are independent sums -, and the overall line is their count-weighted combination.  Then finetune() with
    --episode_mix reports both names."""
    from vla_adapter_amd import finetune as F
    rig = Rig(False)
    ta, tb = _tables_a(), _tables_b()
    mix = MX.EpisodeMix.from_dicts([(ta, 1.0), (tb, 1.0)], DEV, chunk=CHUNK, holdout=FRACTION)
    assert mix.Nv == 10 and mix.heldout["suite_b"]["heldout_windows"] == 2
    cfg = _cfg(phase="Inference")
    got = rig.sweeper(mix, cfg).sweep(3)
    assert list(got["per_dataset"]) == ["suite_a", "suite_b"] and got["val_samples_count"] == 10 and got["val_batches_count"] == 3
    for t, name in ((ta, "suite_a"), (tb, "suite_b")):
        alone = rig.sweeper(EP.EpisodeStore.from_dict(t, DEV, chunk=CHUNK, holdout=FRACTION), cfg).sweep(3)
        assert got["per_dataset"][name] == alone["per_dataset"][name], name
        for k in DATASET_KEYS - {"l1_by_action_dim_raw"}:
            assert got["per_dataset"][name][k] == alone[k], (name, k)
    a, b = got["per_dataset"]["suite_a"], got["per_dataset"]["suite_b"]
    assert (a["val_samples_count"], b["val_samples_count"]) == (8, 2)
    for k in ("loss_value", "curr_action_l1_loss", "next_actions_l1_loss"):
        assert math.isclose(got[k], (8 * a[k] + 2 * b[k]) / 10, rel_tol=1e-14), k
    assert b["l1_by_action_dim_raw"][-1] == b["l1_by_action_dim"][-1] and b["l1_by_action_dim_raw"][0] != b["l1_by_action_dim"][0], "suite_b's mask leaves its last column raw"
    paths = []
    for t, name in ((ta, "suite_a"), (tb, "suite_b")):
        torch.save(t, tmp_path / f"{name}.pt")
        paths.append(str(tmp_path / f"{name}.pt"))
    out = F.finetune(F.parse_args(_ft_args(tmp_path / "m", "true", "adapter", ["--episode_mix", ",".join(paths), "--use_val_set", "True", "--val_episode_fraction",
                                                                                str(FRACTION), "--val_freq", "2", "--max_steps", "2"])))
    (v,) = out["val_log"]
    assert list(v["per_dataset"]) == ["suite_a", "suite_b"] and v["val_samples_count"] == 10 and set(out["heldout"]["datasets"]) == {"suite_a", "suite_b"}
    pa, pb = v["per_dataset"]["suite_a"], v["per_dataset"]["suite_b"]
    assert math.isclose(v["loss_value"], (8 * pa["loss_value"] + 2 * pb["loss_value"]) / 10, rel_tol=1e-14)
    assert out["mixture"]["windows"] == [16, 4]


# ---------------------------------------------------------------------------------------------------------------- 6: the time limit
def test_time_limit_zero_ends_the_sweep_at_the_first_host_wait():
    rig = Rig(False)
    store = EP.EpisodeStore.from_dict(_tiny_tables(LONG, (3, 9, 4), "long", 4), DEV, chunk=CHUNK, holdout=0.67)
    assert store.Nv == 246
    sw = rig.sweeper(store, _cfg(extra=["--val_time_limit", "0"]))
    assert sw.n_batches == 62
    got = sw.sweep(1)
    assert got["val_batches_count"] == HO.SYNC_EVERY == 8 and got["val_samples_count"] == 32 and got["val_windows_total"] == 246
    assert got["loss_value"] > 0


# ---------------------------------------------------------------------------------------------------------------- 7: two ranks
def test_two_ranks_share_one_sweep(tmp_path):
    """Two gloo ranks on one GPU (tools/heldout_two_ranks.py) at learning rate 0 - the model stays the seeded one on any number of
    ranks -: rank 0 runs global batch 0, rank 1 global batch 1, one all-reduce merges the sums.  Both report the same entry, which
    equals the one-rank sweep's up to the order of a handful of f64 additions."""
    from vla_adapter_amd import finetune as F
    torch.save(_tables_a(), tmp_path / "episodes.pt")
    args = [a for a in _ft_args(tmp_path / "one", "true", "adapter", ["--episode_file", str(tmp_path / "episodes.pt"), "--use_val_set", "True",
                                                                        "--val_episode_fraction", str(FRACTION), "--val_freq", "2", "--max_steps", "2"])]
    args[args.index("--learning_rate") + 1] = "0"
    one = F.finetune(F.parse_args(args))
    (want,) = one["val_log"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VLA_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    i = args.index("--run_root_dir")
    rest = args[:i] + args[i + 2:]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join("tools", "heldout_two_ranks.py"), str(tmp_path)] + rest,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("heldout-two-ranks-ok") == 2, r.stdout[-3000:]
    logs = [json.load(open(tmp_path / f"rank{k}.json")) for k in range(2)]
    assert logs[0]["world"] == 2 and logs[0]["val_log"] == logs[1]["val_log"] and logs[0]["heldout"]["batches_per_rank"] == 1 == logs[1]["heldout"]["batches_per_rank"]
    (got,) = logs[0]["val_log"]
    assert got["val_samples_count"] == want["val_samples_count"] == 8 and got["val_batches_count"] == 2 and set(got) == ENTRY_KEYS

    def close(x, y):
        if isinstance(x, list):
            return all(close(p, q) for p, q in zip(x, y))
        return abs(x - y) <= 1e-12 * abs(y)
    for k in ("loss_value", "loss", "curr_action_l1_loss", "next_actions_l1_loss", "l1_by_chunk_step", "l1_by_action_dim"):
        assert close(got[k], want[k]) and close(got["per_dataset"]["suite_a"][k], want["per_dataset"]["suite_a"][k]), k


# ---------------------------------------------------------------------------------------------------------------- 8: no host work
def test_a_second_sweep_takes_no_device_memory_and_never_synchronises():
    """After the first sweep, with the method of test_sample_allocates_nothing_and_never_synchronises_after_the_first_call: under
    torch's sync debug mode "error" the whole second sweep up to its read-back (two batches: no 8-batch event falls due) raises on any
    synchronising call.  The sweep's own kernels - naming the windows, the gather, the accumulation - into its own buffers take not
    one block from the allocator; the collator and the forward take theirs from torch's caching allocator exactly as in a training
    step, so for the whole sweep the check is that no device memory is reserved."""
    from vla_adapter_amd import ops
    rig = Rig(True)
    store = EP.EpisodeStore.from_dict(_tables_a(), DEV, chunk=CHUNK, holdout=FRACTION)
    sw = rig.sweeper(store, _cfg(graph="true"))
    first = sw.sweep(2)
    ptrs = {k: v.data_ptr() for k, v in sw.draw(0).items()}
    pred, tgt = _bf16(4, CHUNK, 7, seed=1).to(DEV), _bf16(4, CHUNK, 7, seed=2).to(DEV)
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
        again = sw.draw(1)
        ops.heldout_l1_accumulate(pred, tgt, None, again["valid"], sw.acc, sw.cnt)
        after = torch.cuda.memory_stats()["allocation.all.allocated"]
        reserved = torch.cuda.memory_stats()["reserved_bytes.all.allocated"]
        n = sw.launch(2)                               # a read-back or a synchronising call inside raises here
        reserved_after = torch.cuda.memory_stats()["reserved_bytes.all.allocated"]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        print("torch.cuda.set_sync_debug_mode is not honoured by this build: the no-sync check did not run")
    assert after == before, "the sweep's own kernels allocated device memory"
    assert {k: v.data_ptr() for k, v in again.items()} == ptrs
    assert reserved_after == reserved, "the second sweep reserved device memory"
    assert n == 2 and sw.finish(2) == first, "and it repeats the first sweep's entry"
