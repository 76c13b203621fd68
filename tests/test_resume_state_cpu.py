"""CPU checks of --save_train_state / --resume_train_state / --log_state_digest (vla_adapter_amd/train_state.py):
the flags and their defaults, every refusal with its cause, the resumed loop plan as the tail of the straight one with a continuous
learning rate, the batch stream's position, the fingerprint, the digest limbs, and the state file's round trip."""
import dataclasses
import json

import pytest
import torch

from vla_adapter_amd import finetune as F
from vla_adapter_amd import train_state as TS


def _cfg(*extra):
    return F.parse_args(["--use_proprio", "True", "--use_fz", "True", *extra])


def _state(cfg, k, ga, **over):
    """The position part of a state written at log step k of a straight run."""
    fp = TS.fingerprint(cfg, F.train_mode(cfg), 1, 1)
    st = dict(version=TS.FORMAT_VERSION, mode=F.train_mode(cfg), log_step=k, next_grad_step=k + 1, next_micro_step=(k + 1) * ga,
              fingerprint=json.dumps(fp, sort_keys=True))
    st.update(over)
    return st, fp


# ---------------------------------------------------------------------------------------------------------------- flags and defaults
def test_the_flags_default_to_off_and_parse():
    cfg = _cfg()
    assert (cfg.save_train_state, cfg.resume_train_state, cfg.log_state_digest) == (False, False, False)
    on = _cfg("--save_train_state", "True", "--resume_train_state", "true", "--log_state_digest", "1")
    assert (on.save_train_state, on.resume_train_state, on.log_state_digest) == (True, True, True)
    for f in dataclasses.fields(F.FinetuneConfig):
        assert getattr(cfg, f.name) == (True if f.name in ("use_proprio", "use_fz") else f.default), f.name
    F.check_supported(cfg, cfg._explicit)
    ok = _cfg("--save_train_state", "True", "--log_state_digest", "True")
    F.check_supported(ok, ok._explicit)


def test_with_the_flags_off_the_plan_is_the_plan():
    """grad accumulation 2, save_freq 2, max_steps 3, fresh and plain --resume: the items as the reference's bookkeeping gives them."""
    cfg = _cfg("--grad_accumulation_steps", "2", "--save_freq", "2", "--max_steps", "3")
    want = [(0, 0, 0, False, False, False), (1, 0, 0, True, False, False), (2, 1, 1, False, False, False), (3, 1, 1, True, False, False),
            (4, 2, 2, False, False, False), (5, 2, 2, True, True, False), (6, 3, 3, False, False, True)]
    assert list(F.loop_plan(cfg)) == list(F.loop_plan(cfg, None)) == want
    res = _cfg("--grad_accumulation_steps", "2", "--save_freq", "2", "--max_steps", "4", "--resume", "True", "--resume_step", "2")
    assert list(F.loop_plan(res)) == [(0, 0, 2, False, False, False), (1, 0, 2, True, False, False), (2, 1, 3, False, False, False),
                                      (3, 1, 3, True, False, False), (4, 2, 4, False, False, True)], "plain --resume starts over at batch 0"
    assert F.lr_at(0, cfg) == cfg.learning_rate * (0.1 + 0.9 * min(1 / 0.1, 1.0))


@pytest.mark.parametrize("warmup", ["0.1", "8", "0"])
@pytest.mark.parametrize("ga", [1, 2])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_the_resumed_plan_is_the_tail_of_the_straight_plan(k, ga, warmup):
    flags = ["--grad_accumulation_steps", str(ga), "--save_freq", "2", "--max_steps", "7", "--lr_warmup_steps", warmup, "--num_steps_before_decay", "4"]
    straight = list(F.loop_plan(_cfg(*flags)))
    res = _cfg(*flags, "--resume", "True", "--resume_step", str(k), "--resume_train_state", "True")
    st, fp = _state(res, k, ga)
    TS.check(st, fp=fp, mode="adapter", resume_step=k)
    start = TS.resumed_position(st)
    assert start == ((k + 1) * ga, 0)
    resumed = list(F.loop_plan(res, start))
    assert resumed == straight[(k + 1) * ga:] and resumed[0][1:3] == (k + 1, k + 1) and resumed[-1][5]
    # lr_at continues: the resumed items' learning rates are the straight run's, and (warm-up of 8 steps) still on the ramp
    assert [F.lr_at(it[1], res) for it in resumed] == [F.lr_at(it[1], _cfg(*flags)) for it in straight[(k + 1) * ga:]]
    if warmup == "8":
        assert F.lr_at(resumed[0][1], res) > F.lr_at(0, res), "no second warm-up"
    if warmup == "0":
        assert [F.lr_at(g, res) / res.learning_rate for g in (3, 4)] == [1.0, 0.1], "the decay step is met at its gradient step"


def test_a_state_written_by_a_plainly_resumed_run_goes_on_from_its_own_counters():
    """A run that did the reference's --resume at step 10 and saved at log step 12 (its gradient step 2): the resumed plan goes on with
    gradient step 3 at log step 13 - its schedule position and its label each continue."""
    cfg = _cfg("--max_steps", "14", "--save_freq", "2", "--resume", "True", "--resume_step", "12", "--resume_train_state", "True")
    st, _ = _state(cfg, 12, 1, next_grad_step=3, next_micro_step=3)
    items = list(F.loop_plan(cfg, TS.resumed_position(st)))
    assert [(b, g, s) for b, g, s, *_ in items] == [(3, 3, 13), (4, 4, 14)] and items[-1][4] and items[-1][5]


# ---------------------------------------------------------------------------------------------------------------- the refusals
def test_resume_train_state_without_resume_is_refused():
    cfg = _cfg("--resume_train_state", "True")
    with pytest.raises(ValueError, match="--resume_train_state without --resume"):
        F.check_supported(cfg, cfg._explicit)
    cfg = _cfg("--resume_train_state", "True", "--resume", "True")
    with pytest.raises(ValueError, match="--resume needs --resume_step"):
        F.check_supported(cfg, cfg._explicit)
    ok = _cfg("--resume_train_state", "True", "--resume", "True", "--resume_step", "3")
    F.check_supported(ok, ok._explicit)


def test_a_directory_without_a_state_file_is_refused(tmp_path):
    with pytest.raises(ValueError, match=r"no state file in .*train_state--3_checkpoint\.pt.*--save_train_state"):
        TS.load(tmp_path, 3)
    torch.save(dict(version=99), tmp_path / "train_state--3_checkpoint.pt")
    with pytest.raises(ValueError, match="format version 99"):
        TS.load(tmp_path, 3)


def test_a_fingerprint_mismatch_names_the_flags():
    cfg = _cfg("--resume", "True", "--resume_step", "3", "--resume_train_state", "True")
    st, fp = _state(cfg, 3, 1)
    TS.check(st, fp=fp, mode="adapter", resume_step=3)
    other = _cfg("--seed", "7", "--batch_size", "16", "--max_grad_norm", "1.0", "--episode_file", "e.pt", "--max_seq_len", "96")
    with pytest.raises(ValueError) as ei:
        TS.check(st, fp=TS.fingerprint(other, "adapter", 2, 1), mode="adapter", resume_step=3)
    msg = str(ei.value)
    for flag in ("seed: recorded 0, now 7", "batch_size: recorded 8, now 16", "max_grad_norm: recorded None, now 1.0", "world_size: recorded 1, now 2",
                 "batch_source: recorded 'synthetic', now 'episode_file'", "batch_source_path", "max_seq_len"):
        assert flag in msg, flag
    assert "learning_rate" not in msg and "lora_rank" not in msg, "only the differing flags"
    with pytest.raises(ValueError, match="mode: recorded 'adapter', now 'lora'"):
        TS.check(st, fp=TS.fingerprint(_cfg("--use_lora", "True"), "lora", 1, 1), mode="lora", resume_step=3)


def test_what_is_not_fingerprinted():
    base = TS.fingerprint(_cfg(), "adapter", 1, 1)
    other = _cfg("--max_steps", "9", "--save_freq", "4", "--val_freq", "3", "--val_time_limit", "7", "--wandb_log_freq", "2", "--log_state_digest", "True",
                 "--run_root_dir", "elsewhere", "--save_train_state", "True", "--resume", "True", "--resume_step", "3", "--resum_vla_path", "x",
                 "--resume_train_state", "True")
    assert TS.fingerprint(other, "adapter", 1, 1) == base
    assert not set(TS.NOT_FINGERPRINTED) & set(base)
    for flag in ("seed", "batch_size", "grad_accumulation_steps", "learning_rate", "lr_warmup_steps", "num_steps_before_decay", "mode", "lora_rank",
                 "lora_dropout", "fp8_base_weights", "objective", "max_grad_norm", "batch_source", "batch_source_path", "max_seq_len", "image_aug",
                 "episode_mix", "episode_mix_balance", "val_episode_fraction", "world_size", "phase", "use_graph", "conservative_rows", "backbone",
                 "num_images_in_input"):
        assert flag in base, flag
    assert json.loads(json.dumps(base)) == base


def test_a_step_mismatch_is_refused():
    cfg = _cfg("--resume", "True", "--resume_step", "4", "--resume_train_state", "True")
    st, fp = _state(cfg, 3, 1)
    with pytest.raises(ValueError, match="records step 3, --resume_step is 4"):
        TS.check(st, fp=fp, mode="adapter", resume_step=4)


def _Owner(spec):
    """The optimizer-state half of schedule.StepControls over a flat buffer on the host."""
    from vla_adapter_amd import engine as E, schedule

    class _Owner(schedule.StepControls):
        def _state_buffers(self):
            return [("head", self.P)]
    o = _Owner()
    o.P, o.step_count = E.FlatParams(spec, "cpu"), 0
    return o


def test_an_offsets_table_mismatch_is_refused():
    a = _Owner([("w", (3, 5)), ("b", (5,))])
    rec = dict(buffers=dict(head=dict(offsets=TS.offsets_hash(a.P), numel=a.P.numel)))
    a._check_tables(rec, a._state_buffers())
    for spec in ([("w", (5, 3)), ("b", (5,))], [("b", (5,)), ("w", (3, 5))], [("w", (3, 5)), ("bias", (5,))], [("w", (3, 5)), ("b", (5,)), ("c", (1,))]):
        b = _Owner(spec)
        with pytest.raises(ValueError, match="offsets-table mismatch in buffer 'head'"):
            b._check_tables(rec, b._state_buffers())
        with pytest.raises(ValueError, match="offsets-table mismatch"):
            b.load_optimizer_state(dict(rec, step_counts={"_Owner": 1}))
    with pytest.raises(ValueError, match=r"offsets-table mismatch - the state holds the buffers \['backbone', 'head'\]"):
        a._check_tables(dict(buffers=dict(rec["buffers"], backbone=rec["buffers"]["head"])), a._state_buffers())
    assert TS.offsets_hash(a.P) == TS.offsets_hash(_Owner([("w", (3, 5)), ("b", (5,))]).P)


# ---------------------------------------------------------------------------------------------------------------- the pieces
def test_digest_limbs_round_trip_through_f32():
    vals = [0, 1, 0xFFFF, 0x10000, 2 ** 63, 2 ** 64 - 1, 0x9E3779B97F4A7C15, 0x0123456789ABCDEF]
    d = torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=torch.int64)
    limbs = TS.limbs_f32(d)
    assert limbs.dtype == torch.float32 and limbs.numel() == 4 * len(vals) and float(limbs.max()) == 65535.0
    assert TS.from_limbs(torch.cat([torch.tensor([0.5, 1.25]), limbs]).tolist()[2:]) == vals
    assert TS.hex64(vals[-1]) == "0x0123456789abcdef" and TS.hex64(-1) == "0xffffffffffffffff"
    bufs = [("head", None), ("backbone", None)]
    assert TS.digest_dict(bufs, range(6)) == {"head": dict(data=TS.hex64(0), m=TS.hex64(1), v=TS.hex64(2)),
                                              "backbone": dict(data=TS.hex64(3), m=TS.hex64(4), v=TS.hex64(5))}


def test_file_names_follow_the_checkpoint_files(tmp_path):
    assert TS.file_name(3) == "train_state--3_checkpoint.pt" and TS.file_name(3, True) == TS.file_name(None) == "train_state--latest_checkpoint.pt"
    st = dict(version=TS.FORMAT_VERSION, mode="adapter", log_step=3, buffers=dict(head=dict(m=torch.ones(4, dtype=torch.bfloat16), numel=4, offsets="ab",
                                                                                          digest=dict(data="0x01", m="0x02", v="0x03"))),
              step_counts={"VLAEngine": 4}, counters={}, generator=torch.arange(16, dtype=torch.uint8), generator_offset=12, row0=-1,
              next_grad_step=4, next_micro_step=4, fingerprint="{}")
    TS.save(st, tmp_path, 3, latest_only=True)
    assert (tmp_path / "train_state--latest_checkpoint.pt").exists()
    back = TS.load(tmp_path, 3)                                    # step-named first, else the latest file
    assert back["step_counts"] == {"VLAEngine": 4} and torch.equal(back["buffers"]["head"]["m"], st["buffers"]["head"]["m"]) and back["row0"] == -1


@pytest.mark.parametrize("start", [0, 3])
def test_the_batch_stream_starts_at_a_position(start, tmp_path):
    """An explicit iterable and a directory of batch files, three batches each, rank 1: the stream from `start` is the stream from 0
    with its first `start` batches dropped."""
    import itertools
    cfg = _cfg()
    mk = lambda i: dict(input_ids=torch.full((1, 4), i), labels=torch.full((1, 4), i), attention_mask=torch.ones(1, 4, dtype=torch.bool))
    items = [mk(i) for i in range(3)]
    take = lambda it, n: [int(b["input_ids"][0, 0]) for b in itertools.islice(it, n)]
    whole = take(F.batch_stream(cfg, None, "cpu", 1, batches=items), 8)
    assert whole == [0, 1, 2, 0, 1, 2, 0, 1]
    assert take(F.batch_stream(cfg, None, "cpu", 1, batches=items, start=start), 5) == whole[start:start + 5]
    for i, b in enumerate(items):
        torch.save(b, tmp_path / f"b{i}.pt")
    fcfg = _cfg("--batch_file", str(tmp_path))
    whole = take(F.batch_stream(fcfg, None, "cpu", 1), 8)
    assert whole == [1, 2, 0, 1, 2, 0, 1, 2], "rank 1 starts at its own offset"
    assert take(F.batch_stream(fcfg, None, "cpu", 1, start=start), 5) == whole[start:start + 5]
