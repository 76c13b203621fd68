"""The fine-tune driver's host pieces on their own, no device: the named log read-back (finetune.LogReadback), the four forms of a
training step against a recording owner (finetune.StepRunner) and the collator's micro-step counter (batches.Collator)."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from vla_adapter_amd import batches as BT, finetune as F

# ---------------------------------------------------------------------------------------------------------------- LogReadback
OPTIONAL = dict(ce=[11.0, 12.0, 13.0, 14.0], jpeg=[21.0], grad_norm=[31.0], digest=[41.0, 42.0, 43.0, 44.0, 45.0, 46.0])
ORDER = ("loss", "ce", "jpeg", "grad_norm", "digest")           # the order the driver adds them in: what crosses the bus


class Counted(torch.Tensor):
    """A tensor that counts every ``tolist`` taken of it or of anything torch makes of it (torch.cat keeps the subclass)."""
    taken = []

    def tolist(self):
        Counted.taken.append(torch.Tensor.tolist(self))
        return Counted.taken[-1]


@pytest.mark.parametrize("present", [c for n in range(5) for c in itertools.combinations(OPTIONAL, n)], ids=lambda c: "+".join(c) or "loss_only")
def test_log_readback_returns_every_part_by_name_from_one_tolist(present, monkeypatch):
    values = dict(loss=[1.0, 2.0, 3.0], **{k: OPTIONAL[k] for k in present})
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda ts, *a, **k: cats.append(len(ts)) or real_cat(ts, *a, **k))
    Counted.taken = []
    rb = F.LogReadback()
    for name in ORDER:
        if name in values:
            rb.add(name, torch.tensor(values[name]).as_subclass(Counted))
    got = rb.read()
    assert got == values and list(got) == [n for n in ORDER if n in values]
    assert Counted.taken == [[x for n in ORDER if n in values for x in values[n]]]         # one tolist, of the parts in order
    assert cats == ([len(values)] if present else [])                                       # the loss alone: read as it is, no cat


# ---------------------------------------------------------------------------------------------------------------- StepRunner
class Slot:
    """A batch tensor that records what is done with it: ``clone`` gives the static slot of the same key."""

    def __init__(self, calls, name):
        self.calls, self.name = calls, name

    def clone(self):
        return Slot(self.calls, f"static.{self.name}")

    def copy_(self, src):
        self.calls.append(("copy", self.name, src.name))


class Owner:
    """Engine or trainer: every call the runner makes of it, in order."""

    def __init__(self, calls, who):
        self.calls, self.who = calls, who

    def capture(self, static, noise, **kw):
        self.calls.append((f"{self.who}.capture", tuple(static), noise is not None, kw))

    def train_step(self, batch, lr, noise):
        self.calls.append((f"{self.who}.train_step", batch["input_ids"].name, lr, noise is not None))
        return "loss3"

    def train_step_graphed(self, lr):
        self.calls.append((f"{self.who}.train_step_graphed", lr))
        return "loss3"

    def stage_next_pixels(self, px):
        self.calls.append((f"{self.who}.stage_next_pixels", px.name))


KEYS = ("input_ids", "attention_mask", "pixel_values", "labels", "actions", "proprio")
SMALL = tuple(k for k in KEYS if k != "pixel_values")
MCFG = SimpleNamespace(chunk=2, action_dim=3, llm=SimpleNamespace(d=4))


def runner_calls(with_trainer: bool, use_graph: bool, resume_state=None, **kw):
    calls = []
    eng, trainer = Owner(calls, "eng"), Owner(calls, "trainer") if with_trainer else None
    batch = lambda i: {k: Slot(calls, f"b{i}.{k}") for k in KEYS}
    b0, b1, b2 = batch(0), batch(1), batch(2)
    runner = F.StepRunner(eng, trainer, MCFG, "cpu", use_graph, **kw)
    assert runner.owner is (trainer or eng) and runner.noise.shape == (2, 12) and runner.noise.dtype == torch.bfloat16
    runner.capture(b0, resume_state)
    captured = list(calls)
    del calls[:]
    assert runner.step(b0, b1, 0.5) == "loss3" and runner.step(b1, b2, 0.25) == "loss3"
    return captured, calls


def copies(i, keys):
    return [("copy", f"static.b0.{k}", f"b{i}.{k}") for k in keys]


def test_step_runner_engine_captured():
    captured, steps = runner_calls(False, True, conservative_rows=True)
    assert captured == [("eng.capture", KEYS, True, dict(conservative_rows=True, row0=None))]
    assert steps == (copies(0, KEYS) + [("eng.stage_next_pixels", "b1.pixel_values"), ("eng.train_step_graphed", 0.5)]        # step one: every tensor
                     + copies(1, SMALL) + [("eng.stage_next_pixels", "b2.pixel_values"), ("eng.train_step_graphed", 0.25)])   # then the small ones only


def test_step_runner_engine_capture_takes_the_resumed_window_and_the_phase():
    assert runner_calls(False, True, dict(row0=64))[0] == [("eng.capture", KEYS, True, dict(conservative_rows=False, row0=64))]
    assert runner_calls(False, True, dict(row0=-1), training=False)[0] == [("eng.capture", KEYS, False, dict(conservative_rows=False, row0=None))]


def test_step_runner_trainer_captured():
    captured, steps = runner_calls(True, True)
    assert captured == [("trainer.capture", KEYS, True, {})]
    assert steps == copies(0, KEYS) + [("trainer.train_step_graphed", 0.5)] + copies(1, KEYS) + [("trainer.train_step_graphed", 0.25)]


@pytest.mark.parametrize("with_trainer", [False, True])
def test_step_runner_eager(with_trainer):
    who = "trainer" if with_trainer else "eng"
    captured, steps = runner_calls(with_trainer, False)
    assert captured == [] and steps == [(f"{who}.train_step", "b0.input_ids", 0.5, True), (f"{who}.train_step", "b1.input_ids", 0.25, True)]
    assert runner_calls(with_trainer, False, training=False)[1][0] == (f"{who}.train_step", "b0.input_ids", 0.5, False)


# ---------------------------------------------------------------------------------------------------------------- Collator
class StubStage:
    """Stands for GPUInputStage: records the step it is handed and the step of the augmentation built for it."""

    def __init__(self):
        self.seen = []

    def collate(self, frames, prompts, actions, proprio, *, step, augment, **kw):
        self.seen.append(("raw", step, augment.step if augment is not None else None))
        return dict(collated=True)

    def pixels(self, frames, augment=None):
        self.seen.append(("frames", None, augment.step if augment is not None else None))
        return frames


def collator(start, image_aug=True):
    cfg = F.FinetuneConfig(image_aug=image_aug, max_seq_len=16)
    c = BT.Collator(cfg, None, "cpu", 0, (), start)
    c.stage, c.norm_stats = StubStage(), {"toy": dict(action={}, proprio={})}
    return c


RAW = dict(frames_u8=torch.zeros(1, 1, 2, 2, 3, dtype=torch.uint8), prompt_flat=torch.zeros(3, dtype=torch.int64),
           prompt_off=torch.tensor([0, 3], dtype=torch.int32), actions_raw=torch.zeros(1, 8, 7), proprio_raw=torch.zeros(1, 8))
FRAMES = dict(frames_u8=RAW["frames_u8"], input_ids=torch.zeros(1, 4, dtype=torch.int64))
COLLATED = dict(pixel_values=torch.zeros(1, 3, 2, 2), input_ids=torch.zeros(1, 4, dtype=torch.int64))


@pytest.mark.parametrize("start", [0, 5])
def test_collator_hands_batch_i_the_step_start_plus_i(start):
    c = collator(start)
    for _ in range(3):
        c(dict(RAW))
    assert c.stage.seen == [("raw", start + i, start + i) for i in range(3)] and c.step == start + 3
    c = collator(start)
    for _ in range(3):
        assert "pixel_values" in c(dict(FRAMES))
    assert c.stage.seen == [("frames", None, start + i) for i in range(3)] and c.step == start + 3
    c = collator(start, image_aug=False)                # no augmentation: the counter still runs (the collator's filler ids are keyed by it)
    c(dict(RAW)), c(dict(FRAMES)), c(dict(RAW))
    assert c.stage.seen == [("raw", start, None), ("frames", None, None), ("raw", start + 2, None)]


@pytest.mark.parametrize("start", [0, 5])
def test_collator_does_not_count_collated_batches(start):
    c = collator(start)
    assert sorted(c(dict(COLLATED))) == sorted(COLLATED) and c.step == start and c.stage.seen == []
    c(dict(RAW)), c(dict(COLLATED)), c(dict(COLLATED)), c(dict(FRAMES))
    assert c.stage.seen == [("raw", start, start), ("frames", None, start + 1)] and c.step == start + 2


def test_batch_stats_picks_one_entry_bare_or_one_per_name():
    st = dict(a=dict(action=1, proprio=2), b=dict(action=3, proprio=4))
    assert BT.batch_stats(st, ("b",), False) == (3, 4) and BT.batch_stats(st, ("b", "a"), True) == ((3, 1), (4, 2))
    assert BT.batch_stats(dict(a=st["a"]), (None,), False) == (1, 2)
    with pytest.raises(KeyError, match="hold no entry 'c'"):
        BT.batch_stats(st, ("a", "c"), True)


def test_finetune_still_names_what_moved_out_of_it():
    from vla_adapter_amd import validation as V
    for name in ("RAW_BATCH_KEYS", "raw_batch_stats", "mixture_stats", "batch_stream", "pad_to"):
        assert getattr(F, name) is getattr(BT, name)
    for name in ("validation_due", "validation_noise", "ValidationPass"):
        assert getattr(F, name) is getattr(V, name)
    assert F._pad_to is BT.pad_to                   # the earlier name of pad_to
