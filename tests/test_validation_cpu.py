"""CPU checks of the validation pass's host side (--use_val_set): flag handling and when a sweep is due."""
import pytest
import torch

from vla_adapter_amd import engine as E, finetune as F

BASE = ["--use_proprio", "True"]


def _check(argv, **kw):
    cfg = F.parse_args(BASE + argv)
    F.check_supported(cfg, cfg._explicit, **kw)
    return cfg


def test_use_val_set_with_a_source_is_accepted():
    _check(["--use_val_set", "True", "--val_batch_file", "val/"])
    _check(["--use_val_set", "True", "--val_batch_file", "val/", "--val_freq", "5", "--val_time_limit", "30"])
    _check(["--use_val_set", "True", "--val_freq", "5"], val_batches=True)                  # finetune(val_batches=...)
    _check(["--use_val_set", "True", "--val_batch_file", "val/", "--use_lora", "True", "--lora_dropout", "0.1"])


def test_use_val_set_without_a_source_names_the_flag():
    for kw in (dict(), dict(frame_batches=True)):
        with pytest.raises(NotImplementedError, match="--val_batch_file"):
            _check(["--use_val_set", "True"], **kw)


def test_use_val_set_with_token_ce_is_refused():
    with pytest.raises(NotImplementedError, match="token_ce"):
        _check(["--use_val_set", "True", "--val_batch_file", "val/", "--use_lora", "True", "--objective", "token_ce"])


def test_val_flags_without_use_val_set_stay_refused():
    for argv in (["--val_freq", "5"], ["--val_time_limit", "3"], ["--val_freq", "5", "--val_batch_file", "val/"]):
        with pytest.raises((NotImplementedError, ValueError)):
            _check(argv)
    with pytest.raises(ValueError, match="use_val_set"):            # a source alone would be inert
        _check(["--val_batch_file", "val/"])
    with pytest.raises(ValueError, match="use_val_set"):
        _check([], val_batches=True)
    with pytest.raises(ValueError, match="val_freq"):
        _check(["--use_val_set", "True", "--val_batch_file", "val/", "--val_freq", "0"])


def _due(**kw):
    cfg = F.FinetuneConfig(use_val_set=True, **kw)
    return [(it[0], it[2]) for it in F.loop_plan(cfg) if F.validation_due(cfg, it)]


def test_validation_due_fresh_start():
    """finetune.py:1101: log_step > 0 and log_step % val_freq == 0, behind the optimizer step of that gradient step."""
    assert _due(max_steps=10, val_freq=3) == [(3, 3), (6, 6), (9, 9)]
    assert _due(max_steps=10, val_freq=5) == [(5, 5), (10, 10)]          # the last step of the run when max_steps % val_freq == 0
    assert not any(F.validation_due(F.FinetuneConfig(max_steps=10, val_freq=5), it) for it in F.loop_plan(F.FinetuneConfig(max_steps=10)))


def test_validation_due_after_resume():
    """log_step includes resume_step; unlike the checkpoint (gradient_step_idx > 0) the sweep only needs log_step > 0."""
    assert _due(max_steps=110, val_freq=5, resume=True, resume_step=100) == [(0, 100), (5, 105), (10, 110)]
    assert _due(max_steps=7, val_freq=2, resume=True, resume_step=3) == [(1, 4), (3, 6)]


def test_validation_due_once_per_gradient_step_under_accumulation():
    """The reference re-validates on every micro-batch of a due gradient step; here once, behind the optimizer step that completes
    it - and behind the run's last micro-batch, the first of gradient step max_steps (the reference breaks before its update)."""
    cfg = F.FinetuneConfig(use_val_set=True, max_steps=6, val_freq=3, grad_accumulation_steps=2, save_freq=3)
    plan = list(F.loop_plan(cfg))
    due = [it for it in plan if F.validation_due(cfg, it)]
    assert [(it[0], it[2]) for it in due] == [(7, 3), (12, 6)]
    assert due[0][3] and due[0][4]                                  # behind the optimizer step and the checkpoint of step 3
    assert due[1][5] and not due[1][3]                              # the last micro-batch: no optimizer step there
    assert [(b, s) for b, s in _due(max_steps=5, val_freq=2, grad_accumulation_steps=3)] == [(8, 2), (14, 4)]


def test_loop_plan_items_are_unchanged():
    for kw in (dict(max_steps=6, save_freq=3, grad_accumulation_steps=2), dict(max_steps=4, resume=True, resume_step=2)):
        a = list(F.loop_plan(F.FinetuneConfig(**kw)))
        b = list(F.loop_plan(F.FinetuneConfig(use_val_set=True, val_freq=1, **kw)))
        assert a == b and all(len(x) == 6 for x in a)


def test_validation_noise_is_keyed_and_leaves_the_global_generator_alone():
    cfg, mcfg = F.FinetuneConfig(seed=3), E.tiny_config()
    state = torch.random.get_rng_state()
    a = F.validation_noise(cfg, mcfg, 0, 10, 0)
    assert torch.equal(torch.random.get_rng_state(), state)
    assert a.dtype == torch.bfloat16 and tuple(a.shape) == (mcfg.chunk, mcfg.action_dim * mcfg.llm.d)
    assert torch.equal(a, F.validation_noise(cfg, mcfg, 0, 10, 0))
    for other in (F.validation_noise(cfg, mcfg, 1, 10, 0), F.validation_noise(cfg, mcfg, 0, 11, 0), F.validation_noise(cfg, mcfg, 0, 10, 1),
                  F.validation_noise(F.FinetuneConfig(seed=4), mcfg, 0, 10, 0)):
        assert not torch.equal(a, other)
    assert abs(a.float().std().item() - 0.02) < 2e-3
