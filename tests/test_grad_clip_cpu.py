"""--max_grad_norm without a GPU: the config field and flag, refusal of bad values, the host-arithmetic slot count of the
sum-of-squares pass, and the new exports in header and binding."""
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("vla_grad_sumsq_slots", "vla_grad_sumsq", "vla_grad_norm_finalise", "vla_adamw_clipped_bf16")
BASE = ["--tiny", "true", "--use_proprio", "True"]


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def test_config_field_and_flag():
    import dataclasses
    from vla_adapter_amd import finetune as F
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["max_grad_norm"]
    assert f.default is None, "clipping is off unless asked for"
    assert F.parse_args(BASE).max_grad_norm is None
    cfg = F.parse_args(BASE + ["--max_grad_norm", "1.0"])
    assert cfg.max_grad_norm == 1.0 and isinstance(cfg.max_grad_norm, float)
    F.check_supported(cfg, cfg._explicit)


@pytest.mark.parametrize("bad", ["0", "-1.0", "nan", "-inf"])
def test_bad_values_raise(bad):
    from vla_adapter_amd import finetune as F, schedule
    cfg = F.parse_args(BASE + [f"--max_grad_norm={bad}"])      # ("=": argparse takes a bare -inf for a flag)
    with pytest.raises(ValueError, match="max_grad_norm"):
        F.check_supported(cfg, cfg._explicit)
    with pytest.raises(ValueError, match="max_grad_norm"):
        schedule.check_max_grad_norm(float(bad))


def test_inf_is_accepted():
    from vla_adapter_amd import finetune as F, schedule
    cfg = F.parse_args(BASE + ["--max_grad_norm", "inf"])
    assert math.isinf(cfg.max_grad_norm) and cfg.max_grad_norm > 0
    F.check_supported(cfg, cfg._explicit)
    assert schedule.check_max_grad_norm(float("inf")) == float("inf") and schedule.check_max_grad_norm(None) is None


def test_slot_count_is_monotone_host_arithmetic(lib, monkeypatch):
    """The slot count of a slice is a function of its length alone: non-decreasing, one slot from the first element on, never more
    than one slot per element, the same under any device-visibility setting (it never asks for the CU count), and it covers
    lengths past 2^31."""
    from vla_adapter_amd import ops
    ns = [1, 7, 8, 9, 255, 256, 4096, 4097, 16383, 16384, 16385, 65536 + 3, (1 << 20) + 5, 1 << 24, 600_000_000, (1 << 31) + 11, 1 << 40]
    got = [ops.grad_sumsq_slots(n) for n in ns]
    assert ops.grad_sumsq_slots(0) == 0 and got[0] == 1
    assert all(a <= b for a, b in zip(got, got[1:])), got
    assert all(1 <= k <= n for k, n in zip(got, ns))
    assert got[-1] > got[-2] > got[-3], "long slices keep getting more slots (64-bit arithmetic)"
    dense = [ops.grad_sumsq_slots(n) for n in range(1, 40000)]
    assert all(0 <= b - a <= 1 for a, b in zip(dense, dense[1:]))
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("VLA_TRAINER_STREAMS", "1")
    assert [ops.grad_sumsq_slots(n) for n in ns] == got


def test_new_symbols_in_header_binding_and_library(lib):
    from vla_adapter_amd import native
    txt = open(os.path.join(ROOT, "include", "vla_native.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), f"{name} is not declared in vla_native.h"
        assert name in native.family("native").protos and hasattr(lib, name)
    assert int(re.search(r"#define VLA_ABI_VERSION (\d+)", txt).group(1)) == native.ABI_VERSION == 8, "added without a version change"
    assert "vla_adamw_clipped_bf16" in re.search(r"Added since without a version change.*?\*/", txt, flags=re.S).group(0)


def test_argument_validation_without_gpu(lib):
    """Bad arguments are refused on the host, before any launch."""
    assert lib.vla_grad_sumsq(None, None, 8, 0, 1.0, None) == -1
    assert lib.vla_grad_sumsq(None, 4096, 0, 0, 1.0, 4096) == -1
    assert lib.vla_grad_sumsq(None, 4097, 8, 0, 1.0, 4096) == -1 and b"misaligned" in lib.vla_last_error()
    assert lib.vla_grad_norm_finalise(None, 4096, 0, 1.0, 4096) == -1
    assert lib.vla_grad_norm_finalise(None, 4096, 4, 0.0, 4096) == -1
    assert lib.vla_grad_norm_finalise(None, 4096, 4, float("nan"), 4096) == -1
    assert lib.vla_adamw_clipped_bf16(None, 4096, 4096, 4096, 4096, 8, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0, 1.0, None) == -1
    assert b"coefficient" in lib.vla_last_error()


def test_shared_step_controls_on_cpu_tensors():
    """schedule.StepControls - the accumulation and clipping members VLAEngine and BackboneTrainer share - driven by a bare owner
    with CPU gradient buffers, as far as it goes without the native library: ga reset and fold boundary, the handling of
    None / inf / <= 0 / NaN by set_max_grad_norm, the properties reading None while clipping is off, the "before capture()"
    assertion, and the owner's _set_clip hook seeing every new clip object and every drop."""
    import torch
    from vla_adapter_amd import schedule

    class Owner(schedule.StepControls):
        def __init__(self):
            self._graphs, self.seen = None, []
            self.bufs = [torch.zeros(8), torch.zeros(4)]
            self._init_step_controls(lambda dst, src: dst.copy_(src), lambda dst, src: dst.add_(src))

        def _grad_buffers(self):
            return self.bufs

        def _set_clip(self, clip):
            self.seen.append(clip)
            self._clip = clip

    o = Owner()
    assert o.ga == 1 and o._accum.fold() and o.max_grad_norm is None and o.grad_norm is None and o.clip_coef is None
    # accumulation: three micro-steps, the buffers hold the sums on the boundary; a reset starts a new window
    o.set_grad_accumulation(3)
    assert o.ga == 3
    boundary = []
    for k in (1.0, 2.0, 4.0, 8.0, 16.0, 32.0):
        for b in o.bufs:
            b.fill_(k)
        boundary.append(o._accum.fold())
        if boundary[-1]:
            assert all(bool((b == (7.0 if k == 4.0 else 56.0)).all()) for b in o.bufs), (k, o.bufs)
    assert boundary == [False, False, True, False, False, True]
    o._accum.fold()                                  # (one micro-step into a window ...)
    o.set_grad_accumulation(2)                       # (... that the reset drops)
    assert o.ga == 2 and [o._accum.fold(), o._accum.fold()] == [False, True]
    o.set_grad_accumulation(1)
    assert o.ga == 1 and o._accum.fold() and not o._accum._pairs
    with pytest.raises(AssertionError):
        o.set_grad_accumulation(0)
    # clipping: a clip object over the owner's buffers per valid setting, dropped by None, bad values refused and nothing changed
    o.set_max_grad_norm(1.0)
    clip = o._clip
    assert isinstance(clip, schedule.GradClip) and o.seen == [clip] and clip.bufs[0] is o.bufs[0] and clip.bufs[1] is o.bufs[1]
    assert o.max_grad_norm == 1.0 and o.grad_norm.shape == () and o.clip_coef.shape == (1,)
    assert o.grad_norm.dtype == o.clip_coef.dtype == torch.float32 and o.clip_coef.data_ptr() == clip.out[1:].data_ptr()
    for bad in (0, 0.0, -1.0, float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            o.set_max_grad_norm(bad)
    assert o._clip is clip and o.seen == [clip], "a refused value leaves the setting alone and never reaches the owner"
    o.set_max_grad_norm(float("inf"))
    assert math.isinf(o.max_grad_norm) and o._clip is not clip and o.grad_norm is not None
    o.set_max_grad_norm(None)
    assert o.seen[-1] is None and len(o.seen) == 3
    assert o.max_grad_norm is None and o.grad_norm is None and o.clip_coef is None
    o._graphs = [object()]                           # captured: the accumulation factor is baked into the loss kernel
    with pytest.raises(AssertionError, match=r"before capture\(\)"):
        o.set_grad_accumulation(2)


def test_engine_and_trainer_keep_no_copy_of_the_step_controls():
    """The six members live in schedule.StepControls alone; VLAEngine and BackboneTrainer inherit them."""
    from vla_adapter_amd import engine, schedule, trainers
    for name in ("set_grad_accumulation", "ga", "set_max_grad_norm", "max_grad_norm", "grad_norm", "clip_coef"):
        for cls in (engine.VLAEngine, trainers.BackboneTrainer, trainers.FullFinetune, trainers.LoRAFinetune):
            assert issubclass(cls, schedule.StepControls) and name not in vars(cls), (cls.__name__, name)
            assert getattr(cls, name) is getattr(schedule.StepControls, name)
