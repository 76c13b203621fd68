"""--max_grad_norm without a GPU: the config field and flag, refusal of bad values, the host-arithmetic slot count of the
sum-of-squares pass, and the new exports in header and binding."""
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vla_grad_sumsq_slots", "vla_grad_sumsq", "vla_grad_norm_finalise", "vla_adamw_clipped_bf16")
BASE = ["--tiny", "true", "--use_proprio", "True"]


@pytest.fixture(scope="module")
def lib():
    from vla_adapter_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load()


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
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), f"{name} is not declared in vla_native.h"
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
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
