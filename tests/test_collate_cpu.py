"""The on-device collator without a GPU: the --raw_batch_file flag and its refusals, the two entry points in header / binding /
library with their host-side argument validation, and the host half of GPUInputStage.collate (offsets and token length)."""
import ctypes
import json
import os
import re

import pytest

from vla_adapter_amd import finetune as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("vla_normalize_bounds", "vla_collate_tokens")
PROMPT_LENS = [2, 3, 9, 40, 51]


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def test_raw_batch_file_is_accepted_with_statistics(tmp_path):
    cfg = F.parse_args(["--use_proprio", "True", "--raw_batch_file", str(tmp_path), "--dataset_statistics_file", "stats.json", "--image_aug", "True",
                        "--max_seq_len", "128"])
    F.check_supported(cfg, cfg._explicit)                 # raw batches carry frames: --image_aug is honoured
    assert cfg.raw_batch_file == str(tmp_path) and cfg.max_seq_len == 128


@pytest.mark.parametrize("other", ["--batch_file", "--frame_batch_file"])
def test_two_batch_sources_are_refused(other):
    cfg = F.parse_args(["--use_proprio", "True", "--raw_batch_file", "raw", other, "b", "--dataset_statistics_file", "stats.json"])
    with pytest.raises(ValueError, match="batch sources"):
        F.check_supported(cfg, cfg._explicit)


def test_three_batch_sources_are_refused():
    cfg = F.parse_args(["--use_proprio", "True", "--raw_batch_file", "raw", "--batch_file", "a", "--frame_batch_file", "b",
                        "--dataset_statistics_file", "stats.json"])
    with pytest.raises(ValueError, match="3 batch sources"):
        F.check_supported(cfg, cfg._explicit)


def test_raw_batch_file_without_statistics_is_refused():
    cfg = F.parse_args(["--use_proprio", "True", "--raw_batch_file", "raw"])
    with pytest.raises(ValueError, match="dataset_statistics_file"):
        F.check_supported(cfg, cfg._explicit)


def test_raw_batches_handed_to_the_stream_without_statistics_are_refused():
    import torch
    cfg = F.parse_args(["--use_proprio", "True"])
    raw = dict(frames_u8=torch.zeros(1, 1, 2, 2, 3, dtype=torch.uint8), prompt_flat=torch.zeros(4, dtype=torch.int64),
               prompt_off=torch.tensor([0, 4], dtype=torch.int32), actions_raw=torch.zeros(1, 8, 7), proprio_raw=torch.zeros(1, 8))
    with pytest.raises(ValueError, match="dataset_statistics_file"):
        next(F.batch_stream(cfg, None, "cpu", 0, [raw], cfg._explicit))
    with pytest.raises(ValueError, match="proprio_raw"):
        next(F.batch_stream(cfg, None, "cpu", 0, [{k: v for k, v in raw.items() if k != "proprio_raw"}], cfg._explicit))


def test_unknown_dataset_key_is_refused_with_the_keys(tmp_path):
    entry = dict(action=dict(q01=[0.0], q99=[1.0]), proprio=dict(q01=[0.0], q99=[1.0]))
    one, two = {"libero_object": entry}, {"libero_object": entry, "libero_goal": entry}
    assert F.raw_batch_stats(one) is entry and F.raw_batch_stats(one, "libero_object") is entry        # the only key / the named key
    assert F.raw_batch_stats(two, "libero_goal") is entry
    with pytest.raises(KeyError, match=r"libero_goal.*libero_object"):
        F.raw_batch_stats(two)                            # two entries and no dataset_name
    with pytest.raises(KeyError, match=r"'bridge'.*libero_object"):
        F.raw_batch_stats(one, "bridge")
    with pytest.raises(KeyError, match="proprio"):
        F.raw_batch_stats({"x": dict(action=entry["action"])})
    # the same through the stream: the statistics file is read when the first raw batch arrives
    import torch
    f = tmp_path / "stats.json"
    f.write_text(json.dumps(two))
    cfg = F.parse_args(["--use_proprio", "True", "--dataset_statistics_file", str(f)])
    raw = dict(frames_u8=torch.zeros(1, 1, 2, 2, 3, dtype=torch.uint8), prompt_flat=torch.zeros(4, dtype=torch.int64),
               prompt_off=torch.tensor([0, 4], dtype=torch.int32), actions_raw=torch.zeros(1, 8, 7), proprio_raw=torch.zeros(1, 8),
               dataset_name="bridge")
    with pytest.raises(KeyError, match="bridge"):
        next(F.batch_stream(cfg, None, "cpu", 0, [raw], cfg._explicit))


def test_new_symbols_in_header_binding_and_library(lib):
    from vla_adapter_amd import native
    txt = open(os.path.join(ROOT, "include", "vla_native.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in vla_native.h"
        assert name in native.family("native").protos and hasattr(lib, name)
        assert name in re.search(r"Added since without a version change.*?\*/", txt, flags=re.S).group(0)
    assert lib.vla_version() == native.ABI_VERSION == int(re.search(r"#define VLA_ABI_VERSION (\d+)", txt).group(1))


def test_argument_validation_without_gpu(lib):
    """Bad arguments are refused on the host, before any launch (the pointers are never dereferenced)."""
    P = 4096
    assert lib.vla_normalize_bounds(None, None, P, 56, 7, P, P, None, None) == -1
    assert lib.vla_normalize_bounds(None, P, P, 0, 7, P, P, None, None) == -1
    assert lib.vla_normalize_bounds(None, P, P, 55, 7, P, P, None, None) == -1 and b"multiple of D" in lib.vla_last_error()
    col = lambda flat=P, off=P, n_flat=10, B=2, n_act=56, L=70, nbins=256, lo=-1.0, hi=1.0, nt=64: lib.vla_collate_tokens(
        None, flat, off, n_flat, P, P, P, P, P, B, n_act, L, nbins, lo, hi, 151643, 151643, -100, nt, 0, 0, 0)
    assert col(off=None) == -1 and b"null" in lib.vla_last_error()
    assert col(flat=None) == -1 and b"prompt_flat" in lib.vla_last_error()
    assert col(B=0) == -1 and col(n_act=0) == -1 and col(L=0) == -1 and col(n_flat=-1) == -1 and col(nbins=1) == -1 and col(lo=1.0) == -1
    assert col(nt=0) == -1 and col(nt=257) == -1 and b"num_tokens" in lib.vla_last_error()


def test_host_layout_of_the_five_prompt_lengths():
    """Offsets and token length come from the prompt lengths on the host (datasets.py:76-79: a prompt of three or more ids loses
    three): rows of 2 + 64, 0 + 64, 6 + 64, 37 + 64, 48 + 64 ids."""
    from vla_adapter_amd.input_stage import collate_layout
    off, L = collate_layout(PROMPT_LENS, 2048)
    assert off == [0, 2, 5, 14, 54, 105] and L == 112
    assert collate_layout(PROMPT_LENS, 70)[1] == 70                       # model_max_length cuts
    assert collate_layout([3], 2048) == ([0, 3], 64) and collate_layout([2], 2048) == ([0, 2], 66) and collate_layout([0], 2048) == ([0, 0], 64)
    assert collate_layout([10, 4], 2048, num_tokens=8) == ([0, 10, 14], 15)


def test_normal_normalisation_and_device_offsets_without_length_are_refused():
    import torch
    from vla_adapter_amd.input_stage import GPUInputStage
    st = GPUInputStage("cpu")
    with pytest.raises(NotImplementedError, match="bounds"):
        st.normalize(torch.zeros(2, 7), dict(mean=[0.0] * 7, std=[1.0] * 7), kind="normal")
    with pytest.raises(KeyError, match="q01"):
        st.normalize(torch.zeros(2, 7), dict(min=[0.0] * 7, max=[1.0] * 7), kind="bounds_q99")
