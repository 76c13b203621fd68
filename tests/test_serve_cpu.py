"""CPU checks of the serving batch (predict_actions): the host-side layout, the second header against its signature table and the
built library, the untouched training ABI, the completeness guard of tests/test_serve_memory_contract_gpu.py, and the refusals of
the public call that need no device."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def serve_header_symbols():
    txt = open(os.path.join(ROOT, "include", "vla_serve.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vla_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    from vla_adapter_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load()


# ---------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("lens", [[1, 5, 19, 12], [1, 2, 19, 40], [31], [32], [63, 1], [200, 3, 77]])
def test_serve_layout_against_per_row_prepare_inference_inputs(lens):
    from vla_adapter_amd import constants as K
    from vla_adapter_amd.input_stage import serve_layout
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction as V
    rows = []
    for n in lens:
        ids = torch.arange(3, 3 + n).view(1, n)
        rows.append(V.prepare_inference_inputs(ids, torch.ones_like(ids, dtype=torch.bool))[0].shape[1])
    assert rows == [n + K.NUM_TOKENS + 1 for n in lens]
    off, L = serve_layout(lens)
    assert off == [sum(lens[:i]) for i in range(len(lens) + 1)]
    assert L % 32 == 0 and max(rows) <= L < max(rows) + 32, "the longest row rounded up to the next multiple of 32"
    assert serve_layout(lens, 1)[1] == max(rows), "len_multiple 1: the longest row itself"
    assert serve_layout(lens, 64)[1] % 64 == 0 and max(rows) <= serve_layout(lens, 64)[1] < max(rows) + 64


def test_serve_layout_lands_a_stream_of_calls_on_few_shapes():
    from vla_adapter_amd.input_stage import serve_layout
    assert len({serve_layout([p, 7])[1] for p in range(8, 31)}) == 1            # rows of 73 .. 95 ids: all L = 96
    with pytest.raises(ValueError):
        serve_layout([3], 0)


# ---------------------------------------------------------------------------------------------------------------- the two tables
def test_serve_header_and_binding_agree():
    from vla_adapter_amd import native
    assert serve_header_symbols() == native.SERVE_SYMBOLS == sorted(native.SERVE_PROTOS)
    assert {"vla_serve_tokens", "vla_normalize_proprio_serve", "vla_unnormalize_actions"} <= set(native.SERVE_PROTOS)
    assert not set(native.SERVE_PROTOS) & set(native._PROTOS), "an entry point belongs to one header"


def test_library_exports_every_serve_symbol(lib):
    from vla_adapter_amd import native
    for name in serve_header_symbols():
        fn = getattr(lib, name, None)
        assert fn is not None, f"libvla_native.so does not export {name}"
        args, res = native.SERVE_PROTOS[name]
        assert list(fn.argtypes) == list(args) and fn.restype is res, f"{name}: native.load() binds the table's signature"


def test_serve_signatures_match_the_header_argument_counts():
    """Each prototype of the header has as many parameters as its ctypes signature (a dropped or added argument shifts every later one)."""
    from vla_adapter_amd import native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vla_serve.h")).read(), flags=re.S)
    for name, params in re.findall(r"\bint\s+(vla_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        assert len(params.split(",")) == len(native.SERVE_PROTOS[name][0]), name


def test_training_abi_is_unchanged():
    from vla_adapter_amd import native
    txt = open(os.path.join(ROOT, "include", "vla_native.h")).read()
    assert native.ABI_VERSION == 8 == int(re.search(r"#define VLA_ABI_VERSION (\d+)", txt).group(1))
    assert native.ABI_SYMBOLS == sorted(list(native._PROTOS) + ["vla_last_error"])
    assert len(native._PROTOS) == 69 and not [k for k in native._PROTOS if "serve" in k or k == "vla_unnormalize_actions"]
    stripped = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(vla_[a-z0-9_]+)\s*\(", stripped))) == native.ABI_SYMBOLS, "vla_native.h declares the training table only"


def test_every_serve_symbol_has_a_memory_contract_case_or_an_exemption():
    from tests import test_serve_memory_contract_gpu as M
    from vla_adapter_amd import native
    table = set(native.SERVE_PROTOS)
    covered, exempt = set(M.COVERED), set(M.EXEMPT)
    assert not (covered | exempt) - table, f"names that are no serving entry points: {sorted((covered | exempt) - table)}"
    assert not covered & exempt, f"both tested and exempt: {sorted(covered & exempt)}"
    assert not table - covered - exempt, f"entry points with neither a case nor an exemption: {sorted(table - covered - exempt)}"
    for name, reason in M.EXEMPT.items():
        assert isinstance(reason, str) and 4 <= len(reason) and "\n" not in reason, f"{name}: a one-line reason"
    for name, tests in M.COVERED.items():
        for t in tests:
            assert callable(getattr(M, t, None)), f"{name}: case {t} does not exist"


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture()
def bare_model():
    """The public call refuses before it touches the engine: an instance without one is enough (and needs no device)."""
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    return object.__new__(OpenVLAForActionPrediction)


def test_predict_actions_refuses_both_or_neither_pixel_source(bare_model):
    px = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="exactly one"):
        bare_model.predict_actions([[5, 6]], proprio=[[0.0] * 8])
    with pytest.raises(ValueError, match="exactly one"):
        bare_model.predict_actions([[5, 6]], pixel_values=px, frames_u8=torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8), proprio=[[0.0] * 8])


def test_predict_actions_refuses_film_diffusion_and_the_token_branch(bare_model):
    px = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="FiLM"):
        bare_model.predict_actions([[5, 6]], pixel_values=px, proprio=[[0.0] * 8], use_film=True)
    with pytest.raises(NotImplementedError, match="FiLM / diffusion"):
        bare_model.predict_actions([[5, 6]], pixel_values=px, proprio=[[0.0] * 8], noisy_action_projector=object())
    with pytest.raises(NotImplementedError, match="lm_head"):
        bare_model.predict_actions([[5, 6]], pixel_values=px, proprio=[[0.0] * 8], action_head=None)


def test_predict_actions_refuses_an_overlong_or_empty_host_prompt(bare_model):
    px = torch.zeros(2, 3, 8, 8)
    pr = [[0.0] * 8] * 2
    with pytest.raises(ValueError, match="needs L >= 106"):
        bare_model.predict_actions([[5] * 41, [6]], pixel_values=px, proprio=pr, L=105)
    with pytest.raises(ValueError, match="at least one id"):
        bare_model.predict_actions([[5, 6], []], pixel_values=px, proprio=pr)
    # the same through host-resident offset tensors; device-resident ones rely on row_ok and need L
    flat, off = torch.arange(41, dtype=torch.int64), torch.tensor([0, 41, 41], dtype=torch.int32)
    with pytest.raises(ValueError, match="at least one id"):
        bare_model.predict_actions((flat, off), pixel_values=px, proprio=pr)


def test_serve_check_needs_l_for_device_offsets_without_reading_them():
    from vla_adapter_amd.input_stage import serve_check

    class DeviceOffsets(torch.Tensor):                   # stands for offsets on the device: any read of it would raise
        is_cuda = True

        def diff(self, *a, **k):
            raise AssertionError("device offsets must not be read back")
    off = torch.tensor([0, 3, 9], dtype=torch.int32).as_subclass(DeviceOffsets)
    flat = torch.arange(9)
    with pytest.raises(ValueError, match="explicit L"):
        serve_check((flat, off))
    assert serve_check((flat, off), L=96) == (None, 96)
