"""CPU checks of the serving batch (predict_actions): the host-side layout and the refusals of the public call that need no device
(tests/test_abi_families.py checks include/vla_serve.h against the binding, the library and the memory-contract cases)."""
import pytest
import torch


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
