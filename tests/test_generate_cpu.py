"""Greedy action decoding without a GPU: what generate_actions refuses, by message, before it touches the engine; what every entry
point of include/vla_decode.h refuses on the host, before any launch (the pointers are never dereferenced); and the host-side layout
of the prompt-only batch."""
import pytest
import torch

from tests import abi_headers as H


@pytest.fixture()
def model():
    """The refusals come before any device work: an instance with a configuration, statistics and a stand-in engine is enough."""
    from types import SimpleNamespace

    from vla_adapter_amd import engine as E
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    m = object.__new__(OpenVLAForActionPrediction)
    m.cfg = E.tiny_config()
    m.engine = SimpleNamespace(fp8_frozen=False)
    m.norm_stats = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    return m


PX = torch.zeros(1, 3, 8, 8)


def test_generate_actions_refuses_a_token_count_it_cannot_shape(model):
    with pytest.raises(ValueError, match="at least 1"):
        model.generate_actions([[5, 6]], pixel_values=PX, max_new_tokens=0)
    with pytest.raises(ValueError, match="not a multiple of action_dim = 7"):
        model.generate_actions([[5, 6]], pixel_values=PX, max_new_tokens=10)
    assert model.cfg.chunk * model.cfg.action_dim == 56, "the default T: the action ids the collator puts behind the prompt"


def test_generate_actions_refuses_film_and_fp8(model):
    with pytest.raises(NotImplementedError, match="FiLM"):
        model.generate_actions([[5, 6]], pixel_values=PX, use_film=True)
    model.engine.fp8_frozen = True
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate_actions([[5, 6]], pixel_values=PX)


def test_generate_actions_refuses_a_missing_statistics_entry(model):
    with pytest.raises(ValueError, match="no statistics entry for unnorm_key = 'bridge'"):
        model.generate_actions([[5, 6]], pixel_values=PX, unnorm_key="bridge")
    model.norm_stats["bridge"] = {"action": {"min": [0.0] * 7, "max": [1.0] * 7}}
    with pytest.raises(ValueError, match="no statistics entry for unnorm_key = None"):
        model.generate_actions([[5, 6]], pixel_values=PX)                       # two data sets and no key
    with pytest.raises(ValueError, match="q01 and q99"):
        model.generate_actions([[5, 6]], pixel_values=PX, unnorm_key="bridge")  # openvla.py:99-105 reads the quantiles
    model.norm_stats = {}
    with pytest.raises(ValueError, match="no statistics entry"):
        model.generate_actions([[5, 6]], pixel_values=PX)


def test_generate_actions_refuses_bad_pixel_sources_and_prompts(model):
    with pytest.raises(ValueError, match="exactly one"):
        model.generate_actions([[5, 6]])
    with pytest.raises(ValueError, match="exactly one"):
        model.generate_actions([[5, 6]], pixel_values=PX, frames_u8=torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="policy_resize works on raw frames"):
        model.generate_actions([[5, 6]], pixel_values=PX, policy_resize=True)
    with pytest.raises(ValueError, match="at least one id"):
        model.generate_actions([[5, 6], []], pixel_values=PX)


def test_predict_action_keeps_its_refusal(model):
    """generate_actions is the autoregressive path of the token-CE objective; the parallel-decoding branch stays refused."""
    with pytest.raises(NotImplementedError, match="lm_head"):
        model.predict_action(torch.zeros(1, 4, dtype=torch.int64), action_head=None)


# ---------------------------------------------------------------------------------------------------------------- host-side refusals
@pytest.fixture(scope="module")
def lib():
    return H.load_library()


P = 4096            # a non-null 16-B aligned stand-in for a device pointer: refused calls never dereference it


def test_decode_prompt_argument_validation(lib):
    f = lambda flat=P, off=P, n_flat=10, ids=P, B=2, L=32, Np=16: lib.vla_decode_prompt(None, flat, off, n_flat, ids, P, P, P, P, B, L, Np, 0)
    assert f(off=None) == -1 and b"null" in lib.vla_last_error()
    assert f(flat=None) == -1 and b"prompt_flat" in lib.vla_last_error()
    assert f(ids=None) == -1 and f(B=0) == -1 and f(L=0) == -1 and f(Np=-1) == -1 and f(n_flat=-1) == -1
    assert f(B=1 << 20, L=1 << 12) == -1 and b"int32 row index" in lib.vla_last_error()


def test_decode_rope_append_argument_validation(lib):
    f = lambda qkv=P, pos=P, k=P, v=P, B=2, Hq=4, Hkv=2, dh=64, ld=512, S_cap=32, sb=32 * 128, ss=128: lib.vla_decode_rope_append(
        None, qkv, P, P, pos, k, v, B, Hq, Hkv, dh, ld, S_cap, sb, ss)
    assert f(qkv=None) == -1 and f(pos=None) == -1 and b"null" in lib.vla_last_error()
    assert f(dh=63) == -1 and b"dh even" in lib.vla_last_error()
    assert f(ld=504) == -1 and b"ld_qkv" in lib.vla_last_error()
    assert f(k=None) == -1 and f(v=P + 2) == -1 and b"16-B aligned" in lib.vla_last_error()
    assert f(ss=120) == -1 and f(ss=132) == -1 and f(sb=31 * 128) == -1 and f(S_cap=0) == -1 and b"cache_ss" in lib.vla_last_error()


def test_decode_attn_argument_validation(lib):
    f = lambda q=P, out=P, k=P, B=2, Hq=4, Hkv=2, dh=64, ldq=256, ldo=256, S_cap=32, sb=32 * 128, ss=128: lib.vla_decode_attn(
        None, q, k, P, P, out, B, Hq, Hkv, dh, ldq, ldo, S_cap, sb, ss, 0.125)
    assert f(q=None) == -1 and f(out=None) == -1 and b"null" in lib.vla_last_error()
    assert f(Hq=5) == -1 and f(Hq=18) == -1 and b"at most 8 query heads per kv head" in lib.vla_last_error()
    assert f(dh=32) == -1 and b"head dim 64 or 128" in lib.vla_last_error()
    assert f(ldq=255) == -1 and f(ldo=0) == -1 and b"row strides" in lib.vla_last_error()
    assert f(k=P + 8) == -1 and f(sb=8) == -1 and f(B=0) == -1


def test_decode_lm_head_argmax_argument_validation(lib):
    f = lambda x=P, W=P, ws=P, B=2, D=64, V=1000, ldx=64, logits=None, ldl=0, out_ids=None, T=4, step=P, emb=P, xn=P, lde=64: lib.vla_decode_lm_head_argmax(
        None, x, ldx, W, 64, B, D, V, ws, P, P, logits, ldl, out_ids, T, step, P, None, emb, 1000, lde, xn, 64)
    assert f(x=None) == -1 and f(W=None) == -1 and f(ws=None) == -1 and b"null" in lib.vla_last_error()
    assert f(B=0) == -1 and f(B=65) == -1 and f(D=60) == -1 and f(D=4104) == -1 and f(V=0) == -1 and b"B in [1, 64]" in lib.vla_last_error()
    assert f(ldx=56) == -1 and f(x=P + 2) == -1 and b"16-B aligned" in lib.vla_last_error()
    assert f(logits=P, ldl=999) == -1 and b"ld_logits" in lib.vla_last_error()
    assert f(out_ids=P, T=0) == -1 and f(out_ids=P, step=None) == -1 and f(out_ids=P, emb=None) == -1 and b"the advance needs" in lib.vla_last_error()
    assert f(out_ids=P, lde=60) == -1 and f(out_ids=P, xn=P + 4) == -1 and b"embed / x_next" in lib.vla_last_error()
    assert lib.vla_decode_argmax_slabs(1016) == 8 and lib.vla_decode_argmax_slabs(151936) == 1187 and lib.vla_decode_argmax_slabs(0) == 0


def test_wrappers_refuse_on_the_host_before_any_launch():
    from vla_adapter_amd import ops
    with pytest.raises(ValueError, match="contiguous int64"):
        ops.decode_prompt(torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 32, 16, pad_id=0)
    with pytest.raises(ValueError, match="int32 \\[B \\+ 1\\] on the device"):
        ops.decode_prompt(torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), 32, 16, pad_id=0)   # offsets on the host


def test_prompt_layout_pads_to_a_multiple_of_32():
    from vla_adapter_amd import input_stage as IS
    stage = object.__new__(IS.GPUInputStage)
    with pytest.raises(ValueError, match="at least 1"):
        stage.decode_prompt([[1, 2], []], 16)
    with pytest.raises(ValueError, match="len_multiple"):
        stage.decode_prompt([[1, 2]], 16, len_multiple=0)
