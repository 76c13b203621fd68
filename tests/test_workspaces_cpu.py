"""Buffer sets of the LLM and the action head (engine._BufferSets): declared by build_buffer_set, installed by bind_buffer_set,
taken - with the per-forward fields - by buffer_set.  Host code only: the sets are built on the CPU, no kernel runs."""
import pytest
import torch

from vla_adapter_amd import engine as E, synthetic

CFG = E.tiny_config()
LLM_SHAPES, HEAD_SHAPES = ((2, 64), (3, 96)), ((2, 16), (3, 16))
DT = {torch.bfloat16: "bf16", torch.float32: "f32", torch.int32: "i32"}

# name -> (*shape, dtype) of every member, recorded from LLM._alloc / Head._alloc as they were before the sets were declared
# (LLM: keep_per_layer(True), the largest set; the smaller ones lack the names of PER_LAYER / NORM_GRADS)
LLM_TABLE = {
    (2, 64): {
        'AO': (2, 128, 256, 'bf16'), 'GU': (2, 128, 1024, 'bf16'), 'G_d1': (2, 128, 256, 'bf16'), 'G_gu': (2, 128, 1024, 'bf16'),
        'G_n1': (2, 128, 256, 'bf16'), 'G_n2': (2, 128, 256, 'bf16'), 'G_qkv': (2, 128, 512, 'bf16'), 'G_res': (2, 128, 256, 'bf16'),
        'HS': (4, 2, 64, 256, 'bf16'), 'Hs': (2, 128, 512, 'bf16'), 'LSE': (2, 2, 4, 64, 'f32'), 'N1': (2, 128, 256, 'bf16'),
        'N2': (2, 128, 256, 'bf16'), 'QKV': (2, 128, 512, 'bf16'), 'R1': (2, 128, 'f32'), 'R2': (2, 128, 'f32'), 'RF': (128, 'f32'),
        'X1': (2, 128, 256, 'bf16'), 'cos': (64, 32, 'f32'), 'd_a': (128, 256, 'bf16'), 'd_b': (128, 256, 'bf16'), 'd_gu': (128, 1024, 'bf16'),
        'd_last': (128, 256, 'bf16'), 'd_n': (128, 256, 'bf16'), 'd_qkv': (128, 512, 'bf16'), 'hbuf': (128, 512, 'bf16'), 'nbuf': (128, 256, 'bf16'),
        'sin': (64, 32, 'f32'),
    },
    (3, 96): {
        'AO': (2, 288, 256, 'bf16'), 'GU': (2, 288, 1024, 'bf16'), 'G_d1': (2, 288, 256, 'bf16'), 'G_gu': (2, 288, 1024, 'bf16'),
        'G_n1': (2, 288, 256, 'bf16'), 'G_n2': (2, 288, 256, 'bf16'), 'G_qkv': (2, 288, 512, 'bf16'), 'G_res': (2, 288, 256, 'bf16'),
        'HS': (4, 3, 96, 256, 'bf16'), 'Hs': (2, 288, 512, 'bf16'), 'LSE': (2, 3, 4, 96, 'f32'), 'N1': (2, 288, 256, 'bf16'),
        'N2': (2, 288, 256, 'bf16'), 'QKV': (2, 288, 512, 'bf16'), 'R1': (2, 288, 'f32'), 'R2': (2, 288, 'f32'), 'RF': (288, 'f32'),
        'X1': (2, 288, 256, 'bf16'), 'cos': (96, 32, 'f32'), 'd_a': (288, 256, 'bf16'), 'd_b': (288, 256, 'bf16'), 'd_gu': (288, 1024, 'bf16'),
        'd_last': (288, 256, 'bf16'), 'd_n': (288, 256, 'bf16'), 'd_qkv': (288, 512, 'bf16'), 'hbuf': (288, 512, 'bf16'), 'nbuf': (288, 256, 'bf16'),
        'sin': (96, 32, 'f32'),
    },
}
NORM_GRADS = {"G_n1", "G_n2"}
PER_LAYER = {"N1", "N2", "Hs", "G_res", "G_d1", "G_gu", "G_qkv", "d_last"} | NORM_GRADS
_B_F32 = {'b_x': (2, 768, 'f32'), 'b_adp': (2, 512, 'f32'), 'b_task': (2, 512, 'f32'), 'b_o': (2, 256, 'f32'), 'b_ffn': (2, 256, 'f32'),
          'fc1_b': (256, 'f32'), 'fc2_b': (7, 'f32'), 'p_fc1_b': (256, 'f32'), 'p_fc2_b': (256, 'f32')}
HEAD_TABLE = {
    (2, 16): {
        'AOx': (2, 16, 256, 'bf16'), 'KV_adp': (2, 130, 512, 'bf16'), 'KV_task': (2, 32, 512, 'bf16'), 'Ka': 65, 'Kt': 16,
        'LNo': (2, 16, 256, 'bf16'), 'O2': (2, 16, 256, 'bf16'), 'QKVx': (2, 16, 768, 'bf16'), 'R': 16, 'X': (3, 16, 256, 'bf16'),
        '_idx_scratch': (2, 65, 'i32'), 'acc32': (11020, 'f32'), 'b_f32': _B_F32,
        'dFF': (2, 16, 256, 'bf16'), 'dKV_adp': (2, 130, 512, 'bf16'), 'dKV_task': (2, 32, 512, 'bf16'), 'dO2': (2, 16, 256, 'bf16'),
        'dQKVx': (2, 16, 768, 'bf16'), 'd_pf32': (2, 256, 'f32'), 'dfc2': (64, 256, 'bf16'), 'dgate': (2, 'f32'), 'dh_adp': (2, 130, 256, 'bf16'),
        'dpad': (16, 64, 'bf16'), 'dpfc1': (256, 64, 'bf16'), 'guard': (1, 'f32'), 'h_adp': (2, 2, 65, 256, 'bf16'),
        'h_task_c': (2, 32, 256, 'bf16'), 'ln1_db': (1792, 'f32'), 'ln1_dw': (1792, 'f32'), 'ln2_db': (256, 'f32'), 'ln2_dw': (256, 'f32'),
        'ln_db': (2, 256, 'f32'), 'ln_dw': (2, 256, 'f32'), 'pr_in': (2, 64, 'bf16'), 'probs': (2, 2, 8, 8, 89, 'f32'),
        'rope_tab': ((65, 32, 'f32'), (65, 32, 'f32')), 'row_idx_ka': (2, 65, 'i32'), 'row_idx_live_ka': (2, 65, 'i32'), 'stats': (2, 16, 2, 'f32'),
        'x_in': (16, 1792, 'bf16'),
    },
    (3, 16): {
        'AOx': (2, 24, 256, 'bf16'), 'KV_adp': (2, 195, 512, 'bf16'), 'KV_task': (2, 48, 512, 'bf16'), 'Ka': 65, 'Kt': 16,
        'LNo': (2, 24, 256, 'bf16'), 'O2': (2, 24, 256, 'bf16'), 'QKVx': (2, 24, 768, 'bf16'), 'R': 24, 'X': (3, 24, 256, 'bf16'),
        '_idx_scratch': (3, 65, 'i32'), 'acc32': (11276, 'f32'), 'b_f32': _B_F32,
        'dFF': (2, 24, 256, 'bf16'), 'dKV_adp': (2, 195, 512, 'bf16'), 'dKV_task': (2, 48, 512, 'bf16'), 'dO2': (2, 24, 256, 'bf16'),
        'dQKVx': (2, 24, 768, 'bf16'), 'd_pf32': (3, 256, 'f32'), 'dfc2': (64, 256, 'bf16'), 'dgate': (2, 'f32'), 'dh_adp': (2, 195, 256, 'bf16'),
        'dpad': (24, 64, 'bf16'), 'dpfc1': (256, 64, 'bf16'), 'guard': (1, 'f32'), 'h_adp': (2, 3, 65, 256, 'bf16'),
        'h_task_c': (2, 48, 256, 'bf16'), 'ln1_db': (1792, 'f32'), 'ln1_dw': (1792, 'f32'), 'ln2_db': (256, 'f32'), 'ln2_dw': (256, 'f32'),
        'ln_db': (2, 256, 'f32'), 'ln_dw': (2, 256, 'f32'), 'pr_in': (3, 64, 'bf16'), 'probs': (2, 3, 8, 8, 89, 'f32'),
        'rope_tab': ((65, 32, 'f32'), (65, 32, 'f32')), 'row_idx_ka': (3, 65, 'i32'), 'row_idx_live_ka': (3, 65, 'i32'), 'stats': (2, 24, 2, 'f32'),
        'x_in': (24, 1792, 'bf16'),
    },
}
KEYS = ("_buf_key", "_prep_key")       # the set's key and the head's reset of its backward-prep key: not buffers


def make_llm():
    return E.LLM(CFG.llm, synthetic.llm_weights(CFG.llm, torch.Generator().manual_seed(0), "cpu", 0.0), "cpu")


def make_head():
    return E.Head(CFG, "cpu")


CASES = [pytest.param(make_llm, LLM_SHAPES, id="llm"), pytest.param(make_head, HEAD_SHAPES, id="head")]


def sig(v):
    if torch.is_tensor(v):
        return (*v.shape, DT[v.dtype])
    if isinstance(v, dict):
        return {k: sig(t) for k, t in v.items()}
    return tuple(sig(t) for t in v) if isinstance(v, tuple) else v


def tensors(v):
    if torch.is_tensor(v):
        return [v]
    return [t for x in (v.values() if isinstance(v, dict) else v if isinstance(v, tuple) else ()) for t in tensors(x)]


def fields_of(obj, tag):
    """Stand-ins for what fwd_begin / prep_backward record (Head.fwd_begin launches kernels: the fields are set as it sets them)."""
    return {k: (tag, k) for k in obj._FWD_FIELDS}


@pytest.mark.parametrize("make, shapes", CASES)
def test_building_a_set_touches_no_attribute(make, shapes):
    obj = make()
    obj._alloc(*shapes[0])
    before = dict(vars(obj))
    built = obj.build_buffer_set(*shapes[1])
    assert vars(obj).keys() == before.keys() and all(vars(obj)[k] is v for k, v in before.items())
    assert built["_buf_key"] == shapes[1] and obj._buf_key == shapes[0]


@pytest.mark.parametrize("make, shapes", CASES)
def test_a_set_comes_back_whole(make, shapes):
    """Bind A, then B, then A: the identical tensors, A's key and A's per-forward fields; no storage shared between A and B."""
    obj = make()
    obj._alloc(*shapes[0])
    vars(obj).update(fields_of(obj, "a"))
    A = obj.buffer_set()
    assert set(obj._FWD_FIELDS) <= A.keys() and obj.buffer_set() is not None
    obj._alloc(*shapes[1])
    assert obj._buf_key == shapes[1] and all(getattr(obj, k) == ("a", k) for k in obj._FWD_FIELDS if k != "_prep_key"), \
        "a fresh set leaves the per-forward fields to the next forward"
    vars(obj).update(fields_of(obj, "b"))
    Bs = obj.buffer_set()
    obj.bind_buffer_set(A)
    assert obj._buf_key == shapes[0] and obj._bound is A
    assert all(getattr(obj, k) is v for k, v in A.items()), "every attribute A names is the object A holds"
    assert all(getattr(obj, k) == ("a", k) for k in obj._FWD_FIELDS)
    obj.bind_buffer_set(Bs)
    assert obj._buf_key == shapes[1] and all(getattr(obj, k) == ("b", k) for k in obj._FWD_FIELDS)
    ptr = lambda s: {t.untyped_storage().data_ptr() for v in s.values() for t in tensors(v) if t.numel()}
    assert ptr(A) and ptr(Bs) and not (ptr(A) & ptr(Bs))
    obj._alloc(*shapes[1])                       # bound key equal: nothing is built
    assert obj._bound is Bs


@pytest.mark.parametrize("make, shapes", CASES)
def test_unbind_makes_the_next_alloc_fresh(make, shapes):
    obj = make()
    assert obj.buffer_set() is None, "nothing is bound to a new object"
    obj._alloc(*shapes[0])
    A = obj.buffer_set()
    obj._alloc(*shapes[0])
    assert obj._bound is A
    obj.unbind()
    assert obj.buffer_set() is None
    obj._alloc(*shapes[0])
    new = obj.buffer_set()
    assert new.keys() == A.keys() and obj._buf_key == shapes[0]
    assert all(new[k] is not A[k] for k in A if tensors(A[k])), "new tensors of the old shape: A's holders keep A"


def test_keep_per_layer_sets_hold_the_per_layer_slots():
    llm = make_llm()
    llm._alloc(2, 64)
    plain = llm.buffer_set()
    assert not (PER_LAYER & plain.keys())
    llm.keep_per_layer(True)
    assert llm.buffer_set() is None, "keep_per_layer unbinds: the bound set has no per-layer slots"
    llm._alloc(2, 64)
    assert PER_LAYER <= llm.buffer_set().keys() and llm.HS is not plain["HS"] and llm.N1.shape == (2, 128, 256)


@pytest.mark.parametrize("per_layer", [None, False, True])
@pytest.mark.parametrize("shape", LLM_SHAPES)
def test_llm_set_is_the_recorded_table(shape, per_layer):
    llm = make_llm()
    if per_layer is not None:
        llm.keep_per_layer(per_layer)
    absent = PER_LAYER if per_layer is None else NORM_GRADS if not per_layer else set()
    want = {k: v for k, v in LLM_TABLE[shape].items() if k not in absent}
    got = {k: sig(v) for k, v in llm.build_buffer_set(*shape).items() if k not in KEYS}
    assert got == want and len(want) == {None: 18, False: 26, True: 28}[per_layer]


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_set_is_the_recorded_table(shape):
    built = make_head().build_buffer_set(*shape)
    assert {k: sig(v) for k, v in built.items() if k not in KEYS} == HEAD_TABLE[shape] and len(HEAD_TABLE[shape]) == 40
    assert built["_prep_key"] is None
    # the fp32 accumulators are views of the one buffer a single fill zeroes, and start zeroed with the other zero-filled members
    acc = built["acc32"]
    views = [built[k] for k in ("dgate", "ln_dw", "ln_db", "ln1_dw", "ln1_db", "ln2_dw", "ln2_db", "d_pf32")] + list(built["b_f32"].values())
    assert all(v.untyped_storage().data_ptr() == acc.untyped_storage().data_ptr() for v in views)
    assert all(not built[k].any() for k in ("acc32", "guard", "x_in", "pr_in", "dpad"))
