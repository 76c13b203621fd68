"""The kernels' scratch arena on the device (vla_adapter_amd/scratch.py): a capture through
schedule.capture_graph finds its stream's scratch reserved, a graph's scratch outlives a larger request on its stream, and the
digest's partial sums are per stream.  The smallest shapes that take each path through the scratch."""
import gc

import pytest
import torch

from tests.arena import assert_bits_equal
from vla_adapter_amd import ops, schedule
from vla_adapter_amd.scratch import ARENA

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def nt_split():
    """gemm_nt forced to two K slices on one 128 x 128 tile (the split excludes the skinny route): 2 * 128 * 128 floats."""
    a, b, out = gen(128, 256, seed=1), gen(128, 256, seed=2, scale=0.05), torch.empty(128, 128, dtype=BF, device=DEV)
    return (lambda: ops.gemm_nt(a, b, out=out, split_k=2)), [out], 4 * 2 * 128 * 128


def tn_split():
    """gemm_tn over two slices of the contraction, the shape of test_memory_contract_gpu.py::test_gemm_tn[128-split]."""
    N1, N2, M = 136, 264, 129
    a, b, out = gen(M, N1, seed=21), gen(M, N2, seed=22), torch.empty(N1, N2, dtype=BF, device=DEV)
    return (lambda: ops.gemm_tn(a, b, out=out, split=2)), [out], 4 * 2 * N1 * N2


def head_bwd():
    """head_attn_bwd on the MFMA path at the shape of test_memory_contract_gpu.py::test_head_attention (its forward runs once, here)."""
    nb, T, Ka, Kt, H, dh = 2, 8, 9, 33, 2, 16
    D = H * dh
    q, ks, vs = (gen(nb, T, D, seed=100 + i) for i in range(3))
    ka, va = gen(nb, Ka, D, seed=103), gen(nb, Ka, D, seed=104)
    kt, vt = gen(nb, Kt, D, seed=105), gen(nb, Kt, D, seed=106)
    gate, dout = torch.tensor([0.3], dtype=BF, device=DEV), gen(nb, T, D, seed=107)
    out, probs = ops.head_attn_fwd(q, ks, vs, ka, va, kt, vt, gate, H=H)
    grads = [torch.empty_like(t) for t in (q, ks, vs, ka, va, kt, vt)]
    dgate = torch.zeros(1, dtype=F32, device=DEV)

    def call():
        dgate.zero_()                                # (an accumulator)
        ops.head_attn_bwd(dout, out, q, ks, vs, ka, va, kt, vt, gate, probs, dgate, *grads, H=H)
    return call, grads + [dgate], 4 * nb * H * ((T + Ka + Kt + 31) // 32) * (T * dh + 1)


PATHS = {"gemm_nt": nt_split, "gemm_tn": tn_split, "head_attn_bwd": head_bwd}


def key_of(stream):
    return (stream.cuda_stream, str(stream.device))


def poison(outs):
    for o in outs:
        o.fill_(float("nan"))


def warm_up_and_capture(path):
    """The path run eagerly on a stream X, then captured through schedule.capture_graph on another stream Y -> (graph, outputs, the
    eager outputs, Y, the path's request in bytes).  Asserts that Y's scratch stood, large enough and held, when the capture began,
    and that the capture allocated none."""
    call, outs, nbytes = PATHS[path]()
    X, Y = torch.cuda.Stream(), torch.cuda.Stream()
    assert key_of(X) != key_of(Y)
    X.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(X):
        call()
        eager = [o.clone() for o in outs]
    X.synchronize()
    assert key_of(X) in ARENA.buffers and ARENA.high_water[str(X.device)] >= nbytes, f"{path} did not go through the scratch"
    poison(outs)
    count, at_begin = ARENA.under_capture, {}

    def fn():
        at_begin.update(capturing=torch.cuda.is_current_stream_capturing(), stream=torch.cuda.current_stream().cuda_stream,
                        buf=ARENA.buffers.get(key_of(Y)), held=ARENA.is_held(key_of(Y)))
        call()
    g = schedule.capture_graph(fn, torch.cuda.graph_pool_handle(), Y)
    assert at_begin["capturing"] and at_begin["stream"] == Y.cuda_stream
    assert at_begin["buf"] is not None and at_begin["buf"].numel() >= nbytes and at_begin["held"], "Y's scratch must stand before the capture begins"
    assert ARENA.buffers[key_of(Y)] is at_begin["buf"] and ARENA.under_capture == count, "the capture allocated scratch"
    return g, outs, eager, Y, nbytes


def replay_equals(g, outs, eager, what):
    poison(outs)
    g.replay()
    torch.cuda.synchronize()
    for i, (o, e) in enumerate(zip(outs, eager)):
        assert_bits_equal(o, e, f"{what}: output {i}, replayed against eager")


@pytest.mark.parametrize("path", list(PATHS))
def test_capture_finds_its_scratch_reserved(path):
    g, outs, eager, _, _ = warm_up_and_capture(path)
    replay_equals(g, outs, eager, path)


def test_a_graphs_scratch_outlives_growth_on_its_stream(monkeypatch):
    """A larger request on the capture stream after the capture: the graph's scratch is retired, not released.  Blocks of its size
    allocated afterwards (on the stream that reserved it, and on the capture stream) and filled with a NaN pattern do not land on
    it: they keep their pattern through a replay, and the replay's result keeps its bits."""
    monkeypatch.setattr(ARENA, "floor", 4096)
    g, outs, eager, Y, _ = warm_up_and_capture("gemm_nt")
    captured = ARENA.buffers[key_of(Y)]
    ptr, size = captured.data_ptr(), captured.numel()
    with torch.cuda.stream(Y):
        grown = ARENA.get(size + 1, Y.device)
    assert grown.data_ptr() != ptr and grown.numel() > size and ARENA.buffers[key_of(Y)] is grown
    del captured
    gc.collect()
    torch.cuda.synchronize()
    fill = [torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(4)]
    with torch.cuda.stream(Y):
        fill += [torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(4)]
    Y.synchronize()
    assert ptr not in [t.data_ptr() for t in fill]
    replay_equals(g, outs, eager, "after growth")
    assert all(bool((t == 0xFF).all()) for t in fill), "the replay wrote its partials into memory the allocator had handed out again"
    assert ptr in [t.data_ptr() for t in list(ARENA.buffers.values()) + list(ARENA.retired)]


def test_digest_scratch_is_per_stream():
    """state_digest on two streams with no event between the calls: each sums in its own stream's scratch, and both values are
    those of one stream."""
    t1, t2 = gen(1 << 20, seed=31), gen((1 << 20) + 24, seed=32)
    want = [ops.digest_value(ops.state_digest(t, salt=7)) for t in (t1, t2)]
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert key_of(S1) != key_of(S2)
    for s in (S1, S2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(S1):
        d1 = ops.state_digest(t1, salt=7)
    with torch.cuda.stream(S2):
        d2 = ops.state_digest(t2, salt=7)
    b1, b2 = ARENA.buffers[key_of(S1)], ARENA.buffers[key_of(S2)]
    assert b1 is not b2 and b1.data_ptr() != b2.data_ptr()
    torch.cuda.synchronize()
    assert [ops.digest_value(d1), ops.digest_value(d2)] == want
