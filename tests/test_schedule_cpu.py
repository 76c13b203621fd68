"""The host-side pieces of the segment schedule (vla_adapter_amd/schedule.py) that need no GPU."""
import pytest
import torch

from vla_adapter_amd.schedule import GradAccumulator, Segment, chunks, pipeline_backward, pipeline_forward, turnaround_chunks


def test_chunks_cover_the_layers_with_the_given_sizes():
    assert chunks(24, [4] * 5 + [2, 1, 1]) == [(0, 4), (4, 8), (8, 12), (12, 16), (16, 20), (20, 22), (22, 23), (23, 24)]
    assert chunks(5, [1]) == [(i, i + 1) for i in range(5)]
    assert chunks(10, [4]) == [(0, 4), (4, 8), (8, 10)]                 # the last size repeats and is clipped
    assert chunks(3, [1, 2, 4, 7]) == [(0, 1), (1, 3)]
    assert chunks(0, [4]) == []


def test_segment_is_positional():
    """tools/*_timeline.py read seg[2] (wait), seg[3] (signal) and seg[4] (ranges)."""
    fn = object()
    sg = Segment("H", fn, ("f", 0))
    assert tuple(sg) == ("H", fn, ("f", 0), None, None)
    assert (sg[0], sg[1], sg[2], sg[3], sg[4]) == (sg.stream, sg.fn, sg.wait, sg.signal, sg.ranges)


# ---- the LLM-and-head pipeline ------------------------------------------------------------------------------------------------
# Specification: the chunk rules and segment loops as engine.VLAEngine._segments / _predict_segments and
# trainers.BackboneTrainer._segments spelled them out, each for itself, before schedule.py built them - (stream, wait, signal,
# ranges) per segment, in list order.
def _spec_chunks(rule, n, el=4):
    if rule == "step":
        return chunks(n, [4] * max(0, (n - 4) // 4) + [2, 1, 1]) if n >= 8 else chunks(n, [1])
    if rule == "predict":
        return chunks(n, [6] * max(0, (n - 6) // 6) + [4, 2]) if n >= 12 else chunks(n, [1])
    return chunks(n, [el] * max(0, (n - 4) // el) + [2, 1, 1]) if n >= 8 else chunks(n, [el])


def _spec_step(fch):
    segs = []
    for c, (lo, hi) in enumerate(fch):
        segs.append(("M", None, ("f", c), None))
        segs.append(("H", ("f", c), None, None))
    for k, (lo, hi) in enumerate(reversed(fch)):
        segs.append(("H", None, ("b", k), None))
        segs.append(("M", ("b", k), None, None))
    return segs


def _spec_predict(ch, n_vits):
    segs = []
    for c, (lo, hi) in enumerate(ch):
        segs.append(("M", [("v", j) for j in range(n_vits)] if c == 0 else None, ("f", c), None))
        segs.append(("H", ("f", c), ("end", 0) if c == len(ch) - 1 else None, None))
    return segs


def _spec_trainer(lch, nb, ranges):
    segs = []
    for c, (lo, hi) in enumerate(lch):
        segs.append(("M", None, ("f", c), None))
        segs.append(("H", ("f", c), None, None))
    n_forward = len(segs)
    for k, (lo, hi) in enumerate(reversed(lch)):
        wait = None
        if min(hi, nb) > lo:
            segs.append(("H", None, ("b", k), None))
            wait = ("b", k)
        segs.append(("M", wait, ("m", k), None))
        segs.append(("G", ("m", k), ("g", k), ranges(lo, hi - 1)))
    return segs, n_forward


class _Head:
    """Stub action head with nb blocks: logs (name, args)."""

    def __init__(self, nb, log):
        self.nb, self.log = nb, log

    def fwd_begin(self, *args):
        self.log.append(("fwd_begin", args))

    def refresh_transposes(self):
        self.log.append(("refresh_transposes", ()))

    def fwd_layer(self, i):
        self.log.append(("fwd_layer", (i,)))

    def bwd_layer(self, i, dhs):
        assert dhs == "dHS"
        self.log.append(("bwd_layer", (i,)))


def _shape(segs):
    return [(sg.stream, sg.wait, sg.signal, sg.ranges) for sg in segs]


def _ranges(lo, hi):
    return [("grad", lo, hi)]


def _build(kind, ch, nb, log):
    """-> (forward half, backward half) as the caller of that kind asks for them, every callback logging (name, args)."""
    head = _Head(nb, log)
    cb = lambda name: lambda *a: log.append((name, a))
    args = lambda: ("HS", "pos1", "proprio", "Np", "noise")
    if kind == "predict":
        return pipeline_forward(head, ch, cb("llm_fwd"), args, cb("at_end"), wait=[("v", 0), ("v", 1)], signal=("end", 0)), []
    fwd = pipeline_forward(head, ch, cb("llm_fwd"), args, cb("at_end"), refresh=True)
    handover = (lambda k, lo, hi: Segment("G", cb("flush"), ("m", k), ("g", k), _ranges(lo, hi - 1))) if kind == "trainer" else None
    return fwd, pipeline_backward(head, ch, cb("llm_bwd"), lambda: "dHS", handover)


def test_pipeline_segments_written_out():
    """One case of each form, the tiny two-layer stack: forward half, forward-only half, backward half, backward half with
    the trainers' hand-overs."""
    ch = [(0, 1), (1, 2)]
    assert turnaround_chunks(2, 4, [2, 1, 1], 1) == ch == turnaround_chunks(2, 6, [4, 2], 1)
    fwd, bwd = _build("step", ch, 2, [])
    assert _shape(fwd) == [("M", None, ("f", 0), None), ("H", ("f", 0), None, None),
                           ("M", None, ("f", 1), None), ("H", ("f", 1), None, None)]
    assert _shape(bwd) == [("H", None, ("b", 0), None), ("M", ("b", 0), None, None),
                           ("H", None, ("b", 1), None), ("M", ("b", 1), None, None)]
    assert _shape(_build("predict", ch, 2, [])[0]) == [("M", [("v", 0), ("v", 1)], ("f", 0), None), ("H", ("f", 0), None, None),
                                                       ("M", None, ("f", 1), None), ("H", ("f", 1), ("end", 0), None)]
    assert turnaround_chunks(2, 1, [2, 1, 1], 1) == ch
    fwd, bwd = _build("trainer", ch, 2, [])
    assert _shape(fwd) == [("M", None, ("f", 0), None), ("H", ("f", 0), None, None),
                           ("M", None, ("f", 1), None), ("H", ("f", 1), None, None)]
    assert _shape(bwd) == [("H", None, ("b", 0), None), ("M", ("b", 0), ("m", 0), None), ("G", ("m", 0), ("g", 0), [("grad", 1, 1)]),
                           ("H", None, ("b", 1), None), ("M", ("b", 1), ("m", 1), None), ("G", ("m", 1), ("g", 1), [("grad", 0, 0)])]


@pytest.mark.parametrize("n", [24, 8, 2])
def test_pipeline_segments_equal_the_three_hand_written_lists(n):
    fwd, bwd = _build("step", turnaround_chunks(n, 4, [2, 1, 1], 1), n, [])
    assert _shape(fwd + bwd) == _spec_step(_spec_chunks("step", n))
    fwd, _ = _build("predict", turnaround_chunks(n, 6, [4, 2], 1), n, [])
    assert _shape(fwd) == _spec_predict(_spec_chunks("predict", n), 2)
    for el in (4, 2):
        fwd, bwd = _build("trainer", turnaround_chunks(n, el, [2, 1, 1], el), n, [])
        spec, n_forward = _spec_trainer(_spec_chunks("trainer", n, el), n, _ranges)
        assert _shape(fwd + bwd) == spec and len(fwd) == n_forward


@pytest.mark.parametrize("kind", ["step", "predict", "trainer"])
@pytest.mark.parametrize("n,nb", [(24, 24), (8, 8), (2, 2), (28, 24)])
def test_pipeline_calls_in_list_order(kind, n, nb):
    """Run in list order, the segments call the head's blocks 0 .. nb - 1 upwards and downwards, once each, between one
    fwd_begin and one at_end - also when the chunks reach above the head's last block (n = 28, nb = 24)."""
    ch = {"step": turnaround_chunks(n, 4, [2, 1, 1], 1), "predict": turnaround_chunks(n, 6, [4, 2], 1),
          "trainer": turnaround_chunks(n, 4, [2, 1, 1], 4)}[kind]
    log = []
    fwd, bwd = _build(kind, ch, nb, log)
    segs = fwd + bwd
    for sg in segs:
        sg.fn()
    names = [name for name, _ in log]
    head_calls = [(name, a) for name, a in log if name in ("fwd_begin", "refresh_transposes", "fwd_layer", "at_end", "bwd_layer")]
    first = [("fwd_begin", ("HS", "pos1", "proprio", "Np", "noise"))] + [("refresh_transposes", ())] * (kind != "predict")
    assert head_calls == (first + [("fwd_layer", (i,)) for i in range(nb)] + [("at_end", ())]
                          + ([] if kind == "predict" else [("bwd_layer", (i,)) for i in reversed(range(nb))]))
    assert log[0] == ("llm_fwd", (0,) + ch[0]) and log[1][0] == "fwd_begin"          # the head begins behind the first LLM chunk
    assert [a for name, a in log if name == "llm_fwd"] == [(c, lo, hi) for c, (lo, hi) in enumerate(ch)]
    assert names.index("at_end") > max(i for i, name in enumerate(names) if name == "llm_fwd")
    if kind != "predict":
        assert [a for name, a in log if name == "llm_bwd"] == [(k, lo, hi) for k, (lo, hi) in enumerate(reversed(ch))]
        for k, (lo, hi) in enumerate(reversed(ch)):           # a layer's backward runs behind the head blocks that feed it
            at = log.index(("llm_bwd", (k, lo, hi)))
            assert all(log.index(("bwd_layer", (i,))) < at for i in range(lo, min(hi, nb)))
        m_segs = [sg for sg in bwd if sg.stream == "M"]
        for k, (lo, hi) in enumerate(reversed(ch)):           # chunks above the head: no "H" segment, the "M" segment waits for nothing
            assert (("b", k) in [sg.signal for sg in bwd]) == (lo < nb)
            assert m_segs[k].wait == (("b", k) if lo < nb else None)
        assert sum(sg.stream == "H" for sg in bwd) == sum(lo < nb for lo, _ in ch)
    # every wait key is the signal of an earlier segment (what schedule.run relies on); predict's vision events come from its caller
    seen = {("v", 0), ("v", 1)} if kind == "predict" else set()
    for sg in segs:
        for w in ([] if sg.wait is None else sg.wait if isinstance(sg.wait, list) else [sg.wait]):
            assert w in seen, (w, sg)
        seen.add(sg.signal)


def test_pipeline_above_the_head_emits_the_trainers_rule():
    """n = 28 layers over nb = 24 blocks in uniform four-layer chunks: the top chunk (24, 28) has no head work at all."""
    ch = chunks(28, [4])
    log = []
    fwd, bwd = _build("trainer", ch, 24, log)
    spec, n_forward = _spec_trainer(ch, 24, _ranges)
    assert _shape(fwd + bwd) == spec and len(fwd) == n_forward
    assert _shape(bwd)[:2] == [("M", None, ("m", 0), None), ("G", ("m", 0), ("g", 0), [("grad", 24, 27)])]
    for sg in fwd + bwd:
        sg.fn()
    assert all(a[0] < 24 for name, a in log if name in ("fwd_layer", "bwd_layer"))


def test_turnaround_chunks_equals_the_three_inline_rules():
    for n in range(1, 41):
        assert turnaround_chunks(n, 4, [2, 1, 1], 1) == _spec_chunks("step", n)
        assert turnaround_chunks(n, 6, [4, 2], 1) == _spec_chunks("predict", n)
        for el in (1, 2, 4, 7):
            assert turnaround_chunks(n, el, [2, 1, 1], el) == _spec_chunks("trainer", n, el)


# ---- gradient accumulation ----------------------------------------------------------------------------------------------------
def test_grad_accumulator_folds_three_micro_steps_in_bf16():
    calls = []
    copy = lambda dst, src: (calls.append("copy"), dst.copy_(src))
    add = lambda dst, src: (calls.append("add"), dst.add_(src))
    gen = torch.Generator().manual_seed(0)
    micro = [[torch.randn(257, generator=gen).to(torch.bfloat16), torch.randn(33, generator=gen).to(torch.bfloat16)] for _ in range(3)]
    grads = [torch.zeros(257, dtype=torch.bfloat16), torch.zeros(33, dtype=torch.bfloat16)]
    acc = GradAccumulator(copy, add)
    assert acc.ga == 1 and acc.fold() is True and calls == []          # ga == 1 touches nothing
    acc.reset(3, grads)
    assert acc.ga == 3
    for rounds in range(2):                                            # the counter resets: the second round folds like the first
        want = []
        for j in range(2):
            w = micro[0][j].clone()
            w += micro[1][j]
            w += micro[2][j]
            want.append(w)
        done = []
        for m in micro:
            for g, src in zip(grads, m):
                g.copy_(src)
            done.append(acc.fold())
        assert done == [False, False, True]
        assert all(torch.equal(g, w) for g, w in zip(grads, want))
    assert calls == (["copy"] * 2 + ["add"] * 4 + ["copy"] * 2) * 2
    acc.reset(1, grads)
    before, n_calls = [g.clone() for g in grads], len(calls)
    assert acc.fold() is True and len(calls) == n_calls and all(torch.equal(g, b) for g, b in zip(grads, before))
