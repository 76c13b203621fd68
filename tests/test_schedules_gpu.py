"""Step schedules against the serial step, bit for bit.

The training step runs as up to four concurrent streams (trainers.BackboneTrainer._segments: M the dX chain, G gradient-only work
and the range-by-range AdamW, H the action head, V the second vision backbone), eagerly or as one hipGraph per segment; the
adapter-only engine as two (engine.VLAEngine._segments: LLM and head) plus the vision lead of the captured step.  Every schedule
runs the same kernels on the same data, so after several optimiser steps every loss, parameter and AdamW moment must equal the
single-stream eager step's BITS: a missing event or a scratch buffer shared between two streams gives no error, only slightly
different numbers, and a tolerance would hide it.  Bit-identity holds because no kernel on these steps adds with a float atomic
in an order that depends on timing (the L1 objective's reductions are fixed-order since the reproducible-step work).

Where a schedule changes the arithmetic by design this file says so instead of comparing: the ungrouped weight-gradient products
(gemm_tn with automatic split, taken when no gradient stream exists or VLA_NO_GROUPED_TN is set) split their contraction over
the rows once a product has >= 1024 rows and few tiles, and meet the slices in an fp32 workspace - another association than
the grouped launch (vla_gemm_bf16_tn_grouped, never split).  The batches here keep every product below 1024 rows, so that all
schedules are compared, not excused.

A race only shows up in a bit comparison when the two streams really overlap in time, which at plumbing size they may not;
test_trainer_scratch_has_one_owner_stream checks ownership of the trainer's per-shape scratch deterministically instead."""
import gc
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))

DEV, BF = "cuda", torch.bfloat16
KNOBS = ("VLA_TRAINER_STREAMS", "VLA_SERIAL_BACKBONES", "VLA_NO_UPDATE_OVERLAP", "VLA_NO_GROUPED_TN", "VLA_UNIFORM_CHUNKS",
         "VLA_FWD_CHUNKS", "VLA_VIS_AFTER", "VLA_HEAD_ATTN_VALU", "VLA_NO_SPLITK")
LR = 1e-3


@pytest.fixture(autouse=True)
def _collect_cycles():
    """Every case leaves trainers / engines with captured graphs in reference cycles: collect them here, between cases."""
    yield
    gc.collect()


def _cfg(geom):
    from vla_adapter_amd import engine as E
    if geom == "tiny":
        return E.tiny_config()
    if geom == "tiny_fused":
        return E.tiny_fused_config()
    if geom == "twin":
        return E.tiny_twin_config()
    assert geom == "deep"        # 8 LLM layers under 8 head blocks: the 4/2/1/1 chunking differs from uniform chunks (n_active >= 8)
    c = E.tiny_config()
    c.llm = E.LLMCfg(256, 8, 4, 2, 64, 512, 1e-6, 1e6, 1024)
    c.num_blocks = 8
    return c


def _env(monkeypatch, sched):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in sched.items():
        monkeypatch.setenv(k, v)


def _batch(cfg, B):
    from vla_adapter_amd import synthetic as S
    return S.make_batch(cfg, B, DEV, seed=70 + B, P=20, ragged=True)


def _trainer(cfg, mode):
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.trainers import FullFinetune, LoRAFinetune
    eng = E.VLAEngine(cfg, S.make_weights(cfg, DEV, seed=5, std=0.05), DEV)
    if mode == "full":
        return FullFinetune(eng)
    tr = LoRAFinetune(eng, rank=16, seed=2, fp8=mode == "lora_fp8", dropout=0.1 if mode == "lora_drop" else 0.0)
    g = torch.Generator(device=DEV).manual_seed(9)          # B = 0 at init: give both branches of every pair signal from step 1
    for l in tr.L.values():
        for p, _ in l.projs:
            Bv = tr.P.view(f"{l.name}.{p}.lora_B")
            Bv[:l.n_real, :l.r] = (torch.randn(min(l.n_real, Bv.shape[0]), l.r, generator=g, device=DEV) * 0.02).to(BF)
    tr.refresh()
    return tr


def _trainer_state(tr, losses):
    torch.cuda.synchronize()
    return dict(losses=torch.stack(losses).cpu(), P=tr.P.data.clone(), m=tr.P.m.clone(), v=tr.P.v.clone(),
                hP=tr.head.P.data.clone(), hm=tr.head.P.m.clone(), hv=tr.head.P.v.clone())


def _run_trainer(cfg, mode, batch, captured):
    """Four optimiser steps -> (trainer, state after step 2, state after step 4).  Eager: four eager steps.  Captured: two eager
    steps, then capture() and two replays (the warm-up forwards of capture() bump lora_dropout's mask counter; it is put back, so
    that step k draws the masks of step k in both runs)."""
    tr = _trainer(cfg, mode)
    losses = [tr.train_step(batch, LR).clone() for _ in range(2)]
    mid = _trainer_state(tr, losses)
    if captured:
        ctr = tr._drop_step.clone() if mode == "lora_drop" else None
        tr.capture(batch, None)
        if ctr is not None:
            tr._drop_step.copy_(ctr)
        losses += [tr.train_step_graphed(LR).clone() for _ in range(2)]
    else:
        losses += [tr.train_step(batch, LR).clone() for _ in range(2)]
    return tr, mid, _trainer_state(tr, losses)


def _assert_same(ref, got, what):
    for k in ref:
        if k == "losses":
            assert torch.equal(ref[k], got[k]), f"{what}: loss triples differ\n{ref[k]}\n{got[k]}"
        else:
            assert torch.equal(ref[k], got[k]), \
                f"{what}: {k} differs at {int((ref[k] != got[k]).sum())} of {ref[k].numel()} elements"


_REF = {}


def _trainer_ref(monkeypatch, geom, mode, B):
    key = (geom, mode, B)
    if key not in _REF:
        _env(monkeypatch, {"VLA_TRAINER_STREAMS": "1"})
        cfg = _cfg(geom)
        tr, mid, end = _run_trainer(cfg, mode, _batch(cfg, B), captured=False)
        assert tr.gstream is None and tr.hstream is None and tr.vstream is None
        _REF[key] = (mid, end)
        del tr
    return _REF[key]


SCHED = {
    "streams1": {"VLA_TRAINER_STREAMS": "1"},           # (captured only: the eager one-stream step IS the reference)
    "streams2": {"VLA_TRAINER_STREAMS": "2"},
    "streams3": {},
    "serial_backbones": {"VLA_SERIAL_BACKBONES": "1"},
    "no_update_overlap": {"VLA_NO_UPDATE_OVERLAP": "1"},
    "no_grouped_tn": {"VLA_NO_GROUPED_TN": "1"},
    "uniform_chunks": {"VLA_UNIFORM_CHUNKS": "1"},
}
# Pruned matrix.  VLA_SERIAL_BACKBONES only differs with two backbones (tiny_fused, twin); VLA_UNIFORM_CHUNKS only once
# n_active >= 8 or a backbone has >= 14 blocks (deep).  fp8 needs contraction lengths that are multiples of 128: the twin ViTs
# and the 256-wide LLM (tiny_fused's 192-wide backbone would stay bf16, so fp8 runs on twin and deep).  lora_dropout runs on
# twin (the geometry whose two backbones share shapes) and deep (its own masks on every LLM pair); LoRA bf16 on deep is the fp8
# case's schedule without the quantisation.
_MODES = {"tiny_fused": ("full", "lora"), "twin": ("full", "lora", "lora_drop", "lora_fp8"), "deep": ("full", "lora_fp8", "lora_drop")}
_SCHEDS = {"tiny_fused": ("streams1", "streams2", "streams3", "serial_backbones", "no_update_overlap", "no_grouped_tn"),
           "twin": ("streams1", "streams2", "streams3", "serial_backbones", "no_update_overlap", "no_grouped_tn"),
           "deep": ("streams1", "streams2", "streams3", "no_update_overlap", "no_grouped_tn", "uniform_chunks")}
CASES = [(g, m, s, 2) for g in _MODES for m in _MODES[g] for s in _SCHEDS[g]]
# batch 8 (from which the engine once ran the LLM forward as two half-batch pipelines): the race-prone twin geometry on the
# default schedule, 8 x (32 + 84) = 928 rows per LLM product - below the ungrouped products' split (see top)
CASES += [("twin", m, "streams3", 8) for m in ("full", "lora_fp8", "lora_drop")]


@pytest.mark.parametrize("geom,mode,sched,B", CASES, ids=[f"{g}-{m}-{s}-B{b}" for g, m, s, b in CASES])
def test_trainer_schedule_equals_the_serial_step(geom, mode, sched, B, monkeypatch):
    """Two eager steps, then two replays of the captured step, on the schedule under test == four eager steps of the one-stream
    schedule: loss triples of every step, trainable parameters, head parameters and AdamW moments after steps 2 and 4."""
    ref_mid, ref_end = _trainer_ref(monkeypatch, geom, mode, B)
    _env(monkeypatch, SCHED[sched])
    cfg = _cfg(geom)
    tr, mid, end = _run_trainer(cfg, mode, _batch(cfg, B), captured=True)
    if mode == "lora_fp8":
        fk, bk = tr.fp8_keys()
        assert fk and bk and (geom != "twin" or any(k.startswith("vit1.") for k in fk)), "the fp8 base products must engage"
    if sched in ("streams3", "no_update_overlap", "no_grouped_tn"):
        assert (tr.vstream is not None) == (len(cfg.vit) == 2)
    _assert_same(ref_mid, mid, f"{geom}/{mode}/{sched}/B{B} after two eager steps")
    _assert_same(ref_end, end, f"{geom}/{mode}/{sched}/B{B} after two captured steps")


# ---- ownership of the trainer's scratch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["lora_fp8", "lora_drop"])
def test_trainer_scratch_has_one_owner_stream(mode, monkeypatch):
    """Timing-independent race check on the twin geometry with every stream on: during an eager step, and while the step is
    captured, every buffer of LoRAFinetune's per-shape scratch (_qscratch: fp8 row codes / scales, _uscratch: lora_dropout's u / h),
    the norm -> quantise hand-over (_xq) and the per-stream kernel scratch (scratch.ARENA.get: split-K and TN planes, head-backward
    partials, digest sums) is used from ONE stream only.  The only cross-stream edges inside a step are the segment events, and none
    of them orders two uses of one of these buffers - so a second stream is a race, whether or not the streams happened to overlap.
    The capture allocates no scratch: every capture stream's buffer was reserved before its capture began (the arena's
    under-capture counter does not move)."""
    from vla_adapter_amd.scratch import ARENA
    _env(monkeypatch, {})
    cfg = _cfg("twin")
    batch = _batch(cfg, 2)
    tr = _trainer(cfg, mode)
    assert tr.vstream is not None and tr.gstream is not None and tr.hstream is not None
    if mode == "lora_fp8":
        assert any(k.startswith("vit0.") for k in tr.Q) and any(k.startswith("vit1.") for k in tr.Q), sorted(tr.Q)
    uses, phase = {}, ["?"]

    gc_during_capture = []

    def record(what, tensors):
        where = torch.cuda.current_stream().cuda_stream
        ph = "capture" if torch.cuda.is_current_stream_capturing() else phase[0]
        if ph == "capture":
            gc_during_capture.append(gc.isenabled())
        for t in tensors:
            uses.setdefault(ph, {}).setdefault((what, t.data_ptr()), set()).add(where)

    q0, u0, quant0, ws0, run0 = tr._qscratch, tr._uscratch, tr._quant, ARENA.get, tr._run

    def qscratch(rows, cols, slot):
        b = q0(rows, cols, slot)
        record("_qscratch", b)
        return b

    def uscratch(rows, cols, slot):
        b = u0(rows, cols, slot)
        record("_uscratch", (b,))
        return b

    def quant(x, slot):
        hand_over = tr._xq is not None and tr._xq[0] == (x.data_ptr(), tuple(x.shape))
        out = quant0(x, slot)
        if hand_over:
            record("_xq", out)
        return out

    def scratch(nbytes, device):
        ws = ws0(nbytes, device)
        record("scratch", (ws,))
        return ws

    def run(*a, **k):
        phase[0] = f"step {tr.step_count}"
        return run0(*a, **k)
    monkeypatch.setattr(tr, "_qscratch", qscratch)
    monkeypatch.setattr(tr, "_uscratch", uscratch)
    monkeypatch.setattr(tr, "_quant", quant)
    monkeypatch.setattr(ARENA, "get", scratch)
    monkeypatch.setattr(tr, "_run", run)
    tr.train_step(batch, LR)
    under_capture = ARENA.under_capture
    tr.capture(batch, None)
    assert ARENA.under_capture == under_capture, "scratch was allocated while the step was captured"
    tr.train_step_graphed(LR)
    torch.cuda.synchronize()
    kinds = {w for ph in uses.values() for (w, _) in ph}
    want = {"_qscratch", "_xq", "scratch"} if mode == "lora_fp8" else {"_uscratch", "scratch"}
    assert want <= kinds, (want, kinds)
    assert "capture" in uses and len(uses) >= 2, sorted(uses)
    shared = [(ph, w, len(s)) for ph, d in uses.items() for (w, _), s in d.items() if len(s) > 1]
    assert not shared, f"scratch used from two streams within one step (phase, buffer kind, streams): {shared}"
    assert gc_during_capture and not any(gc_during_capture), "the cyclic GC must be paused while the step is captured (schedule.graph_capture)"


# ---- the head backward's gate reduction ---------------------------------------------------------------------------------------
def test_no_schedule_reaches_the_atomic_gate_reduction(monkeypatch):
    """The gate gradient of the action head's attention is summed in a fixed order on the MFMA backward (head_bwd_tiles +
    head_dq_reduce), the only backward head_attn_mfma.hip has: the library refuses a call at an MFMA width without the full workspace
    (test_head_attention_bwd_requires_workspace), so nothing about the workspace is left to check here.  The VALU backward
    (head_attn.hip: head dims the MFMA kernels do not cover, or VLA_HEAD_ATTN_VALU) still adds per-wave partials with atomicAdd.  No
    trainer or engine schedule reaches it: every head width of the shipped geometries is an MFMA one, T <= 32, and the training
    schedules never set the switch.  Pinned here on every head backward of a LoRA trainer step and an adapter-only step, eager and
    captured, at the geometries of this file."""
    from vla_adapter_amd import engine as E, ops
    _env(monkeypatch, {})
    calls = []
    bwd0 = ops.head_attn_bwd

    def head_attn_bwd(*a, **k):
        H = a[19] if len(a) > 19 else k.get("H", 8)
        B, T, D = a[0].shape
        calls.append((D // H, T))
        if torch.cuda.is_current_stream_capturing():
            gc_during_capture.append(gc.isenabled())
        return bwd0(*a, **k)
    gc_during_capture = []
    monkeypatch.setattr(ops, "head_attn_bwd", head_attn_bwd)
    for geom in ("tiny", "twin", "deep"):
        cfg = _cfg(geom)
        batch = _batch(cfg, 2)
        tr = _trainer(cfg, "lora")
        tr.train_step(batch, LR)
        tr.capture(batch, None)
        tr.train_step_graphed(LR)
        e = E.VLAEngine(cfg, _trainer_weights(cfg), DEV)
        e.train_step(batch, LR)
        e.capture({k: v.clone() for k, v in batch.items()}, None)
        e.train_step_graphed(LR)
        e.flush()
        torch.cuda.synchronize()
        del tr, e
    for c in E.NAMED_CONFIGS.values():                       # every shipped geometry's head width is an MFMA one
        D = c().llm.d
        assert D % 8 == 0 and D // 8 in (16, 32, 64, 112, 128, 192), (c.__name__, D)
    assert calls and all(dh in (16, 32, 64, 112, 128, 192) and 1 <= T <= 32 for dh, T in calls), set(calls)
    assert gc_during_capture and not any(gc_during_capture), "trainer and engine captures must pause the cyclic GC (schedule.graph_capture)"
    assert not os.environ.get("VLA_HEAD_ATTN_VALU")


def _trainer_weights(cfg):
    from vla_adapter_amd import synthetic as S
    return S.make_weights(cfg, DEV, seed=5, std=0.05)


# ---- the adapter-only engine --------------------------------------------------------------------------------------------------
def _engine_state(e, losses):
    torch.cuda.synchronize()
    P = e.head.P
    return dict(losses=torch.stack(losses).cpu(), P=P.data.clone(), g=P.grad.clone(), m=P.m.clone(), v=P.v.clone())


def _run_engine(cfg, batch, how):
    from vla_adapter_amd import engine as E
    e = E.VLAEngine(cfg, _trainer_weights(cfg), DEV)
    if how == "sequential":
        losses = [e.train_step(batch, LR).clone() for _ in range(3)]
    elif how == "pipelined":
        losses = [e.train_step_pipelined(batch, LR).clone() for _ in range(3)]
    else:
        e.capture({k: v.clone() for k, v in batch.items()}, None)
        losses = [e.train_step_graphed(LR).clone() for _ in range(3)]
        e.flush()
    return _engine_state(e, losses)


_EREF = {}
ENGINE_SCHED = {"default": {}, "chunks2_vis0": {"VLA_FWD_CHUNKS": "2", "VLA_VIS_AFTER": "0"},
                "chunks31_vis1": {"VLA_FWD_CHUNKS": "3,1", "VLA_VIS_AFTER": "1"}}
ENGINE_CASES = [(g, B, s) for g, B in (("tiny", 3), ("tiny", 8), ("deep", 3), ("twin", 3)) for s in ENGINE_SCHED]


@pytest.mark.parametrize("geom,B,sched", ENGINE_CASES, ids=[f"{g}-B{b}-{s}" for g, b, s in ENGINE_CASES])
def test_engine_schedule_equals_the_sequential_step(geom, B, sched, monkeypatch):
    """Adapter-only step: train_step (forward, loss, backward, AdamW one after the other on one stream) is the reference;
    train_step_pipelined (head beside the LLM on its own stream) and the captured step (segment graphs, vision lead of the next
    step, deferred update, flush()) must give the same loss triples, gradients, parameters and AdamW moments after three steps."""
    key = (geom, B)
    cfg = _cfg(geom)
    batch = _batch(cfg, B)
    if key not in _EREF:
        _env(monkeypatch, {})
        _EREF[key] = _run_engine(cfg, batch, "sequential")
    _env(monkeypatch, ENGINE_SCHED[sched])
    for how in ("pipelined", "captured"):
        _assert_same(_EREF[key], _run_engine(cfg, batch, how), f"engine {geom}/B{B}/{sched} {how}")


# ---- the adapter-only engine's one update -------------------------------------------------------------------------------------
UPDATE_CASES = {"unclipped": (None, 1), "clip1": (1.0, 1), "clip_inf": (float("inf"), 1), "ga2": (None, 2)}


@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_engine_update_is_one_through_optimizer_step_and_flush(case, monkeypatch):
    """VLAEngine._apply_update in its two placements, directly instead of through whole schedules: two engines from the same
    weights run the same eager two-stream forward + backward (_fwd_bwd) on the same batch and noise; one applies every update
    through optimizer_step() (both ranges on the current stream), the other leaves it pending the way train_step_graphed does
    (fold, the event of the summed gradient, _pending_lr) and applies it through flush() (head range on the head stream).  After
    each of three steps parameters, both AdamW moments and the step count are the same bits - and, clipped, the norm and the
    coefficient: the sums of squares land in the same slots whichever stream took them, and AdamW is elementwise."""
    from vla_adapter_amd import engine as E
    _env(monkeypatch, {})
    max_norm, ga = UPDATE_CASES[case]
    cfg = _cfg("tiny")
    batch = _batch(cfg, 2)
    noise = (torch.randn(cfg.chunk, cfg.action_dim * cfg.llm.d, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.02).to(BF)
    engines = [E.VLAEngine(cfg, _trainer_weights(cfg), DEV) for _ in range(2)]
    for e in engines:
        e.set_grad_accumulation(ga)
        e.set_max_grad_norm(max_norm)
        e._ensure_streams()
    direct, pending = engines
    cur, start = torch.cuda.current_stream(), direct.head.P.data.clone()
    assert torch.equal(start, pending.head.P.data)
    for step in range(1, 4):
        for _ in range(ga):
            for e in engines:
                e._fwd_bwd(batch, noise)
                if not e._accum.fold():
                    continue
                if e is direct:
                    e.optimizer_step(LR)
                    continue
                if ga > 1:                           # (train_step_graphed: the summed gradient is final on the current stream)
                    e._h_end = torch.cuda.Event()
                    e._h_end.record(cur)
                e._pending_lr = LR
                assert e.step_count == step - 1, "the update stays pending until flush()"
                e.flush()
        torch.cuda.synchronize()
        assert direct.step_count == pending.step_count == step
        for k in ("data", "m", "v"):
            a, b = getattr(direct.head.P, k), getattr(pending.head.P, k)
            assert torch.equal(a, b), f"{case} step {step}: P.{k} differs at {int((a != b).sum())} of {a.numel()} elements"
        if max_norm is None:
            assert direct.grad_norm is None and pending.clip_coef is None
        else:
            assert torch.isfinite(direct.grad_norm) and direct.grad_norm > 0
            assert torch.equal(direct.grad_norm, pending.grad_norm) and torch.equal(direct.clip_coef, pending.clip_coef), \
                f"{case} step {step}: norm {direct.grad_norm.item()!r} vs {pending.grad_norm.item()!r}"
    assert not torch.equal(direct.head.P.data, start), "the steps moved the parameters"
