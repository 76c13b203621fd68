"""--max_grad_norm on the GPU: the sum-of-squares pass against fp64, the finalise against torch.nn.utils.clip_grad_norm_, AdamW with
the device coefficient against the golden-pinned ops.adamw_, and the clipped step of both trainers and the adapter-only engine
on every schedule.

Bounds.  Sum of squares: fixed-order fp32 accumulation over at most 2^20 terms (8 per lane per 16-B group, 64 adds per lane, a
64-lane butterfly, four waves), combined in fp64, errs by about log2(n) 2^-24 < 2e-6 relative; the bound is 1e-5.  The norm is
its square root (half the relative error) rounded once to fp32 (2^-24): 1e-5 as well.  Everything else here is bit-identity."""
import gc
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV, BF, F32 = "cuda", torch.bfloat16, torch.float32
LR = 1e-3
KNOBS = ("VLA_TRAINER_STREAMS", "VLA_SERIAL_BACKBONES", "VLA_NO_UPDATE_OVERLAP", "VLA_NO_GROUPED_TN", "VLA_UNIFORM_CHUNKS",
         "VLA_FWD_CHUNKS", "VLA_VIS_AFTER")
NS = (1, 7, 8, 9, 4097, 65536 + 3, (1 << 20) + 5)
GSCALES = (1.0, 0.5, 1.0 / 3.0)


@pytest.fixture(autouse=True)
def _collect_cycles():
    yield
    gc.collect()


def _values(n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.rand(n, device=DEV, generator=g) * 8.0 - 4.0
    x[torch.randint(0, n, (min(n, 5),), device=DEV, generator=g)] = 1e3
    return x


def _consumed(g, gscale):
    """The value AdamW consumes, as torch forms it: an f32 gradient scaled in fp32 and rounded to bf16; a bf16 one scaled (fp32
    product, one rounding) only when a scale applies."""
    gscale = torch.tensor(gscale, dtype=F32).item()
    if g.dtype == F32:
        return (g * gscale).to(BF)
    return (g.float() * gscale).to(BF) if gscale != 1.0 else g


# ---- kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("offset", [0, 1, 5])
def test_sumsq_against_fp64(dtype, offset):
    """Slices at element offsets 0 / 1 / 5 of a NaN-filled buffer (a read outside the slice poisons the sum), every n and gscale:
    the slots add up to the fp64 sum of squares of the consumed values within 1e-5, and no slot beyond the count is written."""
    from vla_adapter_amd import ops
    for n in NS:
        buf = torch.full((offset + n + 13,), float("nan"), device=DEV, dtype=dtype)
        g = buf[offset:offset + n]
        g.copy_(_values(n, 100 + n % 97))
        k = ops.grad_sumsq_slots(n)
        for gscale in GSCALES:
            slots = torch.full((k + 9,), -7.0, device=DEV, dtype=F32)
            assert ops.grad_sumsq_(g, slots, gscale) == k
            truth = _consumed(g, gscale).double().square().sum().item()
            got = slots[:k].double().sum().item()
            rel = abs(got - truth) / truth
            print(f"sumsq {dtype} offset {offset} n {n} gscale {gscale:.4f}: slots {k} rel err {rel:.3e}")
            assert rel <= 1e-5, (n, gscale, got, truth)
            assert torch.equal(slots[k:], torch.full((9,), -7.0, device=DEV)), "slots beyond the returned count were written"
        again = torch.empty(k, device=DEV, dtype=F32)
        ops.grad_sumsq_(g, again, GSCALES[-1])
        assert torch.equal(again, slots[:k]), "the same gradients must give the same bits"


def _norm_of(g, max_norm, pieces=None):
    """(device out [2], slots) of the pass over g - as one slice or as consecutive pieces - and the finalise."""
    from vla_adapter_amd import ops
    pieces = pieces or [g.numel()]
    slots = torch.empty(sum(ops.grad_sumsq_slots(p) for p in pieces), device=DEV, dtype=F32)
    lo = s = 0
    for p in pieces:
        s += ops.grad_sumsq_(g[lo:lo + p], slots[s:])
        lo += p
    assert s == slots.numel() and lo == g.numel()
    return ops.grad_norm_finalise_(slots, max_norm, torch.zeros(2, device=DEV, dtype=F32))


def test_finalise_against_torch_clip_grad_norm():
    """torch.nn.utils.clip_grad_norm_ on fp32 copies of the gradients split into several tensors: total_norm within 1e-5; the
    coefficient is exactly 1.0f when the norm is below max_norm and when max_norm = inf, and torch's value when it clips."""
    pieces = [5, 4097, 70001, 8, 131072 + 3]
    g = _values(sum(pieces), 7).to(BF)
    params = [torch.nn.Parameter(torch.zeros(p, device=DEV)) for p in pieces]
    lo = 0
    for p, q in zip(params, pieces):
        p.grad = g[lo:lo + q].float()
        lo += q
    ref = torch.nn.utils.clip_grad_norm_(params, float("inf")).item()        # (max_norm = inf: nothing is scaled)
    for max_norm, clips in ((ref * 0.25, True), (ref * 4.0, False), (float("inf"), False)):
        out = _norm_of(g, max_norm, pieces).tolist()
        print(f"finalise max_norm {max_norm}: total_norm {out[0]!r} torch {ref!r} coef {out[1]!r}")
        assert abs(out[0] - ref) / ref <= 1e-5
        if clips:
            # clip_grad_norm_'s own expression on the fp32 norm (Tensor.__rtruediv__: reciprocal, then the product - each within
            # 2^-24 relative of exact, so two evaluations differ by at most 2^-22)
            want = torch.clamp(max_norm / (torch.tensor(out[0], device=DEV) + 1e-6), max=1.0).item()
            assert out[1] < 1.0 and abs(out[1] - want) <= 2.0 ** -22 * want, (out[1], want)
        else:
            assert out[1] == 1.0
    assert torch.equal(_norm_of(g, 1.0, pieces), _norm_of(g, 1.0, pieces))
    g[17] = float("nan")                             # non-finite input propagates, as with error_if_nonfinite=False
    bad = _norm_of(g, 1.0, pieces).tolist()
    assert bad[0] != bad[0] and bad[1] != bad[1]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("offset", [0, 1])
def test_clipped_adamw_against_adamw_on_scaled_gradients(dtype, offset):
    """ops.adamw_ (pinned to torch's golden) on g2 = bf16(float(bf16(g gscale)) coef), coef read back from the device, must equal
    the clipped entry on g bit for bit - n = 8 k + 3 at an aligned (16-B kernel + tail) and an odd (scalar kernel) offset; with
    coef = 1 the clipped entry is ops.adamw_ on g itself."""
    from vla_adapter_amd import ops
    n = 8 * 1031 + 3
    gen = torch.Generator(device=DEV).manual_seed(31 + offset)
    r = lambda scale: (torch.randn(offset + n, device=DEV, generator=gen) * scale)
    g_all = (r(0.05)).to(dtype)
    state = [r(0.5).to(BF), r(0.01).to(BF), (r(0.01) ** 2).to(BF)]
    g = g_all[offset:]
    for gscale in (1.0, 0.5):
        for max_norm in (0.37, float("inf")):
            out = _norm_of(g, max_norm)
            coef = out[1].item()
            assert (coef < 1.0) == (max_norm != float("inf"))
            a = [t.clone() for t in state]
            b = [t.clone() for t in state]
            ops.adamw_clipped_(a[0][offset:], g, a[1][offset:], a[2][offset:], out[1:2], 3, LR, gscale=gscale)
            if max_norm == float("inf"):
                ops.adamw_(b[0][offset:], g, b[1][offset:], b[2][offset:], 3, LR, gscale=gscale)
            else:
                g2 = (_consumed(g, gscale).float() * coef).to(BF)
                ops.adamw_(b[0][offset:], g2, b[1][offset:], b[2][offset:], 3, LR)
            for name, x, y in zip("pmv", a, b):
                assert torch.equal(x, y), f"{name} differs at {int((x != y).sum())} of {n} (gscale {gscale}, max_norm {max_norm})"
            assert not torch.equal(a[0], state[0])


# ---- trainers ------------------------------------------------------------------------------------------------------------------
def _env(monkeypatch, **kv):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in kv.items():
        monkeypatch.setenv(k, v)


def _cfg(geom):
    from vla_adapter_amd import engine as E
    cfg = E.tiny_config()
    if geom == "dead_layer":     # 3 LLM layers under 2 head blocks: the top layer and the final norm have no gradient (_adam_ranges)
        cfg.llm = E.LLMCfg(256, 3, 4, 2, 64, 512, 1e-6, 1e6, 1024)
        cfg.num_blocks = 2
    return cfg


def _trainer(cfg, mode, max_norm=None, ga=1):
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.trainers import FullFinetune, LoRAFinetune
    eng = E.VLAEngine(cfg, S.make_weights(cfg, DEV, seed=3, std=0.05), DEV)
    if mode == "full":
        tr = FullFinetune(eng)
    else:
        tr = LoRAFinetune(eng, rank=8, seed=1)
        gen = torch.Generator(device=DEV).manual_seed(9)      # B = 0 at init: give both halves of every pair a gradient from step 1
        for l in tr.L.values():
            for p, _ in l.projs:
                Bv = tr.P.view(f"{l.name}.{p}.lora_B")
                Bv[:l.n_real, :l.r] = (torch.randn(min(l.n_real, Bv.shape[0]), l.r, generator=gen, device=DEV) * 0.02).to(BF)
        tr.refresh()
    if ga > 1:
        tr.set_grad_accumulation(ga)
    if max_norm is not None:
        tr.set_max_grad_norm(max_norm)
    return tr


def _batch(cfg, seed=4):
    from vla_adapter_amd import synthetic as S
    return S.make_batch(cfg, 3, DEV, seed=seed, P=20, ragged=True)


def _state(tr):
    torch.cuda.synchronize()
    return dict(P=tr.P.data.clone(), m=tr.P.m.clone(), v=tr.P.v.clone(), hP=tr.head.P.data.clone(), hm=tr.head.P.m.clone(),
                hv=tr.head.P.v.clone())


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs at {int((a[k] != b[k]).sum())} of {a[k].numel()} elements"


def _flat_norm(tr):
    """fp64 norm of the flat gradient buffers over exactly what AdamW updates: _adam_ranges() and the head's buffer."""
    s = sum(tr.P.grad[lo:hi].double().square().sum() for lo, hi in tr._adam_ranges()) + tr.head.P.grad.double().square().sum()
    return s.sqrt().item()


_N0 = {}
CASES = [("tiny", "full"), ("tiny", "lora"), ("dead_layer", "full"), ("dead_layer", "lora")]   # (each mode has its own dead-layer _adam_ranges)
IDS = [f"{g}-{m}" for g, m in CASES]


def _first_norm(geom, mode, monkeypatch):
    """max_grad_norm = inf against the unclipped trainer with the un-overlapped update, two steps -> the norm of step 1."""
    if (geom, mode) not in _N0:
        _env(monkeypatch)
        cfg = _cfg(geom)
        batch = _batch(cfg)
        plain = _trainer(cfg, mode)
        plain.overlap_update = False
        assert plain.grad_norm is None
        l_plain = [plain.train_step(batch, LR).clone() for _ in range(2)]
        tr = _trainer(cfg, mode, float("inf"))
        l_inf, norms = [], []
        for _ in range(2):
            l_inf.append(tr.train_step(batch, LR).clone())
            norms.append(tr.grad_norm.item())
            assert tr.clip_coef.item() == 1.0
        _same(_state(plain), _state(tr), f"{geom}/{mode}: max_grad_norm=inf against the unclipped step")
        assert torch.equal(torch.stack(l_plain), torch.stack(l_inf))
        assert all(n == n and 0.0 < n < float("inf") for n in norms), norms
        _N0[(geom, mode)] = norms[0]
    return _N0[(geom, mode)]


@pytest.mark.parametrize("geom,mode", CASES, ids=IDS)
def test_trainer_inf_clips_nothing(geom, mode, monkeypatch):
    _first_norm(geom, mode, monkeypatch)


@pytest.mark.parametrize("geom,mode", CASES, ids=IDS)
def test_trainer_clipped_step_is_clipped_adamw_on_its_gradients(geom, mode, monkeypatch):
    """max_grad_norm = n0 / 4: per step grad_norm is the fp64 norm of the flat buffers over the AdamW ranges within 1e-5, the
    coefficient lies below 1, and parameters and moments equal clipped AdamW applied by hand to the step's gradients; what lies
    outside the AdamW ranges keeps its bits."""
    from vla_adapter_amd import ops
    n0 = _first_norm(geom, mode, monkeypatch)
    _env(monkeypatch)
    cfg = _cfg(geom)
    batch = _batch(cfg)
    tr = _trainer(cfg, mode, n0 / 4)
    assert tr.max_grad_norm == n0 / 4
    for step in (1, 2):
        before = _state(tr)
        tr.train_step(batch, LR)
        torch.cuda.synchronize()
        got, coef, want = tr.grad_norm.item(), tr.clip_coef.item(), _flat_norm(tr)
        print(f"{geom}/{mode} step {step}: grad_norm {got!r} fp64 {want!r} coef {coef!r} n0 {n0!r}")
        assert abs(got - want) / want <= 1e-5
        assert 0.0 < coef < 1.0
        if step == 1:
            assert got == n0, "the first step's norm does not depend on max_grad_norm"
        for (p, m, v), P, ranges in (((before["P"], before["m"], before["v"]), tr.P, tr._adam_ranges()),
                                     ((before["hP"], before["hm"], before["hv"]), tr.head.P, [(0, tr.head.P.numel)])):
            for lo, hi in ranges:
                ops.adamw_clipped_(p[lo:hi], P.grad[lo:hi], m[lo:hi], v[lo:hi], tr.clip_coef, step, LR)
        _same(before, _state(tr), f"{geom}/{mode} step {step}: the trainer against clipped AdamW by hand")


@pytest.mark.parametrize("geom,mode", [("tiny", "full"), ("tiny", "lora")], ids=["tiny-full", "tiny-lora"])
def test_trainer_clipped_step_is_the_same_on_every_schedule(geom, mode, monkeypatch):
    """Clipping active: one stream against three streams, eager against captured - parameters, moments and grad_norm bit for bit."""
    n0 = _first_norm(geom, mode, monkeypatch)
    res = {}
    for name, streams, captured in (("streams1", "1", False), ("streams3", "3", False), ("streams3-captured", "3", True),
                                    ("streams1-captured", "1", True)):
        _env(monkeypatch, VLA_TRAINER_STREAMS=streams)
        cfg = _cfg(geom)
        batch = _batch(cfg)
        tr = _trainer(cfg, mode, n0 / 4)
        assert (tr.gstream is None) == (streams == "1")
        if captured:
            tr.capture(batch, None)
        norms = []
        for _ in range(2):
            tr.train_step_graphed(LR) if captured else tr.train_step(batch, LR)
            norms.append(tr.grad_norm.clone())
        st = _state(tr)
        st["norms"] = torch.stack(norms)
        res[name] = st
        assert float(tr.clip_coef) < 1.0
        del tr
    for name in res:
        _same(res["streams1"], res[name], f"{geom}/{mode}: {name} against the eager one-stream step")


@pytest.mark.parametrize("mode", ["full", "lora"])
def test_gradient_accumulation_takes_the_norm_of_the_folded_sums(mode, monkeypatch):
    from vla_adapter_amd import ops
    _env(monkeypatch)
    cfg = _cfg("tiny")
    b1, b2 = _batch(cfg, 4), _batch(cfg, 5)
    tr = _trainer(cfg, mode, 0.01, ga=2)
    before = _state(tr)
    tr.train_step(b1, LR)
    assert tr.step_count == 0
    tr.train_step(b2, LR)
    torch.cuda.synchronize()
    assert tr.step_count == 1
    got, want = tr.grad_norm.item(), _flat_norm(tr)          # (the gradient buffers hold the folded sums after the boundary step)
    print(f"ga=2 {mode}: grad_norm {got!r} fp64 norm of the folded sums {want!r} coef {tr.clip_coef.item()!r}")
    assert abs(got - want) / want <= 1e-5 and tr.clip_coef.item() < 1.0
    for (p, m, v), P, ranges in (((before["P"], before["m"], before["v"]), tr.P, tr._adam_ranges()),
                                 ((before["hP"], before["hm"], before["hv"]), tr.head.P, [(0, tr.head.P.numel)])):
        for lo, hi in ranges:
            ops.adamw_clipped_(p[lo:hi], P.grad[lo:hi], m[lo:hi], v[lo:hi], tr.clip_coef, 1, LR)
    _same(before, _state(tr), f"ga=2 {mode}: one clipped update on the sums")


# ---- adapter-only engine -----------------------------------------------------------------------------------------------------------
def _engine(cfg, max_norm=None):
    from vla_adapter_amd import engine as E, synthetic as S
    e = E.VLAEngine(cfg, S.make_weights(cfg, DEV, seed=3, std=0.05), DEV)
    if max_norm is not None:
        e.set_max_grad_norm(max_norm)
    return e


def _estate(e):
    torch.cuda.synchronize()
    P = e.head.P
    return dict(P=P.data.clone(), m=P.m.clone(), v=P.v.clone())


def test_engine_clipping(monkeypatch):
    """VLAEngine: inf == the unclipped step bit for bit; n0 / 4: grad_norm is the fp64 norm of head.P.grad (action queries
    included) within 1e-5, coef < 1, parameters equal clipped AdamW by hand; the pipelined and the captured step (deferred update,
    flush()) give the eager clipped step's bits."""
    from vla_adapter_amd import ops
    _env(monkeypatch)
    cfg = _cfg("tiny")
    batch = _batch(cfg)
    plain, inf = _engine(cfg), _engine(cfg, float("inf"))
    assert plain.grad_norm is None
    lp = [plain.train_step(batch, LR).clone() for _ in range(2)]
    li, norms = [], []
    for _ in range(2):
        li.append(inf.train_step(batch, LR).clone())
        norms.append(inf.grad_norm.item())
        assert inf.clip_coef.item() == 1.0
    _same(_estate(plain), _estate(inf), "engine: max_grad_norm=inf against the unclipped step")
    assert torch.equal(torch.stack(lp), torch.stack(li))
    n0 = norms[0]
    e = _engine(cfg, n0 / 4)
    enorms = []
    for step in (1, 2):
        before = _estate(e)
        e.train_step(batch, LR)
        torch.cuda.synchronize()
        P = e.head.P
        got, coef, want = e.grad_norm.item(), e.clip_coef.item(), P.grad.double().square().sum().sqrt().item()
        print(f"engine step {step}: grad_norm {got!r} fp64 {want!r} coef {coef!r}")
        assert abs(got - want) / want <= 1e-5 and 0.0 < coef < 1.0
        aq = P.offsets["action_queries"][0]
        assert P.grad[aq:].float().abs().max().item() > 0.0, "the action queries' gradient is part of the norm"
        ops.adamw_clipped_(before["P"], P.grad, before["m"], before["v"], e.clip_coef, step, LR)
        _same(before, _estate(e), f"engine step {step}: against clipped AdamW by hand")
        enorms.append(e.grad_norm.clone())
    ref = dict(_estate(e), norms=torch.stack(enorms))
    for how in ("pipelined", "captured"):
        e2 = _engine(cfg, n0 / 4)
        got = []
        if how == "captured":
            e2.capture({k: v.clone() for k, v in batch.items()}, None)
        for _ in range(2):
            if how == "captured":
                e2.train_step_graphed(LR)
                e2.flush()
            else:
                e2.train_step_pipelined(batch, LR)
            got.append(e2.grad_norm.clone())
        _same(ref, dict(_estate(e2), norms=torch.stack(got)), f"engine {how} clipped step against the eager one")


# ---- two ranks, entry point --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,captured", [("full", "0"), ("lora", "1"), ("adapter", "1")])
def test_two_gloo_ranks_report_the_same_norm(mode, captured):
    """Two gloo ranks on one GPU (tools/ddp_rehearsal_grad_clip.py): every rank takes the norm of the same averaged gradients - the
    same grad_norm bit for bit, a coefficient below 1, identical parameters at the end - with no collective added."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, VLA_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", VLA_TRAINER=mode, VLA_CAPTURED=captured)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), os.path.join("tools", "ddp_rehearsal_grad_clip.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("grad-clip-ranks-in-sync-ok") == 2, r.stdout[-3000:]


@pytest.mark.parametrize("extra", [["--use_fz", "True"], ["--use_lora", "True", "--lora_rank", "8"]], ids=["adapter", "lora"])
def test_finetune_logs_grad_norm(extra, tmp_path):
    """finetune(...) with max_grad_norm logs a finite grad_norm on every logged step (captured step, the adapter-only engine's
    deferred update included); without it the log has no such key."""
    import math
    from vla_adapter_amd import engine as E, finetune as F, synthetic as S
    batches = [S.make_batch(E.tiny_config(), 4, "cuda", seed=810 + i, P=24, ragged=True) for i in range(2)]
    args = ["--tiny", "true", "--batch_size", "4", "--max_steps", "3", "--learning_rate", "1e-3", "--wandb_log_freq", "1", "--save_freq", "100",
            "--run_root_dir", str(tmp_path), "--phase", "Inference", "--use_proprio", "True"] + extra
    on = F.finetune(F.parse_args(args + ["--max_grad_norm", "1.0", "--run_id_override", "on"]), batches=batches)["log"]
    assert len(on) >= 3 and all(math.isfinite(r["grad_norm"]) and r["grad_norm"] > 0.0 for r in on), on
    assert len({r["grad_norm"] for r in on}) > 1, "every logged step carries its own norm"
    assert all(r["grad_norm"] not in (r["loss_value"], r["curr_action_l1_loss"], r["next_actions_l1_loss"]) for r in on), on
    # the norm is taken before clipping: the first step's does not depend on max_grad_norm, the later ones follow the clipped updates
    inf = F.finetune(F.parse_args(args + ["--max_grad_norm", "inf", "--run_id_override", "inf"]), batches=batches)["log"]
    assert inf[0]["grad_norm"] == on[0]["grad_norm"] > 1.0 and inf[-1]["grad_norm"] != on[-1]["grad_norm"], (on, inf)
    off = F.finetune(F.parse_args(args + ["--run_id_override", "off"]), batches=batches)["log"]
    assert len(off) == len(on) and all("grad_norm" not in r for r in off)
    assert [r["loss_value"] for r in inf] == [r["loss_value"] for r in off], "max_grad_norm = inf trains as the unclipped run does"
