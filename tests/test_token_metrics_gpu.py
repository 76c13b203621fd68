"""Token-CE training metrics (prismatic/training/strategies/base_strategy.py:316-356): vla_token_ce_metrics - the loss of
vla_token_ce plus, for the action rows, the argmax over the vocabulary and integer counters of token accuracy / decoded-bin
distance - from the kernel up to trainer.token_metrics and the finetune log.

References: torch.argmax on the same bf16 logits moved to the CPU (predicted ids, exactly), a torch-CPU recount (the six
counters, exactly), vla_token_ce (loss to 1e-6: the two kernels add the same per-row terms, float atomics in another order; count
exactly), and tests/golden/token_metrics.npz - the reference's own metric functions on seeded ids (tools/make_golden_token_metrics.py;
1e-6: the reference divides in f32 / averages in fp64, the device rounds one fp64 quotient to f32)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "token_metrics.npz")
NAMES = ("action_accuracy", "l1_loss", "next_actions_accuracy", "next_actions_l1_loss")
BIG = 12.0           # a planted maximum: the random logits are N(0, 1.5^2), |x| < 9


@pytest.fixture(scope="module")
def ops():
    from vla_adapter_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---- planted rows: each returns (label, class) after writing into the row -------------------------------------------------------
def col0(x, V):
    x[0] = BIG
    return 0, 1                                              # (a correct prediction)


def last(x, V):
    x[V - 1] = BIG
    return V - 2, 2


def ties_near(x, V):
    """The same maximum in two columns of one thread (24, 25), two lanes (24, 40), two waves (24, 536) and two strides of one thread
    (24, 2072 = 2048 + 24), where the row is long enough."""
    for c in (24, 25, 40, 536, 2072):
        if c < V:
            x[c] = BIG
    return 24, 1


def ties_cross(x, V):
    """The lowest index sits in a HIGHER thread / wave than the other copies: column 800 (thread 100, wave 1) against columns
    2048 and 4096 (thread 0, later strides) - a reduction that breaks ties by lane or wave instead of by index returns 2048."""
    cols = [c for c in (800, 2048, 4096, 150000) if c < V] if V > 2048 else [250, 9]
    for c in cols:
        x[c] = BIG
    return min(cols), 2


def all_equal(x, V):
    x[:] = 0.5
    return 0, 2


def nan_row(x, V):
    """A NaN beats the largest finite value wherever it stands, and the first NaN wins."""
    x[5] = BIG
    x[V // 2] = float("nan")
    x[V - 3] = float("nan")
    return V // 2, 1


def ignored(x, V):
    x[7] = BIG
    return -100, 0


def non_action(x, V):
    """A valid label that is no action token: counts for the loss, not for the metrics."""
    x[11] = BIG
    return 3, 0


def plain(x, V):
    return 17, 2


SETS = {"a": [col0, last, ties_near, all_equal, nan_row], "b": [ignored, non_action, ties_cross, ties_near, plain],
        "real_a": [last, ties_cross, nan_row], "real_b": [col0, all_equal, ignored]}
# V: below one 2048-column stride of the workgroup, one stride + 8, two strides + 8, the real vocabulary
CASES = [(V, s) for V in (264, 2056, 4104) for s in ("a", "b")] + [(151936, "real_a"), (151936, "real_b")]


def build(V, which, strided=False):
    specs = SETS[which]
    g = torch.Generator().manual_seed(V + len(which))
    x = (torch.randn(len(specs), V, generator=g) * 1.5).to(BF)
    meta = [sp(x[r], V) for r, sp in enumerate(specs)]
    tgt = torch.tensor([m[0] for m in meta], dtype=torch.int64)
    cls = torch.tensor([m[1] for m in meta], dtype=torch.uint8)
    xd = x.to(DEV)
    if strided:                                              # rows 8 elements apart from dense
        buf = torch.zeros(len(specs), V + 8, device=DEV, dtype=BF)
        buf[:, :V] = xd
        xd = buf[:, :V]
    return x, xd, tgt, cls


def recount(pred, tgt, cls, tlen, nb):
    """The six counters on the CPU from predicted ids."""
    c = torch.zeros(6, dtype=torch.int64)
    for k in (1, 2):
        m = cls == k
        dp, dt = (tlen - pred[m] - 1).clamp(0, nb - 2), (tlen - tgt[m] - 1).clamp(0, nb - 2)
        c[3 * (k - 1):3 * k] = torch.stack([m.sum(), (pred[m] == tgt[m]).sum(), (dp - dt).abs().sum()])
    return c


def launch(ops, xd, tgt, cls, tlen, nb=256):
    out = torch.zeros(2, device=DEV)
    cnt = torch.zeros(6, device=DEV, dtype=torch.int64)
    pred = torch.full((xd.shape[0],), -7, device=DEV, dtype=torch.int32)
    ops.token_ce_metrics(xd, tgt.to(DEV), cls.to(DEV), out, cnt, pred, tlen, nb)
    torch.cuda.synchronize()
    return out.cpu(), cnt.cpu(), pred.cpu().long()


@pytest.mark.parametrize("V,which", CASES)
def test_kernel_against_torch_argmax_and_token_ce(ops, V, which):
    x, xd, tgt, cls = build(V, which, strided=(V == 2056))
    tlen = 151643 if V == 151936 else V - 3
    out, cnt, pred = launch(ops, xd, tgt, cls, tlen)
    am = x.argmax(dim=1)                                     # torch on the CPU, the same bf16 values
    act = cls > 0
    print(f"V={V} set={which}: kernel {pred.tolist()}  torch.argmax {am.tolist()}  counters {cnt.tolist()}")
    assert torch.equal(pred[act], am[act]), "predicted ids of the action rows"
    assert (pred[~act] == -1).all()
    for r, sp in enumerate(SETS[which]):                      # the planted answers themselves (torch's rule, stated independently)
        want = {col0: 0, last: V - 1, ties_near: 24, all_equal: 0, nan_row: V // 2}.get(sp)
        if want is not None:
            assert int(pred[r]) == want, sp.__name__
    assert torch.equal(cnt, recount(am, tgt, cls, tlen, 256)), "six counters against the CPU recount"
    ref = ops.token_ce(xd.contiguous(), tgt.to(DEV), torch.zeros(2, device=DEV)).cpu()
    print(f"    loss sums: metrics {out[0].item()!r}  vla_token_ce {ref[0].item()!r}  counts {out[1].item()} {ref[1].item()}")
    assert out[1].item() == ref[1].item() == int(((tgt >= 0) & (tgt < V)).sum())
    if ref[0].item() == ref[0].item():
        assert abs(out[0].item() - ref[0].item()) <= 1e-6 * abs(ref[0].item())
    else:                                                    # a valid NaN row: both sums are NaN
        assert nan_row in SETS[which] and out[0].item() != out[0].item()
    out2, cnt2, pred2 = launch(ops, xd, tgt, cls, tlen)
    assert torch.equal(cnt2.view(torch.uint8), cnt.view(torch.uint8)) and torch.equal(pred2, pred), "two launches, the same bits"


def test_action_row_with_a_label_outside_the_vocabulary(ops):
    """Vocabularies smaller than the tokenizer (the tiny configurations): the label of an action row is no column.  The row adds
    nothing to the loss, as in vla_token_ce, and still counts for the metrics."""
    V = 2056
    x, xd, tgt, cls = build(V, "b")
    tgt[2], tgt[4] = 151400, 151642
    out, cnt, pred = launch(ops, xd, tgt, cls, 151643)
    assert torch.equal(pred[cls > 0], x.argmax(dim=1)[cls > 0])
    assert torch.equal(cnt, recount(x.argmax(dim=1), tgt, cls, 151643, 256))
    ref = ops.token_ce(xd, tgt.to(DEV), torch.zeros(2, device=DEV)).cpu()
    assert out[1].item() == ref[1].item() == 2 and abs(out[0].item() - ref[0].item()) <= 1e-6 * abs(ref[0].item())


def _finish(ops, cnt):
    m = ops.token_metrics_finish(cnt.to(DEV))
    assert list(m) == list(NAMES) and all(v.dim() == 0 and v.dtype == torch.float32 for v in m.values())
    return [float(v) for v in m.values()]


def test_fixture_ids_planted_as_row_maxima(ops, gold):
    """The reference's four metrics from the kernel: the fixture's predicted ids are planted as the maxima of [3 * 95, 151936]
    logits, the row classes come from vla_token_row_class on the fixture's labels."""
    pred, gt = torch.from_numpy(gold["pred_ids"]), torch.from_numpy(gold["gt_ids"])
    B, L = gt.shape
    V = 151936
    x = (torch.randn(B * L, V, device=DEV, generator=torch.Generator(DEV).manual_seed(5)) * 1.5).to(BF)
    x[torch.arange(B * L, device=DEV), pred.view(-1).to(DEV)] = BIG
    want_cls = torch.from_numpy(gold["current_mask"].astype(np.uint8) + 2 * gold["next_mask"].astype(np.uint8))
    cls = ops.token_row_class(gt.to(DEV), 0)
    labels = torch.cat([torch.full((B, 1), 151640, dtype=torch.int64), gt], dim=1).to(DEV)     # the trainer's call: labels[:, 1:]
    assert torch.equal(cls.cpu(), want_cls) and torch.equal(ops.token_row_class(labels, 1).cpu(), want_cls)
    for case, sl in enumerate([slice(0, 3), slice(0, 1), slice(1, 2), slice(2, 3)]):
        rows = slice(sl.start * L, sl.stop * L)
        out, cnt, got_pred = launch(ops, x[rows], gt[sl].reshape(-1), cls[sl].reshape(-1).cpu(), 151643)
        act = want_cls[sl].reshape(-1) > 0
        assert torch.equal(got_pred[act], pred[sl].reshape(-1)[act])
        assert [int(cnt[0]), int(cnt[3])] == gold["mask_counts"][case].tolist()
        got = _finish(ops, cnt)
        for name, g, w in zip(NAMES, got, gold["metrics"][case].tolist()):
            print(f"{gold['cases'][case]} {name}: device {g!r}  reference {w!r}")
            assert (g != g) if w != w else abs(g - w) <= 1e-6 * abs(w), (name, g, w)
        assert out[1].item() == int((gt[sl] >= 0).sum())


# ---- trainers ----------------------------------------------------------------------------------------------------------------
TLEN = 1023          # tiny vocabulary 1024: action ids = the 256 ids below 1023, ACTION_TOKEN_BEGIN_IDX = 766; the batch's 64-token blocks
                     # (ids 724 .. 1022) then hold action rows and valid non-action rows


def _batch(cfg, B, seed):
    from vla_adapter_amd import synthetic as S
    batch = S.make_batch(cfg, B, DEV, seed=seed, P=20, ragged=True)
    batch["labels"] = torch.where(batch["labels"] != -100, batch["input_ids"], batch["labels"])
    return batch


def _trainer(mode, cfg, **kw):
    from vla_adapter_amd import engine as E, synthetic as S
    from vla_adapter_amd.trainers import FullFinetune, LoRAFinetune
    eng = E.VLAEngine(cfg, S.make_weights(cfg, DEV, seed=15, std=0.05), DEV)
    tr = FullFinetune(eng) if mode == "full" else LoRAFinetune(eng, rank=8, seed=2)
    tr.set_objective("token_ce", tokenizer_len=TLEN, **kw)
    return tr


def _cpu_classes(tgt2d, begin):
    c = torch.cumsum(tgt2d != -100, dim=1)
    a = tgt2d > begin
    return (a & (c >= 1) & (c <= 7)).to(torch.uint8) + 2 * (a & (c > 7)).to(torch.uint8)


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_trainer_metrics_eager_and_captured(ops, monkeypatch, mode):
    """token_metrics after an eager step = the metrics recomputed on the CPU from that step's logits (copied when the segment hands
    them to the kernel, before the backward overwrites them in place); the captured step leaves the same counters, bit for bit."""
    from vla_adapter_amd import engine as E
    from vla_adapter_amd.input_stage import GPUInputStage
    cfg = E.tiny_config()
    batch = _batch(cfg, 2, 16)
    seen = {}
    orig = ops.token_ce_metrics

    def spy(logits, tgt, cls, *a, **k):
        seen.update(logits=logits.clone(), tgt=tgt.clone(), cls=cls.clone())
        return orig(logits, tgt, cls, *a, **k)
    monkeypatch.setattr(ops, "token_ce_metrics", spy)
    tr = _trainer(mode, cfg)
    loss3 = tr.train_step(batch, 1e-3)
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "token_ce_metrics", orig)
    eager_cnt, eager_m = tr.ce_counters.cpu(), {k: float(v) for k, v in tr.token_metrics.items()}
    assert list(eager_m) == list(NAMES) and all(v.is_cuda and v.dim() == 0 for v in tr.token_metrics.values())
    assert loss3[0].item() == loss3[1].item() == loss3[2].item()          # loss3 as before: the loss in all three slots
    logits, tgt = seen["logits"].cpu(), seen["tgt"].cpu()
    cls = _cpu_classes(batch["labels"][:, 1:].cpu(), TLEN - 257)
    assert torch.equal(seen["cls"].cpu(), cls) and tgt.numel() == logits.shape[0] == cls.numel()
    cls = cls.view(-1)
    assert int((cls == 1).sum()) > 0 and int((cls == 2).sum()) > 0 and int(((cls == 0) & (tgt >= 0)).sum()) > 0
    am = logits.argmax(dim=1)
    assert torch.equal(eager_cnt, recount(am, tgt, cls, TLEN, 256))
    stage = GPUInputStage("cpu", tokenizer_len=TLEN)
    from vla_adapter_amd import train_utils as TU
    want = []
    for k in (1, 2):
        m = cls == k
        want += [float(TU.compute_token_accuracy(am, tgt, m)), float(TU.compute_actions_l1_loss(stage, am, tgt, m))]
    print(f"{mode}: counters {eager_cnt.tolist()}  metrics {eager_m}  CPU {want}")
    for (name, g), w in zip(eager_m.items(), want):
        assert abs(g - w) <= 1e-6 * abs(w), (name, g, w)
    # the captured step: fresh trainer, same weights and batch
    tc = _trainer(mode, cfg)
    tc.capture({k: v.clone() for k, v in batch.items()}, None)
    tc.train_step_graphed(1e-3)
    torch.cuda.synchronize()
    assert torch.equal(tc.ce_counters.cpu(), eager_cnt)
    assert [float(v) for v in tc.token_metrics.values()] == list(eager_m.values())


@pytest.mark.parametrize("mode", ["lora", "full"])
def test_parameters_do_not_depend_on_the_metrics(ops, monkeypatch, mode):
    """Two steps with vla_token_ce_metrics in the segment leave the parameters that two steps with plain vla_token_ce leave.  Two
    runs of the plain form are compared first: they are bit-identical on the MI355X (printed below), so bit identity is required."""
    from vla_adapter_amd import engine as E
    cfg = E.tiny_config()
    batch = _batch(cfg, 2, 16)

    def run():
        tr = _trainer(mode, cfg)
        for _ in range(2):
            tr.train_step(batch, 1e-3)
        torch.cuda.synchronize()
        return tr.P.data.clone()
    with monkeypatch.context() as mp:
        mp.setattr(ops, "token_ce_metrics", lambda logits, tgt, cls, out, *a, **k: ops.token_ce(logits, tgt, out))
        p0, p1 = run(), run()
    deterministic = torch.equal(p0.view(torch.int16), p1.view(torch.int16))
    got = run()
    d_plain, d_new = (p0.float() - p1.float()).abs().max().item(), (got.float() - p0.float()).abs().max().item()
    print(f"{mode}: two plain runs bit-identical: {deterministic} (max |diff| {d_plain}); metrics run vs plain max |diff| {d_new}")
    assert deterministic, "the plain token-CE step is expected to repeat bit for bit"
    assert torch.equal(got.view(torch.int16), p0.view(torch.int16))


def test_finetune_logs_the_four_metrics(tmp_path):
    from vla_adapter_amd import finetune as F
    out = F.finetune(F.parse_args(["--tiny", "true", "--objective", "token_ce", "--use_lora", "True", "--lora_rank", "8", "--batch_size", "2",
                                   "--max_steps", "1", "--wandb_log_freq", "1", "--use_proprio", "True", "--run_root_dir", str(tmp_path),
                                   "--run_id_override", "r"]))
    assert len(out["log"]) == 2
    for rec in out["log"]:
        print(rec)
        assert {"step", "loss_value", "curr_action_l1_loss", "lr", *NAMES} <= set(rec)
        assert rec["loss_value"] == rec["curr_action_l1_loss"]
        for k in ("action_accuracy", "next_actions_accuracy"):
            assert 0.0 <= rec[k] <= 1.0
        for k in ("l1_loss", "next_actions_l1_loss"):
            assert 0.0 <= rec[k] <= 2.0 * 254 / 255
