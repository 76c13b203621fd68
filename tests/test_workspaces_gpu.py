"""Every holder of captured graphs keeps the workspace it was captured on and binds it before a replay: calls of
other shapes - predict() at two batch sizes, first use and replay, generate() - between the steps of a captured training run, or
between a forward and its backward, change nothing the run computes.  Every comparison is bit for bit, on integer views."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def inputs():
    """cfg, the training batch (B = 2), predict batches at B = 1 and B = 3, a validation batch, a generate() prompt batch at B = 3."""
    from vla_adapter_amd import engine as E, ops, synthetic as S
    cfg = E.tiny_config()
    train, p1, p3, val = (S.make_batch(cfg, B, DEV, seed=s, P=24, ragged=True) for B, s in ((2, 31), (1, 32), (3, 33), (2, 34)))
    lens = [20, 17, 25]
    g = torch.Generator().manual_seed(35)
    flat = torch.randint(0, cfg.llm.vocab - 300, (sum(lens),), generator=g).to(DEV)
    off = torch.tensor([0, 20, 37, 62], dtype=torch.int32, device=DEV)
    ids, am, pos, last_row, _ = ops.decode_prompt(flat, off, 32, cfg.n_patches, pad_id=cfg.llm.vocab - 1)
    gen = dict(input_ids=ids, attention_mask=am.view(torch.bool), pixel_values=p3["pixel_values"], pos=pos, last_row=last_row)
    return cfg, train, p1, p3, val, gen


def engine(cfg):
    from vla_adapter_amd import engine as E, synthetic as S
    return E.VLAEngine(cfg, S.make_weights(cfg, DEV, seed=30, std=0.05), DEV)


def interrupt(eng, p1, p3, gen):
    """Other shapes on the same engine: predict at B = 1 and B = 3, each captured on its first call and replayed on its second, and a
    generate at B = 3."""
    for b in (p1, p3):
        for _ in range(2):
            assert eng.predict(b).shape[0] == b["input_ids"].shape[0]
    assert tuple(eng.generate(gen, 3).shape) == (3, 3)
    assert eng.B == 3 and eng.llm.HS.shape[1] == 3, "generate puts back what was bound before it: predict's B = 3 workspace"


def test_generate_between_forward_and_backward(inputs):
    cfg, train, _, _, _, gen = inputs
    grads = []
    for with_generate in (False, True):
        eng = engine(cfg)
        pred = eng.forward(train, for_training=True)
        if with_generate:
            eng.generate(gen, 3)
            assert eng.B == 2 and eng.llm.B == 2 and eng.llm.HS.shape[1:3] == (2, eng.S)
        eng.loss_and_backward(pred, train["actions"])
        torch.cuda.synchronize()
        grads.append(eng.head.P.grad.clone())
    assert grads[0].any() and same(*grads)


def test_captured_adapter_step_interrupted(inputs):
    cfg, train, p1, p3, _, gen = inputs
    res = []
    for interrupted in (False, True):
        eng = engine(cfg)
        eng.capture({k: v.clone() for k, v in train.items()}, None)
        losses = []
        for step in range(3):
            losses.append(eng.train_step_graphed(1e-3).clone())
            if interrupted and step == 0:
                interrupt(eng, p1, p3, gen)
            else:
                assert eng.B == 2 and eng.llm.HS.shape[1:3] == (2, train["input_ids"].shape[1] + cfg.n_patches)
        eng.flush()
        torch.cuda.synchronize()
        res.append((torch.stack(losses), eng.head.P.data.clone()))
    assert torch.isfinite(res[0][0]).all() and not same(res[0][0][0], res[0][0][2]), "the run trains"
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])


def test_captured_lora_step_and_validation_interrupted(inputs):
    from vla_adapter_amd.lora_finetune import LoRAFinetune
    cfg, train, p1, p3, val, gen = inputs
    res = []
    for interrupted in (False, True):
        eng = engine(cfg)
        lo = LoRAFinetune(eng, rank=8, seed=2)
        lo.capture({k: v.clone() for k, v in train.items()}, None)
        losses = [lo.train_step_graphed(1e-3).clone()]
        if interrupted:
            interrupt(eng, p1, p3, gen)
        lo.begin_validation()
        vloss = lo.val_step_graphed({k: v.clone() for k, v in val.items()}, None).clone()
        lo.end_validation()
        for _ in range(2):
            losses.append(lo.train_step_graphed(1e-3).clone())
        assert eng.B == 2 and eng.llm.HS.shape[1] == 2
        torch.cuda.synchronize()
        res.append((torch.stack(losses), vloss, lo.P.data.clone(), eng.head.P.data.clone()))
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all() and res[0][2].any()
    assert all(same(a, b) for a, b in zip(*res))


def test_predict_shapes_alternate(inputs):
    cfg, _, p1, p3, _, _ = inputs
    eng = engine(cfg)
    out1 = eng.predict(p1).clone()
    hs1 = eng.llm.HS.clone()
    out3 = eng.predict(p3).clone()
    assert out3.shape[0] == 3 and eng.llm.HS.shape[1] == 3
    out = eng.predict(p1)
    torch.cuda.synchronize()
    assert same(out, out1) and same(eng.llm.HS, hs1) and len(eng._predict_graphs) == 2
    assert same(eng.predict(p3), out3)
    for ent in eng._predict_graphs.values():         # the cache entry: named fields, the workspace its graphs were captured on
        assert ent["static"]["input_ids"].shape[0] == ent["ws"].fields["B"] == ent["ws"].llm["HS"].shape[1] and ent["graphs"] and ent["segs"]
    assert eng.llm.HS is ent["ws"].llm["HS"] and eng.head.X is ent["ws"].head["X"]
