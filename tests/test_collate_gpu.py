"""The on-device collator (csrc/collate.hip, GPUInputStage.normalize / collate): normalize_action_and_proprio against a float32
restatement in numpy (the reference's own function needs TensorFlow), the token assembly against build() and against a Python
restatement of datasets.py:76-89, 124 plus the collator's right padding, capture into a graph (no host round trip), and a
fine-tune fed raw transitions against the same run fed their pre-collated form."""
import json
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGN = -100
PROMPT_LENS = [2, 3, 9, 40, 51]          # len < 3 (nothing dropped), len == 3 (the block starts at 0), ragged rows
NT = 64                                  # NUM_TOKENS
IMG = 16


def _stats(seed, D):
    """One dataset_statistics entry: dimension 1 unmasked, dimension 2 with min == max, dimension 4 with q01 == q99 but min != max."""
    r = np.random.default_rng(seed)
    q01 = r.uniform(-2.0, -0.5, D).astype(np.float32)
    q99 = r.uniform(0.5, 2.0, D).astype(np.float32)
    mn, mx = q01 - np.float32(1.5), q99 + np.float32(1.5)
    mx[2] = mn[2]
    q99[4] = q01[4]
    mask = np.ones(D, bool)
    mask[1] = False
    return dict(q01=q01.tolist(), q99=q99.tolist(), min=mn.tolist(), max=mx.tolist(), mask=mask.tolist())


def _np_normalize(x, stats, kind):
    """data_utils.py:67-90 in numpy, every intermediate float32: where(mask, clip(2 * (x - low) / (high - low + 1e-8) - 1, -1, 1), x),
    then where(min == max, 0, .)."""
    f = np.float32
    lo_k, hi_k = ("min", "max") if kind == "bounds" else ("q01", "q99")
    low, high = np.asarray(stats[lo_k], f), np.asarray(stats[hi_k], f)
    with np.errstate(over="ignore", divide="ignore"):
        t = (f(2) * (x - low)) / ((high - low) + f(1e-8)) - f(1)
    assert t.dtype == f
    y = np.where(np.asarray(stats["mask"], bool), np.minimum(np.maximum(t, f(-1)), f(1)), x)
    return np.where(np.asarray(stats["min"], f) == np.asarray(stats["max"], f), f(0), y).astype(f)


@pytest.fixture(scope="module")
def stage():
    from vla_adapter_amd.input_stage import GPUInputStage
    return GPUInputStage(DEV, backbones=("siglip",), image_size=IMG)


@pytest.fixture(scope="module")
def rows():
    """The five samples every assembly test uses (left unchanged): prompts, a normalised 8 x 7 window with values beyond +-1, proprio, frames."""
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, 1000, (n,), generator=g).tolist() for n in PROMPT_LENS]
    B = len(prompts)
    return dict(prompts=prompts, actions=torch.rand(B, 8, 7, generator=g) * 2.4 - 1.2, proprio=torch.rand(B, 8, generator=g) * 2 - 1,
                frames=[torch.randint(0, 256, (B, IMG, IMG, 3), generator=g, dtype=torch.uint8)])


def _collate(stage, rows, **kw):
    kw = dict(dict(seed=3, rank=1, step=7), **kw)
    return stage.collate(rows["frames"], kw.pop("prompts", rows["prompts"]), kw.pop("actions", rows["actions"]), rows["proprio"], **kw)


def _kept(n):
    return n - 3 if n >= 3 else n


def _fill_mask(L, n_act=56):
    m = torch.zeros(len(PROMPT_LENS), L, dtype=torch.bool)
    for b, n in enumerate(PROMPT_LENS):
        m[b, _kept(n) + n_act:_kept(n) + NT] = True
    return m.to(DEV)


@pytest.mark.parametrize("kind", ["bounds_q99", "bounds"])
def test_normalize_matches_float32_numpy_bit_for_bit(stage, kind):
    D = 7
    stats = _stats(5, D)
    x = (np.random.default_rng(6).standard_normal((5, 8, D)) * 2).astype(np.float32)
    edges = [np.asarray(stats[k], np.float32) for k in ("q01", "q99", "min", "max")]
    for i, e in enumerate(edges):                  # exactly at, and beyond, every low / high
        x[0, i], x[1, i] = e, e + np.float32(-1.0 if i % 2 == 0 else 1.0)
    x[2, 0], x[2, 1] = np.nextafter(edges[0], np.float32(-9)), np.nextafter(edges[1], np.float32(9))
    got = stage.normalize(torch.from_numpy(x), stats, kind)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == x.shape
    ref = _np_normalize(x, stats, kind)
    g = got.cpu().numpy()
    diff = np.flatnonzero(g.view(np.int32) != ref.view(np.int32))
    print(f"{kind}: {diff.size} of {g.size} elements differ in bits")
    assert diff.size == 0, (g.ravel()[diff[:8]], ref.ravel()[diff[:8]])
    assert np.array_equal(g[..., 1], x[..., 1]) and not g[..., 2].any()                     # unmasked: untouched; min == max: zero
    assert np.all(np.abs(g[..., [0, 3, 4, 5, 6]]) <= 1)
    if kind == "bounds_q99":
        assert np.all(np.abs(g[..., 4]) == 1)                                                # q01 == q99: every value lands on a bound
    stage.normalize(torch.from_numpy(x), stats, kind)
    assert len([k for k in stage._stats if k[0] == id(stats)]) == 1                         # uploaded once per (stats, kind)


def test_tokens_match_build(stage, rows):
    ref = stage.build(rows["frames"], rows["prompts"], rows["actions"], rows["proprio"], rng=random.Random(0))
    got = _collate(stage, rows)
    assert set(got) == set(ref)
    L = ref["input_ids"].shape[1]
    assert L == 112 and got["input_ids"].shape == (5, L) and got["attention_mask"].dtype == torch.bool
    fill = _fill_mask(L)
    for k in ("input_ids", "labels"):
        assert got[k].dtype == torch.int64 and torch.equal(got[k][~fill], ref[k][~fill]), k       # prompt ids, the 56 action ids, padding
    assert torch.equal(got["labels"][fill], got["input_ids"][fill])                           # the block lies inside the last 65 positions
    for k in ("attention_mask", "pixel_values", "actions", "proprio"):
        assert torch.equal(got[k], ref[k]), k
    ids = got["input_ids"].cpu()
    for b, n in enumerate(PROMPT_LENS):
        p = _kept(n)
        assert ids[b, :p].tolist() == rows["prompts"][b][:p]
        own = set(ids[b, p:p + 56].tolist())
        assert all(t in own for t in ids[b, p + 56:p + NT].tolist()), f"row {b}: a filler id is not one of the row's own 56"


def test_fill_draws_follow_the_seed_words(stage, rows):
    L = 112
    fill = _fill_mask(L)
    a = _collate(stage, rows)
    draws = a["input_ids"][fill]
    assert draws.numel() == 5 * 8 and draws.unique().numel() > 1, "all filler draws of the batch are equal"
    again = _collate(stage, rows)
    assert all(torch.equal(a[k], again[k]) for k in a)
    for other in (dict(step=8), dict(seed=4), dict(rank=0)):
        b = _collate(stage, rows, **other)
        assert not torch.equal(b["input_ids"][fill], draws), other
        assert torch.equal(b["input_ids"][~fill], a["input_ids"][~fill])
    # device-resident (prompt_flat, prompt_off): the same batch
    flat = torch.tensor([t for r in rows["prompts"] for t in r], dtype=torch.int64, device=DEV)
    off = torch.tensor(np.cumsum([0] + PROMPT_LENS), dtype=torch.int32, device=DEV)
    c = _collate(stage, rows, prompts=(flat, off), L=L)
    assert all(torch.equal(a[k], c[k]) for k in a)
    with pytest.raises(ValueError, match="explicit L"):
        _collate(stage, rows, prompts=(flat, off))
    d = _collate(stage, rows, prompts=(flat.cpu(), off.cpu()))           # offsets on the host: L from the lengths
    assert all(torch.equal(a[k], d[k]) for k in a)


def _expected(prompts, tok, fill, L, pad):
    """datasets.py:76-89, 124 and the collator's right padding (data_utils.py:114-134), truncated at L as build() truncates."""
    B = len(prompts)
    ids, lab = np.full((B, L), pad, np.int64), np.full((B, L), IGN, np.int64)
    for b in range(B):
        r = list(prompts[b])
        if len(r) >= 3:
            del r[-3:]
        r = r + tok[b][:NT] + fill[b]
        l = list(r)
        for k in range(len(l) - (NT + 1)):
            l[k] = IGN
        n = min(len(r), L)
        ids[b, :n], lab[b, :n] = r[:n], l[:n]
    return ids, lab, ids != pad


@pytest.mark.parametrize("L", [30, 70, 160])
def test_truncation_and_static_length(stage, rows, L):
    """L = 70 cuts the rows of 101 and 112 ids, L = 160 pads every row, L = 30 (added: none of the five rows is cut inside its prompt at
    70) cuts the two long rows inside their prompts."""
    tok = stage.tokenize_actions(rows["actions"].reshape(5, -1)).cpu().tolist()
    nat = _collate(stage, rows)["input_ids"].cpu()
    fill = [nat[b, _kept(n) + 56:_kept(n) + NT].tolist() for b, n in enumerate(PROMPT_LENS)]      # (membership: test_tokens_match_build)
    got = _collate(stage, rows, L=L)
    ids, lab, am = _expected(rows["prompts"], tok, fill, L, stage.pad)
    assert np.array_equal(got["input_ids"].cpu().numpy(), ids)
    assert np.array_equal(got["labels"].cpu().numpy(), lab)
    assert np.array_equal(got["attention_mask"].cpu().numpy(), am)
    g_ids, g_lab, g_am = got["input_ids"].cpu(), got["labels"].cpu(), got["attention_mask"].cpu()
    for b, n in enumerate(PROMPT_LENS):
        row_len = _kept(n) + NT
        if row_len >= L:                                   # cut (or exactly full): no pad in it
            assert (g_ids[b] != stage.pad).all() and g_am[b].all()
        else:                                              # beyond the row: pad / ignore / False
            assert (g_ids[b, row_len:] == stage.pad).all() and (g_lab[b, row_len:] == IGN).all() and not g_am[b, row_len:].any()
        first = max(row_len - (NT + 1), 0)
        assert (g_lab[b, :min(first, L)] == IGN).all()
        assert torch.equal(g_lab[b, first:min(row_len, L)], g_ids[b, first:min(row_len, L)])
    if L == 70:
        assert (g_lab[2, 5:70] != IGN).all() and (g_lab[2, :5] == IGN).all()          # len 9: 6 + 64 ids, unmasked from 70 - 65
    if L == 30:
        assert (g_lab[3] == IGN).all() and (g_lab[4] == IGN).all()                      # cut inside the prompt: nothing to learn from


def test_long_windows_take_the_first_64_ids_and_draw_nothing(stage, rows):
    g = torch.Generator().manual_seed(12)
    actions = torch.rand(5, 10, 7, generator=g) * 2.4 - 1.2                            # 70 ids >= 64
    ref = stage.build(rows["frames"], rows["prompts"], actions, rows["proprio"], rng=random.Random(0))
    a, b = _collate(stage, rows, actions=actions), _collate(stage, rows, actions=actions, step=8, seed=9)
    for k in ref:
        assert torch.equal(a[k], ref[k]) and torch.equal(b[k], ref[k]), k
    tok = stage.tokenize_actions(actions.reshape(5, -1))
    for i, n in enumerate(PROMPT_LENS):
        assert torch.equal(a["input_ids"][i, _kept(n):_kept(n) + NT], tok[i, :NT])


def test_collate_captures_into_a_graph_and_replays(stage, rows):
    """Device-resident inputs: kernels only.  A sync or a device-to-host copy inside the capture would fail it."""
    L = 112
    a_stats, p_stats = _stats(21, 7), _stats(22, 8)
    g = torch.Generator().manual_seed(13)
    raw = [torch.randn(5, 8, 7, generator=g) * 2 for _ in range(3)]
    flat = torch.tensor([t for r in rows["prompts"] for t in r], dtype=torch.int64, device=DEV)
    off = torch.tensor(np.cumsum([0] + PROMPT_LENS), dtype=torch.int32, device=DEV)
    frames = [rows["frames"][0].to(DEV)]
    s_act, s_pro = raw[0].to(DEV), (rows["proprio"] * 3).to(DEV)
    call = lambda act: stage.collate(frames, (flat, off), act, s_pro, action_stats=a_stats, proprio_stats=p_stats, L=L, seed=3, rank=1, step=7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s_act)                                        # warm-up: the statistics reach the device once, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = call(s_act)
    for act in raw[1:]:
        s_act.copy_(act)
        graph.replay()
        torch.cuda.synchronize()
        eager = call(act.to(DEV))
        assert set(eager) == set(out)
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
        assert torch.equal(out["actions"].cpu(), torch.from_numpy(_np_normalize(act.numpy(), a_stats, "bounds_q99")))


def test_finetune_consumes_raw_batches(tmp_path):
    """Adapter-only on the tiny config: raw transitions through batch_stream give, bit for bit, the losses of the run fed the batches
    collate() makes of them up front (same seed words, no augmentation)."""
    from vla_adapter_amd import engine as E, finetune as F
    from vla_adapter_amd.input_stage import GPUInputStage, backbone_norms
    mcfg = E.NAMED_CONFIGS["tiny"]()
    g = torch.Generator().manual_seed(14)
    lens = [10, 24, 27]
    B, L = len(lens), 96
    stats = {"toy": dict(action=_stats(31, mcfg.action_dim), proprio=_stats(32, mcfg.proprio_dim))}
    f = tmp_path / "dataset_statistics.json"
    f.write_text(json.dumps(stats))
    raw = dict(frames_u8=torch.randint(0, 256, (B, mcfg.n_img, mcfg.vit[0].img, mcfg.vit[0].img, 3), generator=g, dtype=torch.uint8),
               prompt_flat=torch.randint(0, 700, (sum(lens),), generator=g), prompt_off=torch.tensor(np.cumsum([0] + lens), dtype=torch.int32),
               actions_raw=torch.randn(B, mcfg.chunk, mcfg.action_dim, generator=g) * 2, proprio_raw=torch.randn(B, mcfg.proprio_dim, generator=g) * 2,
               dataset_name="toy")
    args = lambda tmp: ["--tiny", "true", "--backbone", "tiny", "--batch_size", str(B), "--max_steps", "2", "--learning_rate", "1e-3",
                        "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                        "--run_root_dir", str(tmp), "--max_seq_len", str(L), "--dataset_statistics_file", str(f), "--seed", "5"]
    a = F.finetune(F.parse_args(args(tmp_path / "a") + ["--image_aug", "False"]), batches=[raw] * 3)
    st = GPUInputStage(DEV, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img)
    loaded = json.load(open(f))["toy"]
    pre = [st.collate(raw["frames_u8"], (raw["prompt_flat"], raw["prompt_off"]), raw["actions_raw"], raw["proprio_raw"], action_stats=loaded["action"],
                      proprio_stats=loaded["proprio"], L=L, seed=5, rank=0, step=i) for i in range(4)]      # 3 steps + the look-ahead batch
    assert not torch.equal(pre[0]["input_ids"], pre[1]["input_ids"])                                         # the step word reaches the draws
    b = F.finetune(F.parse_args(args(tmp_path / "b")), batches=pre)
    losses = lambda out: [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in out["log"]]
    assert len(a["log"]) == 3 and all(np.isfinite(x) for l in losses(a) for x in l)
    assert losses(a) == losses(b)
