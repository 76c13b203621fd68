"""GPU checks of the serving batch: the three kernels of include/vla_serve.h bit for bit against restatements of the reference's host
code, and OpenVLAForActionPrediction.predict_actions - a ragged batch in one device pass - against the batch-1 oracle and against
predict_action itself (tiny configurations).

Tolerances.  The kernels and every exactness claim (replay, neighbour independence, batch 1 against predict_action) are bit for bit.
The end-to-end comparison with oracle.predict_action_batch1 (bf16-emulating mode) uses the relative L2 criterion < 2e-2 of
tests/test_host_api_gpu.py::test_predict_action_batch1_inference_matches_oracle: two valid bf16 evaluations of the same sample at
different batch sizes sit 6e-3 to 9e-3 apart (another summation order in the head), so nothing tighter can be asked end to end."""
import numpy as np
import pytest
import torch

from oracle import vla_oracle as O

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
PAD, IGN = 1023, -100                       # the tiny configurations pad with vocab - 1

STATS = {"libero_object": {
    "action": {"q01": [-0.5, -0.4, -0.3, -0.2, -0.1, -0.6, 0.0], "q99": [0.5, 0.6, 0.7, 0.8, 0.9, 0.4, 1.0],
               "min": [-1.0, -1.1, -1.2, -0.9, -0.8, -1.3, -1.0], "max": [1.0, 1.2, 0.9, 1.1, 1.3, 0.7, 1.0], "mask": [True] * 6 + [False]},
    "proprio": {"q01": [-0.8, -0.7, -0.6, -0.5, 0.25, -0.9, -0.2, -1.0], "q99": [0.9, 0.8, 0.7, 0.6, 0.25, 0.4, 0.3, 1.0],
                "min": [-1.5, -1.4, -1.3, -1.2, 0.25, -1.6, -0.7, -2.0], "max": [1.6, 1.5, 1.4, 1.3, 0.25, 1.1, 0.8, 2.0],
                "mask": [True, True, False, True, True, True, False, True]}}}     # dimension 4: high == low; 2 and 6 unmasked
KEY = "libero_object"


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def tensor_bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def normalize_proprio_numpy(proprio, norm_stats, kind):
    """experiments/robot/openvla_utils.py:671-701, restated."""
    if kind == "bounds":
        mask = norm_stats.get("mask", np.ones_like(norm_stats["min"], dtype=bool))
        proprio_high, proprio_low = np.array(norm_stats["max"]), np.array(norm_stats["min"])
    elif kind == "bounds_q99":
        mask = norm_stats.get("mask", np.ones_like(norm_stats["q01"], dtype=bool))
        proprio_high, proprio_low = np.array(norm_stats["q99"]), np.array(norm_stats["q01"])
    else:
        raise ValueError("Unsupported action/proprio normalization type detected!")
    return np.clip(np.where(mask, 2 * (proprio - proprio_low) / (proprio_high - proprio_low + 1e-8) - 1, proprio), a_min=-1.0, a_max=1.0)


@pytest.fixture(scope="module")
def stage():
    from vla_adapter_amd.input_stage import GPUInputStage
    return GPUInputStage(DEV, pad_token_id=PAD)


# ================================================================================================================ tokens
def _prompts(lens, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 700, (n,), generator=g).tolist() for n in lens]


def _expected_rows(prompts, L):
    """Each row's prepare_inference_inputs, right-padded with pad_id / ignore_index / 0."""
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction as V
    ids = torch.full((len(prompts), L), PAD, dtype=torch.int64)
    lab = torch.full((len(prompts), L), IGN, dtype=torch.int64)
    am = torch.zeros(len(prompts), L, dtype=torch.bool)
    for b, p in enumerate(prompts):
        t = torch.tensor(p, dtype=torch.int64).view(1, -1)
        i, a, l = V.prepare_inference_inputs(t, torch.ones_like(t, dtype=torch.bool))
        n = i.shape[1]
        ids[b, :n], lab[b, :n], am[b, :n] = i[0], l[0], a[0]
    return ids, lab, am


def _raw_serve_tokens(prompts, L):
    """The raw entry point on PRE-POISONED outputs (an element it left unwritten would show as 7 / 0x7f / 77)."""
    import ctypes as C
    from vla_adapter_amd import constants as K, native as N, ops
    lens = [len(p) for p in prompts]
    B = len(lens)
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    off = torch.tensor([sum(lens[:i]) for i in range(B + 1)], dtype=torch.int32, device=DEV)
    ids, lab = torch.full((B, L), 7, dtype=torch.int64, device=DEV), torch.full((B, L), 7, dtype=torch.int64, device=DEV)
    am = torch.full((B, L), 0x7F, dtype=torch.uint8, device=DEV)
    hid, ok = torch.full((B,), 77, dtype=torch.int32, device=DEV), torch.full((B,), 0x7F, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    N.check(ops._lib().vla_serve_tokens(ops._st(), p(flat), p(off), flat.numel(), p(ids), p(lab), p(am), p(hid), p(ok), B, L, K.NUM_TOKENS, 1,
                                        K.STOP_INDEX, K.ACTION_TOKEN_BEGIN_IDX + 1, PAD, IGN), "serve_tokens")
    return ids.cpu(), lab.cpu(), am.cpu(), hid.cpu().tolist(), ok.cpu().tolist()


@pytest.mark.parametrize("L", [105, 128])
def test_serve_tokens_equal_per_row_prepare_inference_inputs(L):
    lens = [1, 2, 19, 40]                                 # 40 + 65 = 105: the longest row fills L = 105 to its last element
    prompts = _prompts(lens)
    ids, lab, am, hid, ok = _raw_serve_tokens(prompts, L)
    e_ids, e_lab, e_am = _expected_rows(prompts, L)
    assert torch.equal(ids, e_ids) and torch.equal(lab, e_lab)
    assert set(am.unique().tolist()) <= {0, 1} and torch.equal(am.bool(), e_am)
    assert hid == [n - 1 for n in lens] and ok == [1, 1, 1, 1]


def test_serve_tokens_bad_rows_get_the_substitute_row():
    """A fifth row of 41 ids at L = 105 (41 + 65 = 106) and an empty row give row_ok == 0 and the documented substitute: the
    well-formed row of the one-id prompt [pad_id]."""
    from vla_adapter_amd import constants as K, ops
    L, lens = 105, [1, 2, 19, 40, 41, 0]
    prompts = _prompts(lens)
    ids, lab, am, hid, ok = _raw_serve_tokens(prompts, L)
    e_ids, e_lab, e_am = _expected_rows(prompts[:4] + [[PAD], [PAD]], L)
    assert torch.equal(ids, e_ids) and torch.equal(lab, e_lab) and torch.equal(am.bool(), e_am)
    assert ok == [1, 1, 1, 1, 0, 0] and hid == [0, 1, 18, 39, 0, 0]
    with pytest.raises(ValueError):
        ops.serve_tokens(torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV), K.NUM_TOKENS + 1, pad_id=PAD)


def test_stage_serve_tokens_lists_and_tensors(stage):
    prompts = _prompts([5, 19, 12])
    a = stage.serve_tokens(prompts)
    assert a["input_ids"].shape == (3, 96) and a["attention_mask"].dtype == torch.bool
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 5, 24, 36], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="explicit L"):
        stage.serve_tokens((flat, off))
    b = stage.serve_tokens((flat, off), L=96)
    assert all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        stage.serve_tokens(prompts, L=83)                # 19 + 65 = 84


# ================================================================================================================ proprio
@pytest.mark.parametrize("kind", ["bounds", "bounds_q99"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_normalize_proprio_bits_equal_the_evaluators_numpy(stage, kind, dtype):
    st = STATS[KEY]["proprio"]
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.2, 1.2, size=(6, 8)).astype(dtype)
    x[0] = np.array(st["min"]) - 0.5                     # below every bound
    x[1] = np.array(st["max"]) + 0.5                     # above every bound
    x[2, 2], x[2, 6] = 3.25, -1.75                       # unmasked dimensions with |x| > 1: must come back clipped
    x[3] = np.array(st["q01"])
    x[4] = np.array(st["q99"])
    x[5, 4] = 0.25 + 1e-9                                # the high == low dimension, next to its bound
    want = normalize_proprio_numpy(x, st, kind)
    assert want.dtype == np.float64
    want = want.astype(np.float32)
    got = stage.normalize_proprio(x, st, kind).cpu().numpy()
    assert bits_equal(got, want), np.abs(got.astype(np.float64) - want).max()
    assert got[2, 2] == 1.0 and got[2, 6] == -1.0 and np.abs(got).max() <= 1.0
    got_t = stage.normalize_proprio(torch.from_numpy(x).to(DEV), st, kind).cpu().numpy()
    assert bits_equal(got_t, want)
    with pytest.raises(ValueError):
        stage.normalize_proprio(x, st, "normal")


# ================================================================================================================ un-normalise
def _bare_vla():
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    vla = object.__new__(OpenVLAForActionPrediction)         # _unnormalize_actions reads norm_stats only
    vla.norm_stats = STATS
    return vla


@pytest.mark.parametrize("kind", ["bounds", "bounds_q99"])
def test_unnormalize_actions_bits_equal_the_host_function(stage, kind, monkeypatch):
    from vla_adapter_amd import constants as K
    monkeypatch.setattr(K, "ACTION_PROPRIO_NORMALIZATION_TYPE", kind)
    g = torch.Generator().manual_seed(9)
    pred = torch.randn(4, 8, 7, generator=g)
    pred[1] *= 1e-4                                      # tiny magnitudes: a + 1 rounds in fp32
    pred[2, :4] *= 3e-9
    pred[3, 0, :3] = torch.tensor([0.0, -1.0, 1.0])
    pred = pred.to(BF).to(DEV)
    want = _bare_vla()._unnormalize_actions(pred.float().cpu().numpy(), KEY)
    assert want.dtype == np.float64 and want.shape == (4, 8, 7)
    got = stage.unnormalize_actions(pred, STATS[KEY]["action"], kind)
    assert got.dtype == torch.float64 and bits_equal(got.cpu().numpy(), want)
    assert bits_equal(got.cpu().numpy()[..., 6], pred.float().cpu().numpy()[..., 6].astype(np.float64)), "the unmasked dimension stays normalised"
    ok = torch.tensor([1, 0, 1, 1], dtype=torch.uint8, device=DEV)
    got2 = stage.unnormalize_actions(pred, STATS[KEY]["action"], kind, row_ok=ok).cpu().numpy()
    assert np.isnan(got2[1]).all() and bits_equal(got2[[0, 2, 3]], want[[0, 2, 3]])


# ================================================================================================================ end to end
class Served:
    """One tiny model with the weights of test_predict_action_batch1_inference_matches_oracle, its oracle weights and three samples."""

    def __init__(self, fused=False):
        from vla_adapter_amd import engine as E, synthetic as S
        from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
        self.cfg = cfg = E.tiny_fused_config() if fused else E.tiny_config()
        self.W = W = S.make_weights(cfg, DEV, seed=5, std=0.05)
        self.vla = OpenVLAForActionPrediction(cfg, W, DEV, norm_stats=STATS)
        f = lambda sd: {k: v.float().cpu() for k, v in sd.items()}
        llm = f(W["llm"])
        self.OW = dict(vit=[f(s) for s in W["vit"]], proj=f(W["proj"]), llm=llm, embed=llm["embed_tokens.weight"],
                       action_queries=W["action_queries"].float().cpu(), head=f(W["head"]), proprio=f(W["proprio"]))
        self.ocfg = dict(vit=[v.as_oracle() for v in cfg.vit], fused=cfg.fused, llm=cfg.llm.as_oracle(), n_img=cfg.n_img, pro=cfg.pro,
                         num_blocks=cfg.num_blocks)
        self.img, self.C = cfg.vit[0].img, 3 * len(cfg.vit) * cfg.n_img

    def sample(self, lens, seed):
        g = torch.Generator().manual_seed(seed)
        prompts = [torch.randint(3, 700, (n,), generator=g).tolist() for n in lens]
        px = torch.randn(len(lens), self.C, self.img, self.img, generator=g).clamp_(-3, 3).to(BF)
        proprio = (torch.rand(len(lens), 8, generator=g, dtype=torch.float64) * 3 - 1.5).numpy()        # raw: partly outside the bounds
        return prompts, px, proprio


@pytest.fixture(scope="module")
def served():
    return Served()


LENS = [5, 19, 12]


@pytest.fixture(scope="module")
def first_call(served):
    prompts, px, proprio = served.sample(LENS, 31)
    act, hid = served.vla.predict_actions(prompts, pixel_values=px, proprio=proprio, unnorm_key=KEY)
    return prompts, px, proprio, act, hid.clone(), served.vla.engine._pred_out.float().cpu().numpy()


def test_predict_actions_rows_match_the_batch1_oracle(served, first_call):
    from vla_adapter_amd import constants as K
    prompts, px, proprio, act, hid, pred = first_call
    cfg = served.cfg
    assert act.shape == (3, cfg.chunk, 7) and act.dtype == np.float64 and tuple(hid.shape) == (3, 1, K.NUM_TOKENS, cfg.llm.d)
    assert served.vla.engine._predict_graphs and next(iter(served.vla.engine._predict_graphs))[0] == (3, 96)
    pn = normalize_proprio_numpy(proprio, STATS[KEY]["proprio"], "bounds_q99").astype(np.float32)
    for b in range(3):
        ids = torch.tensor(prompts[b]).view(1, -1)
        ref_un, _, ref_hid = O.predict_action_batch1(ids, torch.ones_like(ids, dtype=torch.bool), px[b:b + 1].float(),
                                                     torch.tensor(pn[b]).to(BF).float(), served.OW, served.ocfg, STATS[KEY]["action"], emu=True)
        err = np.linalg.norm(act[b] - ref_un) / np.linalg.norm(ref_un)
        herr = rel(hid[b:b + 1], ref_hid)
        print(f"sample {b} (P = {LENS[b]}): actions rel {err:.3e}, hidden rel {herr:.3e}")
        assert err < 2e-2, (b, err)
        assert herr < 2e-2, (b, herr)
    assert bits_equal(act[:, :, 6], pred[:, :, 6].astype(np.float64)), "the masked dimension stays normalised"
    assert np.isfinite(act).all()


def test_replay_reproduces_the_first_call_and_new_inputs_flow(served, first_call):
    prompts, px, proprio, act, hid, _ = first_call
    n0 = len(served.vla.engine._predict_graphs)
    act2, hid2 = served.vla.predict_actions(prompts, pixel_values=px, proprio=proprio, unnorm_key=KEY)
    assert bits_equal(act2, act) and tensor_bits_equal(hid2, hid), "a replayed call reproduces the first bit for bit"
    # neighbour independence at a fixed (B, L): row 0 kept, other prompts (other lengths), pixels and proprio in rows 1 and 2
    p2, x2, r2 = served.sample([5, 9, 23], 77)
    p2[0], x2[0], r2[0] = prompts[0], px[0], proprio[0]
    act3, hid3 = served.vla.predict_actions(p2, pixel_values=x2, proprio=r2, unnorm_key=KEY)
    assert bits_equal(act3[0], act[0]) and tensor_bits_equal(hid3[0], hid[0]), "row 0 does not depend on its neighbours"
    assert not np.allclose(act3[1], act[1]) and not np.allclose(act3[2], act[2]), "new inputs flow through the static buffers"
    assert len(served.vla.engine._predict_graphs) == n0, "same (B, L): no new graph"


def test_batch_of_one_is_predict_action_bit_for_bit(served, first_call):
    """predict_actions of one sample with L = P + 65 and proprio_normalized=True against predict_action on it, both orders of first
    use; and predict_action's own output is unchanged by batched calls in between (each shape keeps its buffers)."""
    prompts, px, proprio, act, hid, _ = first_call
    vla = served.vla
    pn = normalize_proprio_numpy(proprio, STATS[KEY]["proprio"], "bounds_q99").astype(np.float32)
    one = lambda b: vla.predict_action(input_ids=torch.tensor(prompts[b]).view(1, -1), unnorm_key=KEY, proprio=pn[b], proprio_projector=True,
                                       action_head=True, pixel_values=px[b:b + 1],
                                       attention_mask=torch.ones(1, len(prompts[b]), dtype=torch.bool))
    a1, h1 = one(1)                                           # P = 19: L = 84, captured by predict_action
    h1 = h1.clone()
    assert a1.shape == (8, 7) and tuple(h1.shape) == (1, 1, 64, served.cfg.llm.d)
    b1, g1 = vla.predict_actions([prompts[1]], pixel_values=px[1:2], proprio=pn[1:2], proprio_normalized=True, unnorm_key=KEY, L=19 + 65)
    assert bits_equal(b1[0], a1) and tensor_bits_equal(g1, h1)
    b2, g2 = vla.predict_actions([prompts[2]], pixel_values=px[2:3], proprio=pn[2:3], proprio_normalized=True, unnorm_key=KEY, L=12 + 65)
    g2 = g2.clone()                                           # P = 12: L = 77, captured by predict_actions
    a2, h2 = one(2)
    assert bits_equal(b2[0], a2) and tensor_bits_equal(g2, h2)
    # a batched call of another shape in between leaves predict_action's output alone
    act_b, hid_b = vla.predict_actions(prompts, pixel_values=px, proprio=proprio, unnorm_key=KEY)
    assert bits_equal(act_b, act) and tensor_bits_equal(hid_b, hid)
    a1b, h1b = one(1)
    assert bits_equal(a1b, a1) and tensor_bits_equal(h1b, h1), "predict_action before and after a batched call"
    # the batched rows agree with the batch-1 calls to bf16 accuracy (another summation order in the head: not bit for bit)
    assert np.linalg.norm(act[1] - a1) / np.linalg.norm(a1) < 2e-2


def test_one_graph_per_rounded_length(served):
    eng = served.vla.engine
    pa, xa, ra = served.sample([100, 7], 91)                  # 165 -> L = 192
    pb, xb, rb = served.sample([3, 120], 92)                  # 185 -> L = 192
    n0 = len(eng._predict_graphs)
    a, _ = served.vla.predict_actions(pa, pixel_values=xa, proprio=ra, unnorm_key=KEY)
    assert len(eng._predict_graphs) == n0 + 1
    b, _ = served.vla.predict_actions(pb, pixel_values=xb, proprio=rb, unnorm_key=KEY)
    assert len(eng._predict_graphs) == n0 + 1, "longest prompts of 100 and 120 ids round to the same L: one graph"
    assert np.isfinite(a).all() and np.isfinite(b).all() and ((2, 192) in [k[0] for k in eng._predict_graphs])


def test_device_resident_prompts_bad_row_becomes_nan_and_return_tensors(served, first_call):
    """Offsets on the device: nothing is validated on the host; the row that does not fit L comes back as NaN, its neighbours as
    in the host-list call.  return_tensors=True under the synchronisation debug mode, where this torch build honours it."""
    prompts, px, proprio, act, hid, _ = first_call
    vla = served.vla
    flat = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=DEV)
    off = torch.tensor([0, 5, 24, 36], dtype=torch.int32, device=DEV)
    pr_dev, px_dev = torch.from_numpy(proprio).to(DEV), px.to(DEV)
    with pytest.raises(ValueError, match="explicit L"):
        vla.predict_actions((flat, off), pixel_values=px_dev, proprio=pr_dev, unnorm_key=KEY)
    a_t, h_t = vla.predict_actions((flat, off), pixel_values=px_dev, proprio=pr_dev, unnorm_key=KEY, L=96, return_tensors=True)
    assert a_t.is_cuda and a_t.dtype == torch.float64 and bits_equal(a_t.cpu().numpy(), act) and tensor_bits_equal(h_t, hid)
    # a 40-id prompt in row 1 at L = 96 (40 + 65 = 105): row_ok == 0
    long_flat = torch.cat([flat[:5], torch.randint(3, 700, (40,), device=DEV), flat[24:]])
    long_off = torch.tensor([0, 5, 45, 57], dtype=torch.int32, device=DEV)
    a_bad, _ = vla.predict_actions((long_flat, long_off), pixel_values=px_dev, proprio=pr_dev, unnorm_key=KEY, L=96)
    assert np.isnan(a_bad[1]).all() and bits_equal(a_bad[0], act[0]) and np.isfinite(a_bad[2]).all()
    # no host synchronisation on a replayed shape
    torch.cuda.synchronize()
    honoured = False
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).item()
        except RuntimeError:
            honoured = True
        if honoured:
            a_s, h_s = vla.predict_actions((flat, off), pixel_values=px_dev, proprio=pr_dev, unnorm_key=KEY, L=96, return_tensors=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if honoured:
        assert bits_equal(a_s.cpu().numpy(), act)
    else:
        print("torch.cuda.set_sync_debug_mode is not honoured by this build: the no-sync check did not run")


# ================================================================================================================ two images, raw frames
def test_two_image_raw_frames_center_crop():
    s = Served(fused=True)
    cfg, vla = s.cfg, s.vla
    assert cfg.n_img == 2 and len(cfg.vit) == 2
    g = torch.Generator().manual_seed(41)
    frames = torch.randint(0, 256, (2, 2, s.img, s.img, 3), generator=g, dtype=torch.uint8)
    prompts, _, proprio = s.sample([7, 15], 42)
    act, hid = vla.predict_actions(prompts, frames_u8=frames, center_crop=True, proprio=proprio, unnorm_key=KEY)
    hid = hid.clone()
    px = vla.input_stage().pixels(frames, center_crop=True)
    assert tuple(px.shape) == (2, s.C, s.img, s.img)
    plain = vla.input_stage().pixels(frames)
    assert not torch.equal(px, plain), "the crop must change the pixels for the check to mean anything"
    act2, hid2 = vla.predict_actions(prompts, pixel_values=px, proprio=proprio, unnorm_key=KEY)
    assert act.shape == (2, cfg.chunk, 7) and np.isfinite(act).all()
    assert bits_equal(act, act2) and tensor_bits_equal(hid, hid2)
    act3, _ = vla.predict_actions(prompts, pixel_values=plain, proprio=proprio, unnorm_key=KEY)
    assert not np.allclose(act3, act)
