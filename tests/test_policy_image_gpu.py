"""The evaluator's frame pipeline on the device (include/vla_policy_image.h) against the numpy rule (tests/policy_image_rule_np.py),
exact in every byte: the JPEG round trip, the lanczos3 resize, GPUInputStage.policy_frames end to end, predict_actions(policy_resize=
True) on the tiny two-image configuration, GPUInputStage(resize="lanczos3") and a short fine-tune with --frame_resize lanczos3.  The
rule itself is pinned to Pillow / libjpeg-turbo (round trip) and compared with Pillow's LANCZOS (resize) on the host
(tests/test_policy_image_cpu.py); TensorFlow's own last bits are pinned nowhere."""
import functools

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import policy_image_rule_np as P

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def stage():
    from vla_adapter_amd.input_stage import GPUInputStage
    return GPUInputStage(DEV)


def differ(got, want):
    return f"{(got != want).sum()} of {want.size} values differ, max |diff| {np.abs(got.astype(int) - want.astype(int)).max()}"


# ---------------------------------------------------------------------------------------------------------------- the round trip
@functools.lru_cache(maxsize=None)
def trip_images(H, W):
    """uint8 [3, H, W, 3] per content: N = 3 images of the kind, seeds 0 .. 2 (flat: three colours)."""
    out = {}
    for kind in JC.CONTENTS:
        imgs = [JC.content(kind, H, W, seed=s) for s in range(3)]
        if kind == "flat":
            imgs = [np.full((H, W, 3), c, np.uint8) for c in ((200, 30, 90), (0, 0, 0), (255, 255, 254))]
        if kind == "ramp":
            imgs = [imgs[0], imgs[0][::-1].copy(), imgs[0][:, ::-1, ::-1].copy()]
        out[kind] = np.stack(imgs)
    return out


@pytest.mark.parametrize("quality", [95, 30])
@pytest.mark.parametrize("H, W", [(16, 16), (32, 48), (48, 16), (256, 256)])
def test_the_round_trip_equals_the_rule(stage, H, W, quality):
    from vla_adapter_amd import input_stage as IS, ops
    qtab = torch.from_numpy(IS.jpeg_quant_tables(quality).view(np.int16).copy()).to(DEV)
    image = H * W * 3
    for kind, imgs in trip_images(H, W).items():
        want = np.stack([P.jpeg_round_trip(a, quality) for a in imgs])
        # an image stride larger than an image, once a multiple of 16 (uint4 loads) and once odd (byte loads)
        for pad in (16, 7):
            buf = torch.full((3, image + pad), 0xA5, dtype=torch.uint8, device=DEV)
            fr = buf[:, :image].view(3, H, W, 3)
            fr.copy_(torch.from_numpy(imgs))
            assert fr.stride(0) == image + pad
            got = ops.policy_jpeg_round_trip(fr, qtab).cpu().numpy()
            assert np.array_equal(got, want), f"{kind}, stride pad {pad}: {differ(got, want)}"
            assert torch.equal(fr.cpu(), torch.from_numpy(imgs)) and (buf[:, image:] == 0xA5).all(), "the input is left alone"
        assert np.array_equal(stage.jpeg_round_trip(torch.from_numpy(imgs), quality).cpu().numpy(), want), kind


def test_the_round_trip_refuses_partial_mcus(stage):
    for H, W in ((250, 256), (16, 24), (8, 16)):
        with pytest.raises(ValueError, match="multiples of 16"):
            stage.jpeg_round_trip(torch.zeros(1, H, W, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="multiples of 16"):
        stage.policy_frames(torch.zeros(1, 1, 250, 256, 3, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- the resize
@pytest.mark.parametrize("H, W, oh, ow", [(256, 256, 224, 224), (32, 48, 24, 40), (16, 16, 224, 224), (5, 7, 3, 4), (48, 32, 48, 24), (32, 48, 40, 48)],
                         ids=["256-to-224", "32x48-to-24x40", "16-to-224", "5x7-to-3x4", "horizontal-only", "vertical-only"])
def test_the_resize_equals_the_rule_on_noise(stage, H, W, oh, ow):
    imgs = np.stack([JC.content("noise", H, W, seed=s) for s in range(2)] + [JC.content("saturated", H, W)])
    want = np.stack([P.tf_lanczos3_resize(a, oh, ow) for a in imgs])
    got = stage.lanczos3_resize(torch.from_numpy(imgs), oh, ow).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), differ(got, want)
    if (H, W) == (256, 256):
        plain = np.stack([P._pass(P._pass(a.astype(np.float32), oh).transpose(1, 0, 2), ow).transpose(1, 0, 2) for a in imgs])
        assert (plain < -0.5).any() and (plain > 255.5).any(), "noise overshoots on both sides: the clamp is exercised"


def test_equal_sizes_launch_nothing(stage):
    fr = torch.from_numpy(JC.content("noise", 224, 224)).to(DEV)[None]
    assert stage.lanczos3_resize(fr, 224, 224) is fr


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def policy_case(size):
    """(frames uint8 [2, 2, 256, 256, 3], the rule's frames uint8 [2, 2, size, size, 3]): noise, ramp, saturated and a smooth scene."""
    g = np.random.default_rng(11)
    sm = np.kron(g.normal(128, 40, (16, 16, 3)), np.ones((16, 16, 1))) + g.normal(0, 6, (256, 256, 3))
    fr = np.stack([JC.content("noise", 256, 256), JC.content("ramp", 256, 256), JC.content("saturated", 256, 256),
                   np.clip(sm, 0, 255).astype(np.uint8)]).reshape(2, 2, 256, 256, 3)
    want = np.stack([P.policy_frame(a, size) for a in fr.reshape(4, 256, 256, 3)]).reshape(2, 2, size, size, 3)
    return fr, want


def test_policy_frames_equal_rule_after_rule(stage):
    fr, want = policy_case(224)
    got = stage.policy_frames(torch.from_numpy(fr))
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (2, 2, 224, 224, 3)
    assert np.array_equal(got.cpu().numpy(), want), differ(got.cpu().numpy(), want)
    as_list = stage.policy_frames([torch.from_numpy(fr[:, 0].copy()), torch.from_numpy(fr[:, 1].copy())])
    assert torch.equal(as_list, got), "the list form pixels() takes"
    # the processor behind it: the evaluator's crop on the device-made frames and on the host-made ones
    assert torch.equal(stage.pixels(got, center_crop=True), stage.pixels(torch.from_numpy(want), center_crop=True))
    # another size and quality
    small = stage.policy_frames(torch.from_numpy(fr[:1, :1]), size=56, quality=30).cpu().numpy()
    assert np.array_equal(small[0, 0], P.policy_frame(fr[0, 0], 56, 30))


def test_predict_actions_with_policy_resize_equals_the_rules_frames():
    """The tiny two-image configuration (56 x 56 images): 256 x 256 frames through policy_resize against the rule's 56 x 56 frames,
    center crop on both; a predict_action call before and after is bit-identical."""
    from tests.test_serve_gpu import KEY, Served, bits_equal, normalize_proprio_numpy, STATS, tensor_bits_equal
    s = Served(fused=True)
    vla, size = s.vla, s.img
    fr, want = policy_case(size)
    prompts, px, proprio = s.sample([7, 15], 42)
    pn = normalize_proprio_numpy(proprio, STATS[KEY]["proprio"], "bounds_q99").astype(np.float32)
    one = lambda: vla.predict_action(input_ids=torch.tensor(prompts[0]).view(1, -1), unnorm_key=KEY, proprio=pn[0], proprio_projector=True, action_head=True,
                                     pixel_values=px[0:1], attention_mask=torch.ones(1, len(prompts[0]), dtype=torch.bool))
    a0, h0 = one()
    h0 = h0.clone()
    act, hid = vla.predict_actions(prompts, frames_u8=torch.from_numpy(fr), center_crop=True, proprio=proprio, unnorm_key=KEY, policy_resize=True)
    hid = hid.clone()
    act2, hid2 = vla.predict_actions(prompts, frames_u8=torch.from_numpy(want), center_crop=True, proprio=proprio, unnorm_key=KEY)
    assert act.shape == (2, s.cfg.chunk, 7) and np.isfinite(act).all()
    assert bits_equal(act, act2) and tensor_bits_equal(hid, hid2.clone())
    act3, _ = vla.predict_actions(prompts, frames_u8=torch.from_numpy(fr), center_crop=True, proprio=proprio, unnorm_key=KEY)
    assert not np.allclose(act3, act), "the bicubic path gives other pixels: the comparison means something"
    a1, h1 = one()
    assert bits_equal(a0, a1) and tensor_bits_equal(h0, h1)
    with pytest.raises(ValueError, match="policy_resize"):
        vla.predict_actions(prompts, pixel_values=px, proprio=proprio, unnorm_key=KEY, policy_resize=True)


# ---------------------------------------------------------------------------------------------------------------- resize="lanczos3"
def test_the_lanczos3_stage_resizes_by_the_rule_and_the_default_stage_by_pillow():
    from PIL import Image
    from vla_adapter_amd.input_stage import GPUInputStage
    fr = np.stack([JC.content("noise", 32, 48, seed=s) for s in range(4)]).reshape(2, 2, 32, 48, 3)
    lz, default = GPUInputStage(DEV, resize="lanczos3"), GPUInputStage(DEV)
    rule = np.stack([P.tf_lanczos3_resize(a, 224, 224) for a in fr.reshape(4, 32, 48, 3)]).reshape(2, 2, 224, 224, 3)
    pil = np.stack([np.asarray(Image.fromarray(a).resize((224, 224), resample=Image.BICUBIC)) for a in fr.reshape(4, 32, 48, 3)]).reshape(2, 2, 224, 224, 3)
    assert not np.array_equal(rule, pil)
    for kw in (dict(), dict(center_crop=True)):
        assert torch.equal(lz.pixels(torch.from_numpy(fr), **kw), default.pixels(torch.from_numpy(rule), **kw)), kw
        assert torch.equal(default.pixels(torch.from_numpy(fr), **kw), default.pixels(torch.from_numpy(pil), **kw)), f"{kw}: the default stays Pillow's bicubic"
    # frames at the model's size: the mode changes nothing
    assert torch.equal(lz.pixels(torch.from_numpy(rule)), default.pixels(torch.from_numpy(rule)))


def test_finetune_with_frame_resize_lanczos3_equals_finetune_on_the_rules_frames(tmp_path):
    """Adapter-only on the tiny config (56 x 56 images), 2 steps at batch 4 from an episode file of raw 32 x 48 frames with
    --frame_resize lanczos3, against the same episodes with the rule's 56 x 56 frames: the same losses, bit for bit; the default
    flag on the 32 x 48 frames gives other losses (Pillow's bicubic)."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny"]()
    size, lengths, h, w = mcfg.vit[0].img, (9, 10, 12), 32, 48
    T = sum(lengths)
    frames = np.stack([JC.content("noise", h, w, seed=t) // 2 + JC.content("ramp", h, w) // 2 for t in range(T)])
    d = JC.episode_dict([JC.encode(frames[0], quality=90, subsampling=2)] * T, 1, h, w, lengths, A=mcfg.action_dim, Pd=mcfg.proprio_dim, raw=True)
    d["prompt_flat"], d["dataset_name"] = d["prompt_flat"] % 700, "toy"
    d["frames_u8"] = torch.from_numpy(frames.reshape(T, 1, h, w, 3).copy())
    torch.save(d, tmp_path / "native.pt")
    d["frames_u8"] = torch.from_numpy(np.stack([P.tf_lanczos3_resize(a, size, size) for a in frames]).reshape(T, 1, size, size, 3))
    torch.save(d, tmp_path / "rule.pt")
    args = lambda name, *more: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "1", "--learning_rate", "1e-3",
                                "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                                "--run_root_dir", str(tmp_path / ("run-" + name + "-".join(more))), "--max_seq_len", "96", "--seed", "5",
                                "--episode_file", str(tmp_path / f"{name}.pt"), *more]
    a = F.finetune(F.parse_args(args("native", "--frame_resize", "lanczos3")))
    b = F.finetune(F.parse_args(args("rule")))
    c = F.finetune(F.parse_args(args("native")))
    assert len(a["log"]) == 2 and a["log"] == b["log"], "the same losses, bit for bit"
    assert c["log"] != a["log"], "the default resize is another one"
