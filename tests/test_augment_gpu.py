"""Training-time image augmentation and the evaluator's center crop on the GPU input stage (vla_augment_stats / _apply).

TF and dlimp are not installed, so the reference's ops are restated here in float32 numpy, formula by formula in the order the
kernel evaluates them (tf.image.convert_image_dtype, crop_and_resize's bilinear sampler, adjust_brightness / _contrast, the
fused AdjustSaturation / AdjustHue HSV round trip, the saturating uint8 conversion): parity with TF itself is unpinned
(DESIGN.md section 8); the kernel is checked against this restatement."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
INV255 = F(1.0 / 255.0)
ALL = ("random_resized_crop", "random_brightness", "random_contrast", "random_saturation", "random_hue")


def _clip(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def ref_crop_and_resize(x, y1, x1, y2, x2):
    """tf.image.crop_and_resize of one box back to the image's own size, bilinear, extrapolation value 0 (x: f32 [H, W, 3])."""
    H, W = x.shape[:2]
    hs = (y2 - y1) * F(H - 1) / F(H - 1)
    ws = (x2 - x1) * F(W - 1) / F(W - 1)
    in_y = y1 * F(H - 1) + np.arange(H, dtype=F) * hs
    in_x = x1 * F(W - 1) + np.arange(W, dtype=F) * ws
    vy = (in_y >= 0) & (in_y <= F(H - 1))
    vx = (in_x >= 0) & (in_x <= F(W - 1))
    ty = np.where(vy, np.floor(in_y), 0).astype(np.int64)
    by = np.where(vy, np.minimum(np.ceil(in_y), H - 1), 0).astype(np.int64)
    lx = np.where(vx, np.floor(in_x), 0).astype(np.int64)
    rx = np.where(vx, np.minimum(np.ceil(in_x), W - 1), 0).astype(np.int64)
    yl = (in_y - np.floor(in_y))[:, None, None]
    xl = (in_x - np.floor(in_x))[None, :, None]
    tl, tr = x[ty][:, lx], x[ty][:, rx]
    bl, br = x[by][:, lx], x[by][:, rx]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    out = top + (bot - top) * yl
    return np.where((vy[:, None] & vx[None, :])[..., None], _clip(out), F(0))


def rgb_to_hsv(r, g, b):
    v = np.maximum(r, np.maximum(g, b))
    rng = v - np.minimum(r, np.minimum(g, b))
    s = np.where(v > 0, rng / np.where(v > 0, v, F(1)), F(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        n = F(1) / (F(6) * rng)
        h = np.where(r == v, n * (g - b), np.where(g == v, n * (b - r) + F(2) / F(6), n * (r - g) + F(4) / F(6)))
    h = np.where(rng > 0, h, F(0))
    h = np.where(h < 0, h + F(1), h)
    return h.astype(F), s.astype(F), v


def hsv_to_rgb(h, s, v):
    c = s * v
    m = v - c
    dh = h * F(6)
    k = np.clip(np.floor(dh), 0, 5).astype(np.int64)
    x = c * (F(1) - np.abs(np.fmod(dh, F(2)) - F(1)))
    z = np.zeros_like(c)
    rr = np.choose(k, [c, x, z, z, x, c])
    gg = np.choose(k, [x, c, c, x, z, z])
    bb = np.choose(k, [z, z, x, c, c, x])
    return rr + m, gg + m, bb + m


def ref_augment(img_u8, p, ops=ALL):
    """One image, uint8 [H, W, 3] -> uint8 [H, W, 3]; p = the 9 parameters (ops.AUG_P_* columns)."""
    x = img_u8.astype(F) * INV255
    if "random_resized_crop" in ops:
        x = ref_crop_and_resize(x, p[1], p[2], p[3], p[4])
    if "random_brightness" in ops:
        x = _clip(x + p[5])
    if "random_contrast" in ops:
        mean = x.astype(np.float64).mean(axis=(0, 1)).astype(F)
        x = _clip((x - mean) * p[6] + mean)
    if "random_saturation" in ops:
        h, s, v = rgb_to_hsv(x[..., 0], x[..., 1], x[..., 2])
        x = _clip(np.stack(hsv_to_rgb(h, np.minimum(np.maximum(s * p[7], F(0)), F(1)), v), -1))
    if "random_hue" in ops:
        h, s, v = rgb_to_hsv(x[..., 0], x[..., 1], x[..., 2])
        t = h + p[8]
        t = np.where(t < 0, t + F(1), np.where(t >= 1, t - F(1), t))
        x = _clip(np.stack(hsv_to_rgb(t, s, v), -1))
    return np.minimum(x * F(255.5), F(255)).astype(np.uint8)


def mapping(u, aug):
    """The draw mapping restated: every parameter = (hi - lo) * u + lo in f32 from the same u."""
    u = np.asarray(u, F)
    side = np.sqrt(F(aug.crop_scale))
    uni = lambda lo, hi: (F(hi) - F(lo)) * u + F(lo)
    off = (F(1) - side) * u + F(0)
    return np.stack([u, off, off, off + side, off + side, uni(-aug.brightness, aug.brightness), uni(*aug.contrast),
                     uni(*aug.saturation), uni(-aug.hue, aug.hue)], -1)


def _frames(B, n_img, H, W, seed, flat_every=0):
    g = torch.Generator().manual_seed(seed)
    fr = torch.randint(0, 256, (B, n_img, H, W, 3), generator=g, dtype=torch.uint8)
    if flat_every:                       # some flat images (zero range: the hue / saturation edge cases, mean == every pixel)
        fr[::flat_every] = torch.randint(0, 256, (1, 1, 1, 3), generator=g, dtype=torch.uint8)
    return fr


def _normalise(stage, fr5):
    return stage.pixels(list(fr5.to(DEV).unbind(1)))


@pytest.mark.parametrize("size", [224, 56])
def test_center_crop_is_bit_exact_and_ends_in_the_existing_normalise(size):
    from vla_adapter_amd.input_stage import GPUInputStage, center_crop_params
    st = GPUInputStage(DEV, backbones=("dino", "siglip"), image_size=size)
    fr = _frames(3, 2, size, size, seed=11)
    px, aux = st.pixels(fr, center_crop=True, return_aux=True)
    got = aux["frames_u8"].cpu().numpy()
    p = center_crop_params(1)[0].numpy()
    for b in range(3):
        for im in range(2):
            want = ref_augment(fr[b, im].numpy(), p, ops=("random_resized_crop",))
            assert np.array_equal(got[b, im], want), (b, im, int((got[b, im] != want).sum()))
    assert not np.array_equal(got, fr.numpy()), "the crop must change the frames"
    assert torch.equal(px, _normalise(st, aux["frames_u8"]))
    assert torch.equal(px, st.pixels(fr, center_crop=True))          # without the auxiliary outputs: same bits


@pytest.mark.parametrize("size", [224, 56])
def test_crop_and_brightness_with_supplied_parameters_are_bit_exact(size):
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    st = GPUInputStage(DEV, backbones=("siglip",), image_size=size, out_dtype=torch.float32)
    B, n_img = 4, 2
    fr = _frames(B, n_img, size, size, seed=12)
    aug = ImageAugment()
    u = np.linspace(0, 1, B * n_img, dtype=F)
    params = torch.from_numpy(mapping(u, aug))
    aug = ImageAugment(ops=("random_resized_crop", "random_brightness"), params=params)
    px, aux = st.pixels(fr, augment=aug, return_aux=True)
    got = aux["frames_u8"].cpu().numpy()
    for n in range(B * n_img):
        want = ref_augment(fr[n // n_img, n % n_img].numpy(), params[n].numpy(), ops=aug.ops)
        assert np.array_equal(got[n // n_img, n % n_img], want), n
    assert torch.equal(aux["params"].cpu().reshape(-1, 9), params)
    assert torch.equal(px, _normalise(st, aux["frames_u8"]))


@pytest.mark.parametrize("size", [224, 56])
def test_full_chain_matches_the_restatement(size):
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    st = GPUInputStage(DEV, backbones=("dino", "siglip"), image_size=size)
    B, n_img = 6, 2
    fr = _frames(B, n_img, size, size, seed=13, flat_every=3)
    u = np.concatenate([[0, 1], np.linspace(0, 1, B * n_img - 2)]).astype(F)        # both ends of the u range
    params = torch.from_numpy(mapping(u, ImageAugment()))
    px, aux = st.pixels(fr, augment=ImageAugment(params=params), return_aux=True)
    got = aux["frames_u8"].cpu().numpy().astype(np.int32)
    want = np.stack([np.stack([ref_augment(fr[b, im].numpy(), params[b * n_img + im].numpy()) for im in range(n_img)]) for b in range(B)])
    d = np.abs(got - want.astype(np.int32))
    assert d.max() <= 1, d.max()
    assert (d == 0).mean() >= 0.999, (d == 0).mean()
    assert not np.array_equal(got, fr.numpy().astype(np.int32))
    assert torch.equal(px, _normalise(st, aux["frames_u8"]))


def test_disabled_ops_are_skipped_not_run_neutral():
    """An op mask of nothing is the plain normalise (convert -> quantise is the identity on uint8), bit for bit."""
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    st = GPUInputStage(DEV, backbones=("dino", "siglip"), image_size=56)
    fr = _frames(3, 2, 56, 56, seed=14)
    px, aux = st.pixels(fr, augment=ImageAugment(ops=()), return_aux=True)
    assert torch.equal(aux["frames_u8"].cpu(), fr)
    assert torch.equal(px, _normalise(st, fr))


def test_draws_are_uniform_follow_the_mapping_and_depend_on_every_key():
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    st = GPUInputStage(DEV, backbones=("siglip",), image_size=8)
    B, n_img = 2048, 2                                                       # 4096 images
    fr = _frames(B, n_img, 8, 8, seed=15)

    def draw(**key):
        _, aux = st.pixels(fr, augment=ImageAugment(**key), return_aux=True)
        return aux["params"].cpu().numpy().reshape(-1, 9)
    p = draw(seed=3, rank=0, step=0)
    u = p[:, 0]
    assert np.all(u * F(1 << 24) == np.floor(u * F(1 << 24))) and u.min() >= 0 and u.max() < 1     # 24-bit variates
    assert abs(u.mean() - 0.5) < 0.02
    assert np.all(np.histogram(u, bins=10, range=(0, 1))[0] > 0)
    assert np.array_equal(p, mapping(u, ImageAugment()))                                        # the mapping, exactly
    assert len(np.unique(u)) > 4000
    assert not np.array_equal(u.reshape(B, n_img)[:, 0], u.reshape(B, n_img)[:, 1])            # image
    assert not np.array_equal(u.reshape(B, n_img)[0], u.reshape(B, n_img)[1])                  # sample
    for key in (dict(seed=4, rank=0, step=0), dict(seed=3, rank=1, step=0), dict(seed=3, rank=0, step=1)):
        q = draw(**key)[:, 0]
        assert (q != u).mean() > 0.99, key
    assert np.array_equal(draw(seed=3, rank=0, step=0), p)


def test_same_key_gives_bit_identical_outputs():
    from vla_adapter_amd.input_stage import GPUInputStage, ImageAugment
    st = GPUInputStage(DEV, backbones=("dino", "siglip"), image_size=224)
    fr = _frames(8, 2, 224, 224, seed=16)
    a, aa = st.pixels(fr, augment=ImageAugment(seed=5, rank=2, step=7), return_aux=True)
    b, ab = st.pixels(fr, augment=ImageAugment(seed=5, rank=2, step=7), return_aux=True)
    assert torch.equal(a, b) and torch.equal(aa["frames_u8"], ab["frames_u8"]) and torch.equal(aa["params"], ab["params"])
    c = st.pixels(fr, augment=ImageAugment(seed=5, rank=2, step=8))
    assert not torch.equal(a, c)
    # the drawn parameters, supplied back, reproduce the drawn run
    d = st.pixels(fr, augment=ImageAugment(params=aa["params"]))
    assert torch.equal(a, d)


# ---- through finetune() ------------------------------------------------------------------------------------------------
def _frame_batches(mcfg, n, B=3, seed0=900):
    from vla_adapter_amd import synthetic as S
    out = []
    for i in range(n):
        b = S.make_batch(mcfg, B, DEV, seed=seed0 + i, P=24, ragged=True)
        del b["pixel_values"]
        g = torch.Generator().manual_seed(seed0 + i)
        b["frames_u8"] = torch.randint(0, 256, (B, mcfg.n_img, mcfg.vit[0].img, mcfg.vit[0].img, 3), generator=g, dtype=torch.uint8)
        out.append(b)
    return out


def _prenormalised(mcfg, frame_batches):
    from vla_adapter_amd.input_stage import GPUInputStage, backbone_norms
    st = GPUInputStage(DEV, backbones=backbone_norms(mcfg), image_size=mcfg.vit[0].img)
    out = []
    for b in frame_batches:
        c = {k: v for k, v in b.items() if k != "frames_u8"}
        c["pixel_values"] = st.pixels(list(b["frames_u8"].to(DEV).unbind(1)))
        out.append(c)
    return out


def _args(backbone, mode, graph, tmp, extra=()):
    n_img = "2" if backbone == "tiny_fused" else "1"
    return (["--tiny", "true", "--backbone", backbone, "--num_images_in_input", n_img, "--batch_size", "3", "--max_steps", "3",
             "--learning_rate", "1e-3", "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True",
             "--use_graph", graph, "--run_root_dir", str(tmp)] + (["--use_lora", "True", "--lora_rank", "16"] if mode == "lora" else ["--use_fz", "True"])
            + list(extra))


def _losses(out):
    return [(l["loss_value"], l["curr_action_l1_loss"], l["next_actions_l1_loss"]) for l in out["log"]]


@pytest.mark.parametrize("backbone", ["tiny", "tiny_fused"])
@pytest.mark.parametrize("mode", ["adapter", "lora"])
@pytest.mark.parametrize("graph", ["true", "false"])
def test_frame_batches_without_augmentation_equal_prenormalised_batches(tmp_path, backbone, mode, graph):
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS[backbone]()
    fb = _frame_batches(mcfg, 3)
    a = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "a", ["--image_aug", "False"])), batches=fb)
    b = F.finetune(F.parse_args(_args(backbone, mode, graph, tmp_path / "b")), batches=_prenormalised(mcfg, fb))
    assert len(a["log"]) == 4 and _losses(a) == _losses(b)


@pytest.mark.parametrize("backbone", ["tiny", "tiny_fused"])
def test_augmented_training_is_seeded_and_differs_from_plain(tmp_path, backbone):
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS[backbone]()
    fb = _frame_batches(mcfg, 3)
    run = lambda name, extra: F.finetune(F.parse_args(_args(backbone, "lora", "true", tmp_path / name, extra)), batches=fb)
    plain = run("plain", ["--image_aug", "False"])
    aug = run("aug", ["--image_aug", "True"])
    again = run("again", ["--image_aug", "True"])
    assert all(np.isfinite(x) for l in _losses(aug) for x in l)
    assert _losses(aug) == _losses(again)
    assert _losses(aug) != _losses(plain)
    # --frame_batch_file: the same batches from disk (one rank: files in sorted order) give the same run
    d = tmp_path / "frames"
    d.mkdir()
    for i, b in enumerate(fb):
        torch.save({k: v.cpu() for k, v in b.items()}, d / f"{i:03d}.pt")
    from_file = F.finetune(F.parse_args(_args(backbone, "lora", "true", tmp_path / "file", ["--image_aug", "True", "--frame_batch_file", str(d)])))
    assert _losses(from_file) == _losses(aug)


def test_seed_changes_the_augmentation_and_nothing_else_in_the_stream():
    """batch_stream with frame batches: --seed picks the draws (a different seed augments differently), --image_aug False gives the
    plain normalise whatever the seed, and consecutive micro-steps of one rank draw afresh."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny_fused"]()
    fb = _frame_batches(mcfg, 1)
    px = lambda argv: [next(s)["pixel_values"] for s in [F.batch_stream(F.parse_args(argv), mcfg, DEV, 0, fb)] for _ in range(2)]
    a0, a1 = px(["--seed", "0"])
    b0, _ = px(["--seed", "1"])
    p0, p1 = px(["--seed", "0", "--image_aug", "False"])
    q0, _ = px(["--seed", "1", "--image_aug", "False"])
    assert not torch.equal(a0, b0) and not torch.equal(a0, a1)
    assert torch.equal(p0, q0) and torch.equal(p0, p1)
    assert torch.equal(a0, px(["--seed", "0"])[0])
