"""Image augmentation without a GPU: the fine-tune flags, the ABI 7 entry points and their host-side argument validation."""
import ctypes

import pytest

from vla_adapter_amd import finetune as F


@pytest.fixture(scope="module")
def lib():
    from tests.abi_headers import load_library
    return load_library()


def test_image_aug_is_honoured_with_a_frame_source(tmp_path):
    cfg = F.parse_args(["--use_proprio", "True", "--image_aug", "True", "--frame_batch_file", str(tmp_path)])
    F.check_supported(cfg, cfg._explicit)
    assert cfg.image_aug and cfg.frame_batch_file == str(tmp_path)
    cfg = F.parse_args(["--use_proprio", "True", "--image_aug", "False"])
    F.check_supported(cfg, cfg._explicit, frame_batches=True)          # finetune() handed an iterable: checked per batch


def test_image_aug_without_frames_is_still_refused():
    cfg = F.parse_args(["--use_proprio", "True", "--image_aug", "True"])
    with pytest.raises(NotImplementedError, match="frame_batch_file"):
        F.check_supported(cfg, cfg._explicit)
    cfg = F.parse_args(["--use_proprio", "True", "--batch_file", "a.pt", "--frame_batch_file", "b"])
    with pytest.raises(ValueError):
        F.check_supported(cfg, cfg._explicit)


def test_batches_without_frames_refuse_an_explicit_image_aug():
    import torch
    cfg = F.parse_args(["--use_proprio", "True", "--image_aug", "True"])
    stream = F.batch_stream(cfg, None, "cpu", 0, [{"pixel_values": torch.zeros(1, 3, 2, 2)}], cfg._explicit)
    with pytest.raises(NotImplementedError, match="cannot be augmented"):
        next(stream)


def test_backbone_norms_follow_the_model_config():
    from vla_adapter_amd import engine as E
    from vla_adapter_amd.input_stage import backbone_norms
    assert backbone_norms(E.tiny_config()) == ("siglip",)
    assert backbone_norms(E.tiny_fused_config()) == ("dino", "siglip")
    assert backbone_norms(E.dinosiglip_05b_config()) == ("dino", "siglip")
    assert backbone_norms(E.config2()) == ("siglip",)


def test_augment_settings_map_to_the_kernel_arguments():
    import numpy as np
    from vla_adapter_amd import ops
    from vla_adapter_amd.input_stage import ImageAugment, center_crop_params
    a = ImageAugment()
    assert a.mask() == ops.AUG_CROP | ops.AUG_BRIGHTNESS | ops.AUG_CONTRAST | ops.AUG_SATURATION | ops.AUG_HUE | ops.AUG_DRAW
    assert ImageAugment(ops=("random_hue",), params=object()).mask() == ops.AUG_HUE
    with pytest.raises(ValueError):
        ImageAugment(ops=("random_flip",)).mask()
    assert a.cfg7() == [float(np.sqrt(np.float32(0.9))), 0.2, 0.8, 1.2, 0.8, 1.2, 0.05]
    p = center_crop_params(2).numpy()
    side = np.sqrt(np.float32(0.9))
    assert p.shape == (2, 9) and p[0, 1] == p[0, 2] == (np.float32(1) - side) / np.float32(2) and p[1, 3] == p[0, 1] + side


def test_library_exports_the_augment_entry_points_at_abi_8(lib):
    from vla_adapter_amd import native
    assert lib.vla_version() == native.ABI_VERSION == 8          # (the augment entry points arrived in ABI 7)
    for name in ("vla_augment_slab_floats", "vla_augment_stats", "vla_augment_apply"):
        assert name in native.family("native").protos and hasattr(lib, name)
    # 224 x 224: 28 units of 8 pixels per row, 224 rows -> 25 chunks of 256 units per image, 3 channel sums each
    assert lib.vla_augment_slab_floats(64, 224, 224) == 64 * 25 * 3
    assert lib.vla_augment_slab_floats(0, 224, 224) == -1


def test_augment_argument_validation_without_gpu(lib):
    cfg = (ctypes.c_float * 7)(0.9486833, 0.2, 0.8, 1.2, 0.8, 1.2, 0.05)
    m = (ctypes.c_float * 6)(0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
    s = (ctypes.c_float * 6)(0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
    P = 4096                                   # never dereferenced: every call below fails on the host
    stats = lambda N, H, W, n_img, ops, c=cfg, slab=P: lib.vla_augment_stats(None, P, P, slab, N, H, W, n_img, ops, c, 0, 0, 0)
    apply = lambda N, H, W, n_img, nb, ops, slab=P, sd=s: lib.vla_augment_apply(None, P, P, slab, P, None, N, H, W, n_img, nb, m, sd, 0, ops, cfg, 0, 0, 0)
    assert stats(0, 224, 224, 1, 63) == -1 and b"N > 0" in lib.vla_last_error()
    assert stats(3, 224, 224, 2, 63) == -1 and b"multiple of n_img" in lib.vla_last_error()
    assert stats(2, 1, 224, 1, 63) == -1
    assert stats(2, 224, 224, 1, 64) == -1 and b"unknown op bits" in lib.vla_last_error()
    assert stats(2, 224, 224, 1, 63, slab=None) == -1 and b"null" in lib.vla_last_error()
    bad = (ctypes.c_float * 7)(1.5, 0.2, 0.8, 1.2, 0.8, 1.2, 0.05)
    assert stats(2, 224, 224, 1, 63, c=bad) == -1 and b"crop side" in lib.vla_last_error()
    assert apply(2, 224, 224, 1, 5, 63) == -1 and b"backbones" in lib.vla_last_error()
    assert apply(2, 224, 224, 1, 2, 63, slab=None) == -1 and b"slab" in lib.vla_last_error()
    z = (ctypes.c_float * 6)(0.5, 0.5, 0.0, 0.5, 0.5, 0.5)
    assert apply(2, 224, 224, 1, 2, 63, sd=z) == -1 and b"zero std" in lib.vla_last_error()
