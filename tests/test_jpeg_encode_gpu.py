"""The JPEG encoder on the device (include/vla_jpeg_encode.h, ops.jpeg_encode, jpeg_store.encode_tables): its bytes and offsets are
Pillow's on mixed corpus frames at every shape, strided and two-camera inputs included; noise at quality 100 - the largest files -
fits the workspace the size call reports; decoding the device's files with the existing store equals vla_policy_jpeg_round_trip of the
same frames; a store loaded from raw frames with jpeg_quality holds what the store loaded from the packed file holds and draws the same
batch; a fine-tune fed raw frames with --episode_jpeg_quality logs the state digests of the one fed the Pillow-packed file; and
tools/pack_episodes_jpeg.py --device cuda writes the Pillow path's tensors."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_encode_rule_np as E
from tests.arena import assert_bits_equal
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import input_stage as IS
from vla_adapter_amd import jpeg_store as JS
from vla_adapter_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 5


def pillow_store(frames: np.ndarray, quality: int, restart_rows: int):
    files = [E.pillow(f, quality, restart_rows) for f in frames]
    return b"".join(files), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


def assert_pillows(data: torch.Tensor, off: torch.Tensor, frames: np.ndarray, quality: int, restart_rows: int, what=""):
    want, want_off = pillow_store(frames, quality, restart_rows)
    assert off.dtype == torch.int64 and off.cpu().tolist() == want_off.tolist(), f"{what}: frame_off"
    got = bytes(data.cpu().numpy())
    assert len(got) == len(want) and got == want, f"{what}: first difference at byte {next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), None)}"


@pytest.mark.parametrize("quality, restart_rows", [(1, 1), (50, 2), (95, 1), (100, 1)])
@pytest.mark.parametrize("H, W", [(16, 16), (32, 48), (160, 16)])
def test_the_devices_bytes_are_pillows(H, W, quality, restart_rows):
    frames = E.mixed_frames(N, H, W)
    data, off = ops.jpeg_encode(torch.from_numpy(frames).to(DEV), quality, restart_rows)
    assert data.is_cuda and off.is_cuda and data.dtype == torch.uint8 and off.shape == (N + 1,)
    assert_pillows(data, off, frames, quality, restart_rows, f"{H}x{W} q{quality} r{restart_rows}")


@pytest.mark.parametrize("quality", [1, 95, 100])
def test_two_cameras_and_a_strided_view(quality):
    """[T, n_img, H, W, 3] in (t, cam) order, the images a stride apart that is larger than an image and no multiple of 16: the byte
    loads of the MCU stage."""
    T, n_img, H, W = 3, 2, 64, 64
    frames = E.mixed_frames(T * n_img, H, W)
    image = H * W * 3
    buf = torch.full((T * n_img, image + 7), 0x7F, dtype=torch.uint8, device=DEV)
    buf[:, :image] = torch.from_numpy(frames).to(DEV).view(T * n_img, image)
    view = buf[:, :image].view(T, n_img, H, W, 3)
    assert view.stride(1) == image + 7 and not view.is_contiguous()
    data, off = ops.jpeg_encode(view, quality, 1)
    assert_pillows(data, off, frames, quality, 1, "strided")
    data2, off2 = ops.jpeg_encode(torch.from_numpy(frames).to(DEV).view(T, n_img, H, W, 3), quality, 1)
    assert_bits_equal(data2, data, "compact and strided")
    assert_bits_equal(off2, off, "compact and strided: frame_off")


def test_noise_at_quality_100_fits_the_reported_workspace():
    """The largest files the forward half can produce stay inside the bit buffer's bound (csrc/jpeg_encode.hip: THE BOUND) and inside
    the workspace of the size call: an interval of 84 blocks takes two rounds of the buffer, the unfinished byte carried over."""
    H = W = 224
    frames = np.stack([E.noise(H, W, seed=s) for s in range(2)])
    need = ops._lib().vla_jpeg_encode_workspace_bytes(2, H, W, 1)
    assert need == 2 * H * W * 3 + 2 * 14 * 12
    data, off = ops.jpeg_encode(torch.from_numpy(frames).to(DEV), 100, 1)
    assert_pillows(data, off, frames, 100, 1, "noise q100")
    per_mcu = (np.diff(off.cpu().numpy()) - 629) / (14 * 14)
    assert per_mcu.max() <= 6 * 2 * 216, "inside 216 bytes a block, doubled by stuffing"
    print(f"noise 224 x 224 at quality 100: {per_mcu.max():.1f} bytes an MCU of the bound's {6 * 2 * 216}")


def test_the_refusals():
    fr = torch.zeros(1, 32, 48, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="restart_rows"):
        ops.jpeg_encode(fr, 95, 0)
    with pytest.raises(ValueError, match="multiples of 16"):
        ops.jpeg_encode(fr[:, :24], 95, 1)
    with pytest.raises(ValueError, match="quality"):
        ops.jpeg_encode(fr, 0, 1)


def test_the_two_halves_agree():
    """Decoding the device's files with the store's decode equals the round trip without an entropy coder, bit for bit."""
    T, n_img, H, W, quality = 6, 1, 32, 48, 95
    frames = E.mixed_frames(T, H, W)
    fr = torch.from_numpy(frames).to(DEV)
    data, off = ops.jpeg_encode(fr, quality, 1)
    jf = JS.JpegFrames(dict(frames_jpeg=data, frame_off=off.cpu(), frame_shape=torch.tensor([n_img, H, W])), DEV)
    assert jf.max_seg == 2 and jf.h2v2 == 1
    out = torch.empty(T, n_img, H, W, 3, dtype=torch.uint8, device=DEV)
    ep, row = torch.zeros(T, dtype=torch.int32, device=DEV), torch.arange(T, dtype=torch.int64, device=DEV)
    status = jf.decode(torch.tensor([0, T], dtype=torch.int64, device=DEV), T, ep, row, out)
    assert not status.any()
    qtab = torch.from_numpy(IS.jpeg_quant_tables(quality).view(np.int16).copy()).to(DEV)
    assert_bits_equal(out.view(T, H, W, 3), ops.policy_jpeg_round_trip(fr, qtab), "decode of the encode against the round trip")


# ---------------------------------------------------------------------------------------------------------------- the store
LENGTHS, N_IMG, H, W, CHUNK = (9, 3, 12, 10), 2, 32, 48, 8


def raw_episodes(lengths=LENGTHS, n_img=N_IMG, h=H, w=W, A=7, Pd=8, name="corpus") -> dict:
    T = sum(lengths)
    d = JC.episode_dict([b""] * (T * n_img), n_img, h, w, lengths, A=A, Pd=Pd)
    for k in JS.JPEG_KEYS:
        del d[k]
    d["frames_u8"] = torch.from_numpy(E.mixed_frames(T * n_img, h, w).reshape(T, n_img, h, w, 3).copy())
    d["dataset_name"] = name
    return d


def pack_tool():
    sys.path.insert(0, os.path.join(JC.ROOT, "tools"))
    try:
        import pack_episodes_jpeg as T
    finally:
        sys.path.pop(0)
    return T


def test_a_store_loaded_with_jpeg_quality_is_the_store_of_the_packed_file(tmp_path):
    raw = raw_episodes()
    torch.save(raw, tmp_path / "raw.pt")
    torch.save(pack_tool().pack(raw, 95, "4:2:0", 1), tmp_path / "packed.pt")
    a = EP.EpisodeStore.load(tmp_path / "raw.pt", DEV, chunk=CHUNK, jpeg_quality=95)
    b = EP.EpisodeStore.load(tmp_path / "packed.pt", DEV, chunk=CHUNK)
    assert a.jpeg is not None and b.jpeg is not None
    assert_bits_equal(a.jpeg.bytes, b.jpeg.bytes, "frames_jpeg")
    for k in ("img_seg", "seg_tab", "img_tab", "qt_pool", "ht_pool"):
        assert_bits_equal(getattr(a.jpeg, k), getattr(b.jpeg, k), k)
    sa, sb = a.sample(7, 5, 1, 2, 3), b.sample(7, 5, 1, 2, 3)
    assert sa.keys() == sb.keys()
    for k in sa:
        if isinstance(sa[k], torch.Tensor):
            assert_bits_equal(sa[k], sb[k], k)
    c = EP.EpisodeStore.load(tmp_path / "packed.pt", DEV, chunk=CHUNK, jpeg_quality=50)
    assert_bits_equal(c.jpeg.bytes, b.jpeg.bytes, "the argument does nothing to a store already in the JPEG form")
    sliced = JS.encode_tables(raw, DEV, 95, slice_frames=5)
    whole = JS.encode_tables(raw, DEV, 95)
    assert_bits_equal(sliced["frames_jpeg"], whole["frames_jpeg"], "slices of 5 steps")
    assert torch.equal(sliced["frame_off"], whole["frame_off"])
    assert torch.equal(whole["frame_off"], torch.load(tmp_path / "packed.pt")["frame_off"]) and whole["frame_shape"].tolist() == [N_IMG, H, W]


def test_finetune_from_raw_frames_with_the_flag_equals_finetune_from_the_packed_file(tmp_path):
    """Adapter-only on the tiny config, 2 steps at batch 4 from --episode_file: raw.pt with --episode_jpeg_quality 95 and the file the
    pack tool's Pillow path writes log equal state_digest strings (and losses)."""
    from vla_adapter_amd import engine as EG, finetune as F
    mcfg = EG.NAMED_CONFIGS["tiny"]()
    raw = raw_episodes((9, 10, 12), 1, 48, 64, A=mcfg.action_dim, Pd=mcfg.proprio_dim, name="toy")
    raw["prompt_flat"] = raw["prompt_flat"] % 700
    torch.save(raw, tmp_path / "raw.pt")
    torch.save(pack_tool().pack(raw, 95, "4:2:0", 1), tmp_path / "packed.pt")
    args = lambda name: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "2", "--learning_rate", "1e-3",
                         "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                         "--run_root_dir", str(tmp_path / name), "--max_seq_len", "96", "--seed", "5", "--log_state_digest", "True",
                         "--episode_file", str(tmp_path / f"{name}.pt")]
    a = F.finetune(F.parse_args(args("raw") + ["--episode_jpeg_quality", "95"]))
    b = F.finetune(F.parse_args(args("packed")))
    assert len(a["log"]) == len(b["log"]) >= 2 and all(l["state_digest"] for l in a["log"])
    assert [l["state_digest"] for l in a["log"]] == [l["state_digest"] for l in b["log"]]
    strip = lambda log: [{k: v for k, v in l.items() if k != "jpeg_bad_segments"} for l in log]
    assert strip(a["log"]) == strip(b["log"]), "losses too"


def test_the_pack_tool_on_the_device_writes_the_pillow_paths_file(tmp_path, capsys):
    T = pack_tool()
    raw = raw_episodes()
    torch.save(raw, tmp_path / "raw.pt")
    T.main([str(tmp_path / "raw.pt"), str(tmp_path / "dev.pt"), "--device", DEV])
    T.main([str(tmp_path / "raw.pt"), str(tmp_path / "cpu.pt")])
    assert '"device": "cuda:0"' in capsys.readouterr().out
    a, b = torch.load(tmp_path / "dev.pt"), torch.load(tmp_path / "cpu.pt")
    assert a.keys() == b.keys() and "frames_u8" not in a
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert not a[k].is_cuda and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k
