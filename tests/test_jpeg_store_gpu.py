"""A store of JPEG frames against its raw twin - the same episodes with the Pillow-decoded frames as frames_u8: EpisodeStore.sample,
EpisodeMix.sample and a fine-tune with a held-out sweep return bit-identical batches, digests, losses and validation entries;
verify_frames passes on the good store and names the frame of a truncated scan; a captured graph holds the decode."""
import pytest
import torch

from tests import jpeg_cases as JC
from tests.arena import assert_bits_equal
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import mixture as MX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS, N_IMG, H, W, CHUNK = (9, 3, 12, 10, 14), 2, 32, 48, 8


def files_of(lengths=LENGTHS, n_img=N_IMG, h=H, w=W, seed=0):
    """Frames that mix three table sets (q50, q95, q95 with optimised tables) and files with and without restart markers."""
    kws = [dict(quality=50), dict(quality=95), dict(quality=95, optimize=True), dict(quality=90, restart_marker_rows=1)]
    return [JC.encode(JC.content(("noise", "ramp", "saturated")[i % 3], h, w, seed=seed + i), subsampling=2, **kws[i % 4])
            for i in range(sum(lengths) * n_img)]


@pytest.fixture(scope="module")
def twins():
    files = files_of()
    return files, JC.episode_dict(files, N_IMG, H, W, LENGTHS), JC.episode_dict(files, N_IMG, H, W, LENGTHS, raw=True)


def same_batch(a: dict, b: dict, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert_bits_equal(a[k], b[k], f"{what}: {k}")
        else:
            assert a[k] == b[k], (what, k)


def test_sample_equals_the_raw_twins(twins):
    _, jd, rd = twins
    a, b = EP.EpisodeStore.from_dict(jd, DEV, chunk=CHUNK), EP.EpisodeStore.from_dict(rd, DEV, chunk=CHUNK)
    assert a.jpeg.max_seg == 2 and a.N == b.N
    for B, seed, rank, world, step in ((4, 5, 0, 1, 0), (7, 5, 1, 2, 3), (32, 9, 2, 3, 11), (1, 0, 0, 1, 40)):
        same_batch(a.sample(B, seed, rank, world, step), b.sample(B, seed, rank, world, step), (B, seed, rank, world, step))
        assert a.decode_status.shape == (B, N_IMG, 2) and not a.decode_status.any()
    assert a.verify_frames(batch=16) == sum(LENGTHS) * N_IMG


def test_a_mix_equals_the_raw_twins():
    fa, fb = files_of((9, 12), seed=100), files_of((5, 11, 10), seed=200)
    mk = lambda f, l, raw, name: dict(JC.episode_dict(f, N_IMG, H, W, l, raw=raw, seed=len(l)), dataset_name=name)
    a = MX.EpisodeMix.from_dicts([(mk(fa, (9, 12), False, "a"), 1.0), (mk(fb, (5, 11, 10), False, "b"), 0.5)], DEV, chunk=CHUNK)
    b = MX.EpisodeMix.from_dicts([(mk(fa, (9, 12), True, "a"), 1.0), (mk(fb, (5, 11, 10), True, "b"), 0.5)], DEV, chunk=CHUNK)
    for B, seed, rank, world, step in ((6, 5, 0, 1, 0), (32, 7, 1, 2, 5)):
        same_batch(a.sample(B, seed, rank, world, step), b.sample(B, seed, rank, world, step), (B, seed, rank, world, step))
    with pytest.raises(ValueError, match="stores its frames as raw"):
        MX.EpisodeMix.from_dicts([(mk(fa, (9, 12), False, "a"), 1.0), (mk(fb, (5, 11, 10), True, "b"), 0.5)], DEV, chunk=CHUNK)


def test_verify_frames_names_the_frame_of_a_truncated_scan(twins):
    files, _, _ = twins
    files = list(files)
    head, scan, tail = JC.split_scan(files[13])
    files[13] = head + scan[:len(scan) // 2] + tail
    st = EP.EpisodeStore.from_dict(JC.episode_dict(files, N_IMG, H, W, LENGTHS), DEV, chunk=CHUNK)
    with pytest.raises(ValueError, match=r"verify_frames: frame 13 \(step 6, image 1\), segment \d: the segment runs out of bytes"):
        st.verify_frames(batch=16)


def test_a_captured_graph_holds_the_decode(twins):
    _, jd, rd = twins
    a = EP.EpisodeStore.from_dict(jd, DEV, chunk=CHUNK)
    B = 6
    buf = a._buffers(B)
    ep, row, off = a.sample_indices(B, 5, 0, 1, 0)
    a.gather(ep, row, off, buf)                                 # warm-up: every buffer exists before the capture
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            a.gather(ep, row, off, buf)
    torch.cuda.synchronize()
    for step in (3, 8):
        a.sample_indices(B, 5, 0, 1, step)                      # new windows in the same index buffers
        buf["frames_u8"].fill_(0x7F)
        g.replay()
        torch.cuda.synchronize()
        rows = buf["row"].tolist()
        assert torch.equal(buf["frames_u8"].cpu(), rd["frames_u8"][rows]), f"step {step}"


def test_finetune_from_a_jpeg_file_equals_finetune_from_its_raw_twin(tmp_path):
    """Adapter-only on the tiny config, 3 steps at batch 4 from --episode_file, with the state digests logged and a held-out sweep every
    2 steps: the same digests, losses and validation entries for the JPEG file and its raw twin (48 x 64 frames, resized to the
    model's 56 x 56 by the input stage behind the decode)."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny"]()
    lengths, h, w = (9, 10, 12, 11, 14), 48, 64
    files = files_of(lengths, 1, h, w, seed=7)
    for raw in (False, True):
        d = JC.episode_dict(files, 1, h, w, lengths, A=mcfg.action_dim, Pd=mcfg.proprio_dim, raw=raw)
        d["prompt_flat"], d["dataset_name"] = d["prompt_flat"] % 700, "toy"
        torch.save(d, tmp_path / ("raw.pt" if raw else "jpeg.pt"))
    args = lambda name: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "2", "--learning_rate", "1e-3",
                         "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                         "--run_root_dir", str(tmp_path / name), "--max_seq_len", "96", "--seed", "5", "--log_state_digest", "True",
                         "--use_val_set", "True", "--val_episode_fraction", "0.4", "--val_freq", "2", "--episode_file", str(tmp_path / f"{name}.pt")]
    a = F.finetune(F.parse_args(args("jpeg") + ["--verify_frames", "True"]))
    b = F.finetune(F.parse_args(args("raw")))
    assert len(a["log"]) == 3 and all(l["jpeg_bad_segments"] == 0 for l in a["log"]) and not any("jpeg_bad_segments" in l for l in b["log"])
    strip = lambda log: [{k: v for k, v in l.items() if k != "jpeg_bad_segments"} for l in log]
    assert strip(a["log"]) == b["log"], "losses and state digests"
    assert all(l["state_digest"] for l in a["log"]) and a["val_log"] and a["val_log"] == b["val_log"] and a["heldout"] == b["heldout"]
