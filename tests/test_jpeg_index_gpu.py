"""The scan index on the device (csrc/jpeg_index.hip, vla_jpeg_decode_rows_at of csrc/jpeg.hip, include/vla_jpeg_index.h): the tables
vla_jpeg_index_build writes equal the host program's (tests/jpeg_index_cases.py; tests/test_jpeg_index_cpu.py runs it under the
sanitizers and pins it to the plain-Python rule) word for word, for both build mappings and with the build cut into slices; the
indexed decode equals the un-indexed decode equals Pillow for both decode mappings, staged pieces beside one longer than STAGE_BYTES
in one launch; files with a marker per row are left alone; a store, a mix, a captured graph, a held-out sweep and a fine-tune give the
same bits with and without the index; damaged scans give the host program's pixels and per-piece status, and verify_frames names the
frame."""
import json

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_index_cases as IC
from tests.arena import assert_bits_equal
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import jpeg_store as JS
from vla_adapter_amd import mixture as MX
from vla_adapter_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STORES = {**{k: [c[3] for c in v] for k, v in JC.stores_of_the_matrix().items()},
          **{k + ("crafted",): [c.data for c in v] for k, v in JC.crafted_stores(JC.crafted_corpus()).items()},
          **{k + ("long",): [c.data for c in v] for k, v in JC.crafted_stores(JC.long_corpus()).items()}}


def key_id(k):
    return f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}" + (f"-{k[3]}" if len(k) > 3 else "")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return IC.build_index_program(tmp_path_factory.mktemp("jpeg_index"))


def device_index(jf: JS.JpegFrames, plan, piece_mcus: int, mapping: int, step: int = None):
    """vla_jpeg_index_build of the whole store, `step` segments per launch -> (seg_tab, seg_ent, index status) on the device; the
    outputs start as 0x55 bytes, as the host program's do."""
    piece_off, _, S2, _ = plan
    S = jf.index.seg_tab.shape[0]
    seg = torch.full((S2, 4), 0x5555555555555555, dtype=torch.int64, device=DEV)
    ent = torch.full((S2, 4), 0x55555555, dtype=torch.int32, device=DEV)
    st = torch.full((S,), 0x55, dtype=torch.uint8, device=DEV)
    po = torch.from_numpy(np.ascontiguousarray(piece_off)).to(DEV)
    step = step or S
    for s0 in range(0, S, step):
        ops.jpeg_index_build(jf.bytes, jf.img_seg, jf.seg_tab, jf.img_tab, jf.qt_pool, jf.ht_pool, jf.H, jf.W, jf.h2v2, piece_mcus, po, s0, min(s0 + step, S),
                             mapping, seg, ent, st)
    return seg, ent, st


def decode_at(jf: JS.JpegFrames, plan, seg, ent, mapping: int, rows=None):
    """The frames `rows` (default: all) of a store of one image per step through the tables (seg, ent) -> (pixels, status) on the host."""
    _, img_seg2, _, max_seg2 = plan
    N = jf.N
    rows = list(range(N)) if rows is None else rows
    B = len(rows)
    eo = torch.tensor([0, N], dtype=torch.int64, device=DEV)
    ep, row = torch.zeros(B, dtype=torch.int32, device=DEV), torch.tensor(rows, dtype=torch.int64, device=DEV)
    out = torch.full((B, 1, jf.H, jf.W, 3), 0x7F, dtype=torch.uint8, device=DEV)
    st = torch.full((B, 1, max_seg2), 0x7F, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.jpeg_workspace_bytes(B, jf.H, jf.W, jf.h2v2), dtype=torch.uint8, device=DEV)
    ops.jpeg_decode_rows(jf.bytes, torch.from_numpy(np.ascontiguousarray(img_seg2)).to(DEV), seg, jf.img_tab, jf.qt_pool, jf.ht_pool, eo, N, ep, row, 1,
                         jf.H, jf.W, jf.h2v2, max_seg2, mapping, ws, out, st, seg_ent=ent)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(B, jf.H, jf.W, 3), st.cpu().numpy().reshape(B, max_seg2)


@pytest.mark.parametrize("build_mapping, sliced", [(0, False), (1, False), (0, True), (1, True)], ids=["lane", "wave", "lane-in-slices", "wave-in-slices"])
@pytest.mark.parametrize("key", sorted(STORES, key=str), ids=key_id)
def test_the_device_index_equals_the_host_programs_and_decodes_to_pillows_pixels(exe, tmp_path, key, build_mapping, sliced):
    H, W = key[:2]
    files = STORES[key]
    tables = JC.pack(files, 1, H, W)
    jf = JS.JpegFrames(tables, DEV)
    want = np.stack([JC.pillow_decode(f) for f in files])
    S = jf.index.seg_tab.shape[0]
    for pm in (1, 2, 5, IC.row_mcus(jf.index)):
        o = IC.run_index(exe, tmp_path, tables, pm, "store")
        seg, ent, st = device_index(jf, o["plan"], pm, build_mapping, max(1, (S + 2) // 3) if sliced else None)
        torch.cuda.synchronize()
        assert np.array_equal(seg.cpu().numpy(), o["seg_tab"]), f"piece_mcus {pm}: seg_tab differs from the host program's"
        assert np.array_equal(ent.cpu().numpy(), o["seg_ent"]), f"piece_mcus {pm}: seg_ent differs from the host program's"
        assert np.array_equal(st.cpu().numpy(), o["index_status"]) and not o["index_status"].any()
        for mapping in (0, 1):
            got, status = decode_at(jf, o["plan"], seg, ent, mapping)
            assert not status.any(), f"piece_mcus {pm}, decode mapping {mapping}: non-zero status"
            assert np.array_equal(got, want), f"piece_mcus {pm}, decode mapping {mapping}: {(got != want).sum()} values differ from Pillow's"


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
def test_one_launch_holds_staged_pieces_beside_a_piece_longer_than_stage_bytes(mapping):
    """The 206 KB scan of the long corpus (4:4:4, 28 MCUs a row) at five rows a piece: pieces of about 37 KB, which the wave mapping
    reads from global memory, a last piece of three rows and the 28 short segments of the file with a marker per row, which it
    stages."""
    cases = JC.crafted_stores(JC.long_corpus())[(224, 224, 0)]
    jf = JS.JpegFrames(JC.pack([c.data for c in cases], 1, 224, 224), DEV)
    un = JS.JpegFrames(JC.pack([c.data for c in cases], 1, 224, 224), DEV)
    assert jf.build_scan_index(piece_mcus=5 * 28) == 6 + 28 and jf.max_seg == 28 and jf.seg_ent is not None
    torch.cuda.synchronize()
    seg = jf.seg_tab.cpu().numpy()
    lens = seg[:, 1] - seg[:, 0]
    assert (lens > JC.stage_bytes()).sum() >= 4 and (lens <= JC.stage_bytes()).sum() >= 29 and not jf.index_status.any()
    eo = torch.tensor([0, 2], dtype=torch.int64, device=DEV)
    ep, row = torch.zeros(3, dtype=torch.int32, device=DEV), torch.tensor([1, 0, 1], dtype=torch.int64, device=DEV)
    a, b = (torch.full((3, 1, 224, 224, 3), 0x7F, dtype=torch.uint8, device=DEV) for _ in range(2))
    sa, sb = jf.decode(eo, 2, ep, row, a, mapping=mapping), un.decode(eo, 2, ep, row, b, mapping=mapping)
    torch.cuda.synchronize()
    assert not sa.any() and not sb.any() and sa.shape == (3, 1, 28) and sb.shape == (3, 1, 28)
    assert_bits_equal(a, b, "indexed and un-indexed decode")
    for i, r in enumerate((1, 0, 1)):
        assert np.array_equal(a[i, 0].cpu().numpy(), cases[r].pixels)


def test_files_with_a_marker_per_row_are_left_alone_and_short_segments_are_cut_only_where_longer():
    rows = [JC.encode(JC.content("noise", 32, 48, seed=i), quality=90, subsampling=2, restart_marker_rows=1) for i in range(4)]
    jf = JS.JpegFrames(JC.pack(rows, 1, 32, 48), DEV)
    before = (jf.img_seg.clone(), jf.seg_tab.clone(), jf.max_seg)
    assert jf.build_scan_index() == 0 and jf.seg_ent is None and jf.index_status is None
    assert torch.equal(jf.img_seg, before[0]) and torch.equal(jf.seg_tab, before[1]) and jf.max_seg == before[2] == 2
    cases = [c for c in JC.crafted_stores(JC.crafted_corpus())[(32, 48, 1)] if "restart-every" in c.name]
    assert [c.name for c in cases] == ["32x48-420-restart-every-2-mcus", "32x48-420-restart-every-5-mcus"]
    jf = JS.JpegFrames(JC.pack([c.data for c in cases], 1, 32, 48), DEV)
    old = jf.seg_tab.cpu().numpy()
    assert jf.build_scan_index(piece_mcus=3) == 3 + 3 and jf.max_seg == 3
    torch.cuda.synchronize()
    seg, ent = jf.seg_tab.cpu().numpy(), jf.seg_ent.cpu().numpy()
    assert np.array_equal(seg[:3], old[:3]) and not ent[:3].any(), "segments of 2 MCUs stay whole, with a zero entry"
    assert seg[:, 2:].tolist() == [[0, 2], [2, 4], [4, 6], [0, 3], [3, 5], [5, 6]] and jf.img_seg.tolist() == [0, 3, 6]
    assert seg[3, 0] == old[3, 0] and seg[4, 1] == old[3, 1] and seg[5].tolist() == old[4].tolist() and not ent[5].any() and not ent[3].any()
    assert old[3, 0] < seg[4, 0] <= seg[3, 1] <= seg[4, 0] + 2
    got, st = decode_at(jf, (None, jf.img_seg.cpu().numpy(), 6, 3), jf.seg_tab, jf.seg_ent, 1)
    assert not st.any() and np.array_equal(got, np.stack([c.pixels for c in cases]))


# ---------------------------------------------------------------------------------------------------------------- store, mix, graph
def markerless(lengths, n_img, h, w, sub, seed=0):
    """Frames of three table sets and no restart marker."""
    kws = [dict(quality=50), dict(quality=95), dict(quality=95, optimize=True)]
    return [JC.encode(JC.content(("noise", "ramp", "saturated")[i % 3], h, w, seed=seed + i), subsampling=sub, **kws[i % 3]) for i in range(sum(lengths) * n_img)]


def same_batch(a: dict, b: dict, what):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert_bits_equal(a[k], b[k], f"{what}: {k}")
        else:
            assert a[k] == b[k], (what, k)


@pytest.mark.parametrize("n_img, h, w, sub, pieces", [(1, 16, 16, 0, 2), (2, 32, 48, 2, 2)], ids=["16x16-444", "32x48-420-two-images"])
def test_sample_is_bit_equal_with_and_without_the_index_eagerly_and_from_a_graph(n_img, h, w, sub, pieces):
    lengths, chunk = (5, 3, 6, 4), 2
    d = JC.episode_dict(markerless(lengths, n_img, h, w, sub), n_img, h, w, lengths)
    a, b = EP.EpisodeStore.from_dict(d, DEV, chunk=chunk, jpeg_scan_index=True), EP.EpisodeStore.from_dict(d, DEV, chunk=chunk)
    assert (a.jpeg.max_seg, b.jpeg.max_seg) == (pieces, 1) and a.jpeg.seg_ent is not None and b.jpeg.seg_ent is None and a.N == b.N
    assert a.jpeg.index_bytes() == 48 * pieces * sum(lengths) * n_img and a.jpeg.index_status.shape == (sum(lengths) * n_img,)
    for B, seed, rank, world, step in ((4, 5, 0, 1, 0), (7, 5, 1, 2, 3), (32, 9, 2, 3, 11), (1, 0, 0, 1, 40)):
        same_batch(a.sample(B, seed, rank, world, step), b.sample(B, seed, rank, world, step), (B, seed, rank, world, step))
        assert a.decode_status.shape == (B, n_img, pieces) and b.decode_status.shape == (B, n_img, 1) and not a.decode_status.any()
    assert a.verify_frames(batch=8) == sum(lengths) * n_img and not a.jpeg.index_status.any()
    # replayed from a captured graph
    B = 6
    bufs, graphs = [], []
    for st in (a, b):
        buf = st._buffers(B)
        ep, row, off = st.sample_indices(B, 5, 0, 1, 0)
        st.gather(ep, row, off, buf)                            # warm-up: every buffer exists before the capture
        torch.cuda.synchronize()
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                st.gather(ep, row, off, buf)
        torch.cuda.synchronize()
        bufs.append(buf)
        graphs.append(g)
    for step in (3, 8):
        for st, buf, g in zip((a, b), bufs, graphs):
            st.sample_indices(B, 5, 0, 1, step)
            buf["frames_u8"].fill_(0x7F)
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bufs[0]["row"], bufs[1]["row"])
        assert_bits_equal(bufs[0]["frames_u8"], bufs[1]["frames_u8"], f"replay, step {step}")
        assert (bufs[0]["frames_u8"] != 0x7F).any()


def captured_gather(st, B: int, seed: int):
    """The store's gather of batch size B captured in a graph, as tests/test_jpeg_store_gpu.py captures it -> (its buffers, the graph);
    a later sample_indices() of the same B puts new windows into the index buffers the graph reads."""
    buf = st._buffers(B)
    ep, row, off = st.sample_indices(B, seed, 0, 1, 0)[-3:]
    st.gather(ep, row, off, buf)                                # warm-up: every buffer exists before the capture
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            st.gather(ep, row, off, buf)
    torch.cuda.synchronize()
    return buf, g


def sweep_draw(st, j: int, B: int) -> dict:
    """Held-out batch j of a store built with holdout= as heldout.HeldOutSweep.draw draws it: vla_heldout_sweep into index buffers of
    its own, then the store's gather into raw-batch buffers of its own."""
    e = torch.empty
    idx = dict(ds=e(B, dtype=torch.int32, device=DEV), ep=e(B, dtype=torch.int32, device=DEV), row=e(B, dtype=torch.int64, device=DEV),
               prompt_off=e(B + 1, dtype=torch.int32, device=DEV), valid=e(B, dtype=torch.uint8, device=DEV))
    raw = dict(frames_u8=torch.full((B,) + st.frame_shape, 0x7F, dtype=torch.uint8, device=DEV), actions_raw=e(B, st.chunk, st.A, dtype=torch.float32, device=DEV),
               proprio_raw=e(B, st.Pd, dtype=torch.float32, device=DEV), prompt_flat=torch.zeros(B * st.Pmax, dtype=torch.int64, device=DEV))
    ops.heldout_sweep(st.val_off, st.episode_off, st.prompt_off, st.dataset_off if st.mixed else None, 0, 1, j, 1, st.Pmax, idx["ds"], idx["ep"], idx["row"],
                      idx["prompt_off"], idx["valid"])
    out = dict(st.gather(idx["ep"], idx["row"], idx["prompt_off"], raw), dataset_index=idx["ds"], valid=idx["valid"])
    torch.cuda.synchronize()
    return out


def test_a_mix_and_its_held_out_sweep_are_bit_equal_with_and_without_the_index():
    """A two-dataset mix with the last episodes of each held out: sample() eagerly, its gather replayed from a captured graph, and the
    batches of the held-out sweep (vla_heldout_sweep, then the same gather)."""
    n_img, h, w, chunk = 2, 32, 48, 4
    fa, fb = markerless((9, 12, 8), n_img, h, w, 2, seed=100), markerless((5, 11, 10), n_img, h, w, 2, seed=200)
    mk = lambda f, l, name: dict(JC.episode_dict(f, n_img, h, w, l, seed=len(l) + len(name)), dataset_name=name)
    entries = [(mk(fa, (9, 12, 8), "a"), 1.0), (mk(fb, (5, 11, 10), "bb"), 0.5)]
    a = MX.EpisodeMix.from_dicts(entries, DEV, chunk=chunk, holdout=0.4, jpeg_scan_index=True)
    b = MX.EpisodeMix.from_dicts(entries, DEV, chunk=chunk, holdout=0.4)
    assert (a.jpeg.max_seg, b.jpeg.max_seg) == (2, 1) and a.Nv == b.Nv > 0
    for B, seed, rank, world, step in ((6, 5, 0, 1, 0), (32, 7, 1, 2, 5)):
        same_batch(a.sample(B, seed, rank, world, step), b.sample(B, seed, rank, world, step), (B, seed, rank, world, step))
        assert not a.decode_status.any()
    B = 6
    (ba, ga), (bb, gb) = captured_gather(a, B, 5), captured_gather(b, B, 5)
    for step in (3, 8):
        for st, buf, g in ((a, ba, ga), (b, bb, gb)):
            st.sample_indices(B, 5, 0, 1, step)
            buf["frames_u8"].fill_(0x7F)
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ba["row"], bb["row"]) and torch.equal(ba["ep"], bb["ep"])
        assert_bits_equal(ba["frames_u8"], bb["frames_u8"], f"replay, step {step}")
        assert (ba["frames_u8"] != 0x7F).any()
    for j in range(-(-a.Nv // 8)):                              # the whole sweep, 8 windows a batch, the last one partly filled
        same_batch(sweep_draw(a, j, 8), sweep_draw(b, j, 8), f"held-out batch {j}")
        assert not a.decode_status.any()


def test_finetune_logs_the_same_losses_with_and_without_the_flag(tmp_path, capsys):
    """Adapter-only on the tiny config, 3 logged steps at batch 4 from a marker-less --episode_file, state digests logged and a held-out
    sweep every 2 steps: the same losses, digests and validation entries with and without --jpeg_scan_index."""
    from vla_adapter_amd import engine as E, finetune as F
    mcfg = E.NAMED_CONFIGS["tiny"]()
    lengths, h, w = (9, 10, 12, 11, 14), 48, 64
    d = JC.episode_dict(markerless(lengths, 1, h, w, 2, seed=7), 1, h, w, lengths, A=mcfg.action_dim, Pd=mcfg.proprio_dim)
    d["prompt_flat"], d["dataset_name"] = d["prompt_flat"] % 700, "toy"
    torch.save(d, tmp_path / "jpeg.pt")
    args = lambda name: ["--tiny", "true", "--backbone", "tiny", "--batch_size", "4", "--max_steps", "2", "--learning_rate", "1e-3",
                         "--wandb_log_freq", "1", "--save_freq", "1000", "--phase", "Training", "--use_proprio", "True", "--use_fz", "True",
                         "--run_root_dir", str(tmp_path / name), "--max_seq_len", "96", "--seed", "5", "--log_state_digest", "True",
                         "--use_val_set", "True", "--val_episode_fraction", "0.4", "--val_freq", "2", "--episode_file", str(tmp_path / "jpeg.pt")]
    capsys.readouterr()
    a = F.finetune(F.parse_args(args("indexed") + ["--jpeg_scan_index", "True", "--verify_frames", "True"]))
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{"jpeg_scan_index"')]
    assert lines == [dict(jpeg_scan_index=dict(pieces_per_frame=3.0, index_bytes=48 * 3 * sum(lengths), jpeg_index_bad_scans=0))]
    b = F.finetune(F.parse_args(args("plain")))
    assert not [l for l in capsys.readouterr().out.splitlines() if l.startswith('{"jpeg_scan_index"')]
    assert len(a["log"]) == 3 and all(l["jpeg_bad_segments"] == 0 for l in a["log"])
    assert a["log"] == b["log"], "losses and state digests"
    assert all(l["state_digest"] for l in a["log"]) and a["val_log"] and a["val_log"] == b["val_log"] and a["heldout"] == b["heldout"]


# ---------------------------------------------------------------------------------------------------------------- damaged scans
@pytest.mark.parametrize("build_mapping, mapping", [(0, 0), (1, 1), (0, 1)], ids=["lane-lane", "wave-wave", "lane-wave"])
@pytest.mark.parametrize("name", ["16x16", "32x16", "32x48-one-segment", "224x224-long"])
def test_damaged_scans_give_the_host_programs_pixels_and_status(exe, tmp_path, name, build_mapping, mapping):
    """JC.corrupt_corpus() (16 x 16 and 32 x 16: truncation at every byte, bit flips, 0xFF runs planted in the scan, a restart marker
    removed - one MCU a segment, so no piece is cut and the tables must come back as they went in, with zero entries),
    IC.piecewise_corrupt_corpus() and JC.long_corrupt_corpus(), at the piece lengths of the host run."""
    if name in ("16x16", "32x16"):
        H, W = (int(x) for x in name.split("x"))
        kept = JC.parse_tolerant(JC.corrupt_corpus()[(H, W)], 1, H, W)[0]
    else:
        H, W, kept = (32, 48, IC.piecewise_corrupt_corpus()) if name.startswith("32") else (224, 224, JC.long_corrupt_corpus())
    names, tables = [n for n, _ in kept], JC.pack([d for _, d in kept], 1, H, W)
    jf = JS.JpegFrames(tables, DEV)
    behind = 0
    for pm in (1, 2, 5, W // 16):
        o = IC.run_index(exe, tmp_path, tables, pm, "damaged")
        behind += IC.check_pieces_of_damaged_scans(o, names)
        seg, ent, st = device_index(jf, o["plan"], pm, build_mapping)
        torch.cuda.synchronize()
        for got, want, what in ((seg, o["seg_tab"], "seg_tab"), (ent, o["seg_ent"], "seg_ent"), (st, o["index_status"], "the walk's status")):
            assert np.array_equal(got.cpu().numpy(), want), f"piece_mcus {pm}: {what} differs from the host program's"
        got, status = decode_at(jf, o["plan"], seg, ent, mapping)
        assert np.array_equal(status, o["status_at"]), f"piece_mcus {pm}: per-piece status differs from the host program's for {[names[i] for i in np.flatnonzero((status != o['status_at']).any(1))[:5]]}"
        bad = np.flatnonzero((got != o["pixels_at"]).reshape(len(kept), -1).any(1))
        assert bad.size == 0, f"piece_mcus {pm}: pixels differ from the host program's for {[names[i] for i in bad[:5]]}"
        if name in ("16x16", "32x16"):                          # a segment of one MCU is not cut: its row comes back as it went in, with
            piece_off = o["plan"][0]                            # a zero entry.  (A 32 x 16 file cut in front of its restart marker is one
            whole = np.flatnonzero(np.diff(piece_off) == 1)     # segment of two MCUs: 306 of the 1298 segments, cut at piece_mcus 1.)
            S = jf.index.seg_tab.shape[0]
            assert whole.size == S if name == "16x16" or pm >= 2 else S // 2 <= whole.size < S
            assert np.array_equal(seg.cpu().numpy()[piece_off[whole]], jf.index.seg_tab[whole]) and not ent.cpu().numpy()[piece_off[whole]].any()
    if name in ("16x16", "32x16"):
        assert o["index_status"].astype(bool).sum() > 200, "the corpus does exercise the error paths"
    else:
        assert behind >= 2


def test_verify_frames_names_the_frame_on_an_indexed_store():
    lengths, n_img, h, w = (9, 3, 12), 2, 32, 48
    files = markerless(lengths, n_img, h, w, 2)
    head, scan, tail = JC.split_scan(files[13])
    files[13] = head + scan[:len(scan) // 2] + tail
    st = EP.EpisodeStore.from_dict(JC.episode_dict(files, n_img, h, w, lengths), DEV, chunk=2, jpeg_scan_index=True)
    assert st.jpeg.max_seg == 2 and st.jpeg.index_status.cpu().nonzero().flatten().tolist() == [13]
    with pytest.raises(ValueError, match=r"verify_frames: frame 13 \(step 6, image 1\), segment [01]: the segment runs out of bytes"):
        st.verify_frames(batch=16)
