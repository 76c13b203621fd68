"""The JPEG decode kernels (csrc/jpeg.hip, include/vla_jpeg.h) on the device: bit for bit Pillow's pixels on the matrix of
tests/jpeg_cases.py, in single launches over stores that mix table sets and files with and without restart markers, with both lane
mappings, n_img 1 and 2, B 1, 3 and 32; the same on the crafted corpus - tables, block structures, stuffing, restart intervals and
headers no run of Pillow's encoder writes - and on 224 x 224 batches whose segments lie on both sides of the wave mapping's staging
limit, one of them damaged behind it; the row clamp of vla_episode_gather on out-of-range windows; and the corrupt corpus inside
poisoned arenas, where pixels and status must equal what the host build of the same core computes (tests/test_jpeg_core_cpu.py runs
that build under the sanitizers over the same, seeded corpus; no sanitizer runs here)."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests.arena import Arena, assert_bits_equal
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import jpeg_store as JS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def decode(jf: JS.JpegFrames, rows, mapping: int, eps=None, episode_off=None):
    """The frames of the windows (eps, rows) of a store of one episode (or of the given episodes) -> (frames u8 [B, n_img, H, W, 3],
    status) on the host."""
    T = jf.N // jf.n_img
    B = len(rows)
    eo = torch.tensor(episode_off if episode_off is not None else [0, T], dtype=torch.int64, device=DEV)
    ep = torch.tensor(eps if eps is not None else [0] * B, dtype=torch.int32, device=DEV)
    out = torch.full((B, jf.n_img, jf.H, jf.W, 3), 0x7F, dtype=torch.uint8, device=DEV)
    st = jf.decode(eo, T, ep, torch.tensor(rows, dtype=torch.int64, device=DEV), out, mapping=mapping)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


@pytest.fixture(scope="module")
def stores():
    """{(H, W, h2v2, n_img): (JpegFrames, Pillow's pixels [N, H, W, 3])} - parsed and uploaded once."""
    out = {}
    for (H, W, h2), cases in JC.stores_of_the_matrix().items():
        for n_img in (1, 2):
            jf = JS.JpegFrames(JC.pack([c[3] for c in cases], n_img, H, W), DEV)
            out[(H, W, h2, n_img)] = (jf, np.stack([c[4] for c in cases]))
    return out


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("n_img, B", [(1, 1), (1, 3), (1, 32), (2, 1), (2, 3), (2, 32)])
@pytest.mark.parametrize("key", sorted(JC.stores_of_the_matrix()), ids=lambda k: f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}")
def test_the_kernels_match_pillow_on_the_matrix(stores, key, n_img, B, mapping):
    jf, want = stores[key + (n_img,)]
    T = jf.N // n_img
    assert jf.max_seg == {(16, 16): 1, (32, 48): 6, (48, 16): 3}[key[:2]] if key[2] else jf.max_seg == 1
    rows = [(5 * b + 2) % T for b in range(B)] if B < T else [b % T for b in range(B)]          # B = 32 visits every frame of the store
    got, st = decode(jf, rows, mapping)
    assert st.shape == (B, n_img, jf.max_seg) and not st.any()
    ref = want.reshape(T, n_img, jf.H, jf.W, 3)[rows]
    assert np.array_equal(got, ref), f"{(got != ref).sum()} of {ref.size} values differ from Pillow's"


def test_a_224_batch_with_and_without_restart_markers():
    imgs = [JC.content("ramp", 224, 224) // 2 + JC.content("noise", 224, 224, seed=s) // 8 for s in range(4)]
    files = [JC.encode(im, quality=95, subsampling=2, **(dict(restart_marker_rows=1) if i % 2 else {})) for i, im in enumerate(imgs)]
    jf = JS.JpegFrames(JC.pack(files, 2, 224, 224), DEV)
    assert jf.max_seg == 14
    want = np.stack([JC.pillow_decode(f) for f in files]).reshape(2, 2, 224, 224, 3)
    for mapping in (0, 1):
        got, st = decode(jf, [1, 0, 1], mapping)
        assert not st.any() and np.array_equal(got, want[[1, 0, 1]])


CRAFTED_STORES = JC.crafted_stores(JC.crafted_corpus())


@pytest.fixture(scope="module")
def crafted():
    """{(H, W, h2v2, n_img): (JpegFrames, the cases in store order)} - a store of n_img views holds whole steps: the first cases again."""
    out = {}
    for (H, W, h2), cases in CRAFTED_STORES.items():
        for n_img in (1, 2):
            cs = cases + cases[:-len(cases) % n_img]
            out[(H, W, h2, n_img)] = (JS.JpegFrames(JC.pack([c.data for c in cs], n_img, H, W), DEV), cs)
    return out


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("n_img", [1, 2])
@pytest.mark.parametrize("key", sorted(CRAFTED_STORES), ids=lambda k: f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}")
def test_the_kernels_match_pillow_on_the_crafted_corpus(crafted, key, n_img, mapping):
    """One launch per store over every crafted file of a shape and sampling (tests/jpeg_cases.py: crafted_corpus)."""
    jf, cases = crafted[key + (n_img,)]
    T = jf.N // n_img
    assert jf.N == len(cases) >= 7 and jf.max_seg == {(32, 48, 0): 12, (32, 48, 1): 3}.get(key, 1)
    got, st = decode(jf, list(range(T)), mapping)
    assert st.shape == (T, n_img, jf.max_seg) and not st.any(), f"non-zero status for {[cases[i].name for i in np.flatnonzero(st.reshape(jf.N, -1).any(1))]}"
    got = got.reshape(jf.N, jf.H, jf.W, 3)
    bad = [f"{c.name}: {(got[i] != c.pixels).sum()} of {c.pixels.size}" for i, c in enumerate(cases) if not np.array_equal(got[i], c.pixels)]
    assert not bad, f"values differ from Pillow's: {bad}"


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("h2v2", [1, 0], ids=["420", "444"])
def test_a_224_batch_of_staged_and_unstaged_segments(h2v2, mapping):
    """One launch holds segments the wave mapping stages in LDS - 14 or 28 short ones of a file with a marker per MCU row, one of
    STAGE_BYTES - 1 and one of exactly STAGE_BYTES - beside segments it reads from global memory: STAGE_BYTES + 1, 59 KB, 206 KB."""
    cases = JC.crafted_stores(JC.long_corpus())[(224, 224, h2v2)]
    assert [c.name.split("224x224-")[1] for c in cases] == (["420-noise-q95-one-segment", "420-padded-to-stage-bytes-1", "420-padded-to-stage-bytes",
                                                              "420-padded-to-stage-bytes+1", "420-a-marker-per-mcu-row"] if h2v2 else
                                                             ["444-noise-q100-one-segment", "444-a-marker-per-mcu-row"])
    jf = JS.JpegFrames(JC.pack([c.data for c in cases], 1, 224, 224), DEV)
    lens = (jf.index.seg_tab[:, 1] - jf.index.seg_tab[:, 0])
    assert jf.max_seg == (14 if h2v2 else 28) and (lens > JC.stage_bytes()).sum() == (2 if h2v2 else 1) and (lens <= JC.stage_bytes()).sum() >= 14
    rows = [0, 4, 1, 2, 3, 4, 0, 2] if h2v2 else [1, 0, 1]
    got, st = decode(jf, rows, mapping)
    assert not st.any()
    for b, r in enumerate(rows):
        assert np.array_equal(got[b, 0], cases[r].pixels), f"{cases[r].name} (sample {b}): {(got[b, 0] != cases[r].pixels).sum()} values differ from Pillow's"


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
def test_a_long_damaged_segment_equals_the_host_core_inside_arenas(tmp_path, mapping):
    """Damage behind STAGE_BYTES, where the wave mapping reads global memory: the scan of the 59 KB file cut at 40 000 bytes, and one
    flipped bit.  The decode ends with the host core's status and pixels and writes nothing outside its extents."""
    from vla_adapter_amd import ops
    kept, H, W = JC.long_corrupt_corpus(), 224, 224
    tables = JC.pack([d for _, d in kept], 1, H, W)
    px, st, ix = JC.run_core(JC.build_core(tmp_path), tmp_path, tables, "long-corrupt")
    assert not st[0].any() and st[1].tolist() == [1], "the intact file decodes; the truncated one runs out of bytes"
    jf = JS.JpegFrames(tables, DEV)
    N = jf.N
    assert (jf.max_seg, jf.h2v2, N) == (1, 1, len(kept)) and int(ix.seg_tab[1, 1] - ix.seg_tab[1, 0]) in (39999, 40000)
    out = Arena((N, H * W * 3), torch.uint8, strides=(H * W * 3 + 20, 1), align=4, device=DEV)
    ws = Arena((ops.jpeg_workspace_bytes(N, H, W, jf.h2v2),), torch.uint8, align=16, device=DEV)
    status = Arena((N, 1, jf.max_seg), torch.uint8, align=1, device=DEV)
    eo = torch.tensor([0, N], dtype=torch.int64, device=DEV)
    ep, row = torch.zeros(N, dtype=torch.int32, device=DEV), torch.arange(N, dtype=torch.int64, device=DEV)
    frames = out.view.as_strided((N, 1, H, W, 3), (H * W * 3 + 20, H * W * 3 + 20, W * 3, 3, 1))
    ops.jpeg_decode_rows(jf.bytes, jf.img_seg, jf.seg_tab, jf.img_tab, jf.qt_pool, jf.ht_pool, eo, N, ep, row, 1, H, W, jf.h2v2, jf.max_seg, mapping,
                         ws.view, frames, status.view)
    torch.cuda.synchronize()
    for a, what in ((out, "out_frames"), (ws, "workspace"), (status, "status")):
        a.assert_outside_intact(what)
    got_st = status.view.cpu().numpy().reshape(N, jf.max_seg)
    assert np.array_equal(got_st, st), f"status {got_st.tolist()} differs from the host core's {st.tolist()}"
    got = out.view.cpu().numpy().reshape(N, H, W, 3)
    bad = np.flatnonzero((got != px).reshape(N, -1).any(1))
    assert bad.size == 0, f"pixels differ from the host core's for {[kept[i][0] for i in bad]}"
    assert np.array_equal(px[0], JC.pillow_decode(kept[0][1]))


def test_rows_are_clamped_as_the_gather_clamps_them():
    """Out-of-range ep and row: the decode of the JPEG store and vla_episode_gather on its raw twin pick the same frames."""
    lengths, n_img, H, W = (3, 1, 6), 2, 16, 32
    files = [JC.encode(JC.content("noise", H, W, seed=i), quality=90, subsampling=2) for i in range(sum(lengths) * n_img)]
    jd, rd = JC.episode_dict(files, n_img, H, W, lengths), JC.episode_dict(files, n_img, H, W, lengths, raw=True)
    a, b = EP.EpisodeStore.from_dict(jd, DEV, chunk=2), EP.EpisodeStore.from_dict(rd, DEV, chunk=2)
    eps = [0, 0, 1, 1, 2, 2, -4, 7, 1, 2]
    rows = [-5, 9, 0, 9, 2, 10 ** 12, 1, 3, -(2 ** 40), 4]
    ep = torch.tensor(eps, dtype=torch.int32, device=DEV)
    row = torch.tensor(rows, dtype=torch.int64, device=DEV)
    off = torch.zeros(len(eps) + 1, dtype=torch.int32, device=DEV)
    ga, gb = a.gather(ep, row, off, a._buffers(len(eps))), b.gather(ep, row, off, b._buffers(len(eps)))
    torch.cuda.synchronize()
    for k in ("frames_u8", "actions_raw", "proprio_raw", "prompt_flat"):
        assert_bits_equal(ga[k], gb[k], k)
    want = [0, 2, 3, 3, 4, 9, 1, 4, 3, 4]                  # ep clamped into [0, E), row into its episode
    assert torch.equal(ga["frames_u8"].cpu(), rd["frames_u8"][want]) and not a.decode_status.any()


@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("shape", sorted(JC.corrupt_corpus()), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_corrupt_corpus_equals_the_host_core_inside_arenas(tmp_path, shape, mapping):
    from vla_adapter_amd import ops
    H, W = shape
    kept, _ = JC.parse_tolerant(JC.corrupt_corpus()[shape], 1, H, W)
    tables = JC.pack([d for _, d in kept], 1, H, W)
    px, st, ix = JC.run_core(JC.build_core(tmp_path), tmp_path, tables, "corrupt")
    jf = JS.JpegFrames(tables, DEV)
    N = jf.N
    assert (jf.max_seg, jf.h2v2) == (ix.max_seg, ix.h2v2) and N == len(kept) > 400
    out = Arena((N, H * W * 3), torch.uint8, strides=(H * W * 3 + 20, 1), align=4, device=DEV)
    ws = Arena((ops.jpeg_workspace_bytes(N, H, W, jf.h2v2),), torch.uint8, align=16, device=DEV)
    status = Arena((N, 1, jf.max_seg), torch.uint8, align=1, device=DEV)
    eo = torch.tensor([0, N], dtype=torch.int64, device=DEV)
    ep, row = torch.zeros(N, dtype=torch.int32, device=DEV), torch.arange(N, dtype=torch.int64, device=DEV)
    frames = out.view.as_strided((N, 1, H, W, 3), (H * W * 3 + 20, H * W * 3 + 20, W * 3, 3, 1))
    ops.jpeg_decode_rows(jf.bytes, jf.img_seg, jf.seg_tab, jf.img_tab, jf.qt_pool, jf.ht_pool, eo, N, ep, row, 1, H, W, jf.h2v2, jf.max_seg, mapping,
                         ws.view, frames, status.view)
    torch.cuda.synchronize()
    for a, what in ((out, "out_frames"), (ws, "workspace"), (status, "status")):
        a.assert_outside_intact(what)
    got_st = status.view.cpu().numpy().reshape(N, jf.max_seg)
    assert np.array_equal(got_st, st), f"status differs from the host core's for {[kept[i][0] for i in np.flatnonzero((got_st != st).any(1))[:5]]}"
    got = out.view.cpu().numpy().reshape(N, H, W, 3)
    bad = np.flatnonzero((got != px).reshape(N, -1).any(1))
    assert bad.size == 0, f"pixels differ from the host core's for {[kept[i][0] for i in bad[:5]]}"
    assert st.any(1).sum() > 200, "the corpus does exercise the error paths"
