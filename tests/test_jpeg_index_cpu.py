"""The scan index of the JPEG store on the host (include/vla_jpeg_index.h, csrc/jpeg_core.h: index_segment and the entry state of
decode_segment): the indexed decode takes the plain one's arguments and the entry table; plan_pieces tiles every segment; a stand-alone
program with its own main (tests/jpeg_index_cases.py: INDEX_MAIN, compiled with g++ here), plain and with
-fsanitize=address,undefined, builds the index of the matrix, the crafted corpus and the long corpus at four piece lengths - its entries equal the plain-Python rule's, the piece-wise decode
gives the whole-segment decode's coefficients and Pillow's pixels, every status is 0; the sanitized program ends without a report on
damaged scans and on hostile tables, with the whole-segment decode's pixels for the former.  Nothing is loaded into Python: the
sanitizers see the program alone.  What this program computes is what the kernels must compute (tests/test_jpeg_index_gpu.py)."""
import dataclasses
import os

import numpy as np
import pytest

from tests import jpeg_cases as JC
from tests import jpeg_index_cases as IC
from vla_adapter_amd import jpeg_store as JS


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_the_indexed_decode_takes_the_decodes_arguments_and_the_entry_table():
    from vla_adapter_amd import native
    at, plain = native.family("jpeg_index").protos["vla_jpeg_decode_rows_at"][0], native.family("jpeg").protos["vla_jpeg_decode_rows"][0]
    assert len(at) == len(plain) + 1 and at[:5] + at[6:] == plain


def test_the_block_walk_is_stated_once():
    csrc = os.path.join(JC.ROOT, "vla_adapter_amd", "csrc")
    core, index, jpeg = (open(os.path.join(csrc, n)).read() for n in ("jpeg_core.h", "jpeg_index.hip", "jpeg.hip"))
    assert core.count("int decode_block(") == 1 and core.count("int decode_symbol(") == 1 and core.count("receive_extend(BitReader") == 1
    assert core.count("decode_block(br,") == 2, "decode_segment and index_segment call the one block decode"
    for txt in (index, jpeg):
        assert "decode_symbol" not in txt and "receive_extend" not in txt and "br_fill" not in txt, "the walk lives in jpeg_core.h"


# ---------------------------------------------------------------------------------------------------------------- the plan
ALL_STORES = {**{k: [c[3] for c in v] for k, v in JC.stores_of_the_matrix().items()},
              **{k + ("crafted",): [c.data for c in v] for k, v in JC.crafted_stores(JC.crafted_corpus()).items()}}
LONG_STORES = {k + ("long",): [c.data for c in v] for k, v in JC.crafted_stores(JC.long_corpus()).items()}


def key_id(k):
    return f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}" + (f"-{k[3]}" if len(k) > 3 else "")


@pytest.mark.parametrize("key", sorted(ALL_STORES, key=str), ids=key_id)
def test_plan_pieces_tiles_every_segment(key):
    H, W = key[:2]
    t = JC.pack(ALL_STORES[key], 1, H, W)
    ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
    S = ix.seg_tab.shape[0]
    for pm in (1, 2, 5, IC.row_mcus(ix), ix.mcus + 3):
        piece_off, img_seg, S2, max_seg = JS.plan_pieces(ix, pm)
        assert piece_off.dtype == np.int64 and piece_off.shape == (S + 1,) and piece_off[0] == 0 and piece_off[-1] == S2
        n = ix.seg_tab[:, 3] - ix.seg_tab[:, 2]
        assert np.array_equal(np.diff(piece_off), np.maximum(1, -(-n // pm))), "max(1, ceil(MCUs / piece_mcus)) pieces per segment"
        assert np.array_equal(img_seg, piece_off[ix.img_seg]) and max_seg == np.diff(img_seg).max()
        for s in range(S):                                                  # the pieces tile [m0, m1) without gap or overlap
            m0, m1 = int(ix.seg_tab[s, 2]), int(ix.seg_tab[s, 3])
            cuts = [min(m0 + j * pm, m1) for j in range(int(piece_off[s + 1] - piece_off[s]) + 1)]
            assert cuts[0] == m0 and cuts[-1] == m1 and all(a < b for a, b in zip(cuts, cuts[1:]))
        if pm > ix.mcus:
            assert S2 == S and max_seg == ix.max_seg, "no piece is cut when none is longer than piece_mcus"
    with pytest.raises(ValueError):
        JS.plan_pieces(ix, 0)


# ---------------------------------------------------------------------------------------------------------------- the host program
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return IC.build_index_program(tmp_path_factory.mktemp("jpeg_index"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return IC.build_index_program(tmp_path_factory.mktemp("jpeg_index_san"), sanitize=True)


def pillow_pixels(files):
    return np.stack([JC.pillow_decode(f) for f in files])


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("key", sorted({**ALL_STORES, **LONG_STORES}, key=str), ids=key_id)
def test_the_index_equals_the_rule_and_the_pieces_decode_to_pillows_pixels(exe, exe_san, tmp_path, key, sanitized):
    H, W = key[:2]
    files = {**ALL_STORES, **LONG_STORES}[key]
    tables, want = JC.pack(files, 1, H, W), pillow_pixels(files)
    for pm in (1, 2, 5, W // 16 if key[2] else W // 8):
        o = IC.run_index(exe_san if sanitized else exe, tmp_path, tables, pm, "store")
        seg, ent = IC.rule_tables(files, o["ix"], pm)
        assert o["seg_tab"].shape == seg.shape and np.array_equal(o["seg_tab"], seg), \
            f"piece_mcus {pm}: rows {np.flatnonzero((o['seg_tab'] != seg).any(1))[:5].tolist()} of seg_tab differ from the rule's"
        assert np.array_equal(o["seg_ent"], ent), f"piece_mcus {pm}: rows {np.flatnonzero((o['seg_ent'] != ent).any(1))[:5].tolist()} of seg_ent differ from the rule's"
        assert not o["index_status"].any() and not o["status"].any() and not o["status_at"].any(), f"piece_mcus {pm}: every status is 0"
        assert o["coef_differ"] == 0, f"piece_mcus {pm}: {o['coef_differ']} coefficients differ from the whole-segment decode's"
        assert np.array_equal(o["pixels_at"], want), f"piece_mcus {pm}: pixels differ from Pillow's"
        # pieces are tight: piece j ends at most two bytes behind the start of piece j + 1
        same = np.setdiff1d(np.arange(seg.shape[0] - 1), o["plan"][0][1:] - 1)        # (rows j whose row j + 1 continues their segment)
        assert ((seg[same, 1] - seg[same + 1, 0]) <= 2).all() and ((seg[same, 1] - seg[same + 1, 0]) >= 0).all()


def test_the_stuffing_cases_yield_every_entry_bit_and_shared_0xff_bytes(exe, tmp_path):
    """Codes that are runs of ones: 0xFF 0x00 pairs at every offset modulo 8 and a stuffed last byte.  At one MCU per piece the
    entries take every bit 0 .. 7, some begin inside a 0xFF byte (their predecessor's hi is two bytes on), and some begin at the byte
    behind a stuffed pair.  The bounds: the stores hold 0 + 5 + 23 + 15 + 63 = 106 MCU boundaries inside scans; seven in eight of
    them fall inside a byte, and a tenth and more of the data bytes are 0xFF (asserted below), so about nine entries share a 0xFF
    byte and about as many stand behind a pair - at least three of each are asked for."""
    bits, shared_ff, behind_pair, pieces = set(), 0, 0, 0
    for (H, W, h2), cs in sorted(IC.stuffing_stores().items()):
        files = [c.data for c in cs]
        tables = JC.pack(files, 1, H, W)
        o = IC.run_index(exe, tmp_path, tables, 1, "stuffing")
        data = tables["frames_jpeg"].numpy()
        seg, ent = o["seg_tab"], o["seg_ent"]
        rule_seg, rule_ent = IC.rule_tables(files, o["ix"], 1)
        assert np.array_equal(seg, rule_seg) and np.array_equal(ent, rule_ent)
        for c in cs:
            f = JC.facts(c.data)
            assert f["pairs"] * 10 >= f["scan_bytes"] and f["pair_offsets"] == 8 and f["last_pair"] == int(c.shape != (64, 64)), c.name
        inner = np.flatnonzero(seg[:, 2] != 0)                              # entries inside a scan
        pieces += inner.size
        bits |= set(ent[inner, 0].tolist())
        ff = inner[(ent[inner, 0] != 0) & (data[seg[inner, 0]] == 0xFF)]
        shared_ff += ff.size
        assert (seg[ff - 1, 1] == seg[ff, 0] + 2).all(), "the piece in front of a shared 0xFF ends behind its stuffed 0x00"
        assert (data[seg[ff, 0] + 1] == 0).all()
        behind_pair += int(((data[seg[inner, 0] - 1] == 0) & (data[seg[inner, 0] - 2] == 0xFF)).sum())
        assert not ((data[seg[inner, 0]] == 0) & (data[seg[inner, 0] - 1] == 0xFF)).any(), "lo never names a stuffed 0x00"
        assert not o["status_at"].any() and o["coef_differ"] == 0 and np.array_equal(o["pixels_at"], np.stack([c.pixels for c in cs]))
    assert bits == set(range(8)), f"entry bits in use: {sorted(bits)}"
    assert pieces == 106 and shared_ff >= 3 and behind_pair >= 3, (pieces, shared_ff, behind_pair)


# ---------------------------------------------------------------------------------------------------------------- hostile input
def damaged_stores():
    out = {f"{H}x{W}": (H, W, JC.parse_tolerant(files, 1, H, W)[0]) for (H, W), files in JC.corrupt_corpus().items()}
    out["32x48-one-segment"] = (32, 48, IC.piecewise_corrupt_corpus())
    out["224x224-long"] = (224, 224, JC.long_corrupt_corpus())
    return out


@pytest.mark.parametrize("name", ["16x16", "32x16", "32x48-one-segment", "224x224-long"])
def test_damaged_scans_under_the_sanitizers(exe_san, exe, tmp_path, name):
    H, W, kept = damaged_stores()[name]
    names, tables = [n for n, _ in kept], JC.pack([d for _, d in kept], 1, H, W)
    behind = 0
    for pm in (1, 2, 5, W // 16):
        o = IC.run_index(exe_san, tmp_path, tables, pm, "damaged")           # (a sanitizer report is a non-zero exit: run_index raises)
        assert not o["status"][0].any() and np.array_equal(o["pixels_at"][0], JC.pillow_decode(kept[0][1]))
        behind += IC.check_pieces_of_damaged_scans(o, names)
        p = IC.run_index(exe, tmp_path, tables, pm, "damaged-plain")
        for k in ("seg_tab", "seg_ent", "index_status", "pixels_at", "status_at"):
            assert np.array_equal(o[k], p[k]), f"{k}: the optimised build computes what the sanitized build computes"
        # a dead piece: nothing to read, a zero entry
        (piece_off, img_seg2, S2, _), ix = o["plan"], o["ix"]
        for s in np.flatnonzero(o["index_status"]):
            rows = np.arange(piece_off[s], piece_off[s + 1])
            dead = rows[o["seg_tab"][rows, 0] == o["seg_tab"][rows, 1]]
            dead = dead[dead > rows[0]]
            assert (o["seg_tab"][dead, 1] == ix.seg_tab[s, 1]).all() and not o["seg_ent"][dead].any()
    assert o["status"].any(1).sum() >= (1 if name.startswith("224") else 100), "the corpus does exercise the error paths"
    if name in ("32x48-one-segment", "224x224-long"):
        assert behind >= (2 if name.startswith("224") else 100), "scans fail in a piece that has pieces behind it"


@pytest.mark.parametrize("hostile_entries", [False, True], ids=["entries-as-built", "entries-hostile"])
def test_hostile_tables_under_the_sanitizers(exe_san, tmp_path, hostile_entries):
    """lo / hi / MCU ranges / pool ids / img_seg out of range, piece_off non-monotone and past S', entry bit 255 and predictors at the
    int32 extremes: the sanitized program ends without a report, and what the build wrote lies inside the store."""
    H, W = 32, 48
    files = ALL_STORES[(32, 48, 1, "crafted")]
    tables = JC.pack(files, 1, H, W)
    ix = JS.parse_frames(tables["frames_jpeg"], tables["frame_off"], tables["frame_shape"])
    n_bytes = int(tables["frames_jpeg"].numel())
    variants = IC.hostile_variants(ix, 1)
    assert len(variants) >= 7
    for name, v, plan in [("good-tables", ix, JS.plan_pieces(ix, 1))] + variants:
        o = IC.run_index(exe_san, tmp_path, tables, 1, name, ix=v, plan=plan, hostile_entries=hostile_entries)
        seg, ent = o["seg_tab"], o["seg_ent"]
        written = seg[:, 0] != 0x5555555555555555
        assert written.any(), name
        w = seg[written]
        assert (w[:, 0] >= 0).all() and (w[:, 0] <= w[:, 1]).all() and (w[:, 1] <= n_bytes).all(), f"{name}: byte ranges inside the store"
        assert (w[:, 2] >= 0).all() and (w[:, 2] <= w[:, 3]).all() and (w[:, 3] <= ix.mcus).all(), f"{name}: MCU ranges inside the image"
        assert (ent[written, 0] >= 0).all() and (ent[written, 0] <= 7).all(), name
        if name == "good-tables" and not hostile_entries:
            assert written.all() and not o["status_at"].any()


# ---------------------------------------------------------------------------------------------------------------- the flag
def test_jpeg_scan_index_flag_defaults_to_off_and_is_not_fingerprinted():
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd import train_state as TS
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["jpeg_scan_index"]
    assert f.default is False and F.parse_args([]).jpeg_scan_index is False and F.parse_args(["--jpeg_scan_index", "True"]).jpeg_scan_index is True
    on, off = F.parse_args(["--jpeg_scan_index", "True", "--episode_file", "e.pt"]), F.parse_args(["--episode_file", "e.pt"])
    assert TS.fingerprint(on, "adapter", 1, 1) == TS.fingerprint(off, "adapter", 1, 1) and "jpeg_scan_index" not in TS.fingerprint(on, "adapter", 1, 1)
    assert "jpeg_scan_index" not in TS.NOT_FINGERPRINTED


def test_the_flag_leaves_a_raw_store_as_it_is():
    """As --verify_frames: with raw frames there is nothing to index."""
    import torch
    from vla_adapter_amd import episodes as EP
    files = [JC.encode(JC.content("noise", 16, 16, seed=i), quality=90, subsampling=2) for i in range(6)]
    d = JC.episode_dict(files, 1, 16, 16, (2, 4), raw=True)
    a, b = EP.EpisodeStore.from_dict(d, "cpu", chunk=2, jpeg_scan_index=True), EP.EpisodeStore.from_dict(d, "cpu", chunk=2)
    assert a.jpeg is None and b.jpeg is None and a.verify_frames() == 0
    assert torch.equal(a.frames_u8, b.frames_u8) and torch.equal(a.valid_off, b.valid_off) and a.N == b.N
