"""CPU checks of the JPEG frame store (vla_adapter_amd/jpeg_store.py, include/vla_jpeg.h): the written-down decode rule
(tests/jpeg_rule_np.py) against Pillow, bit for bit, on the matrix of tests/jpeg_cases.py and on its crafted corpus - files no run of
Pillow's encoder writes, from the coefficient-level writer tests/jpeg_writer.py, which is pinned here too; the parser - its pools, its
segment tables, its refusals, each naming the frame, RGB-coded files among them; fill bytes in front of RSTn; the two storage forms
of an episode dict; concat_shards on JPEG shards; the workspace arithmetic; the flag."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_rule_np as R
from tests import jpeg_writer as JW
from tests.test_episodes_cpu import make_tables
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import jpeg_store as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("i", range(72), ids=[c[0] for c in JC.matrix()])
def test_the_rule_matches_pillow_bit_for_bit(i):
    name, (H, W), _, data, want = JC.matrix()[i]
    got = R.decode(data)
    assert got.shape == (H, W, 3) and np.array_equal(got, want), f"{name}: {(got != want).sum()} of {want.size} values differ"


def test_the_matrix_is_the_issues():
    m = JC.matrix()
    assert len(m) == 72 and len({c[0] for c in m}) == 72
    for name, (H, W), sname, data, _ in m:
        p = R.parse(data)
        assert (p["H"], p["W"]) == (H, W)
        assert ((p["comps"][0][1], p["comps"][0][2]) == (2, 2)) == ("420" in sname), name
        assert (p["dri"] > 0) == ("rst" in sname), name
        if "rst" in sname and (H, W) != (16, 16):
            assert len(p["segments"]) > 1, name


def test_the_rule_on_a_224_frame():
    data = JC.encode(JC.content("ramp", 224, 224) // 2 + JC.content("noise", 224, 224) // 8, quality=95, subsampling=2)
    assert np.array_equal(R.decode(data), JC.pillow_decode(data))


# ---------------------------------------------------------------------------------------------------------------- the crafted corpus
CRAFTED = JC.crafted_corpus() + JC.long_corpus()


def test_the_writer_round_trips_pillows_files():
    """A Pillow file's coefficients, read by the rule's entropy decode and written again with the file's own tables: the same
    entropy-coded bytes - codes, value bits, stuffing, padding and restart markers are T.81's - and the same pixels from Pillow."""
    for kw in (dict(quality=90, subsampling=2), dict(quality=85, subsampling=0, optimize=True), dict(quality=90, subsampling=2, restart_marker_blocks=5),
               dict(quality=80, subsampling=0, restart_marker_rows=1)):
        data = JC.encode(JC.content("ramp", 32, 48) // 2 + JC.content("noise", 32, 48) // 16 + 50, **kw)
        st, p = {}, R.parse(data)
        R.decode(data, st)
        ids = sorted({t for pair in p["scan"] for t in pair})
        spec = JW.Spec(H=32, W=48, h2v2=kw["subsampling"] == 2, qtables={i: [int(q) for q in t] for i, t in p["qt"].items()},
                       dc_tables={i: JW.tables_from_codes(p["ht"][i]) for i in ids}, ac_tables={i: JW.tables_from_codes(p["ht"][0x10 | i]) for i in ids},
                       comp_ids=[c[0] for c in p["comps"]], comp_tq=[c[3] for c in p["comps"]], comp_td=[t[0] for t in p["scan"]],
                       comp_ta=[t[1] for t in p["scan"]], restart=p["dri"] or None)
        again = JW.write(spec, st["quantised"])
        assert R.parse(again)["segments"] == p["segments"] and len(p["segments"]) == (1 if not p["dri"] else -(-(6 if spec.h2v2 else 24) // p["dri"]))
        assert np.array_equal(JC.pillow_decode(again), JC.pillow_decode(data))


def test_the_writer_refuses_blocks_beyond_its_bound_and_tables_that_are_no_prefix_code():
    s = JC._spec(16, 16, 1)
    b = JC._blocks(s, 1)
    JW.write(JC.with_tables(s, b), b)
    b[0][0, 0, 0] = 1001                                                  # x quantiser 2: the block's sum passes 2000 by its DC alone
    with pytest.raises(AssertionError, match="> 2000"):
        JW.write(JC.with_tables(s, b), b)
    assert JW.BOUND == 2000
    JW.huffman_from_lengths([(0, 1), (1, 2), (2, 3), (3, 3)][:3] + [(3, 16)])
    with pytest.raises(AssertionError, match="all-ones"):
        JW.huffman_from_lengths([(0, 1), (1, 2), (2, 3), (3, 3)])       # Kraft sum 1: the last code would be 111
    with pytest.raises(AssertionError, match="all-ones"):
        JW.code_table([1, 2] + [0] * 14, [0, 1, 2])                        # 0, 10 and 11


@pytest.mark.parametrize("i", range(len(CRAFTED)), ids=[c.name for c, _ in CRAFTED])
def test_a_crafted_case_has_its_property_and_the_rule_decodes_it_as_pillow_does(i):
    case, checks = CRAFTED[i]
    f = JC.crafted_facts(case.name)
    listed = checks(f)
    assert listed, "a case without a property"
    for what, got, want in listed:
        assert got >= want if isinstance(want, JC.AtLeast) else got == want, \
            f"{case.name}: {what}: {got}, the case needs {'at least ' if isinstance(want, JC.AtLeast) else ''}{int(want)}"
    assert f["rule"].shape == case.shape + (3,) and np.array_equal(f["rule"], case.pixels), \
        f"{case.name}: {(f['rule'] != case.pixels).sum()} of {case.pixels.size} values differ"


def test_the_crafted_corpus_covers_the_issues_list():
    names = [c.name for c, _ in JC.crafted_corpus()]
    for part in ("codes-of-9-to-16-bits", "commonest-symbols-16-bits", "lengths-1-to-16-mixed", "three-table-pairs", "three-quantisation-tables", "ac-only-at-zigzag-63",
                 "all-63-ac-nonzero", "eob-straight-after-dc", "run-of-15", "zrl-then-eob", "every-category", "runs-of-ones", "restart-every-2", "restart-every-5",
                 "past-the-last-mcu", "dri-0-written", "fill-bytes-in-front-of-rstn", "one-dht-and-one-dqt", "dqt-after-sof0", "defined-twice",
                 "fill-bytes-in-front-of-header", "payloads-full-of-marker-bytes", "no-app0-ids-1-2-3", "jfif-ids-0-1-2", "bytes-behind-eoi", "jfif-with-ids-r-g-b",
                 "adobe-transform-1-without-jfif"):
        assert [n for n in names if part in n], part
    assert {c.shape for c, _ in JC.crafted_corpus()} == {(16, 16), (32, 48)} and {c.shape for c, _ in JC.long_corpus()} == {(224, 224)}
    for key, cases in {**JC.crafted_stores(JC.crafted_corpus()), **JC.crafted_stores(JC.long_corpus())}.items():
        t = JC.pack([c.data for c in cases], 1, key[0], key[1])
        ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
        assert ix.h2v2 == key[2] and ix.N == len(cases), "the parser accepts every crafted file"


def test_stage_bytes_is_what_the_long_corpus_is_built_around():
    assert JC.stage_bytes() == 32768, "STAGE_BYTES of csrc/jpeg.hip moved: the padded files and the long noise files must move with it"
    cases = {c.name: c for c, _ in JC.long_corpus()}
    t = JC.pack([cases[n].data for n in sorted(cases) if "padded" in n], 1, 224, 224)
    ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
    assert sorted((ix.seg_tab[:, 1] - ix.seg_tab[:, 0]).tolist()) == [32767, 32768, 32769], "one segment on either side of the staging limit and one at it"


# ---------------------------------------------------------------------------------------------------------------- the parser
def test_rgb_coded_files_are_refused_and_the_refusal_names_the_frame():
    """libjpeg reads these as RGB - its pixels are far from a YCbCr decode of the same coefficients - so the YCbCr kernels must not."""
    good = {sub: JC.encode(JC.content("ramp", 32, 48), quality=90, subsampling=sub) for sub in (0, 2)}
    seen = JC.refused_colour()
    assert [n for n, *_ in seen] == ["pillow-keep-rgb", "ids-r-g-b-without-jfif-or-adobe", "pillow-420-app0-removed-ids-r-g-b", "adobe-transform-0-ids-1-2-3"]
    for name, shape, data, why in seen:
        want, as_ycc = JC.pillow_decode(data), R.decode(data)
        assert (as_ycc != want).mean() > 0.5, f"{name}: Pillow does not read this file as RGB"
        ok = good[2 if R.parse(data)["comps"][0][1] == 2 else 0]              # (of the file's own sampling: nothing else to refuse)
        msg = _refused([ok, ok, data], shape, r"the store: frame 2 \(step 2, image 0\): the file stores RGB")
        assert why in msg and "not YCbCr: not supported" in msg, msg


def test_the_colour_rule_is_libjpegs():
    rgb, ycc = [82, 71, 66], [1, 2, 3]
    for jfif, adobe, ids, says_rgb in ((True, None, rgb, False), (True, 0, rgb, False), (False, 0, ycc, True), (False, 1, rgb, False), (False, 2, rgb, False),
                                       (False, None, rgb, True), (False, None, ycc, False), (False, None, [0, 1, 2], False), (False, None, [82, 71, 67], False)):
        assert bool(JS._stores_rgb(jfif, adobe, ids)) == says_rgb, (jfif, adobe, ids)
    # a marker too short for libjpeg to examine counts as not seen: "JFIF" in 13 bytes, "Adobe" in 11
    s = JC._spec(16, 16, 1, comp_ids=rgb, layout=[("APP", 0, b"JFIF\0" + bytes(8)), ("DQT", [0, 1]), ("SOF",), ("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)])])
    b = JC._blocks(s, 1)
    data = JW.write(JC.with_tables(s, b), b)
    assert (R.decode(data) != JC.pillow_decode(data)).mean() > 0.5 and "component ids 'R', 'G', 'B'" in _refused([data], (16, 16), "frame 0 ")
    s.layout[0] = ("APP", 14, b"Adobe\0\x64" + bytes(4))
    s.comp_ids = ycc
    data = JW.write(s, b)
    assert np.array_equal(R.decode(data), JC.pillow_decode(data))
    t = JC.pack([data], 1, 16, 16)
    assert JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"]).N == 1


def test_fill_bytes_in_front_of_rstn_and_eoi_are_accepted():
    case = next(c for c, _ in JC.crafted_corpus() if c.name == "32x48-444-fill-bytes-in-front-of-rstn")
    t = JC.pack([case.data], 1, 32, 48)
    ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
    p = R.parse(case.data)
    assert ix.max_seg == 12 == len(p["segments"])
    for k, seg in enumerate(p["segments"]):
        lo, hi, m0, m1 = ix.seg_tab[k].tolist()
        assert case.data[lo:hi] == seg and (m0, m1) == (2 * k, 2 * k + 2)
        assert case.data[hi:hi + 3] == b"\xff\xff\xff" if k < 11 else case.data[hi:] == b"\xff\xff\xd9", "hi is the first 0xFF of the run"
        assert k == 0 or (0xD0 <= case.data[lo - 1] <= 0xD7 and case.data[lo - 2] == 0xFF), "lo is the byte behind the marker code"


def test_fill_bytes_in_front_of_a_stuffed_byte_are_refused_by_name():
    """0xFF 0xFF 0x00 inside entropy-coded data: libjpeg reads one data byte, the decode core the end of the segment - refused."""
    case = next(c for c, _ in JC.crafted_corpus() if c.name == "32x48-420-codes-that-are-runs-of-ones")
    head, scan, tail = JC.split_scan(case.data)
    i = scan.index(b"\xff\x00")
    msg = _refused([case.data, head + scan[:i] + b"\xff" + scan[i:] + tail], (32, 48), r"frame 1 \(step 1, image 0\)")
    assert "1 0xFF fill byte(s) in front of a stuffed 0xFF 0x00" in msg and f"scan byte {i}" in msg and "missing EOI" not in msg


def mixed_store(H=32, W=48):
    """Six frames that mix three table sets: q50, q95 and q95 with optimised Huffman tables."""
    kws = [dict(quality=50), dict(quality=95), dict(quality=95, optimize=True)]
    files = [JC.encode(JC.content("noise" if i % 2 else "ramp", H, W, seed=i), subsampling=2, **kws[i % 3]) for i in range(6)]
    return files, JC.pack(files, 2, H, W)


def test_the_parser_pools_tables_by_content():
    files, t = mixed_store()
    ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
    assert ix.N == 6 and (ix.n_img, ix.H, ix.W, ix.h2v2, ix.max_seg) == (2, 32, 48, 1, 1)
    assert ix.qt_pool.shape == (4, 64), "two quantisation tables (luma, chroma) per quality, shared by the optimised files"
    assert ix.ht_pool.shape[1] == JS.HT_WORDS and 4 < ix.ht_pool.shape[0] <= 12, "the 4 standard tables once, the optimised ones per file"
    assert np.array_equal(ix.img_tab[1, :3], ix.img_tab[4, :3]) and np.array_equal(ix.img_tab[1, 3:9], ix.img_tab[1 + 3 * 0, 3:9])
    assert np.array_equal(ix.img_tab[0, 3:9], ix.img_tab[1, 3:9]), "q50 and q95 share the standard Huffman tables"
    assert not np.array_equal(ix.img_tab[2, 3:9], ix.img_tab[1, 3:9]), "an optimised file has tables of its own"
    assert ix.img_seg.tolist() == list(range(7)) and ix.seg_tab.shape == (6, 4)
    off = t["frame_off"].tolist()
    for i in range(6):
        lo, hi, m0, m1 = ix.seg_tab[i].tolist()
        assert off[i] < lo < hi == off[i + 1] - 2 and (m0, m1) == (0, 6), "the scan ends at the EOI marker; one segment holds every MCU"
        p = R.parse(files[i])
        assert bytes(t["frames_jpeg"][lo:hi].tolist()) == p["segments"][0]
        q = p["qt"][p["comps"][0][3]]
        assert np.array_equal(ix.qt_pool[ix.img_tab[i, 0]], q)


def test_the_parser_finds_the_restart_segments():
    data = JC.encode(JC.content("noise", 48, 32), quality=90, subsampling=2, restart_marker_rows=1)
    t = JC.pack([data], 1, 48, 32)
    ix = JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"])
    p = R.parse(data)
    assert ix.max_seg == 3 == len(p["segments"]) and ix.img_tab[0, JS.IMG_RESTART] == p["dri"] == 2
    for k, seg in enumerate(p["segments"]):
        lo, hi, m0, m1 = ix.seg_tab[k].tolist()
        assert data[lo:hi] == seg and (m0, m1) == (2 * k, 2 * k + 2)


def test_the_derived_huffman_table():
    p_counts = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]             # the standard luminance DC table
    t = JS.derive_huffman(bytes(p_counts), bytes(range(12)))
    codes = R.huffman_codes(p_counts, list(range(12)))
    for (l, code), sym in codes.items():
        assert t[JS.HT_VAL + code + t[JS.HT_VALOFF + l]] == sym and code <= t[JS.HT_MAXCODE + l]
        if l <= 8:
            assert set(t[JS.HT_LOOK + (code << (8 - l)):JS.HT_LOOK + ((code + 1) << (8 - l))].tolist()) == {(l << 8) | sym}
    assert t[JS.HT_MAXCODE + 1] == -1 and t[JS.HT_MAXCODE + 10] == -1 and t[JS.HT_MAXCODE + 17] == 0x7FFFFFFF
    assert (t[JS.HT_LOOK + 0xFF] == 0) and t[JS.HT_MAXCODE + 9] == 0x1FE
    with pytest.raises(ValueError, match="overflow the 1-bit code space"):
        JS.derive_huffman(bytes([3] + [0] * 15), bytes(3))
    with pytest.raises(ValueError, match="overflow the 3-bit code space"):
        JS.derive_huffman(bytes([1, 1, 3] + [0] * 13), bytes(5))


def _refused(files, shape, match):
    t = JC.pack(files, 1, *shape)
    with pytest.raises(ValueError, match=match) as e:
        JS.parse_frames(t["frames_jpeg"], t["frame_off"], t["frame_shape"], "the store")
    return str(e.value)


def test_the_parser_refuses_what_the_kernel_does_not_decode_and_names_the_frame():
    good = JC.encode(JC.content("ramp", 32, 32), quality=90, subsampling=2)
    img = JC.content("ramp", 32, 32)
    assert "progressive" in _refused([good, JC.encode(img, quality=90, progressive=True)], (32, 32), r"the store: frame 1 \(step 1, image 0\)")
    assert "grayscale" in _refused([good, good, JC.encode(img, mode="L", quality=90)], (32, 32), r"frame 2 ")
    assert "sampling factors [(2, 1), (1, 1), (1, 1)]" in _refused([JC.encode(img, quality=90, subsampling=1), good], (32, 32), r"frame 0 ")
    assert "multiples of 16" in _refused([JC.encode(JC.content("ramp", 40, 40), quality=90)], (40, 40), r"frame 0 ")
    assert "header is truncated" in _refused([good, good[:40]], (32, 32), r"frame 1 ")
    assert "size mismatch: the file is 16 x 16" in _refused([good, JC.encode(JC.content("ramp", 16, 16), quality=90)], (32, 32), r"frame 1 ")
    assert "missing EOI" in _refused([good[:-2] + b"\x00\x00", good], (32, 32), r"frame 0 ")
    assert "missing EOI" in _refused([good, good[:-2]], (32, 32), r"frame 1 ")
    assert "4:4:4 differs from frame 0's" in _refused([good, JC.encode(img, quality=90, subsampling=0)], (32, 32), r"frame 1 ")
    assert "CMYK" in _refused([JC.encode(np.zeros((32, 32, 4), dtype=np.uint8), mode="CMYK")], (32, 32), r"frame 0 ")
    # 16-bit quantisation tables, a scan without its components, overflowing code counts: by editing the header of a good file
    i = good.index(b"\xff\xdb")
    assert "16-bit quantisation" in _refused([good[:i + 4] + bytes([0x10]) + good[i + 5:]], (32, 32), r"frame 0 ")
    i = good.index(b"\xff\xda")
    assert "does not list the three components" in _refused([good[:i + 5] + bytes([9]) + good[i + 6:]], (32, 32), r"frame 0 ")
    assert "no scan" in _refused([good[:i] + b"\xff\xd9"], (32, 32), r"frame 0 ")
    i = good.index(b"\xff\xc4")
    assert good[i + 5:i + 8] == bytes([0, 1, 5]), "the standard luminance DC table: six codes of 2 bits in place of one of 2 and five of 3"
    assert "overflow the 2-bit code space" in _refused([good[:i + 5] + bytes([0, 6, 0]) + good[i + 8:]], (32, 32), r"frame 0 ")
    i = good.index(b"\xff\xc0")
    assert "12-bit precision" in _refused([good[:i + 4] + bytes([12]) + good[i + 5:]], (32, 32), r"frame 0 ")


# ---------------------------------------------------------------------------------------------------------------- the two forms
def jpeg_tables(lengths=(3, 9, 12), n_img=2, H=16, W=32, **kw):
    files = [JC.encode(JC.content("noise" if i % 3 else "ramp", H, W, seed=i), quality=(50, 95)[i % 2], subsampling=2, **kw)
             for i in range(sum(lengths) * n_img)]
    return files, JC.episode_dict(files, n_img, H, W, lengths)


def test_an_episode_dict_carries_exactly_one_form():
    files, d = jpeg_tables()
    EP._check_shard(d, "jpeg")
    raw = JC.episode_dict(files, 2, 16, 32, (3, 9, 12), raw=True)
    EP._check_shard(raw, "raw")
    with pytest.raises(ValueError, match=r"both: carries both frames_u8 and \('frames_jpeg', 'frame_off', 'frame_shape'\)"):
        EP._check_shard(dict(d, frames_u8=raw["frames_u8"]), "both")
    neither = {k: v for k, v in raw.items() if k != "frames_u8"}
    with pytest.raises(ValueError, match=r"neither: frames_u8 is missing .*frames_jpeg.*frame_off.*frame_shape"):
        EP._check_shard(neither, "neither")
    with pytest.raises(ValueError, match=r"part: \('frame_off',\) missing"):
        EP._check_shard({k: v for k, v in d.items() if k != "frame_off"}, "part")
    with pytest.raises(ValueError, match=r"frame_off must be int64 \[T \* n_img \+ 1 = 49\]"):
        EP._check_shard(dict(d, frame_off=d["frame_off"][:-1]), "short")
    with pytest.raises(ValueError, match="frame_off must rise from 0"):
        EP._check_shard(dict(d, frame_off=d["frame_off"] + 1), "shifted")
    assert EP.EPISODE_KEYS == ("frames_u8", "actions_raw", "proprio_raw", "episode_off", "prompt_flat", "prompt_off")
    assert JS.JPEG_KEYS == ("frames_jpeg", "frame_off", "frame_shape")


def test_a_jpeg_store_has_the_raw_twins_extents_and_statistics():
    files, d = jpeg_tables()
    raw = JC.episode_dict(files, 2, 16, 32, (3, 9, 12), raw=True)
    a, b = EP.EpisodeStore.from_dict(d, "cpu", chunk=8), EP.EpisodeStore.from_dict(raw, "cpu", chunk=8)
    assert a.frame_shape == b.frame_shape == (2, 16, 32, 3) and a.row_bytes == b.row_bytes and (a.T, a.E, a.N) == (b.T, b.E, b.N)
    assert a.statistics() == b.statistics() and a.frames_u8 is None and b.jpeg is None and a.jpeg.N == 48
    assert b.verify_frames() == 0, "a raw store has nothing to verify"


def test_concat_shards_concatenates_the_bytes_and_rebases_the_offsets():
    f1, d1 = jpeg_tables((3, 9))
    f2, d2 = jpeg_tables((12,))
    out = EP.concat_shards([d1, d2], ["a", "b"])
    assert bytes(out["frames_jpeg"].tolist()) == b"".join(f1 + f2)
    off = out["frame_off"].tolist()
    assert off[0] == 0 and off[-1] == out["frames_jpeg"].numel() and len(off) == 49
    assert [off[i + 1] - off[i] for i in range(48)] == [len(f) for f in f1 + f2]
    assert out["frame_shape"].tolist() == [2, 16, 32] and out["episode_off"].tolist() == [0, 3, 12, 24]
    EP._check_shard(out, "concatenated")
    ix = JS.parse_frames(out["frames_jpeg"], out["frame_off"], out["frame_shape"])
    assert ix.N == 48
    with pytest.raises(ValueError, match=r"b: frame_shape \[2, 32, 16\] differs from a's \[2, 16, 32\]"):
        EP.concat_shards([d1, dict(d2, frame_shape=torch.tensor([2, 32, 16]))], ["a", "b"])


def test_mixed_storage_is_refused():
    files, d = jpeg_tables((12,))
    raw = JC.episode_dict(files, 2, 16, 32, (12,), raw=True)
    with pytest.raises(ValueError, match="b: stores its frames as raw, a as jpeg"):
        EP.concat_shards([d, raw], ["a", "b"])
    with pytest.raises(ValueError, match="b: stores its frames as jpeg, a as raw"):
        EP.EpisodeTables([raw, d], ["a", "b"], "cpu", chunk=8)


def test_a_raw_store_is_what_it_was():
    d = make_tables()
    st = EP.EpisodeStore.from_dict(d, "cpu", chunk=8)
    assert st.jpeg is None and torch.equal(st.frames_u8, d["frames_u8"]) and st.frame_shape == (2, 8, 8, 3)


# ---------------------------------------------------------------------------------------------------------------- the entry points, the flag
def test_workspace_bytes_is_host_arithmetic():
    from vla_adapter_amd import ops
    assert ops.jpeg_workspace_bytes(64, 224, 224, 1) == 64 * 224 * 224 * 3 // 2 * 3        # 1.5 samples per pixel, 2 + 1 bytes each
    assert ops.jpeg_workspace_bytes(1, 16, 16, 0) == 16 * 16 * 3 * 3
    for bad in ((1, 40, 32, 1), (1, 32, 8, 0), (0, 32, 32, 1), (1, 32, 32, 2)):
        with pytest.raises(ValueError):
            ops.jpeg_workspace_bytes(*bad)


def test_the_core_is_stated_once_and_shares_the_row_clamp():
    csrc = os.path.join(ROOT, "vla_adapter_amd", "csrc")
    jpeg, episodes = open(os.path.join(csrc, "jpeg.hip")).read(), open(os.path.join(csrc, "episodes.hip")).read()
    row = open(os.path.join(csrc, "episode_row.h")).read()
    assert row.count("EpisodeRow episode_row(") == 1
    for txt in (jpeg, episodes):
        assert '#include "episode_row.h"' in txt and txt.count("episode_row(episode_off, ep, row, b, E, T)") == 1
        assert "episode_off[w.e" not in txt and "row[b]" not in txt, "the clamp is episode_row's alone"
    for const in ("4433", "15137", "25172", "91881", "116130"):
        assert const not in jpeg, "the arithmetic lives in jpeg_core.h"


def test_verify_frames_flag_defaults_to_off():
    from vla_adapter_amd import finetune as F
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["verify_frames"]
    assert f.default is False and F.parse_args(["--verify_frames", "True"]).verify_frames is True
