"""CPU checks of the JPEG frame store (vla_adapter_amd/jpeg_store.py, include/vla_jpeg.h): the written-down decode rule
(tests/jpeg_rule_np.py) against Pillow, bit for bit, on the matrix of tests/jpeg_cases.py; the parser - its pools, its segment
tables, its refusals, each naming the frame; the two storage forms of an episode dict; concat_shards on JPEG shards; the seventh
header against its signature table and the built library; the flag."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_rule_np as R
from tests.test_episodes_cpu import make_tables
from vla_adapter_amd import episodes as EP
from vla_adapter_amd import jpeg_store as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vla_jpeg.h")


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


# ---------------------------------------------------------------------------------------------------------------- the parser
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


# ---------------------------------------------------------------------------------------------------------------- header, table, flag
def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_jpeg_header_binding_and_library_agree():
    from vla_adapter_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = native.load()
    names = sorted(set(re.findall(r"\b(vla_[a-z0-9_]+)\s*\(", header_text())))
    assert names == native.JPEG_SYMBOLS == sorted(native.JPEG_PROTOS) == ["vla_jpeg_decode_rows", "vla_jpeg_workspace_bytes"]
    for other in (native._PROTOS, native.SERVE_PROTOS, native.EPISODE_PROTOS, native.MIXTURE_PROTOS, native.HELDOUT_PROTOS, native.DIGEST_PROTOS):
        assert not set(native.JPEG_PROTOS) & set(other), "an entry point belongs to one header"
    protos = re.findall(r"\b(?:int|long long)\s+(vla_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header_text())
    assert sorted(n for n, _ in protos) == native.JPEG_SYMBOLS
    for name, params in protos:
        args, res = native.JPEG_PROTOS[name]
        assert len(params.split(",")) == len(args), name
        fn = getattr(lib, name)
        assert list(fn.argtypes) == list(args) and fn.restype is res
    assert native.ABI_VERSION == 8 and len(native._PROTOS) == 69 and not [k for k in native._PROTOS if "jpeg" in k]


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
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "jpeg.hip" in mk and "jpeg_core.h" in mk and "episode_row.h" in mk and "vla_jpeg.h" in mk


def test_verify_frames_flag_defaults_to_off():
    from vla_adapter_amd import finetune as F
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["verify_frames"]
    assert f.default is False and F.parse_args(["--verify_frames", "True"]).verify_frames is True
