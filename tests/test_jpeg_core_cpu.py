"""The decode core (csrc/jpeg_core.h) on the host: a stand-alone program with its own main (tests/jpeg_cases.py: CORE_MAIN, compiled
with g++ here, as tests/test_abi.py compiles its probe) decodes stores packed by the product's parser.  On the matrix its pixels equal
Pillow's bit for bit; built with -fsanitize=address,undefined it runs the corrupt corpus - truncation of the scan at every byte, 200
seeded bit flips, scan bytes replaced by 0xFF, a restart marker removed - and must end without a report, with a non-zero status for
every truncation (a file that lost a restart marker may still decode, to other pixels).  Nothing is loaded into Python: the sanitizers see the program alone.  What this build computes for a malformed
stream is what the kernels must compute for it (tests/test_jpeg_gpu.py)."""
import numpy as np
import pytest

from tests import jpeg_cases as JC


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return JC.build_core(tmp_path_factory.mktemp("jpeg_core"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return JC.build_core(tmp_path_factory.mktemp("jpeg_core_san"), sanitize=True)


@pytest.mark.parametrize("key", sorted(JC.stores_of_the_matrix()), ids=lambda k: f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}")
def test_the_core_matches_pillow_on_the_matrix(exe, tmp_path, key):
    H, W, _ = key
    cases = JC.stores_of_the_matrix()[key]
    px, st, ix = JC.run_core(exe, tmp_path, JC.pack([c[3] for c in cases], 1, H, W))
    assert not st.any(), "every segment of a good file decodes"
    for i, c in enumerate(cases):
        assert np.array_equal(px[i], c[4]), f"{c[0]}: {(px[i] != c[4]).sum()} of {c[4].size} values differ from Pillow's"


def test_the_core_matches_pillow_on_224_frames(exe, tmp_path):
    imgs = [JC.content("ramp", 224, 224) // 2 + JC.content("noise", 224, 224, seed=s) // 8 for s in range(2)]
    files = [JC.encode(imgs[0], quality=95, subsampling=2), JC.encode(imgs[1], quality=95, subsampling=2, restart_marker_rows=1)]
    px, st, ix = JC.run_core(exe, tmp_path, JC.pack(files, 2, 224, 224))
    assert ix.max_seg == 14 and not st.any()
    for i, f in enumerate(files):
        assert np.array_equal(px[i], JC.pillow_decode(f))


CRAFTED_STORES = {**JC.crafted_stores(JC.crafted_corpus()), **JC.crafted_stores(JC.long_corpus())}


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("key", sorted(CRAFTED_STORES), ids=lambda k: f"{k[0]}x{k[1]}-{'420' if k[2] else '444'}")
def test_the_core_matches_pillow_on_the_crafted_corpus(exe, exe_san, tmp_path, key, sanitized):
    H, W, h2v2 = key
    cases = CRAFTED_STORES[key]
    px, st, ix = JC.run_core(exe_san if sanitized else exe, tmp_path, JC.pack([c.data for c in cases], 1, H, W), "crafted")
    assert ix.h2v2 == h2v2 and ix.N == len(cases) and not st.any(), "every segment of a crafted file decodes"
    for i, c in enumerate(cases):
        assert np.array_equal(px[i], c.pixels), f"{c.name}: {(px[i] != c.pixels).sum()} of {c.pixels.size} values differ from Pillow's"


@pytest.mark.parametrize("shape", sorted(JC.corrupt_corpus()), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_corrupt_corpus_under_the_sanitizers(exe_san, exe, tmp_path, shape):
    H, W = shape
    kept, refused = JC.parse_tolerant(JC.corrupt_corpus()[shape], 1, H, W)
    names = [n for n, _ in kept]
    assert names[0] == "intact" and len(refused) < 100, f"{len(refused)} files refused at load"
    assert not [n for n in refused if n.startswith("truncated") or n.startswith("restart")], "truncations keep their EOI: the parser accepts them"
    tables = JC.pack([d for _, d in kept], 1, H, W)
    px, st, ix = JC.run_core(exe_san, tmp_path, tables, "corrupt")          # (a sanitizer report is a non-zero exit: run_core raises)
    assert not st[0].any() and np.array_equal(px[0], JC.pillow_decode(kept[0][1]))
    for i, n in enumerate(names):
        if n.startswith("truncated"):
            assert st[i].any(), f"{n}: a scan that ends early must report it"
    assert sum(bool(s.any()) for s in st) > len([n for n in names if n.startswith("truncated")]), "some flips are caught too"
    px2, st2, _ = JC.run_core(exe, tmp_path, tables, "corrupt-plain")
    assert np.array_equal(px, px2) and np.array_equal(st, st2), "the optimised build computes what the sanitized build computes"
