"""What the scan-index tests share (tests/test_jpeg_index_cpu.py, test_jpeg_index_gpu.py, test_jpeg_index_memory_contract_gpu.py): the
stand-alone host program around csrc/jpeg_core.h that builds the index of a packed store and decodes it piece by piece (its own source
text, compiled with g++ at test time as tests/jpeg_cases.py compiles its program), the index rule in plain Python on top of
tests/jpeg_rule_np.py's bit reader and tables - entries at MCU boundaries from a walk of its own - and the hostile tables.  Not
collected; everything is computed once per process and left unchanged."""
import functools
import os
import struct
import subprocess

import numpy as np

from tests import jpeg_cases as JC
from tests import jpeg_rule_np as R
from vla_adapter_amd import jpeg_store as JS

INDEX_MAIN = r"""
// Builds the scan index of a packed store with csrc/jpeg_core.h on the host and decodes the store twice, whole segments and piece by
// piece: argv[1] the store (tests/jpeg_cases.py: write_packed) followed by int64 [4] (piece_mcus, S', the new max_seg, mode),
// piece_off int64 [S + 1] and the new img_seg int64 [N + 1]; argv[2] the output.  mode & 1: the entry table is overwritten with
// hostile values before the decode.  Every buffer is a heap block of its exact size, so that a sanitizer sees an overrun.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "jpeg_core.h"
using namespace vlajpeg;
template <class T> static T* take(FILE* f, size_t n) {
  T* p = (T*)malloc(n ? n * sizeof(T) : 1);
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short store file\n"); exit(2); }
  return p;
}
static void pixels_of(const short* coef, u8* planes, u8* pixels, i64 nb, int H, int W, int h2v2) {
  for (i64 b = 0; b < nb; ++b) {
    i64 stride;
    const i64 o = plane_offset(b, H, W, h2v2, stride);
    idct_islow(coef + b * 64, planes + o, stride);
  }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) plane_pixel(planes, H, W, h2v2, y, x, pixels + ((size_t)y * W + x) * 3);
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long h[10];
  if (fread(h, 8, 10, f) != 10 || h[0] != 0x4A50454753544F52ll) return 2;
  const long long N = h[1], n_bytes = h[5], S = h[6];
  const int H = (int)h[2], W = (int)h[3], h2v2 = (int)h[4], nQ = (int)h[7], nH = (int)h[8], max_seg = (int)h[9];
  u8* bytes = take<u8>(f, n_bytes);
  i64* img_seg = take<i64>(f, N + 1);
  i64* seg_tab = take<i64>(f, S * SEG_WORDS);
  int* img_tab = take<int>(f, N * IMG_WORDS);
  unsigned short* qt = take<unsigned short>(f, (size_t)nQ * 64);
  int* ht = take<int>(f, (size_t)nH * HT_WORDS);
  i64* x = take<i64>(f, 4);
  const int piece_mcus = (int)x[0], max_seg2 = (int)x[2], mode = (int)x[3];
  const i64 S2 = x[1];
  i64* piece_off = take<i64>(f, S + 1);
  i64* img_seg2 = take<i64>(f, N + 1);
  fclose(f);
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt, nQ, ht, nH};
  i64* seg2 = (i64*)malloc(S2 * SEG_WORDS * sizeof(i64));
  int* ent2 = (int*)malloc(S2 * ENT_WORDS * sizeof(int));
  u8* ix_status = (u8*)malloc(S);
  memset(seg2, 0x55, S2 * SEG_WORDS * sizeof(i64));
  memset(ent2, 0x55, S2 * ENT_WORDS * sizeof(int));
  for (i64 s = 0; s < S; ++s) ix_status[s] = (u8)index_item(st, N, s, H, W, h2v2, piece_mcus, piece_off, S2, seg2, ent2);
  i64* seg2_out = (i64*)malloc(S2 * SEG_WORDS * sizeof(i64));
  int* ent2_out = (int*)malloc(S2 * ENT_WORDS * sizeof(int));
  memcpy(seg2_out, seg2, S2 * SEG_WORDS * sizeof(i64));
  memcpy(ent2_out, ent2, S2 * ENT_WORDS * sizeof(int));
  if (mode & 1)
    for (i64 r = 0; r < S2; ++r) {
      ent2[r * ENT_WORDS + ENT_BIT] = 255;
      ent2[r * ENT_WORDS + ENT_P0] = (r & 1) ? INT_MAX : INT_MIN;
      ent2[r * ENT_WORDS + ENT_P1] = (r & 2) ? INT_MAX : INT_MIN;
      ent2[r * ENT_WORDS + ENT_P2] = INT_MAX;
    }
  Store st2{bytes, n_bytes, img_seg2, seg2, S2, img_tab, qt, nQ, ht, nH};
  st2.seg_ent = ent2;
  const i64 nb = blocks_per_image(H, W, h2v2);
  short* coef = (short*)malloc(nb * 64 * sizeof(short));
  short* coef2 = (short*)malloc(nb * 64 * sizeof(short));
  u8* planes = (u8*)malloc(nb * 64);
  const size_t image = (size_t)H * W * 3;
  u8* pixels = (u8*)malloc((size_t)N * image);
  u8* pixels2 = (u8*)malloc((size_t)N * image);
  u8* status = (u8*)calloc((size_t)N * max_seg, 1);
  u8* status2 = (u8*)calloc((size_t)N * max_seg2, 1);
  i64 coef_differ = 0;
  for (i64 img = 0; img < N; ++img) {
    memset(coef, 0x55, nb * 64 * sizeof(short));
    memset(coef2, 0x55, nb * 64 * sizeof(short));
    for (int k = 0; k < max_seg; ++k) {
      const int rc = decode_item(st, img, k, H, W, h2v2, coef);
      status[img * max_seg + k] = (u8)(rc < 0 ? 0 : rc);
    }
    for (int k = 0; k < max_seg2; ++k) {
      const int rc = decode_item(st2, img, k, H, W, h2v2, coef2);
      status2[img * max_seg2 + k] = (u8)(rc < 0 ? 0 : rc);
    }
    for (i64 i = 0; i < nb * 64; ++i) coef_differ += coef[i] != coef2[i];
    pixels_of(coef, planes, pixels + img * image, nb, H, W, h2v2);
    pixels_of(coef2, planes, pixels2 + img * image, nb, H, W, h2v2);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(&coef_differ, 8, 1, o);
  fwrite(seg2_out, sizeof(i64), S2 * SEG_WORDS, o);
  fwrite(ent2_out, sizeof(int), S2 * ENT_WORDS, o);
  fwrite(ix_status, 1, S, o);
  fwrite(pixels, 1, (size_t)N * image, o);
  fwrite(status, 1, (size_t)N * max_seg, o);
  fwrite(pixels2, 1, (size_t)N * image, o);
  fwrite(status2, 1, (size_t)N * max_seg2, o);
  fclose(o);
  free(bytes); free(img_seg); free(seg_tab); free(img_tab); free(qt); free(ht); free(x); free(piece_off); free(img_seg2); free(seg2); free(ent2);
  free(ix_status); free(seg2_out); free(ent2_out); free(coef); free(coef2); free(planes); free(pixels); free(pixels2); free(status); free(status2);
  return 0;
}
"""


def build_index_program(tmp, sanitize: bool = False) -> str:
    """g++ of the program above around csrc/jpeg_core.h -> the executable's path."""
    src, exe = os.path.join(str(tmp), "jpeg_index_main.cpp"), os.path.join(str(tmp), "jpeg_index_main" + ("_san" if sanitize else ""))
    open(src, "w").write(INDEX_MAIN)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(JC.ROOT, "vla_adapter_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def row_mcus(ix) -> int:
    """One MCU row: the default piece."""
    return ix.W // 16 if ix.h2v2 else ix.W // 8


def run_index(exe: str, tmp, tables: dict, piece_mcus: int, name: str = "store", ix=None, plan=None, hostile_entries: bool = False) -> dict:
    """The host program on the store `tables` -> dict(seg_tab int64 [S', 4], seg_ent int32 [S', 4], index_status u8 [S], pixels /
    status of the whole-segment decode, pixels_at / status_at of the piece-wise decode, coef_differ, ix, plan).  ``ix``: the (possibly
    hostile) index to pack in place of the parser's; ``plan``: (piece_off, img_seg, S', max_seg) in place of plan_pieces'.  A sanitizer
    report ends the program with a non-zero status, which raises here with its text."""
    ix = ix or JS.parse_frames(tables["frames_jpeg"], tables["frame_off"], tables["frame_shape"], name)
    piece_off, img_seg2, S2, max_seg2 = plan or JS.plan_pieces(ix, piece_mcus)
    src, dst = os.path.join(str(tmp), f"{name}-{piece_mcus}.bin"), os.path.join(str(tmp), f"{name}-{piece_mcus}.out")
    JC.write_packed(src, tables, ix)
    with open(src, "ab") as f:
        f.write(struct.pack("<4q", piece_mcus, S2, max_seg2, int(hostile_entries)))
        f.write(np.ascontiguousarray(piece_off, dtype=np.int64).tobytes())
        f.write(np.ascontiguousarray(img_seg2, dtype=np.int64).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: the host index program ended with status {r.returncode}:\n{r.stderr[-4000:]}"
    raw = open(dst, "rb").read()
    S, n, pos = int(ix.seg_tab.shape[0]), ix.N * ix.H * ix.W * 3, 8
    out = dict(coef_differ=struct.unpack("<q", raw[:8])[0], ix=ix, plan=(piece_off, img_seg2, S2, max_seg2))
    for key, dt, count, shape in (("seg_tab", np.int64, S2 * 4, (S2, 4)), ("seg_ent", np.int32, S2 * 4, (S2, 4)), ("index_status", np.uint8, S, (S,)),
                                  ("pixels", np.uint8, n, (ix.N, ix.H, ix.W, 3)), ("status", np.uint8, ix.N * ix.max_seg, (ix.N, ix.max_seg)),
                                  ("pixels_at", np.uint8, n, (ix.N, ix.H, ix.W, 3)), ("status_at", np.uint8, ix.N * max_seg2, (ix.N, max_seg2))):
        nbytes = count * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[pos:pos + nbytes], dtype=dt).reshape(shape).copy()
        pos += nbytes
    assert pos == len(raw)
    return out


# ---------------------------------------------------------------------------------------------------------------- the rule
@functools.lru_cache(maxsize=None)
def mcu_boundaries(data: bytes):
    """The rule's walk of a file, one list per segment: at every MCU of the segment (and behind its last one) the state in front of
    it - (bits consumed so far, the DC predictors of Y, Cb, Cr) - from tests/jpeg_rule_np.py's bit reader and Huffman tables alone.
    -> (parse, [[(bits, p0, p1, p2), ...]], MCUs per segment)."""
    p = R.parse(data)
    comps = p["comps"]
    h2v2 = (comps[0][1], comps[0][2]) == (2, 2)
    n_mcu = (p["W"] // 16) * (p["H"] // 16) if h2v2 else (p["W"] // 8) * (p["H"] // 8)
    order = [0, 0, 0, 0, 1, 2] if h2v2 else [0, 1, 2]
    per = p["dri"] or n_mcu
    out = []
    for si, seg in enumerate(p["segments"]):
        bits, pred, states = R.Bits(seg), [0, 0, 0], []
        for _ in range(si * per, min((si + 1) * per, n_mcu)):
            states.append((bits.pos, pred[0], pred[1], pred[2]))
            for c in order:
                td, ta = p["scan"][c]
                s = bits.symbol(p["ht"][td])
                pred[c] += R.extend(bits.take(s), s)
                k = 1
                while k < 64:
                    rs = bits.symbol(p["ht"][0x10 | ta])
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        bits.take(s)
                    elif r == 15:
                        k += 15
                    else:
                        break
                    k += 1
        out.append(states)
    return p, out, per


def raw_offset(seg: bytes, data_byte: int) -> int:
    """Where data byte `data_byte` of a segment stands among its bytes: a stuffed 0x00 is stepped over with its 0xFF."""
    i = 0
    for _ in range(data_byte):
        i += 2 if seg[i] == 0xFF else 1
    return i


def rule_tables(files, ix, piece_mcus: int):
    """(seg_tab int64 [S', 4], seg_ent int32 [S', 4]) of a store of good files by the rule: a piece begins at every MCU whose distance
    from its segment's first is a multiple of piece_mcus; lo is the byte that holds its first bit, hi the next piece's lo - plus one
    when that piece begins inside a byte, plus two when that byte is 0xFF - and the segment's hi for the last piece."""
    seg_rows, ent_rows, s = [], [], 0
    for data in files:
        p, per_seg, per = mcu_boundaries(data)
        for si, (seg, states) in enumerate(zip(p["segments"], per_seg)):
            lo, hi = int(ix.seg_tab[s, 0]), int(ix.seg_tab[s, 1])
            assert hi - lo == len(seg)
            offs = {}                                   # (one pass over the segment for all of its boundaries)
            want = sorted({st[0] >> 3 for st in states[::piece_mcus]})
            i = d = 0
            for w in want:
                while d < w:
                    i += 2 if seg[i] == 0xFF else 1
                    d += 1
                offs[w] = i
            first = len(seg_rows)
            for j, (c, p0, p1, p2) in enumerate(states[::piece_mcus]):
                at, bit, m0 = offs[c >> 3], c & 7, si * per + j * piece_mcus
                if j:
                    seg_rows[-1][1] = lo + at + (0 if bit == 0 else (2 if seg[at] == 0xFF else 1))
                seg_rows.append([lo + at, hi, m0, min(m0 + piece_mcus, si * per + len(states))])
                ent_rows.append([bit, p0, p1, p2])
            assert len(seg_rows) > first
            s += 1
    return np.array(seg_rows, dtype=np.int64), np.array(ent_rows, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- stuffing
@functools.lru_cache(maxsize=None)
def stuffing_stores():
    """{(H, W, h2v2): [JC.Case]}: the crafted corpus's stuffing cases (codes that are runs of ones: a tenth and more of the scan's
    bytes are stuffed pairs, at every offset modulo 8, and the last byte is one) and two larger ones made the same way, 64 x 64 in
    both samplings, for more MCU boundaries."""
    out = {k: [c for c in v if "codes-that-are-runs-of-ones" in c.name] for k, v in JC.crafted_stores(JC.crafted_corpus()).items()}
    out = {k: v for k, v in out.items() if v}
    for h2 in (1, 0):
        s = JC._spec(64, 64, h2)
        b = JC._blocks(s, 21)
        data = JC.JW.write(JC.with_tables(s, b, JC.ones, JC.ones, every_dc=True), b)
        out[(64, 64, h2)] = [JC.Case(f"64x64-{'420' if h2 else '444'}-codes-that-are-runs-of-ones", (64, 64), h2, data, JC.pillow_decode(data))]
    return out


# ---------------------------------------------------------------------------------------------------------------- damaged scans
@functools.lru_cache(maxsize=None)
def piecewise_corrupt_corpus():
    """[(name, file bytes)] at 32 x 48, 4:2:0, from one file without restart markers - six MCUs in one segment, so that damage falls
    into a piece with pieces in front of it and behind it (the files of JC.corrupt_corpus() hold one MCU per segment): intact, the
    scan truncated at every third byte, 150 seeded single-bit flips; kept as JC.parse_tolerant() keeps them."""
    data = JC.encode(JC.content("noise", 32, 48, seed=7), quality=95, subsampling=2)
    head, scan, tail = JC.split_scan(data)
    files = [("intact", data)] + [(f"truncated-at-{k}", head + scan[:k] + tail) for k in range(0, len(scan), 3)]
    g = np.random.default_rng(3248)
    for i in range(150):
        bit = int(g.integers(0, len(scan) * 8))
        s = bytearray(scan)
        s[bit // 8] ^= 1 << (bit % 8)
        files.append((f"flip-{i}-bit-{bit}", head + bytes(s) + tail))
    kept, _ = JC.parse_tolerant(files, 1, 32, 48)
    assert kept[0][0] == "intact" and len(kept) > 200
    return kept


def check_pieces_of_damaged_scans(o: dict, names) -> int:
    """What holds for the host program's (or the kernels') results `o` on damaged scans: the walk ends with the whole segment's status;
    the pieces in front of the first failing one report 0, every piece behind it a non-zero status; the piece-wise pixels are the
    whole-segment decode's.  -> how many segments failed in a piece that has pieces behind it."""
    ix, (piece_off, img_seg2, S2, max_seg2) = o["ix"], o["plan"]
    behind = 0
    for i in range(ix.N):
        for k in range(int(ix.img_seg[i + 1] - ix.img_seg[i])):
            s = int(ix.img_seg[i]) + k
            r0, r1 = int(piece_off[s] - img_seg2[i]), int(piece_off[s + 1] - img_seg2[i])
            st = o["status_at"][i, r0:r1]
            assert int(o["index_status"][s]) == int(o["status"][i, k]), f"{names[i]}: the walk's status differs from the decode's"
            if o["status"][i, k] == 0:
                assert not st.any(), f"{names[i]}: segment {k} decodes whole, its pieces report {st.tolist()}"
            else:
                bad = np.flatnonzero(st)
                assert bad.size and (st[bad[0]:] != 0).all() and st[bad[0]] == o["status"][i, k], f"{names[i]}: segment {k} fails with {o['status'][i, k]}, its pieces report {st.tolist()}"
                behind += bad[0] < r1 - r0 - 1
    bad = np.flatnonzero((o["pixels"] != o["pixels_at"]).reshape(ix.N, -1).any(1))
    assert bad.size == 0 and o["coef_differ"] == 0, f"piece-wise pixels differ from the whole-segment decode's for {[names[i] for i in bad[:5]]}"
    return behind


# ---------------------------------------------------------------------------------------------------------------- hostile tables
def hostile_variants(ix, piece_mcus: int):
    """[(name, index, plan)]: the tables of a good store with values no parser writes - lo / hi / MCU ranges / pool ids out of range,
    piece_off non-monotone and past S' - for the memory-safety runs (the host program under the sanitizers, then the kernels)."""
    import copy
    plan = JS.plan_pieces(ix, piece_mcus)
    big = 1 << 40
    out = []

    def variant(name, edit_ix=None, edit_plan=None):
        v, pl = copy.deepcopy(ix), [np.array(a) if isinstance(a, np.ndarray) else a for a in plan]
        if edit_ix:
            edit_ix(v)
        if edit_plan:
            edit_plan(pl)
        out.append((name, v, tuple(pl)))

    def lo_hi(v):
        v.seg_tab[0::3, 0], v.seg_tab[1::3, 1], v.seg_tab[2::3, 0] = -big, big, big
    variant("lo-hi-out-of-range", lo_hi)

    def swapped(v):
        v.seg_tab[:, [0, 1]] = v.seg_tab[:, [1, 0]]
    variant("lo-hi-swapped", swapped)

    def mcus(v):
        v.seg_tab[0::2, 2], v.seg_tab[0::2, 3], v.seg_tab[1::2, 3] = -big, big, -5
    variant("mcu-ranges-out-of-range", mcus)

    def pools(v):
        v.img_tab[0::2, :9], v.img_tab[1::2, :9] = 2 ** 31 - 1, -2 ** 31
    variant("pool-ids-out-of-range", pools)

    def img_seg(v):
        v.img_seg[1::2] = big
        v.img_seg[2::4] = -big
    variant("img-seg-out-of-range", img_seg)

    def piece_off_bad(pl):
        pl[0] = pl[0].copy()
        pl[0][1::2] = pl[0][1::2][::-1].copy()          # non-monotone
        pl[0][-1] = big                                 # and past S'
        pl[0][0] = -big
    variant("piece-off-non-monotone-and-past-the-end", None, piece_off_bad)

    def piece_off_huge(pl):
        pl[0] = np.full_like(pl[0], big)
        pl[0][0] = 0
    variant("piece-off-gives-the-first-segment-every-row", None, piece_off_huge)
    return out
