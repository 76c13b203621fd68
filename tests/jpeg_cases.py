"""What the JPEG tests share (tests/test_jpeg_cpu.py, test_jpeg_core_cpu.py, test_jpeg_gpu.py, test_jpeg_store_gpu.py, ...): the matrix
of encoder settings, contents and shapes the decode is pinned on, Pillow as the reference, stores packed from such files, the corrupt
corpus, and the stand-alone host program around csrc/jpeg_core.h (compiled with g++ at test time) whose output is the truth for
malformed input.  Everything here is computed once per process and left unchanged."""
import collections
import functools
import io
import os
import re
import struct
import subprocess

import numpy as np
import torch
from PIL import Image

from tests import jpeg_rule_np as R
from tests import jpeg_writer as JW
from vla_adapter_amd import jpeg_store as JS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16, 16), (32, 48), (48, 16))                 # (H, W)
CONTENTS = ("noise", "ramp", "flat", "saturated")
# the six encoder settings: name -> Pillow save arguments; the first four are 4:2:0, the last two 4:4:4
SETTINGS = {
    "q95_420": dict(quality=95, subsampling=2),
    "q50_420": dict(quality=50, subsampling=2),
    "q90_420_rst_rows": dict(quality=90, subsampling=2, restart_marker_rows=1),
    "q95_420_rst_blocks_opt": dict(quality=95, subsampling=2, restart_marker_blocks=1, optimize=True),
    "q100_444": dict(quality=100, subsampling=0),
    "q75_444_opt": dict(quality=75, subsampling=0, optimize=True),
}


def content(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    g = np.random.default_rng(seed * 1000 + H * 7 + W)
    if kind == "noise":
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "saturated":
        return (g.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    if kind == "flat":
        return np.full((H, W, 3), (200, 30, 90), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], -1).astype(np.uint8)


def encode(arr: np.ndarray, mode: str = "RGB", **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(arr).convert(mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def matrix():
    """The 72 cases: [(name, (H, W), setting, file bytes, Pillow's pixels)]."""
    out = []
    for H, W in SHAPES:
        for kind in CONTENTS:
            for sname, kw in SETTINGS.items():
                data = encode(content(kind, H, W), **kw)
                out.append((f"{H}x{W}-{kind}-{sname}", (H, W), sname, data, pillow_decode(data)))
    return out


def pack(files, n_img: int, H: int, W: int) -> dict:
    """The three JPEG keys of an episode dict from files in (t, cam) order."""
    off = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    return dict(frames_jpeg=torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy()), frame_off=torch.from_numpy(off),
                frame_shape=torch.tensor([n_img, H, W], dtype=torch.int64))


def episode_dict(files, n_img: int, H: int, W: int, lengths, A: int = 7, Pd: int = 8, seed: int = 0, raw: bool = False) -> dict:
    """An episode file's dict over the files (T * n_img of them); raw=True: its raw twin, the Pillow-decoded frames as frames_u8."""
    g = torch.Generator().manual_seed(seed)
    T = sum(lengths)
    assert len(files) == T * n_img
    plens = [(3 + 2 * e) % 7 for e in range(len(lengths))]
    d = dict(actions_raw=torch.randn(T, A, generator=g) * 2, proprio_raw=torch.randn(T, Pd, generator=g) * 2,
             episode_off=torch.tensor(np.cumsum([0] + list(lengths)), dtype=torch.int64),
             prompt_flat=torch.randint(1, 1000, (sum(plens),), generator=g, dtype=torch.int64),
             prompt_off=torch.tensor(np.cumsum([0] + plens), dtype=torch.int32))
    if raw:
        d["frames_u8"] = torch.from_numpy(np.stack([pillow_decode(f) for f in files]).reshape(T, n_img, H, W, 3).copy())
    else:
        d.update(pack(files, n_img, H, W))
    return d


def stores_of_the_matrix():
    """The matrix grouped into stores - one per (shape, sampling), since a store keeps one of each: {(H, W, h2v2): [case, ...]}.  A
    store of 4:2:0 files mixes four table sets and files with and without restart markers."""
    groups = {}
    for case in matrix():
        (H, W), sname = case[1], case[2]
        groups.setdefault((H, W, int("420" in sname)), []).append(case)
    return groups


# ---------------------------------------------------------------------------------------------------------------- the corrupt corpus
def split_scan(data: bytes):
    """(header up to and including the SOS segment, scan bytes, the trailing EOI) of a file JS.parse_frames accepts."""
    b = np.frombuffer(data, dtype=np.uint8)
    ix = JS.parse_frames(b, [0, len(data)], (1,) + pillow_decode(data).shape[:2], "split_scan")
    start = int(ix.seg_tab[0, 0])
    end = int(ix.seg_tab[-1, 1])
    return data[:start], data[start:end], data[end:]


@functools.lru_cache(maxsize=None)
def corrupt_corpus():
    """{(H, W): [(name, file bytes)]} made from a 16 x 16 file and a 32 x 16 one (the latter with a restart marker per MCU):
    truncation of the scan at every byte position, 200 seeded single-bit flips of the scan, scan bytes replaced by 0xFF bytes, and the
    restart marker removed."""
    out = {}
    for (H, W), kw in (((16, 16), dict(quality=95, subsampling=2)), ((32, 16), dict(quality=95, subsampling=2, restart_marker_blocks=1))):
        data = encode(content("noise", H, W, seed=3), **kw)
        head, scan, tail = split_scan(data)
        files = [("intact", data)]
        files += [(f"truncated-at-{k}", head + scan[:k] + tail) for k in range(len(scan))]
        g = np.random.default_rng(H * 100 + W)
        for i in range(200):
            bit = int(g.integers(0, len(scan) * 8))
            s = bytearray(scan)
            s[bit // 8] ^= 1 << (bit % 8)
            files.append((f"flip-{i}-bit-{bit}", head + bytes(s) + tail))
        for k in (0, len(scan) // 3, len(scan) - 8):
            s = bytearray(scan)
            s[k:k + 6] = b"\xff" * 6
            files.append((f"ff-bytes-at-{k}", head + bytes(s) + tail))
        rst = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
        for i in rst[:1]:
            files.append((f"restart-marker-{i}-removed", head + scan[:i] + scan[i + 2:] + tail))
        out[(H, W)] = files
    return out


def parse_tolerant(files, n_img: int, H: int, W: int):
    """(the files parse_frames accepts one by one, the names of those it refuses): a flipped bit may plant a marker in the scan, which
    the parser refuses at load - a refusal is a valid end for a damaged file, and such files reach no decoder."""
    kept, refused = [], []
    for name, data in files:
        try:
            JS.parse_frames(np.frombuffer(data, dtype=np.uint8), [0, len(data)], (1, H, W), name)
            kept.append((name, data))
        except ValueError:
            refused.append(name)
    return kept, refused


# ---------------------------------------------------------------------------------------------------------------- the host program
CORE_MAIN = r"""
// Decodes every image of a packed store with csrc/jpeg_core.h on the host: argv[1] the store, argv[2] the output (pixels u8
// [N, H, W, 3], then status u8 [N, max_seg]).  Every buffer is a heap block of its exact size, so that a sanitizer sees an overrun.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "jpeg_core.h"
using namespace vlajpeg;
template <class T> static T* take(FILE* f, size_t n) {
  T* p = (T*)malloc(n ? n * sizeof(T) : 1);
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short store file\n"); exit(2); }
  return p;
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
  fclose(f);
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt, nQ, ht, nH};
  const i64 nb = blocks_per_image(H, W, h2v2);
  short* coef = (short*)malloc(nb * 64 * sizeof(short));
  u8* planes = (u8*)malloc(nb * 64);
  u8* pixels = (u8*)malloc((size_t)N * H * W * 3);
  u8* status = (u8*)calloc((size_t)N * max_seg, 1);
  for (i64 img = 0; img < N; ++img) {
    memset(coef, 0x55, nb * 64 * sizeof(short));
    for (int k = 0; k < max_seg; ++k) {
      const int rc = decode_item(st, img, k, H, W, h2v2, coef);
      status[img * max_seg + k] = (u8)(rc < 0 ? 0 : rc);
    }
    for (i64 b = 0; b < nb; ++b) {
      i64 stride;
      const i64 o = plane_offset(b, H, W, h2v2, stride);
      idct_islow(coef + b * 64, planes + o, stride);
    }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) plane_pixel(planes, H, W, h2v2, y, x, pixels + ((size_t)img * H * W + (size_t)y * W + x) * 3);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(pixels, 1, (size_t)N * H * W * 3, o);
  fwrite(status, 1, (size_t)N * max_seg, o);
  fclose(o);
  free(bytes); free(img_seg); free(seg_tab); free(img_tab); free(qt); free(ht); free(coef); free(planes); free(pixels); free(status);
  return 0;
}
"""
STORE_MAGIC = 0x4A50454753544F52


def build_core(tmp, sanitize: bool = False) -> str:
    """g++ of the program above around csrc/jpeg_core.h -> the executable's path."""
    src, exe = os.path.join(str(tmp), "jpeg_core_main.cpp"), os.path.join(str(tmp), "jpeg_core_main" + ("_san" if sanitize else ""))
    open(src, "w").write(CORE_MAIN)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "vla_adapter_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def write_packed(path: str, tables: dict, ix: JS.JpegIndex) -> None:
    data = tables["frames_jpeg"].numpy().tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<10q", STORE_MAGIC, ix.N, ix.H, ix.W, ix.h2v2, len(data), ix.seg_tab.shape[0], ix.qt_pool.shape[0],
                            ix.ht_pool.shape[0], ix.max_seg))
        f.write(data)
        for a, dt in ((ix.img_seg, np.int64), (ix.seg_tab, np.int64), (ix.img_tab, np.int32), (ix.qt_pool, np.uint16), (ix.ht_pool, np.int32)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())


def run_core(exe: str, tmp, tables: dict, name: str = "store"):
    """The host program on the store `tables` (the three JPEG keys) -> (pixels u8 [N, H, W, 3], status u8 [N, max_seg], the index).
    A sanitizer report ends the program with a non-zero status, which raises here with its text."""
    ix = JS.parse_frames(tables["frames_jpeg"], tables["frame_off"], tables["frame_shape"], name)
    src, dst = os.path.join(str(tmp), name + ".bin"), os.path.join(str(tmp), name + ".out")
    write_packed(src, tables, ix)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: the host decode ended with status {r.returncode}:\n{r.stderr[-4000:]}"
    out = np.fromfile(dst, dtype=np.uint8)
    n = ix.N * ix.H * ix.W * 3
    return out[:n].reshape(ix.N, ix.H, ix.W, 3), out[n:].reshape(ix.N, ix.max_seg), ix


# ---------------------------------------------------------------------------------------------------------------- the crafted corpus
# Files no run of Pillow's encoder writes, most of them made by tests/jpeg_writer.py from coefficient blocks: Huffman tables of every
# legal shape, block structures, byte stuffing, restart intervals, header layouts, colour markers.  The truth is Pillow's decode of
# the file; every case carries the property that makes it worth having as numbers a test asserts (`checks`: (what, got, want), want a
# number to equal or AtLeast(n)), read from the file by the rule's own parser and entropy decode (tests/jpeg_rule_np.py), so that no
# later edit can empty a case.
Case = collections.namedtuple("Case", "name shape h2v2 data pixels")


class AtLeast(int):
    """In a check: the number is a lower bound, not the value to equal."""
MARKERISH = b"\xff\xd8\xff\xda\xff\xd9\xff\xc4"             # SOI, SOS, EOI and DHT byte pairs, for payloads that must be skipped


def stage_bytes() -> int:
    """STAGE_BYTES of csrc/jpeg.hip: the longest segment the wave mapping stages in LDS."""
    txt = open(os.path.join(ROOT, "vla_adapter_amd", "csrc", "jpeg.hip")).read()
    a, b = re.search(r"constexpr int STAGE_BYTES = (\d+) \* (\d+);", txt).groups()
    return int(a) * int(b)


def soft_planes(H: int, W: int, h2v2: bool, seed: int, amp: int = 10):
    """[Y, Cb, Cr] uint8 planes of a frame (the chroma planes half as large with h2v2): waves under noise of +-amp, gentle enough
    that every block stays far inside the writer's bound."""
    g, out = np.random.default_rng(seed), []
    for c, (h, w) in enumerate([(H, W)] + [(H // 2, W // 2) if h2v2 else (H, W)] * 2):
        y, x = np.mgrid[0:h, 0:w]
        base = 128 + (40 - 12 * c) * np.sin(x / (3.0 + c) + seed) * np.cos(y / (4.0 + c))
        out.append(np.clip(base + g.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8))
    return out


def qtab(a: int, b: int) -> list:
    """A quantisation table that grows along the zigzag: a + b * (k // 8)."""
    return [min(255, a + b * (k // 8)) for k in range(64)]


def _ranked(freq: dict) -> list:
    return [s for s, _ in sorted(freq.items(), key=lambda kv: (-kv[1], kv[0]))]           # the commonest first


_PLAIN = [2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7] + [8] * 4 + [9] * 4 + [10] * 8 + [11] * 8 + [12] * 16 + [13] * 32 + [14] * 64 + [15] * 128
_MIXED = [9, 1, 10, 3, 11, 4, 12, 5, 13, 6, 14, 7, 15, 8, 16] + [9 + i % 8 for i in range(256)]


def plain(freq):
    """Short codes for common symbols, as an encoder would choose."""
    return [(s, _PLAIN[i]) for i, s in enumerate(_ranked(freq))]


def long_codes(freq):
    """Every code has 9 to 16 bits: an 8-bit lookup never hits."""
    return [(s, 9 + i % 8) for i, s in enumerate(_ranked(freq))]


def commonest_16(freq):
    """The four commonest symbols have 16-bit codes, the others plain ones."""
    r = _ranked(freq)
    return [(s, _PLAIN[i]) for i, s in enumerate(r[4:])] + [(s, 16) for s in r[:4]]


def mixed(freq):
    """One code of every length 1, 3, 4 .. 16 - long and short in turn down the ranks, so that both sides of the 8 / 9 boundary are
    common - then lengths 9 .. 16 in turn."""
    return [(s, _MIXED[i]) for i, s in enumerate(_ranked(freq))]


def ones(freq):
    """Codes that are runs of ones: the d rarest symbols take the chain 0, 10, 110, ... of lengths 1 .. d, every other symbol a 16-bit
    code behind it, which starts with d ones, the commonest the largest.  d is the deepest chain that leaves room for the others."""
    r = _ranked(freq)
    d = max(k for k in range(0, 16) if k < len(r) and k + (1 << (16 - k)) - 1 >= len(r))
    return [(s, i + 1) for i, s in enumerate(reversed(r[len(r) - d:]))] + [(s, 16) for s in reversed(r[:len(r) - d])]


def with_tables(spec: JW.Spec, blocks, dc_policy=plain, ac_policy=plain, every_dc: bool = False) -> JW.Spec:
    """The spec with one Huffman table per table id that its components name, holding the symbols those components code, with the
    code lengths the policy gives them (a dict {id: policy} gives every table its own).  every_dc: all twelve DC categories."""
    dcf, acf = JW.symbols_used(spec, blocks)
    for freqs, ids, policy, dest in ((dcf, spec.comp_td, dc_policy, spec.dc_tables), (acf, spec.comp_ta, ac_policy, spec.ac_tables)):
        for tid in sorted(set(ids)):
            f = {s: 0 for s in range(12)} if every_dc and dest is spec.dc_tables else {}
            for c in range(3):
                if ids[c] == tid:
                    for s, n in freqs[c].items():
                        f[s] = f.get(s, 0) + n
            dest[tid] = JW.huffman_from_lengths((policy[tid] if isinstance(policy, dict) else policy)(f))
    return spec


def _spec(H, W, h2v2, **kw) -> JW.Spec:
    kw.setdefault("qtables", {0: qtab(2, 1), 1: qtab(3, 2)})
    return JW.Spec(H=H, W=W, h2v2=bool(h2v2), dc_tables={}, ac_tables={}, **kw)


def _blocks(spec: JW.Spec, seed: int, amp: int = 10):
    return [JW.blocks_from_pixels(pl, spec.qtables[spec.comp_tq[c]]) for c, pl in enumerate(soft_planes(spec.H, spec.W, spec.h2v2, seed, amp))]


def _zero_blocks(spec: JW.Spec):
    bh, bw = spec.H // 8, spec.W // 8
    return [np.zeros(s + (64,), dtype=np.int64) for s in [(bh, bw)] + [(bh // 2, bw // 2) if spec.h2v2 else (bh, bw)] * 2]


def facts(data: bytes) -> dict:
    """What the checks read: the rule's parse of the file (markers, tables, segments) and the counters of its decode."""
    st = {}
    rule = R.decode(data, st)
    p = R.parse(data)
    scan = b"".join(p["segments"])
    pairs = [[i for i in range(len(s) - 1) if s[i] == 0xFF and s[i + 1] == 0] for s in p["segments"]]
    ac = [syms[1:] for _, syms in st["blocks"]]
    return dict(p=p, rule=rule, by_length=st["by_length"], consumed=st["consumed"], blocks=st["blocks"], ac=ac, scan_bytes=len(scan),
                segments=len(p["segments"]), seg_len=[len(s) for s in p["segments"]], pairs=sum(len(x) for x in pairs),
                pair_offsets=len({i % 8 for x in pairs for i in x}), last_pair=sum(1 for s in p["segments"] if s[-2:] == b"\xff\x00"),
                short=sum(st["by_length"][1:9]), long=sum(st["by_length"][9:]), dc_cats={syms[0] for _, syms in st["blocks"]},
                ac_cats={s & 15 for a in ac for s in a if s & 15}, markers=_markers(data))


def _markers(data: bytes) -> list:
    """[(marker code, payload, fill bytes in front of it)] of the header, SOS included."""
    out, pos = [], 2
    while True:
        fill = 0
        while data[pos + 1] == 0xFF:
            pos, fill = pos + 1, fill + 1
        L = (data[pos + 2] << 8) | data[pos + 3]
        out.append((data[pos + 1], data[pos + 4:pos + 2 + L], fill))
        if data[pos + 1] == 0xDA:
            return out
        pos += 2 + L


def _dht_definitions(markers) -> int:
    n = 0
    for m, pl, _ in markers:
        i = 0
        while m == 0xC4 and i < len(pl):
            i, n = i + 17 + sum(pl[i + 1:i + 17]), n + 1
    return n


def _tables_differ(p: dict, keys) -> int:
    return len({repr(sorted(p["ht"][k].items())) for k in keys})


@functools.lru_cache(maxsize=None)
def crafted_corpus():
    """[(Case, checks)]: checks = lambda facts -> [(what, got, want)], want a number to equal or AtLeast(n); 16 x 16 and 32 x 48 in both
    samplings."""
    out = []

    def add(name, spec, blocks, checks):
        data = JW.write(spec, blocks)
        out.append((Case(name, (spec.H, spec.W), int(spec.h2v2), data, pillow_decode(data)), checks))

    def add_file(name, H, W, h2v2, data, checks):
        out.append((Case(name, (H, W), int(h2v2), data, pillow_decode(data)), checks))

    # ---- Huffman tables
    for H, W, h2 in ((16, 16, 1), (32, 48, 1), (32, 48, 0)):
        tag = f"{H}x{W}-{'420' if h2 else '444'}"
        s = _spec(H, W, h2)
        b = _blocks(s, 1)
        add(f"{tag}-codes-of-9-to-16-bits", with_tables(s, b, long_codes, long_codes), b,
            lambda f: [("symbols with codes of 9 or more bits", f["long"], AtLeast(200)), ("symbols with shorter codes", f["short"], 0)])
        s = _spec(H, W, h2)
        add(f"{tag}-commonest-symbols-16-bits", with_tables(s, b, commonest_16, commonest_16), b,
            lambda f: [("symbols with 16-bit codes", f["by_length"][16], AtLeast(100)),
                       ("16-bit codes more than those of any other length", f["by_length"][16] - max(f["by_length"][:16]), AtLeast(1))])
        s = _spec(H, W, h2)
        add(f"{tag}-lengths-1-to-16-mixed", with_tables(s, b, mixed, mixed), b,
            lambda f: [("symbols with codes of 9 or more bits", f["long"], AtLeast(50)), ("symbols with codes of 8 or fewer bits", f["short"], AtLeast(50)),
                       ("code lengths in use", sum(1 for n in f["by_length"] if n), AtLeast(12))])
    for H, W, h2 in ((16, 16, 0), (32, 48, 1)):
        tag = f"{H}x{W}-{'420' if h2 else '444'}"
        s = _spec(H, W, h2, comp_td=(3, 0, 2), comp_ta=(1, 3, 0))
        b = _blocks(s, 2)
        add(f"{tag}-three-table-pairs-ids-0-to-3", with_tables(s, b, {3: plain, 0: mixed, 2: long_codes}, {1: mixed, 3: plain, 0: commonest_16}), b,
            lambda f: [("different DC tables", _tables_differ(f["p"], (3, 0, 2)), 3), ("different AC tables", _tables_differ(f["p"], (0x11, 0x13, 0x10)), 3),
                       ("Huffman table ids in use", len({t for pair in f["p"]["scan"] for t in pair}), 4)])
        s = _spec(H, W, h2, qtables={3: qtab(2, 1), 2: qtab(3, 2), 0: qtab(5, 0)}, comp_tq=(3, 2, 0))
        b = _blocks(s, 3)
        add(f"{tag}-three-quantisation-tables-ids-3-2-0", with_tables(s, b), b,
            lambda f: [("different quantisation tables", len({tuple(f["p"]["qt"][c[3]]) for c in f["p"]["comps"]}), 3),
                       ("components whose table id is not libjpeg's (0, 1, 1)", sum(c[3] != t for c, t in zip(f["p"]["comps"], (0, 1, 1))), 3)])

    # ---- block structure (16 x 16, 4:2:0 and 4:4:4: the structure sits in a Y, a Cb and a Cr block)
    ones_q = {0: [1] * 64, 1: [1] * 64}
    for h2 in (1, 0):
        tag = f"16x16-{'420' if h2 else '444'}"

        def structure(name, fill, checks, seed, **kw):
            s = _spec(16, 16, h2, **kw)
            b = _blocks(s, seed)
            for c in range(3):
                fill(b[c][0, 0] if c else b[c][1, 1], c)
            add(f"{tag}-{name}", with_tables(s, b, plain, mixed), b, checks)

        def only_63(blk, c):
            blk[1:] = 0
            blk[63] = 3 - c
        structure("ac-only-at-zigzag-63", only_63,
                  lambda f: [("blocks coded ZRL, ZRL, ZRL, run 14", sum(a[:3] == [0xF0] * 3 and a[3] >> 4 == 14 and len(a) == 4 for a in f["ac"]), 3)], 4)

        def all_63(blk, c):
            blk[1:] = [(-1) ** k * (1 + (k + c) % 3) for k in range(1, 64)]
        structure("all-63-ac-nonzero", all_63, lambda f: [("blocks of 63 values and no EOB", sum(len(a) == 63 and 0 not in a for a in f["ac"]), 3)], 5)

        def dc_only(blk, c):
            blk[1:] = 0
        structure("eob-straight-after-dc", dc_only, lambda f: [("blocks whose AC part is EOB alone", sum(a == [0] for a in f["ac"]), 3)], 6)

        def run_15(blk, c):
            blk[1:] = 0
            blk[16], blk[32 + c] = 1, -1
        structure("run-of-15-in-a-value-symbol", run_15, lambda f: [("0xF1 symbols", sum(a.count(0xF1) for a in f["ac"]), AtLeast(3))], 7)

        def zrl_then_eob(blk, c):
            blk[1 + 3 * c:] = 0
        s = _spec(16, 16, h2, zrl_eob=((0, 1, 1), (1, 0, 0), (2, 0, 0)))
        b = _blocks(s, 8)
        for c in range(3):
            zrl_then_eob(b[c][0, 0] if c else b[c][1, 1], c)
        add(f"{tag}-zrl-then-eob", with_tables(s, b, plain, mixed), b,
            lambda f: [("blocks that end ZRL, EOB", sum(a[-2:] == [0xF0, 0] for a in f["ac"]), 3)])
    for h2 in (1, 0):                                       # every category: quantiser 1, DC levels that swing to +-1000
        s = _spec(32, 48, h2, qtables=ones_q)
        b = _zero_blocks(s)
        dc = np.cumsum([0, 1, -3, 7, -15, 31, -63, 127, -255, 511, -1023, 1500, -1700, 1900])          # differences of category 0 .. 11
        order = [(y, x) for my in range(2) for mx in range(3) for y in (2 * my, 2 * my + 1) for x in (2 * mx, 2 * mx + 1)] if h2 else \
                [(y, x) for y in range(4) for x in range(6)]
        for i, (y, x) in enumerate(order[:len(dc)]):
            b[0][y, x, 0] = dc[i]
        for cat in range(1, 11):                            # an AC value of every category, on either sign, at a place of its own
            blk = b[1 + cat % 2][(cat // 2) % 2, (cat // 4) % 3]
            blk[cat] = (1 << cat) - 1 if cat % 3 else -(1 << (cat - 1))
        add(f"32x48-{'420' if h2 else '444'}-every-category", with_tables(s, b, mixed, mixed), b,
            lambda f: [("DC difference categories 0 .. 11 in use", len(f["dc_cats"] & set(range(12))), 12),
                       ("AC categories 1 .. 10 in use", len(f["ac_cats"] & set(range(1, 11))), 10)])

    # ---- byte stuffing
    for H, W, h2 in ((16, 16, 1), (32, 48, 1), (32, 48, 0)):
        tag = f"{H}x{W}-{'420' if h2 else '444'}"
        s = _spec(H, W, h2, qtables={0: qtab(2, 1)[:63] + [1], 1: qtab(3, 2)[:63] + [1]})
        b = _blocks(s, 9)
        b[2][-1, -1, 63] = 255                              # the last value's bits are ones, and so is the padding: the last byte is 0xFF
        add(f"{tag}-codes-that-are-runs-of-ones", with_tables(s, b, ones, ones, every_dc=True), b,
            lambda f: [("stuffed pairs, in tenths of the entropy-coded bytes", f["pairs"] * 10 // f["scan_bytes"], AtLeast(1)),
                       ("segments whose last data byte is a stuffed 0xFF 0x00", f["last_pair"], 1),
                       ("offsets modulo 8 at which a stuffed pair stands", f["pair_offsets"], 8)])

    # ---- restart intervals
    noise = content("noise", 32, 48, seed=5)
    for h2, sub in ((1, 2), (0, 0)):
        for n, segs in ((2, 3 if h2 else 12), (5, 2 if h2 else 5)):
            add_file(f"32x48-{'420' if h2 else '444'}-restart-every-{n}-mcus", 32, 48, h2, encode(noise, quality=90, subsampling=sub, restart_marker_blocks=n),
                     lambda f, n=n, segs=segs: [("restart interval", f["p"]["dri"], n), ("segments", f["segments"], segs)])
        add_file(f"32x48-{'420' if h2 else '444'}-restart-interval-past-the-last-mcu", 32, 48, h2, encode(noise, quality=90, subsampling=sub, restart_marker_blocks=100),
                 lambda f: [("restart interval", f["p"]["dri"], 100), ("segments", f["segments"], 1)])
        s = _spec(32, 48, h2, restart=0)
        b = _blocks(s, 10)
        add(f"32x48-{'420' if h2 else '444'}-dri-0-written", with_tables(s, b), b,
            lambda f: [("DRI segments", sum(m == 0xDD for m, _, _ in f["markers"]), 1), ("restart interval", f["p"]["dri"], 0)])
        s = _spec(32, 48, h2, restart=2, rst_fill=2, eoi_fill=1)
        b = _blocks(s, 11)
        add(f"32x48-{'420' if h2 else '444'}-fill-bytes-in-front-of-rstn", with_tables(s, b), b,
            lambda f, segs=3 if h2 else 12: [("segments", f["segments"], segs),
                                             ("RSTn markers with two fill bytes in front", len(re.findall(rb"[^\xff]\xff\xff\xff[\xd0-\xd7]", f["data"])), segs - 1),
                                             ("fill bytes in front of EOI", int(f["data"].endswith(b"\xff\xff\xd9") and not f["data"].endswith(b"\xff\xff\xff\xd9")), 1)])

    # ---- header layout
    for H, W, h2 in ((16, 16, 1), (32, 48, 0)):
        tag = f"{H}x{W}-{'420' if h2 else '444'}"
        dht_all = [(0, 0), (1, 0), (0, 1), (1, 1)]

        def layout(name, items, checks, seed=12, **kw):
            s = _spec(H, W, h2, layout=items, **kw)
            b = _blocks(s, seed)
            add(f"{tag}-{name}", with_tables(s, b), b, checks)
        layout("tables-in-one-dht-and-one-dqt", [("JFIF",), ("DQT", [0, 1]), ("SOF",), ("DHT", dht_all)],
               lambda f: [("DQT segments", sum(m == 0xDB for m, _, _ in f["markers"]), 1), ("DHT segments", sum(m == 0xC4 for m, _, _ in f["markers"]), 1),
                          ("tables in the DHT segment", len(f["p"]["ht"]), 4)])
        layout("dqt-after-sof0", [("JFIF",), ("SOF",), ("DHT", dht_all), ("DQT", [1]), ("DQT", [0])],
               lambda f: [("DQT segments behind SOF0", sum(m == 0xDB for m, _, _ in f["markers"][[m for m, _, _ in f["markers"]].index(0xC0):]), 2)])
        decoy_h = JW.huffman_from_lengths([(s_, 8) for s_ in range(200)])
        layout("tables-defined-twice", [("JFIF",), ("DQT", [(0, [7] * 64), (1, [9] * 64)]), ("DHT", [(0, 0) + decoy_h, (1, 0) + decoy_h, (1, 1) + decoy_h]), ("SOF",),
                                        ("DQT", [0, 1]), ("DHT", dht_all)],
               lambda f: [("quantisation tables defined twice", sum(len(pl) // 65 for m, pl, _ in f["markers"] if m == 0xDB) - len(f["p"]["qt"]), 2),
                          ("Huffman tables defined twice", _dht_definitions(f["markers"]) - len(f["p"]["ht"]), 3)])
        layout("fill-bytes-in-front-of-header-markers", [("FILL", 1), ("JFIF",), ("FILL", 3), ("DQT", [0]), ("FILL", 2), ("DQT", [1]), ("FILL", 1), ("SOF",), ("FILL", 7),
                                                         ("DHT", dht_all), ("FILL", 2)],
               lambda f: [("header markers with fill bytes in front", sum(fill > 0 for _, _, fill in f["markers"]), 6), ("fill bytes in front of SOS", f["markers"][-1][2], 2)])
        layout("payloads-full-of-marker-bytes", [("JFIF",), ("COM", MARKERISH * 40), ("APP", 1, b"Exif\0\0" + MARKERISH * 100), ("DQT", [0, 1]),
                                                 ("APP", 2, MARKERISH * 5000), ("SOF",), ("COM", b"\xff" + MARKERISH), ("DHT", dht_all)],
               lambda f: [("payloads that hold SOI, SOS, EOI and DHT byte pairs", sum(MARKERISH in pl for m, pl, _ in f["markers"] if m in (0xFE, 0xE1, 0xE2)), 4),
                          ("the longest of them, bytes", max(len(pl) for m, pl, _ in f["markers"] if m == 0xE2), AtLeast(32 * 1024 + 1))])
        layout("no-app0-ids-1-2-3", [("DQT", [0]), ("DQT", [1]), ("SOF",), ("DHT", dht_all)],
               lambda f: [("APPn segments", sum(0xE0 <= m <= 0xEF for m, _, _ in f["markers"]), 0),
                          ("component ids 1, 2, 3", int([c[0] for c in f["p"]["comps"]] == [1, 2, 3]), 1)])
        layout("jfif-ids-0-1-2", None, lambda f: [("component ids 0, 1, 2", int([c[0] for c in f["p"]["comps"]] == [0, 1, 2]), 1)], comp_ids=(0, 1, 2))
        layout("bytes-behind-eoi", None, lambda f: [("bytes behind EOI", len(f["data"]) - f["data"].index(b"\xff\xd9", f["data"].index(b"\xff\xda")) - 2, AtLeast(40))],
               trailer=b"\x00\x01" + MARKERISH * 5 + b"tail")
        # ---- colour coding that libjpeg reads as YCbCr
        layout("jfif-with-ids-r-g-b", None,
               lambda f: [("component ids 'R', 'G', 'B' behind a JFIF marker", int([c[0] for c in f["p"]["comps"]] == [82, 71, 66] and f["markers"][0][0] == 0xE0), 1)],
               comp_ids=(82, 71, 66))
        layout("adobe-transform-1-without-jfif", [("ADOBE", 1), ("DQT", [0, 1]), ("SOF",), ("DHT", dht_all)],
               lambda f: [("Adobe markers with transform 1", sum(m == 0xEE and pl[11] == 1 for m, pl, _ in f["markers"]), 1),
                          ("JFIF markers", sum(m == 0xE0 for m, _, _ in f["markers"]), 0)])
    assert len({c.name for c, _ in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def crafted_facts(name: str) -> dict:
    case = next(c for c, _ in crafted_corpus() + long_corpus() if c.name == name)
    return dict(facts(case.data), data=case.data)


def crafted_stores(corpus):
    """The cases of a corpus grouped into stores as stores_of_the_matrix() groups the matrix: {(H, W, h2v2): [Case, ...]}."""
    groups = {}
    for case, _ in corpus:
        groups.setdefault(case.shape + (case.h2v2,), []).append(case)
    return groups


@functools.lru_cache(maxsize=None)
def refused_colour():
    """[(name, (H, W), file bytes, what the refusal says)]: three components that libjpeg reads as RGB."""
    out = [("pillow-keep-rgb", (32, 48), encode(content("noise", 32, 48), quality=90, keep_rgb=True), "Adobe transform 0")]
    s = _spec(32, 48, 1, comp_ids=(82, 71, 66), layout=[("DQT", [0, 1]), ("SOF",), ("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)])])
    b = _blocks(s, 13)
    out.append(("ids-r-g-b-without-jfif-or-adobe", (32, 48), JW.write(with_tables(s, b), b), "component ids 'R', 'G', 'B'"))
    data = encode(content("noise", 32, 48), quality=90, subsampling=2)                 # the issue's second file: a Pillow 4:2:0 file, its
    i, j, k = data.index(b"\xff\xe0"), data.index(b"\xff\xc0"), data.index(b"\xff\xda")          # APP0 removed and its ids rewritten
    d = bytearray(data)
    for at, step in ((j + 10, 3), (k + 5, 2)):
        d[at], d[at + step], d[at + 2 * step] = 82, 71, 66
    L = (data[i + 2] << 8) | data[i + 3]
    out.append(("pillow-420-app0-removed-ids-r-g-b", (32, 48), bytes(d[:i] + d[i + 2 + L:]), "component ids 'R', 'G', 'B'"))
    s = _spec(32, 48, 0, layout=[("ADOBE", 0), ("DQT", [0, 1]), ("SOF",), ("DHT", [(0, 0), (1, 0), (0, 1), (1, 1)])])
    out.append(("adobe-transform-0-ids-1-2-3", (32, 48), JW.write(with_tables(s, _blocks(s, 13)), _blocks(s, 13)), "Adobe transform 0"))
    return out


# ---------------------------------------------------------------------------------------------------------------- long segments
def ramp_noise_224(seed: int = 0) -> np.ndarray:
    return content("ramp", 224, 224) // 2 + content("noise", 224, 224, seed=seed) // 8


@functools.lru_cache(maxsize=None)
def long_corpus():
    """[(Case, checks)] at 224 x 224, around STAGE_BYTES: two single segments far longer, and the ramp + noise frame of the other 224
    tests padded with zero bytes between its scan and EOI (bytes no MCU reads: Pillow's pixels stay) to a segment of exactly
    STAGE_BYTES - 1, STAGE_BYTES and STAGE_BYTES + 1 bytes; then one file of short segments per sampling, a marker per MCU row."""
    out, stage = [], stage_bytes()

    def add_file(name, h2v2, data, checks):
        out.append((Case(name, (224, 224), h2v2, data, pillow_decode(data)), checks))
    add_file("224x224-420-noise-q95-one-segment", 1, encode(content("noise", 224, 224), quality=95, subsampling=2),
             lambda f: [("bytes the decode consumes", f["consumed"][0], AtLeast(stage + 20000)), ("segments", f["segments"], 1)])
    add_file("224x224-444-noise-q100-one-segment", 0, encode(content("noise", 224, 224), quality=100, subsampling=0),
             lambda f: [("bytes the decode consumes", f["consumed"][0], AtLeast(6 * stage)), ("segments", f["segments"], 1)])
    data = encode(ramp_noise_224(), quality=95, subsampling=2)
    head, scan, tail = split_scan(data)
    assert tail[:2] == b"\xff\xd9" and len(scan) < stage - 1
    for d in (-1, 0, 1):
        add_file(f"224x224-420-padded-to-stage-bytes{d:+d}" if d else "224x224-420-padded-to-stage-bytes", 1, head + scan + bytes(stage + d - len(scan)) + tail,
                 lambda f, d=d: [("segment length", f["seg_len"][0], stage + d), ("bytes the decode leaves unread", f["seg_len"][0] - f["consumed"][0], AtLeast(1000))])
    add_file("224x224-420-a-marker-per-mcu-row", 1, encode(ramp_noise_224(1), quality=95, subsampling=2, restart_marker_rows=1),
             lambda f: [("segments", f["segments"], 14), ("a tenth of STAGE_BYTES less the longest segment", stage // 10 - max(f["seg_len"]), AtLeast(0))])
    add_file("224x224-444-a-marker-per-mcu-row", 0, encode(ramp_noise_224(2), quality=95, subsampling=0, restart_marker_rows=1),
             lambda f: [("segments", f["segments"], 28), ("a tenth of STAGE_BYTES less the longest segment", stage // 10 - max(f["seg_len"]), AtLeast(0))])
    return out


@functools.lru_cache(maxsize=None)
def long_corrupt_corpus():
    """[(name, file bytes)] from the 59 KB single segment, damaged far behind STAGE_BYTES, where only the wave mapping's unstaged path
    reads: intact, the scan truncated at 40 000 bytes, and one seeded bit flip beyond byte 33 000 (kept only if the parser accepts
    the file, as parse_tolerant() keeps them)."""
    data = next(c for c, _ in long_corpus() if c.name == "224x224-420-noise-q95-one-segment").data
    head, scan, tail = split_scan(data)
    assert len(scan) > 50000 and stage_bytes() < 33000
    bit = int(np.random.default_rng(224).integers(33000 * 8, len(scan) * 8))
    s = bytearray(scan)
    s[bit // 8] ^= 1 << (bit % 8)
    kept, _ = parse_tolerant([("intact", data), ("truncated-at-40000", head + scan[:40000] + tail), (f"flip-bit-{bit}", head + bytes(s) + tail)], 1, 224, 224)
    assert [n for n, _ in kept][:2] == ["intact", "truncated-at-40000"]
    return kept
