"""What the JPEG tests share (tests/test_jpeg_cpu.py, test_jpeg_core_cpu.py, test_jpeg_gpu.py, test_jpeg_store_gpu.py, ...): the matrix
of encoder settings, contents and shapes the decode is pinned on, Pillow as the reference, stores packed from such files, the corrupt
corpus, and the stand-alone host program around csrc/jpeg_core.h (compiled with g++ at test time) whose output is the truth for
malformed input.  Everything here is computed once per process and left unchanged."""
import functools
import io
import os
import struct
import subprocess

import numpy as np
import torch
from PIL import Image

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
