"""The JPEG encoder on the host (include/vla_jpeg_encode.h, csrc/jpeg_encode_core.h, jpeg_store.encode_tables): the numpy rule
(tests/jpeg_encode_rule_np.py) equals the file Pillow saves, whole, on the corpus; the corpus reaches the hard cases, asserted from the
rule's own symbol statistics as conditions on the inputs; a stand-alone program with its own main around csrc/jpeg_encode_core.h +
csrc/jpeg_forward.h, compiled with g++ plain and with -fsanitize=address,undefined, writes Pillow's bytes (nothing is loaded into
Python: the sanitizers see the program alone); the size function refuses what the calls refuse; the flag parses, is refused outside
0 .. 100 and without an episode source, and enters the fingerprint only when it is set; the pack tool's --device parses."""
import dataclasses
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_encode_rule_np as E
from vla_adapter_amd import input_stage as IS

CASES = [(name, q, r) for name in sorted(E.corpus()) for q in E.QUALITIES for r in (1, 2)]


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name, quality, restart_rows", CASES, ids=[f"{n}-q{q}-r{r}" for n, q, r in CASES])
def test_the_rule_equals_pillows_file(name, quality, restart_rows):
    a = E.corpus()[name]
    mine, theirs = E.encode(a, quality, restart_rows), E.pillow(a, quality, restart_rows)
    assert len(mine) == len(theirs), f"{len(mine)} bytes, Pillow writes {len(theirs)}"
    assert mine == theirs, f"first difference at byte {next(i for i, (x, y) in enumerate(zip(mine, theirs)) if x != y)}"


def test_the_header_is_615_bytes_up_to_sos_and_lists_the_segments_in_pillows_order():
    data = E.encode(E.corpus()["gradient-64x32"], 95, 2)
    assert data.index(b"\xff\xda") == 615 and data[:615] == E.pillow(E.corpus()["gradient-64x32"], 95, 2)[:615]
    markers, i = [], 2
    while data[i + 1] != 0xDA:
        markers.append((data[i + 1], data[i + 4] if data[i + 1] == 0xC4 else None))
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    assert markers == [(0xE0, None), (0xDB, None), (0xDB, None), (0xC0, None), (0xC4, 0x00), (0xC4, 0x10), (0xC4, 0x01), (0xC4, 0x11), (0xDD, None)]


def test_the_corpus_reaches_the_hard_cases():
    """Conditions on the inputs, from the rule's own symbols: not tolerances."""
    C = E.corpus()
    assert E.statistics(C["checkerboard-32x48"], 100)["max_dc_category"] == 11, "a DC difference of the largest category"
    assert E.statistics(C["dots-32x48"], 1)["zrl"] > 0 and E.statistics(C["noise-32x48"], 1)["zrl"] > 0, "ZRL"
    st = E.statistics(C["noise-160x16"], 100)
    assert st["blocks_without_eob"] == st["blocks"] == 60, "a frame in which no block has an EOB: every one ends on coefficient 63"
    assert st["mcu_rows"] >= 10 and st["intervals"] >= 10, "ten intervals: the restart markers wrap from RST7 to RST0"
    data = E.encode(C["noise-160x16"], 100, 1)
    assert b"\xff\xd7" in data and data.count(b"\xff\xd0") >= 2
    for name in C:
        if name.startswith("noise"):
            assert E.statistics(C[name], 95)["stuffed"] >= 1, f"{name}: a stuffed FF 00 pair"
    assert E.statistics(C["noise-224x224"], 100)["max_mcu_bytes"] <= 6 * 2 * 216, "inside the bound of csrc/jpeg_encode_core.h: 216 bytes a block, doubled"


def test_mixed_frames_hold_one_frame_of_every_kind():
    fr = E.mixed_frames(5, 16, 16)
    assert fr.shape == (5, 16, 16, 3) and fr.dtype == np.uint8 and len({f.tobytes() for f in fr}) == 5


# ---------------------------------------------------------------------------------------------------------------- the host program
ENCODE_MAIN = r"""
// The encoder of csrc/jpeg_forward.h + csrc/jpeg_encode_core.h on the host: argv[1] the input (int64 N, H, W, restart_rows; u16 qtab
// [2, 64] in natural order; u8 pixels [N, H, W, 3]), argv[2] the output (int64 size of every file, then the files back to back).  Every
// buffer is a heap block of its exact size - the file's buffer of the size the first, counting pass reported - so that a sanitizer sees
// an overrun.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "jpeg_forward.h"
#include "jpeg_encode_core.h"
using namespace vlajpeg;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long h[4];
  if (fread(h, 8, 4, f) != 4) return 2;
  const long long N = h[0];
  const int H = (int)h[1], W = (int)h[2], R = (int)h[3];
  if (N < 1 || !encode_shape_ok(H, W, R)) return 2;
  unsigned short* qtab = (unsigned short*)malloc(128 * sizeof(unsigned short));
  const size_t image = (size_t)H * W * 3;
  u8* in = (u8*)malloc(N * image);
  if (fread(qtab, 2, 128, f) != 128 || fread(in, 1, N * image, f) != N * image) return 2;
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const i64 nb = blocks_per_image(H, W, 1);
  short* coef = (short*)malloc(nb * 64 * sizeof(short));
  short* quant = (short*)malloc(nb * 64 * sizeof(short));
  const i64 worst = HEADER_BYTES + 2 + nb * (2 * MAX_BLOCK_BYTES) + 4 * (i64)intervals_per_image(H, R);
  long long* sizes = (long long*)malloc(N * sizeof(long long));
  u8** files = (u8**)malloc(N * sizeof(u8*));
  for (i64 img = 0; img < N; ++img) {
    const int mw = W / 16;
    for (int mcu = 0; mcu < mcus_per_image(H, W, 1); ++mcu)
      forward_mcu(in + img * image + ((size_t)(mcu / mw) * 16 * W + (size_t)(mcu % mw) * 16) * 3, (i64)W * 3, mcu, H, W, qtab, coef, quant);
    u8* big = (u8*)malloc(worst);
    const i64 n = encode_image_serial(quant, H, W, qtab, R, big, worst);
    free(big);
    if (n < 0) return 3;
    files[img] = (u8*)malloc(n);                          // the exact size: the second pass must end on its last byte
    if (encode_image_serial(quant, H, W, qtab, R, files[img], n) != n) return 4;
    if (n > 1 && encode_image_serial(quant, H, W, qtab, R, files[img], n - 1) != -1) return 5;      // (one byte short: refused, not overrun)
    if (encode_image_serial(quant, H, W, qtab, R, files[img], n) != n) return 4;
    sizes[img] = n;
  }
  fwrite(sizes, sizeof(long long), N, o);
  for (i64 img = 0; img < N; ++img) {
    fwrite(files[img], 1, sizes[img], o);
    free(files[img]);
  }
  fclose(o);
  free(qtab); free(in); free(coef); free(quant); free(sizes); free(files);
  return 0;
}
"""


def build_encode(tmp, sanitize: bool = False) -> str:
    src, exe = os.path.join(str(tmp), "jpeg_encode_main.cpp"), os.path.join(str(tmp), "jpeg_encode_main" + ("_san" if sanitize else ""))
    open(src, "w").write(ENCODE_MAIN)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(JC.ROOT, "vla_adapter_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run_encode(exe: str, tmp, frames: np.ndarray, quality: int, restart_rows: int, name: str):
    """The host program on uint8 [N, H, W, 3] -> [file bytes].  A sanitizer report ends the program with a non-zero status."""
    N, H, W, _ = frames.shape
    src, dst = os.path.join(str(tmp), name + ".bin"), os.path.join(str(tmp), name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<4q", N, H, W, restart_rows))
        f.write(IS.jpeg_quant_tables(quality).tobytes())
        f.write(np.ascontiguousarray(frames).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: the host encoder ended with status {r.returncode}:\n{r.stderr[-4000:]}"
    raw = open(dst, "rb").read()
    sizes = struct.unpack(f"<{N}q", raw[:8 * N])
    offs = np.concatenate([[8 * N], 8 * N + np.cumsum(sizes)])
    assert offs[-1] == len(raw)
    return [raw[offs[i]:offs[i + 1]] for i in range(N)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_encode(tmp_path_factory.mktemp("jpeg_encode"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build_encode(tmp_path_factory.mktemp("jpeg_encode_san"), sanitize=True)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("restart_rows", [1, 2])
@pytest.mark.parametrize("quality", E.QUALITIES)
def test_the_host_program_writes_pillows_bytes(exe, exe_san, tmp_path, quality, restart_rows, sanitized):
    by_shape = {}
    for name, a in E.corpus().items():
        by_shape.setdefault(a.shape, []).append(name)
    for shape, names in sorted(by_shape.items()):
        files = run_encode(exe_san if sanitized else exe, tmp_path, np.stack([E.corpus()[n] for n in names]), quality, restart_rows,
                           f"{shape[0]}x{shape[1]}-q{quality}-r{restart_rows}")
        for n, got in zip(names, files):
            assert got == E.pillow(E.corpus()[n], quality, restart_rows), f"{n}: the core's file differs from Pillow's"


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_the_training_header_does_not_name_these_calls():
    from tests.abi_headers import header_text
    from vla_adapter_amd import native
    assert not [n for n in native.family("jpeg_encode").protos if n in header_text("vla_native.h")], "the training ABI's header does not move for these calls"


def test_the_size_function_refuses_what_the_calls_refuse():
    from tests.abi_headers import load_library
    ws = load_library().vla_jpeg_encode_workspace_bytes
    assert ws(2, 256, 256, 1) == 2 * 256 * 256 * 3 + 2 * 16 * 12, "int16 coefficients, and an int64 offset and an int32 length per interval"
    assert ws(1, 224, 224, 3) == 224 * 224 * 3 + 5 * 12, "a last interval shorter than the others"
    for H, W, r in ((250, 256, 1), (256, 8, 1), (0, 16, 1), (16, 4112, 1), (32, 32, 0), (32, 32, -1), (4096, 4096, 256)):
        assert ws(1, H, W, r) == -1, (H, W, r)
    assert ws(0, 32, 32, 1) == -1 and ws((1 << 20) + 1, 32, 32, 1) == -1


# ---------------------------------------------------------------------------------------------------------------- the flag, the tool
def test_the_flag_parses_is_refused_out_of_range_and_is_fingerprinted_only_when_set():
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd import train_state as TS
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["episode_jpeg_quality"]
    assert f.default == 0 and F.parse_args([]).episode_jpeg_quality == 0
    on = F.parse_args(["--episode_jpeg_quality", "95", "--episode_file", "raw.pt", "--use_proprio", "True", "--max_seq_len", "64"])
    assert on.episode_jpeg_quality == 95 and isinstance(on.episode_jpeg_quality, int)
    F.check_supported(on, on._explicit)
    mix = F.parse_args(["--episode_jpeg_quality", "50", "--episode_mix", "a.pt=1.0,b.pt=0.5", "--use_proprio", "True", "--max_seq_len", "64"])
    F.check_supported(mix, mix._explicit)
    for bad in ("-1", "101"):
        cfg = F.parse_args(["--episode_jpeg_quality", bad, "--episode_file", "raw.pt", "--use_proprio", "True", "--max_seq_len", "64"])
        with pytest.raises(ValueError, match="episode_jpeg_quality"):
            F.check_supported(cfg, cfg._explicit)
    lone = F.parse_args(["--episode_jpeg_quality", "95", "--use_proprio", "True", "--max_seq_len", "64"])
    with pytest.raises(ValueError, match="episode_jpeg_quality"):
        F.check_supported(lone, lone._explicit)
    off = F.parse_args(["--episode_file", "raw.pt", "--use_proprio", "True", "--max_seq_len", "64"])
    base, fp = TS.fingerprint(off, "adapter", 1, 1), TS.fingerprint(on, "adapter", 1, 1)
    assert "episode_jpeg_quality" not in base, "a state file written before the flag existed still resumes"
    assert base == TS.fingerprint(F.parse_args(["--episode_file", "raw.pt", "--episode_jpeg_quality", "0", "--use_proprio", "True", "--max_seq_len", "64"]), "adapter", 1, 1)
    assert fp["episode_jpeg_quality"] == 95 and TS.fingerprint_differences(base, fp) == ["episode_jpeg_quality: recorded '<absent>', now 95"]
    assert "episode_jpeg_quality" not in TS.NOT_FINGERPRINTED


def raw_tables(H=32, W=48, T=3, n_img=1):
    return dict(
        frames_u8=torch.from_numpy(E.mixed_frames(T * n_img, H, W).reshape(T, n_img, H, W, 3)), actions_raw=torch.zeros(T, 7), proprio_raw=torch.zeros(T, 8),
        episode_off=torch.tensor([0, T]), prompt_flat=torch.tensor([5, 6]), prompt_off=torch.tensor([0, 2], dtype=torch.int32), dataset_name="corpus")


def test_encode_tables_refuses_before_it_touches_a_device():
    from vla_adapter_amd import jpeg_store as JS
    for q in (0, 101, True, 95.0):
        with pytest.raises(ValueError, match="jpeg_quality"):
            JS.encode_tables(raw_tables(), "cpu", q)
    with pytest.raises(ValueError, match="restart_rows"):
        JS.encode_tables(raw_tables(), "cpu", 95, restart_rows=0)
    with pytest.raises(ValueError, match=r"shard-7.*24 x 48.*multiples of 16"):
        JS.encode_tables(raw_tables(H=24), "cpu", 95, where="shard-7")
    packed = JC.episode_dict([E.pillow(a, 95) for a in E.mixed_frames(3, 32, 48)], 1, 32, 48, [3])
    assert JS.encode_tables(packed, "cpu", 95) is packed, "a dict already in the JPEG form comes back as it is"


def test_the_loaders_name_the_dataset_whose_frames_cannot_be_coded(tmp_path):
    from vla_adapter_amd import episodes as EP
    path = tmp_path / "odd_sides.pt"
    torch.save(raw_tables(H=24), str(path))
    with pytest.raises(ValueError, match=r"odd_sides\.pt \(dataset 'corpus'\): frames of 24 x 48.*multiples of 16"):
        EP.load_tables(str(path), "cpu", jpeg_quality=95)
    assert "frames_u8" in EP.load_tables(str(path), "cpu"), "without the argument the tables are what the file holds"


def test_the_pack_tools_device_argument_parses():
    sys.path.insert(0, os.path.join(JC.ROOT, "tools"))
    try:
        import pack_episodes_jpeg as T
    finally:
        sys.path.pop(0)
    ap = T.parser()
    assert ap.parse_args(["a.pt", "b.pt"]).device == "cpu" and ap.parse_args(["a.pt", "b.pt", "--device", "cuda"]).device == "cuda"
    d = ap.parse_args(["a.pt", "b.pt"])
    assert (d.quality, d.subsampling, d.restart_rows) == (95, "4:2:0", 1), "the Pillow path's defaults stay"
    with pytest.raises(ValueError, match="4:2:0"):
        T.pack_on_device(raw_tables(), "cuda", subsampling="4:4:4")
    a = raw_tables()
    out = T.pack(a, 95, "4:2:0", 1)
    files = [E.encode(f, 95, 1) for f in a["frames_u8"].reshape(-1, 32, 48, 3).numpy()]
    assert bytes(out["frames_jpeg"].numpy()) == b"".join(files), "the rule writes the store the tool's Pillow path writes"
