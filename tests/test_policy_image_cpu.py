"""The evaluator's frame pipeline on the host (include/vla_policy_image.h, csrc/jpeg_forward.h, input_stage.tf_lanczos3_spans): the
numpy rule of the JPEG round trip (tests/policy_image_rule_np.py) equals Pillow bit for bit - the quantised coefficients of Pillow's
file and the pixels of Pillow's decode - and the host's quantisation tables are the file's; vla_native.h does not name
these calls; a stand-alone program with its own main around csrc/jpeg_forward.h + csrc/jpeg_core.h, compiled with g++ plain and with
-fsanitize=address,undefined, reproduces the rule's coefficients and pixels (nothing is loaded into Python: the sanitizers see the
program alone); the lanczos3 rule keeps a flat image flat, has weight rows that sum to 1, returns the input at equal sizes and stays
within one grey level of Pillow's LANCZOS on a band-limited image; the flag parses, is refused when unknown and enters the fingerprint
only when it is not the default.  TensorFlow is not installed: its own last bits are not pinned here or anywhere."""
import dataclasses
import functools
import os
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_cases as JC
from tests import jpeg_rule_np as R
from tests import policy_image_rule_np as P
from vla_adapter_amd import input_stage as IS

QUALITIES = (30, 75, 95, 100)


def smooth_256() -> np.ndarray:
    g = np.random.default_rng(0)
    sm = np.kron(g.normal(128, 40, (16, 16, 3)), np.ones((16, 16, 1))) + g.normal(0, 6, (256, 256, 3))
    return np.clip(sm, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def images():
    """{name: uint8 [H, W, 3]}: jpeg_cases.SHAPES x CONTENTS and one 256 x 256 smooth image."""
    out = {f"{H}x{W}-{kind}": JC.content(kind, H, W) for H, W in JC.SHAPES for kind in JC.CONTENTS}
    out["256x256-smooth"] = smooth_256()
    return out


@functools.lru_cache(maxsize=None)
def rule_round_trip(name: str, quality: int):
    st = {}
    return P.jpeg_round_trip(images()[name], quality, st), st["quantised"]


# ---------------------------------------------------------------------------------------------------------------- the round trip
@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("name", sorted(images()))
def test_the_round_trip_rule_equals_pillow(name, quality):
    a = images()[name]
    data = JC.encode(a, quality=quality, subsampling=2)
    got, quantised = rule_round_trip(name, quality)
    st = {}
    R.decode(data, st)
    for c, (mine, theirs) in enumerate(zip(quantised, st["quantised"])):
        assert mine.shape == theirs.shape and np.array_equal(mine, theirs), f"component {c}: {(mine != theirs).sum()} quantised coefficients differ from the file's"
    want = JC.pillow_decode(data)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} values differ from Pillow's decode"


@pytest.mark.parametrize("quality", QUALITIES + (1, 10, 49, 50, 51, 90))
def test_the_hosts_quantisation_tables_are_the_files(quality):
    p = R.parse(JC.encode(JC.content("noise", 16, 16), quality=quality, subsampling=2))
    tabs = IS.jpeg_quant_tables(quality)
    assert tabs.dtype == np.uint16 and tabs.shape == (2, 64)
    for c, comp in enumerate(p["comps"]):
        assert np.array_equal(tabs[min(c, 1)][R.ZIGZAG], np.asarray(p["qt"][comp[3]])), f"component {c}"
    assert np.array_equal(tabs[0].reshape(8, 8), P.quant_table(P.LUMA, quality)) and np.array_equal(tabs[1].reshape(8, 8), P.quant_table(P.CHROMA, quality))
    for bad in (0, 101):
        with pytest.raises(ValueError):
            IS.jpeg_quant_tables(bad)


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_the_training_header_does_not_name_these_calls():
    from tests.abi_headers import header_text
    from vla_adapter_amd import native
    assert not [n for n in native.family("policy_image").protos if n in header_text("vla_native.h")], "the training ABI's header does not move for these calls"


def test_the_size_function_refuses_what_the_calls_refuse():
    from tests.abi_headers import load_library
    ws = load_library().vla_policy_image_workspace_bytes
    assert ws(2, 256, 256, 0, 0, 1) == 2 * (256 * 256 * 3 // 2) * 3, "int16 coefficients and u8 planes of a 4:2:0 image"
    for H, W in ((250, 256), (256, 8), (0, 16), (16, 4112)):
        assert ws(1, H, W, 0, 0, 1) == -1, (H, W)
    assert ws(3, 256, 256, 224, 224, 0) == 3 * 224 * 256 * 3 * 4, "the float32 intermediate of the vertical pass"
    assert ws(3, 48, 32, 48, 24, 0) == 0 and ws(3, 48, 32, 40, 32, 0) == 0, "one pass: no intermediate"
    assert ws(3, 224, 224, 224, 224, 0) == -1 and ws(0, 5, 7, 3, 4, 0) == -1 and ws(1, 5, 7, 0, 4, 0) == -1


def test_the_stage_b_kernels_are_stated_once():
    csrc = os.path.join(JC.ROOT, "vla_adapter_amd", "csrc")
    jpeg, policy = (open(os.path.join(csrc, n)).read() for n in ("jpeg.hip", "policy_image.hip"))
    assert jpeg.count("jpeg_idct_kernel(") == 1 and jpeg.count("hipLaunchKernelGGL(jpeg_idct_kernel") == 1 and jpeg.count("stage_b(st, coef") == 1
    assert "idct_islow" not in policy and "plane_pixel" not in policy and policy.count("stage_b(st, coef") == 1, "the inverse half is launched, not copied"


# ---------------------------------------------------------------------------------------------------------------- the host program
FORWARD_MAIN = r"""
// The JPEG round trip of csrc/jpeg_forward.h + csrc/jpeg_core.h on the host: argv[1] the input (int64 N, H, W; u16 qtab [2, 64] in
// natural order; u8 pixels [N, H, W, 3]), argv[2] the output (pixels u8 [N, H, W, 3], then the quantised coefficients int16
// [N, blocks, 64] in the decode's block layout).  Every buffer is a heap block of its exact size, so that a sanitizer sees an overrun.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "jpeg_forward.h"
using namespace vlajpeg;
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  long long h[3];
  if (fread(h, 8, 3, f) != 3) return 2;
  const long long N = h[0];
  const int H = (int)h[1], W = (int)h[2];
  if (N < 1 || H < 16 || W < 16 || H % 16 || W % 16) return 2;
  unsigned short* qtab = (unsigned short*)malloc(128 * sizeof(unsigned short));
  const size_t image = (size_t)H * W * 3;
  u8* in = (u8*)malloc(N * image);
  if (fread(qtab, 2, 128, f) != 128 || fread(in, 1, N * image, f) != N * image) return 2;
  fclose(f);
  const i64 nb = blocks_per_image(H, W, 1);
  short* coef = (short*)malloc(nb * 64 * sizeof(short));
  short* quant = (short*)malloc((size_t)N * nb * 64 * sizeof(short));
  u8* planes = (u8*)malloc(nb * 64);
  u8* out = (u8*)malloc(N * image);
  for (i64 img = 0; img < N; ++img) {
    memset(coef, 0x55, nb * 64 * sizeof(short));
    const int mw = W / 16;
    for (int mcu = 0; mcu < mcus_per_image(H, W, 1); ++mcu)
      forward_mcu(in + img * image + ((size_t)(mcu / mw) * 16 * W + (size_t)(mcu % mw) * 16) * 3, (i64)W * 3, mcu, H, W, qtab, coef, quant + img * nb * 64);
    for (i64 b = 0; b < nb; ++b) {
      i64 stride;
      const i64 o = plane_offset(b, H, W, 1, stride);
      idct_islow(coef + b * 64, planes + o, stride);
    }
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) plane_pixel(planes, H, W, 1, y, x, out + img * image + ((size_t)y * W + x) * 3);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(out, 1, N * image, o);
  fwrite(quant, sizeof(short), (size_t)N * nb * 64, o);
  fclose(o);
  free(qtab); free(in); free(coef); free(quant); free(planes); free(out);
  return 0;
}
"""


def build_forward(tmp, sanitize: bool = False) -> str:
    """g++ of the program above around csrc/jpeg_forward.h, as jpeg_cases.build_core builds its program -> the executable's path."""
    src, exe = os.path.join(str(tmp), "jpeg_forward_main.cpp"), os.path.join(str(tmp), "jpeg_forward_main" + ("_san" if sanitize else ""))
    open(src, "w").write(FORWARD_MAIN)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(JC.ROOT, "vla_adapter_amd", "csrc"), src, "-o", exe], check=True)
    return exe


def run_forward(exe: str, tmp, frames: np.ndarray, quality: int, name: str):
    """The host program on uint8 [N, H, W, 3] -> (pixels [N, H, W, 3], quantised int16 [N, blocks * 64]).  A sanitizer report ends the
    program with a non-zero status, which raises here with its text."""
    N, H, W, _ = frames.shape
    src, dst = os.path.join(str(tmp), name + ".bin"), os.path.join(str(tmp), name + ".out")
    with open(src, "wb") as f:
        f.write(struct.pack("<3q", N, H, W))
        f.write(IS.jpeg_quant_tables(quality).tobytes())
        f.write(np.ascontiguousarray(frames).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: the host round trip ended with status {r.returncode}:\n{r.stderr[-4000:]}"
    raw = open(dst, "rb").read()
    n = N * H * W * 3
    return np.frombuffer(raw[:n], dtype=np.uint8).reshape(N, H, W, 3), np.frombuffer(raw[n:], dtype=np.int16).reshape(N, -1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_forward(tmp_path_factory.mktemp("jpeg_forward"))


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return build_forward(tmp_path_factory.mktemp("jpeg_forward_san"), sanitize=True)


def rule_quantised_in_block_layout(quantised) -> np.ndarray:
    """[Y, Cb, Cr] in zigzag order -> int16 [blocks * 64] as block_index lays an image out: the Y blocks in raster order, Cb, Cr, natural order."""
    inv = np.argsort(R.ZIGZAG)
    return np.concatenate([q[..., inv].reshape(-1) for q in quantised]).astype(np.int16)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("quality", QUALITIES)
def test_the_host_program_reproduces_the_rule(exe, exe_san, tmp_path, quality, sanitized):
    by_shape = {}
    for name, a in images().items():
        by_shape.setdefault(a.shape, []).append(name)
    for shape, names in sorted(by_shape.items()):
        px, qc = run_forward(exe_san if sanitized else exe, tmp_path, np.stack([images()[n] for n in names]), quality, f"{shape[0]}x{shape[1]}-q{quality}")
        for i, n in enumerate(names):
            want, quantised = rule_round_trip(n, quality)
            assert np.array_equal(qc[i], rule_quantised_in_block_layout(quantised)), f"{n}: quantised coefficients differ from the rule's"
            assert np.array_equal(px[i], want), f"{n}: {(px[i] != want).sum()} of {want.size} values differ from the rule's"


# ---------------------------------------------------------------------------------------------------------------- the lanczos3 rule
@pytest.mark.parametrize("n_in, n_out, span", [(5, 3, 5), (16, 224, 7), (256, 224, 9)])
def test_spans_have_the_stated_length_and_equal_the_rules(n_in, n_out, span):
    starts, w = IS.tf_lanczos3_spans(n_in, n_out)
    r_starts, r_w, r_span = P.spans(n_in, n_out)
    assert r_span == span and w.shape == (n_out, span) and w.dtype == np.float32 and starts.dtype == np.int32 and starts.shape == (n_out,)
    assert np.array_equal(starts, r_starts) and np.array_equal(w, r_w), "the vectorised host function and the rule's loop agree bit for bit"
    assert (starts >= 0).all() and (starts <= n_in - 1).all()
    assert IS.tf_lanczos3_spans(n_in, n_out)[1] is w, "cached per (n_in, n_out)"


@pytest.mark.parametrize("n_in, n_out", [(5, 3), (7, 4), (16, 224), (32, 24), (48, 40), (256, 224), (256, 128), (256, 96), (256, 300), (256, 320), (224, 224)])
def test_every_weight_row_sums_to_one(n_in, n_out):
    _, w = IS.tf_lanczos3_spans(n_in, n_out)
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() < 1e-6


def test_flat_stays_flat():
    for v in (0, 77, 201, 255):
        a = np.full((256, 256, 3), v, np.uint8)
        for oh, ow in ((224, 224), (128, 96), (300, 320)):
            assert (P.tf_lanczos3_resize(a, oh, ow) == v).all(), (v, oh, ow)


def test_equal_sizes_return_the_input():
    a = JC.content("noise", 224, 224)
    assert np.array_equal(P.tf_lanczos3_resize(a, 224, 224), a)
    assert np.array_equal(P.tf_lanczos3_resize(a, 224, 224, skip_equal=False), a), "the passes TF would run at scale 1 change no byte either"


@pytest.mark.parametrize("oh, ow", [(224, 224), (128, 96), (300, 320)])
def test_the_rule_is_within_one_level_of_pillows_lanczos_on_a_band_limited_image(oh, ow):
    a = P.band_limited()
    assert 64 <= a.min() and a.max() <= 192
    got = P.tf_lanczos3_resize(a, oh, ow)
    pil = np.asarray(Image.fromarray(a).resize((ow, oh), Image.LANCZOS))
    d = np.abs(got.astype(int) - pil.astype(int))
    assert d.max() <= 1, f"max difference {d.max()}"
    other = P.tf_lanczos3_resize(a, oh, ow, order=("horizontal", "vertical"))
    assert np.abs(other.astype(int) - got.astype(int)).max() <= 1, "the unconfirmed pass order matters at ties only"


# ---------------------------------------------------------------------------------------------------------------- the flag, the refusals
def test_frame_resize_flag_parses_defaults_to_bicubic_and_is_fingerprinted_only_when_set():
    from vla_adapter_amd import finetune as F
    from vla_adapter_amd import train_state as TS
    f = {x.name: x for x in dataclasses.fields(F.FinetuneConfig)}["frame_resize"]
    assert f.default == "bicubic" and F.parse_args([]).frame_resize == "bicubic"
    on = F.parse_args(["--frame_resize", "lanczos3", "--use_proprio", "True"])
    assert on.frame_resize == "lanczos3"
    F.check_supported(on, on._explicit)
    bad = F.parse_args(["--frame_resize", "nearest", "--use_proprio", "True"])
    with pytest.raises(ValueError, match="frame_resize"):
        F.check_supported(bad, bad._explicit)
    base, lz = TS.fingerprint(F.parse_args([]), "adapter", 1, 1), TS.fingerprint(on, "adapter", 1, 1)
    assert "frame_resize" not in base, "a state file written before the flag existed still resumes"
    assert lz != base and lz["frame_resize"] == "lanczos3" and TS.fingerprint_differences(base, lz) == ["frame_resize: recorded '<absent>', now 'lanczos3'"]
    assert "frame_resize" not in TS.NOT_FINGERPRINTED


def test_the_stage_refuses_an_unknown_resize_mode():
    assert IS.RESIZE_MODES == ("bicubic", "lanczos3")
    with pytest.raises(ValueError, match="resize"):
        IS.GPUInputStage("cpu", resize="nearest")


def test_predict_actions_refuses_policy_resize_on_processed_pixels():
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    bare = object.__new__(OpenVLAForActionPrediction)         # (the call refuses before it touches the engine: tests/test_serve_cpu.py)
    with pytest.raises(ValueError, match="policy_resize"):
        bare.predict_actions([[5, 6]], pixel_values=torch.zeros(1, 3, 8, 8), proprio=[[0.0] * 8], policy_resize=True)
    import inspect
    sig = inspect.signature(OpenVLAForActionPrediction.predict_actions).parameters
    assert list(sig)[-1] == "policy_resize" and sig["policy_resize"].kind is inspect.Parameter.KEYWORD_ONLY and sig["policy_resize"].default is False
