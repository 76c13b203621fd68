"""CPU-side checks of the drop-in boundary of include/vla_native.h: version and descriptor layouts, the published stub, the routing
plans and the host-side refusals (no compute calls here: nothing needs a GPU).  tests/test_abi_families.py checks every header against
the binding and the library."""
import ctypes
import os

import pytest

from tests import abi_headers as H

ROOT = H.ROOT


@pytest.fixture(scope="module")
def lib():
    return H.load_library()


def test_library_reports_the_abi_version_and_the_descriptor_sizes(lib):
    from vla_adapter_amd import native
    assert lib.vla_version() == native.ABI_VERSION
    # the library reports the descriptor sizes it was compiled with; the binding refuses to load on a mismatch (native.load)
    for which, cls in enumerate((native.GemmDesc, native.AttnDesc, native.HeadAttnDesc, native.GemmTnDesc)):
        assert lib.vla_desc_size(which) == ctypes.sizeof(cls), cls.__name__
    assert lib.vla_desc_size(99) == -1


def test_integration_stub_is_current():
    """INTEGRATION.md's ctypes stub is generated from native.py (tools/gen_integration_stub.py); a descriptor that grew without
    the published stub following it would make a maintainer pass a short struct."""
    import subprocess
    import sys
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_integration_stub.py"), "--check"]).returncode == 0, \
        "INTEGRATION.md stub is stale: run tools/gen_integration_stub.py"


def test_gemm256_routing_predicate_is_host_arithmetic(lib):
    """vla_gemm256_extent_ok: the 256-row kernel's 32-bit per-lane byte offsets must cover every operand row: step
    shapes pass, operands of 4 GiB and more (token-CE lm_head at large batch, row groups with a huge stride) are routed away."""
    from vla_adapter_amd import native
    d = native.GemmDesc()
    d.M, d.N, d.K, d.lda, d.ldb, d.batch = 11264, 9728, 896, 896, 896, 1
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 1
    d.M, d.lda = 1 << 20, 4096                      # 1 M rows x 8 KiB = 8 GiB of A
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 0
    d.M, d.lda, d.N, d.ldb = 4096, 896, 151936, 16384      # B: 151936 rows x 32 KiB
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 0
    d.N, d.ldb = 151936, 896                        # the real lm_head: 272 MB
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 1
    d.a_group, d.a_group_stride, d.M = 256, 1 << 24, 256 * 200      # row groups 32 MiB apart, 200 of them: 6.4 GiB span
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 0
    d.fp8 = 1                                       # one byte per element halves every extent
    d.a_group_stride = 1 << 23
    assert lib.vla_gemm256_extent_ok(ctypes.byref(d)) == 1



def _nt(M, N, K, **kw):
    """A descriptor for the routing plan (host arithmetic only: the pointers are never dereferenced, 16-B aligned dummies)."""
    from vla_adapter_amd import native
    d = native.GemmDesc()
    d.A, d.B, d.C = 1 << 20, 1 << 21, 1 << 22
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch = M, N, K, K, K, N, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _nt_plan(lib, d, latency=0, cus=256):
    s = ctypes.c_int(-1)
    return lib.vla_gemm_nt_plan(ctypes.byref(d), latency, cus, ctypes.byref(s)), s.value


ROPE64 = dict(rope_mode=1, rope_dh=64, rope_T=256, rope_cols=1024, rope_cos=1 << 23, rope_sin=1 << 24)
EXT = dict(A2=1 << 25, B2=1 << 26, K2=64, lda2=64, ldb2=64)

# (descriptor, latency hint, expected (kernel, K slices)) at 256 CUs: what route() / choose_tile() / the skinny predicate and
# ops.gemm_nt's split-K policy picked before ABI 8 merged them into the plan.  Slices: the automatic count when split_k is left at 0.
NT_TABLE = [
    # tall-skinny N = 64, M >= 1024: (tile rows + columns) x rounds is least for 32 x 32 (64 rows, one round)
    (_nt(4096, 64, 896), 0, ("NT_SKINNY", 2, 1)),
    # <= 512 rows under the hint: 16 x 16 tiles (56 workgroups, 32 operand rows)
    (_nt(8, 896, 896), 1, ("NT_SKINNY", 0, 1)),
    # ... and without it the 128-row square tile
    (_nt(8, 896, 896), 0, ("NT_128x128", 0, 1)),
    # skinny cost cap: the best tile (64 x 64) pulls 128 > 96 operand rows -> gemm.hip, 96 64-row workgroups <= 256 CUs: six-stage ring
    (_nt(512, 1536, 896), 1, ("NT_64x128_S6", 0, 1)),
    # hint, 288 64-row workgroups > 256 CUs >= 144 128-row ones: four-stage ring
    (_nt(1536, 1536, 1024), 1, ("NT_128x128_S4", 0, 1)),
    # long K, 112 square tiles <= 128: the narrow tile; automatic split-K: 4 even slices (8 would exceed two workgroups per CU)
    (_nt(2048, 896, 9728), 0, ("NT_128x64", 0, 4)),
    # the same with those 4 slices: 448 tiles, no longer narrow
    (_nt(2048, 896, 9728, split_k=4), 0, ("NT_128x128", 0, 4)),
    # 224 square tiles fit one round of two per CU: rounds model 4 vs 2.3 -> 128x128
    (_nt(4096, 896, 896), 0, ("NT_128x128", 0, 1)),
    # LLM down: 176 big tiles (4) against 616 square ones (2 rounds: 4.6) -> 256
    (_nt(11264, 896, 4864), 0, ("NT_256", 0, 1)),
    # SwiGLU forward (gate/up): 256
    (_nt(11264, 9728, 896, act=4, C2=1 << 27, ldc2=4864), 0, ("NT_256", 0, 1)),
    # SwiGLU backward never chooses 256 on its own
    (_nt(11264, 4864, 896, act=5, R=1 << 27, ldr=9728, ldc=9728), 0, ("NT_128x128", 0, 1)),
    # rotate_half at head dim 64 with >= 192 big tiles (whole-batch q|k|v): 256
    (_nt(11264, 1152, 896, **ROPE64), 0, ("NT_256", 0, 1)),
    # ... the half-batch launch (110 big tiles < 192) stays on the 128-row kernel
    (_nt(5632, 1152, 896, **ROPE64), 0, ("NT_128x128", 0, 1)),
    # ... head dim 128: the 256-row kernel's column map is built on 64-wide heads
    (_nt(11264, 1152, 896, **dict(ROPE64, rope_dh=128, rope_cols=1152)), 0, ("NT_128x128", 0, 1)),
    # interleaved RoPE on 256 only with the plain epilogue: K|V projection 256; with a residual 128x128
    (_nt(11264, 1152, 896, rope_mode=2, rope_dh=64, rope_T=8, rope_cols=1152, rope_cos=1 << 23, rope_sin=1 << 24), 0, ("NT_256", 0, 1)),
    (_nt(11264, 1152, 896, rope_mode=2, rope_dh=64, rope_T=8, rope_cols=1152, rope_cos=1 << 23, rope_sin=1 << 24, R=1 << 27, ldr=1152),
     0, ("NT_128x128", 0, 1)),
    # extent fallback: B rows 32 KiB apart over 151936 rows pass 4 GiB -> the 64-bit-pointer 128-row kernel
    (_nt(4096, 151936, 896, ldb=16384), 0, ("NT_128x128", 0, 1)),
    # fp8: 256 only for big squares; the LLM down product stays on the 128-row kernel
    (_nt(8192, 8192, 8192, fp8=1, a_scale=1 << 23, b_scale=1 << 24), 0, ("NT_256", 0, 1)),
    (_nt(11264, 896, 4864, fp8=1, a_scale=1 << 23, b_scale=1 << 24), 0, ("NT_128x128", 0, 1)),
    # K extension on 256: the plain product's rounds model over K + K2; fallbacks: row groups on A, rotate_half under 192 tiles, fp8
    (_nt(11264, 896, 4864, **EXT), 0, ("NT_256", 0, 1)),
    (_nt(11264, 896, 4864, a_group=11264, a_group_stride=11264 * 4864, **EXT), 0, ("NT_128x128", 0, 1)),
    (_nt(5632, 1152, 896, **ROPE64, **EXT), 0, ("NT_128x128", 0, 1)),
    (_nt(11264, 896, 4864, fp8=1, a_scale=1 << 23, b_scale=1 << 24, **EXT), 0, ("NT_128x128", 0, 1)),
    # hint, ViT fc2 256 x 1152 x 4352 (unsplit: 18 square tiles, K >= 4096 -> narrow): uneven automatic split-K, 256 // 36 = 7 slices
    # of 10 K-tiles, and with them 252 64-row workgroups on the six-stage ring
    (_nt(256, 1152, 4352), 1, ("NT_128x64", 0, 7)),
    (_nt(256, 1152, 4352, split_k=7), 1, ("NT_64x128_S6", 0, 7)),
    # ... without the hint: 4 even slices (8 do not divide K)
    (_nt(256, 1152, 4352), 0, ("NT_128x64", 0, 4)),
    # explicit slices that do not divide K: ceil(68 / 16) = 5 K-tiles each, 14 slices run
    (_nt(256, 1152, 4352, split_k=16), 0, ("NT_128x128", 0, 14)),
    # no automatic split: K < 2048, batched, residual rows modulo, interleaved RoPE
    (_nt(256, 1152, 1024), 0, ("NT_128x128", 0, 1)),
    (_nt(256, 1152, 4352, batch=2), 0, ("NT_128x64", 0, 1)),
    (_nt(256, 1152, 4352, res_mod=256, R=1 << 27, ldr=1152), 0, ("NT_128x64", 0, 1)),
]


@pytest.mark.parametrize("row", range(len(NT_TABLE)))
def test_gemm_nt_plan_table(lib, row):
    """vla_gemm_nt_plan at 256 CUs reproduces the routing of every branch (one row per rule, see NT_TABLE)."""
    from vla_adapter_amd import native
    d, lat, (name, tile, split) = NT_TABLE[row]
    assert _nt_plan(lib, d, lat) == (getattr(native, "KERNEL_" + name) + tile, split)


def test_gemm_nt_plan_follows_cus(lib):
    """Split counts and the deep-ring thresholds scale with the CU count (before ABI 8 ops.gemm_nt assumed 256)."""
    from vla_adapter_amd import native as n
    fc2 = _nt(256, 1152, 4352)                       # 36 64-row workgroups
    assert _nt_plan(lib, fc2, 1, 128)[1] == 3 and _nt_plan(lib, fc2, 1, 304)[1] == 8
    sq = _nt(1536, 1536, 1024)                       # 144 128-row / 288 64-row workgroups
    assert _nt_plan(lib, sq, 1, 304)[0] == n.KERNEL_NT_64x128_S6
    assert _nt_plan(lib, sq, 1, 128)[0] == n.KERNEL_NT_128x128
    dx = _nt(2048, 896, 9728)                        # 112 square tiles
    assert _nt_plan(lib, dx, 0, 128)[1] == 2 and _nt_plan(lib, dx, 0, 304)[1] == 4 and _nt_plan(lib, dx, 0, 64)[1] == 1
    assert lib.vla_gemm_nt_plan(ctypes.byref(_nt(0, 64, 64)), 0, 256, None) == -1


def test_gemm_nt_plan_overrides(lib, monkeypatch):
    from vla_adapter_amd import native as n
    bwd = _nt(11264, 4864, 896, act=5, R=1 << 27, ldr=9728, ldc=9728)
    monkeypatch.setenv("VLA_GEMM_TILE", "6")
    assert _nt_plan(lib, bwd)[0] == n.KERNEL_NT_256
    # forced 256 refused by the extent: the square tile, never the narrow one
    assert _nt_plan(lib, _nt(2048, 896, 9728, ldb=1 << 22))[0] == n.KERNEL_NT_128x128
    assert _nt_plan(lib, _nt(4096, 64, 896))[0] == n.KERNEL_NT_256         # (any forced tile keeps gemm_skinny.hip out)
    monkeypatch.setenv("VLA_GEMM_TILE", "3")
    assert _nt_plan(lib, _nt(4096, 896, 896))[0] == n.KERNEL_NT_128x64
    monkeypatch.setenv("VLA_GEMM_TILE", "2")
    assert _nt_plan(lib, _nt(2048, 896, 9728))[0] == n.KERNEL_NT_128x128
    monkeypatch.delenv("VLA_GEMM_TILE")
    monkeypatch.setenv("VLA_NO_SKINNY", "1")
    assert _nt_plan(lib, _nt(4096, 64, 896))[0] == n.KERNEL_NT_128x128
    monkeypatch.delenv("VLA_NO_SKINNY")
    monkeypatch.setenv("VLA_NO_SMALL_ROWS", "1")
    assert _nt_plan(lib, _nt(8, 896, 896), 1)[0] == n.KERNEL_NT_64x128_S6
    assert _nt_plan(lib, _nt(4096, 64, 896))[0] == n.KERNEL_NT_SKINNY + 2
    monkeypatch.setenv("VLA_NO_SPLITK", "1")
    assert _nt_plan(lib, _nt(2048, 896, 9728))[1] == 1


def _tn(M, N1, N2, **kw):
    from vla_adapter_amd import native
    d = native.GemmTnDesc()
    d.A, d.B, d.C = 1 << 20, 1 << 21, 1 << 22
    d.M, d.N1, d.N2, d.lda, d.ldb, d.ldc, d.batch = M, N1, N2, N1, N2, N2, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _tn_plan(lib, d, cus=256):
    s = ctypes.c_int(-1)
    return lib.vla_gemm_tn_plan(ctypes.byref(d), cus, ctypes.byref(s)), s.value


def test_gemm_tn_plan(lib, monkeypatch):
    """vla_gemm_tn_plan: ops.gemm_tn's former split (min(16, 2 CUs / tiles, M / 256) for launches of at most half a CU count of
    128-tiles, M >= 1024; no empty slice) and gemm_tn.hip's 256-tile rule (>= 128 eligible big tiles per launch)."""
    from vla_adapter_amd import native as n
    T128, T256 = n.KERNEL_TN_128, n.KERNEL_TN_256
    assert _tn_plan(lib, _tn(11264, 896, 64)) == (T128, 16)          # LoRA pair: 7 tiles, 16 slices of 704 rows
    assert _tn_plan(lib, _tn(4096, 896, 896)) == (T128, 10)          # 49 tiles: 512 // 49 = 10 slices
    assert _tn_plan(lib, _tn(4096, 896, 896), 128) == (T128, 5)      # 256 // 49
    assert _tn_plan(lib, _tn(4096, 896, 896), 64) == (T128, 1)       # 98 tiles > 64 / 2
    assert _tn_plan(lib, _tn(1000, 896, 896)) == (T128, 1)           # M < 1024
    assert _tn_plan(lib, _tn(600, 896, 896, split=16)) == (T128, 10)  # 64-row slices: 10 of them hold 600 rows
    assert _tn_plan(lib, _tn(11264, 896, 4864)) == (T128, 1)         # down: 76 big tiles < 128
    assert _tn_plan(lib, _tn(11264, 9728, 896)) == (T256, 1)         # gate/up: 152
    assert _tn_plan(lib, _tn(11264, 896, 4864, batch=2)) == (T256, 1)
    monkeypatch.setenv("VLA_TN_TILE", "256")
    assert _tn_plan(lib, _tn(64, 64, 64))[0] == T256
    assert _tn_plan(lib, _tn(4096, 896, 896, split=4)) == (T128, 4)  # a split always runs on the 128-tile kernel
    monkeypatch.setenv("VLA_TN_TILE", "128")
    assert _tn_plan(lib, _tn(11264, 9728, 896))[0] == T128


def test_latency_hint_is_per_thread(lib):
    import threading
    seen = []
    prev = lib.vla_gemm_latency_hint(1)
    try:
        t = threading.Thread(target=lambda: seen.append(lib.vla_gemm_latency_hint(-1)))
        t.start()
        t.join()
        assert lib.vla_gemm_latency_hint(-1) == 1 and seen == [0]
        d = _nt(8, 896, 896)
        assert _nt_plan(lib, d, -1)[0] == 0                          # latency < 0: this thread's hint (skinny 16 x 16)
    finally:
        lib.vla_gemm_latency_hint(prev)


def test_descriptor_layouts_match_header(lib, tmp_path):
    """ctypes mirrors of the descriptor structs must match what a C compiler makes of include/vla_native.h:
    same size and the same offset for every field (checked by compiling a probe with gcc)."""
    import subprocess
    from vla_adapter_amd import native
    structs = {"vla_gemm_desc": native.GemmDesc, "vla_attn_desc": native.AttnDesc, "vla_head_attn_desc": native.HeadAttnDesc,
               "vla_gemm_tn_desc": native.GemmTnDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "vla_native.h")}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_argument_validation_without_gpu(lib):
    """Host-side validation rejects bad descriptors before any launch (safe on a CPU-only box)."""
    from vla_adapter_amd import native
    d = native.GemmDesc()
    assert lib.vla_gemm_bf16_nt(None, ctypes.byref(d)) == -1
    assert b"null" in lib.vla_last_error()
    d.A = d.B = d.C = 4096
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.batch = 8, 8, 100, 104, 104, 8, 1
    assert lib.vla_gemm_bf16_nt(None, ctypes.byref(d)) == -1
    assert b"multiple of 64" in lib.vla_last_error()
    t = native.GemmTnDesc()
    assert lib.vla_gemm_bf16_tn(None, ctypes.byref(t)) == -1 and b"null" in lib.vla_last_error()
    t.A = t.B = t.C = 4096
    t.M, t.N1, t.N2, t.lda, t.ldb, t.ldc, t.batch = 100, 12, 8, 16, 8, 8, 1
    assert lib.vla_gemm_bf16_tn(None, ctypes.byref(t)) == -1 and b"multiples of 8" in lib.vla_last_error()
    t.N1, t.a_group, t.a_group_stride = 16, 100, 4096
    assert lib.vla_gemm_bf16_tn(None, ctypes.byref(t)) == -1 and b"multiples of 64 rows" in lib.vla_last_error()


def test_missing_library_fails_loudly(monkeypatch):
    from vla_adapter_amd import native
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "LIB_PATH", "/nonexistent/libvla_native.so")
    with pytest.raises(native.NativeLibraryMissing):
        native.load()
