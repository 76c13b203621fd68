"""The memory contract of every entry point of include/vla_native.h, on poisoned, strided operands (tests/arena.py).

Every case runs its entry point twice:
  1. on compact, separately allocated operands;
  2. with every device operand a view inside a poisoned arena - at the minimum alignment the entry point's own host check accepts,
     with a row stride larger than the width and a batch / group stride that is no multiple of the row stride -
and requires that the outputs of (2) equal those of (1) BIT FOR BIT, that no input arena changed, and that no output arena changed
outside its declared extent (include/vla_native.h says what that is).  Outputs start as poison in both runs, so an element the entry
point is documented to leave alone (gather index -2, dead c_live rows) compares equal too, and a read past a declared extent meets a
NaN (or an in-range index that changes the result) instead of the zeros or finite garbage a fresh allocation holds.

Where a view legitimately runs another arithmetic (the one-thread-per-column sums taken when an operand is not 16-B aligned: another
fp32 summation order than the fixed-order workgroup reduction) the view run is compared with the fp64 contract the kernel's own test
uses (tests/test_kernel_accuracy_gpu.py), never looser; those cases say so.

No case hands an entry point a pointer it should refuse, none places a view at the end of an allocation, and the three overrun cases
at the end (one row, eight columns too many) stay inside the arenas' margins.

COVERED names the entry points the cases exercise (filled by @case), EXEMPT those without a device footprint;
tests/test_abi_families.py checks on the CPU that the two tables cover the family's signature table.
"""
import ctypes as C
import math

import pytest
import torch

from tests import accuracy as A
from tests.arena import Arena, assert_bits_equal, default_poison
from vla_adapter_amd import native as N
from vla_adapter_amd import ops
from vla_adapter_amd.scratch import ARENA

DEV = "cuda"
BF, F32, U8, I32, I64, F64 = torch.bfloat16, torch.float32, torch.uint8, torch.int32, torch.int64, torch.float64

COVERED = {}
EXEMPT = {
    "vla_version": "host only: returns a constant",
    "vla_desc_size": "host only: sizeof of a descriptor",
    "vla_gemm256_extent_ok": "host arithmetic on a descriptor, no device buffer",
    "vla_gemm_nt_plan": "host routing, no device buffer (every NT case asserts its kernel id through it)",
    "vla_gemm_tn_plan": "host routing, no device buffer (the TN cases assert their tile through it)",
    "vla_gemm_latency_hint": "host only: a per-thread flag",
    "vla_augment_slab_floats": "host only: size arithmetic",
    "vla_grad_sumsq_slots": "host only: size arithmetic",
}


def case_for(covered):
    """-> the decorator case(*symbols) of one module: it marks a GPU case and records in `covered` the entry points it exercises."""
    def case(*symbols):
        def deco(fn):
            for s in symbols:
                covered.setdefault(s, []).append(fn.__name__)
            return pytest.mark.gpu(fn)
        return deco
    return case


case = case_for(COVERED)


# ---------------------------------------------------------------------------------------------------------------- the procedure
def gen(*shape, seed=0, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ld_of(cols, mult=8):
    """The smallest row stride larger than the width that keeps `mult`-element rows."""
    return (cols // mult + 1) * mult


def st2(rows, cols, mult=8):
    return (ld_of(cols, mult), 1)


def st3(nb, rows, cols, mult=8):
    """Row stride > width; batch stride one `mult` past the rows: no multiple of the row stride."""
    ld = ld_of(cols, mult)
    assert (rows * ld + mult) % ld != 0
    return (rows * ld + mult, ld, 1)


class Mk:
    """Hands a case body its operands: compact tensors (arena=False) or arena views (arena=True) of the same contents."""

    def __init__(self, arena):
        self.arena, self.ins, self.outs = arena, [], []

    def _mk(self, shape, dtype, strides, align, poison, data, book, name, cld=None):
        if data is not None:
            data = data.to(DEV)
            shape, dtype = tuple(data.shape), data.dtype
        if not self.arena:
            if cld is not None:                              # the tightest row stride the entry point accepts, where the width is none
                t = torch.empty(shape[:-1] + (cld,), dtype=dtype, device=DEV).fill_(default_poison(dtype) if poison is None else poison)[..., :shape[-1]]
                return t if data is None else t.copy_(data)
            if data is not None:
                return data.contiguous().clone()
            return torch.empty(shape, dtype=dtype, device=DEV).fill_(default_poison(dtype) if poison is None else poison)
        a = Arena(shape, dtype, strides=strides, align=align, poison=poison, device=DEV, data=data)
        book.append((name, a))
        return a.view

    def inp(self, data, strides=None, align=16, poison=None, name="input", cld=None):
        return self._mk(None, None, strides, align, poison, data, self.ins, name, cld)

    def out(self, shape=None, dtype=BF, strides=None, align=16, poison=None, init=None, name="output", cld=None):
        """An output (poison unless `init`: accumulators, in-place operands).  cld: the compact run's row stride (default the width)."""
        return self._mk(shape, dtype, strides, align, poison, init, self.outs, name, cld)

    def check(self):
        torch.cuda.synchronize()
        for name, a in self.ins:
            a.assert_unchanged(name)
        for name, a in self.outs:
            a.assert_outside_intact(name)


def contract(body, inexact=()):
    """Steps 1-5 of the module docstring.  body(mk) -> {name: output tensor}.  `inexact`: outputs the caller compares itself."""
    mc, ma = Mk(False), Mk(True)
    rc = body(mc)
    torch.cuda.synchronize()
    ra = body(ma)
    torch.cuda.synchronize()
    assert rc.keys() == ra.keys()
    for k in rc:
        if k not in inexact:
            assert_bits_equal(ra[k], rc[k], k)
    ma.check()
    return rc, ra


def call(name, *args):
    """The C entry point on the current stream; tensors pass as their data pointers."""
    conv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    N.check(getattr(ops._lib(), name)(ops._st(), *conv), name)


def flat2d(v3):
    """[groups, g, cols] view -> the [groups * g, cols] tensor ops.gemm_* takes with row groups: the first group's pointer and row
    stride (the rows behind the first group are addressed through the group stride, not through this shape)."""
    return v3.as_strided((v3.shape[0] * v3.shape[1], v3.shape[2]), (v3.stride(1), 1))


def cpu64(t):
    return t.detach().cpu().to(F64)


# ================================================================================================================ NT GEMM
NT = {"128x128": (N.KERNEL_NT_128x128, "2", False), "128x64": (N.KERNEL_NT_128x64, "3", False), "256": (N.KERNEL_NT_256, "6", False),
      "64x128_s6": (N.KERNEL_NT_64x128_S6, None, True), "128x128_s4": (N.KERNEL_NT_128x128_S4, None, True)}
# the descriptor features each kernel id accepts (gemm.hip: plan_nt / launch_nt)
NT_FEATURES = {
    "128x128": ["bias_res", "res_mod", "batch", "groups", "c_live", "swiglu", "swiglu_bwd", "rope1", "rope2", "ext", "fp8", "splitk"],
    "128x64": ["bias_res", "res_mod", "batch", "groups", "c_live", "swiglu", "rope2", "splitk"],
    "256": ["bias_res", "res_mod", "batch", "groups", "c_live", "swiglu", "rope1", "rope2", "ext", "fp8"],
    "64x128_s6": ["bias_res", "res_mod", "batch", "groups", "c_live", "swiglu", "rope1", "rope2", "splitk"],
    # (reached through 44 batches of 3 x 2 64-row tiles: more than 256 CUs take, while 44 x (2 x 2) 128-row tiles fit.  Every feature below
    # is combined with that batch; row groups are left to the other ids, and split-K needs batch 1: the four-stage ring would take 43
    # slices of four K-tiles, K = 11008, or an 11010-column product - no small shape reaches it)
    "128x128_s4": ["batch", "res_mod", "c_live", "swiglu", "rope1", "rope2"],
}
NT_CASES = [(k, f) for k, fs in NT_FEATURES.items() for f in fs]


class nt_kernel:
    """Force the kernel the way the existing tests do: VLA_GEMM_TILE, or the latency hint (with the <= 512-row skinny tiles off)."""

    def __init__(self, monkeypatch, name):
        self.mp, (self.kid, self.tile, self.hint) = monkeypatch, NT[name]

    def __enter__(self):
        if self.tile:
            self.mp.setenv("VLA_GEMM_TILE", self.tile)
        if self.hint:
            self.mp.setenv("VLA_NO_SMALL_ROWS", "1")
            self.h = ops.latency_hint()
            self.h.__enter__()
        return self.kid

    def __exit__(self, *exc):
        if self.hint:
            self.h.__exit__(*exc)
            self.mp.delenv("VLA_NO_SMALL_ROWS")
        if self.tile:
            self.mp.delenv("VLA_GEMM_TILE")
        return False


_FP8 = {}


def fp8_operands(M, Nn, K):
    """e4m3 codes and scales of random operands (quantised once by the library's own vla_quant_fp8_rows)."""
    if (M, Nn, K) not in _FP8:
        qa, sa = ops.quant_fp8_rows(gen(M, K, seed=71).to(DEV))
        qb, sb = ops.quant_fp8_rows(gen(Nn, K, seed=72, scale=0.05).to(DEV))
        _FP8[(M, Nn, K)] = tuple(t.cpu() for t in (qa, sa, qb, sb))
    return _FP8[(M, Nn, K)]


@case("vla_gemm_bf16_nt")
@pytest.mark.parametrize("kernel,feature", NT_CASES, ids=[f"{k}-{f}" for k, f in NT_CASES])
def test_gemm_nt(kernel, feature, monkeypatch):
    """M and N one past a tile edge with N % 8 != 0 (129 x 130 on the 128- and 64-row tiles, 257 x 258 on the 256-row tile); C at
    the alignment an ldc that is no multiple of 8 leaves it (2 B) where the epilogue allows, residual with ldr != ldc."""
    big = kernel == "256"
    M, Nn, K = (257, 258, 192) if big else (129, 130, 256)
    plans = []

    def body(mk):
        a, b = gen(M, K, seed=1), gen(Nn, K, seed=2, scale=0.05)
        kw, outs = {}, {}
        n_out = (Nn // 64) * 64                              # 128 / 256 columns: what the SwiGLU / RoPE epilogues take
        if kernel == "128x128_s4":
            nb = 44
            nB = 256 if feature == "swiglu" else Nn          # (two column tiles, or the 64-row tiles would fit the chip)
            A_ = mk.inp(gen(nb, M, K, seed=1), st3(nb, M, K))
            B_ = mk.inp(gen(nb, nB, K, seed=2, scale=0.05), st3(nb, nB, K))
            ldc = ld_of(nB) + 8
            out = mk.out((nb, M, nB), BF, (M * ldc + 8, ldc, 1))
            if feature == "batch":
                kw["bias"] = mk.inp(gen(nb, Nn, seed=3), st2(nb, Nn), name="bias")
                kw["residual"] = mk.inp(gen(nb, M, Nn, seed=4), st3(nb, M, Nn), name="R")
            elif feature == "res_mod":
                kw["residual"], kw["res_mod"] = mk.inp(gen(50, Nn, seed=4), st2(50, Nn), name="R"), 50
            elif feature == "c_live":
                kw["bias"], kw["c_live"] = mk.inp(gen(Nn, seed=3), name="bias"), (40, 17)
            elif feature == "swiglu":
                ld2 = nB // 2 + 4
                kw["act"], kw["out2"] = ops.ACT_SWIGLU, mk.out((nb, M, nB // 2), BF, (M * ld2 + 4, ld2, 1), align=8, name="h")
                outs["h"] = kw["out2"]
            else:
                T, dh = 50, 64
                cos, sin = ops.rope_half_tables(T, dh, 1e6, "cpu") if feature == "rope1" else ops.rope_inter_tables(T, dh, "cpu")
                kw["rope"] = (1 if feature == "rope1" else 2, mk.inp(cos, name="cos"), mk.inp(sin, name="sin"), T, dh, n_out)
                kw["bias"] = mk.inp(gen(Nn, seed=3), name="bias")
        elif feature == "bias_res":
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b, st2(Nn, K))
            kw["bias"] = mk.inp(gen(Nn, seed=3), align=2, name="bias")
            kw["residual"] = mk.inp(gen(M, Nn, seed=4), (Nn + 5, 1), align=2, name="R")            # ldr % 8 != 0: element loads
            out = mk.out((M, Nn), BF, (Nn + 1, 1), align=2)                                       # ldc % 8 != 0
        elif feature == "res_mod":
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b, st2(Nn, K))
            kw["residual"], kw["res_mod"] = mk.inp(gen(50, Nn, seed=4), st2(50, Nn), name="R"), 50
            out = mk.out((M, Nn), BF, (ld_of(Nn) + 8, 1))                                         # ldr != ldc, both vector rows
        elif feature == "batch":
            nb = 3
            A_ = mk.inp(gen(nb, M, K, seed=1), st3(nb, M, K))
            B_ = mk.inp(gen(nb, Nn, K, seed=2, scale=0.05), st3(nb, Nn, K))
            kw["bias"] = mk.inp(gen(nb, Nn, seed=3), st2(nb, Nn), name="bias")
            kw["residual"] = mk.inp(gen(nb, M, Nn, seed=4), st3(nb, M, Nn), name="R")
            ldc = ld_of(Nn) + 8
            out = mk.out((nb, M, Nn), BF, (M * ldc + 8, ldc, 1))
        elif feature == "groups":
            nbg, g, S = (3, 86, 90) if big else (3, 43, 50)  # the [B, row0:, D] window: 43 live rows of 50 per sequence (3 x 43 = 129 = M)
            assert nbg * g in (M, M + 1)                     # (3 x 86 = 258 on the 256-row tile)
            a3 = mk.inp(gen(nbg, g, K, seed=1), (S * ld_of(K) + 8, ld_of(K), 1))
            r3 = mk.inp(gen(nbg, g, Nn, seed=4), (S * ld_of(Nn) + 16, ld_of(Nn), 1), name="R")
            o3 = mk.out((nbg, g, Nn), BF, (S * (ld_of(Nn) + 8) + 8, ld_of(Nn) + 8, 1))
            A_, B_, out = flat2d(a3), mk.inp(b, st2(Nn, K)), flat2d(o3)
            kw["residual"] = flat2d(r3)
            if mk.arena:                                     # (the compact run is the plain product of the same rows)
                kw.update(a_group=(g, a3.stride(0)), c_group=(g, o3.stride(0)), r_group=(g, r3.stride(0)))
            outs["C"] = o3
        elif feature == "c_live":
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b, st2(Nn, K))
            kw["bias"], kw["c_live"] = mk.inp(gen(Nn, seed=3), name="bias"), (40, 17)      # rows m with m % 40 < 17 keep their poison
            out = mk.out((M, Nn), BF, st2(M, Nn))
        elif feature == "swiglu":
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b[:n_out], st2(n_out, K))
            out = mk.out((M, n_out), BF, st2(M, n_out), name="pre")
            kw["act"], kw["out2"] = ops.ACT_SWIGLU, mk.out((M, n_out // 2), BF, (n_out // 2 + 4, 1), align=8, name="h")
            outs["h"] = kw["out2"]
        elif feature in ("rope1", "rope2"):
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b, st2(Nn, K))
            T, dh = 50, 64
            cos, sin = ops.rope_half_tables(T, dh, 1e6, "cpu") if feature == "rope1" else ops.rope_inter_tables(T, dh, "cpu")
            kw["rope"] = (1 if feature == "rope1" else 2, mk.inp(cos, name="cos"), mk.inp(sin, name="sin"), T, dh, n_out)
            kw["bias"] = mk.inp(gen(Nn, seed=3), name="bias")
            out = mk.out((M, Nn), BF, st2(M, Nn))
        elif feature == "ext":
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(b, st2(Nn, K))
            kw["ext"] = (mk.inp(gen(M, 64, seed=5), st2(M, 64), name="A2"), mk.inp(gen(Nn, 64, seed=6, scale=0.05), st2(Nn, 64), name="B2"))
            kw["residual"] = mk.inp(gen(M, Nn, seed=4), st2(M, Nn), name="R")
            out = mk.out((M, Nn), BF, (ld_of(Nn) + 8, 1))
        elif feature == "fp8":
            Kq = 256
            qa, sa, qb, sb = fp8_operands(M, Nn, Kq)
            A_, B_ = mk.inp(qa, st2(M, Kq, 16)), mk.inp(qb, st2(Nn, Kq, 16))
            kw["fp8"] = (mk.inp(sa, align=4, name="a_scale"), mk.inp(sb, align=4, name="b_scale"))
            kw["bias"] = mk.inp(gen(Nn, seed=3), name="bias")
            out = mk.out((M, Nn), BF, st2(M, Nn))
        elif feature == "splitk":
            Nn4, Ks = 132, 512                               # N % 4 == 0, N % 8 != 0; two slices of four K-tiles
            A_, B_ = mk.inp(gen(M, Ks, seed=1), st2(M, Ks)), mk.inp(gen(Nn4, Ks, seed=2, scale=0.05), st2(Nn4, Ks))
            kw["bias"], kw["residual"] = mk.inp(gen(Nn4, seed=3), name="bias"), mk.inp(gen(M, Nn4, seed=4), st2(M, Nn4), name="R")
            kw["split_k"], kw["act"] = 2, ops.ACT_GELU
            out = mk.out((M, Nn4), BF, (ld_of(Nn4) + 8, 1))
            ws = mk.out((2, M, Nn4), F32, name="workspace [split, M, N]")     # changes only inside [split, M, N]
            monkeypatch.setattr(ARENA, "get", lambda nbytes, device: ws.view(-1).view(U8))
        elif feature == "swiglu_bwd":
            I = 128                                          # the product is dH [M, I]; R = GU [M, 2I], C = dGU [M, 2I]
            A_, B_ = mk.inp(a, st2(M, K)), mk.inp(gen(I, K, seed=2, scale=0.05), st2(I, K))
            gu = mk.inp(gen(M, 2 * I, seed=4), (2 * I + 4, 1), align=8, name="GU")                # ldr % 4 == 0, 8-B aligned
            out = mk.out((M, 2 * I), BF, st2(M, 2 * I))
            with nt_kernel(monkeypatch, kernel) as kid:
                plans.append(ops.gemm_swiglu_bwd(A_, B_, gu, out=out, query_plan=True)[0])
                ops.gemm_swiglu_bwd(A_, B_, gu, out=out)
                assert plans[-1] == kid, f"{kernel}/{feature}: planned on kernel id {plans[-1]}, the case is named for {kid}"
            return {"C": out}
        with nt_kernel(monkeypatch, kernel) as kid:
            plans.append(ops.gemm_plan(A_, B_, out=out, **kw)[0])
            ops.gemm_nt(A_, B_, out=out, **kw)
            assert plans[-1] == kid, f"{kernel}/{feature}: planned on kernel id {plans[-1]}, the case is named for {kid}"
        outs.setdefault("C", out)
        return outs

    rc, _ = contract(body)
    assert len(plans) == 2 and plans[0] == plans[1]
    if feature in ("rope1", "rope2"):                        # columns past rope_cols keep the bits of the un-rotated product
        sh = (44,) if kernel == "128x128_s4" else ()
        with nt_kernel(monkeypatch, kernel):
            plain = ops.gemm_nt(gen(*sh, M, K, seed=1).to(DEV), gen(*sh, Nn, K, seed=2, scale=0.05).to(DEV), bias=gen(Nn, seed=3).to(DEV))
        nc = (Nn // 64) * 64
        assert_bits_equal(rc["C"][..., nc:], plain[..., nc:], "columns past rope_cols")
        assert not torch.equal(rc["C"][..., :nc], plain[..., :nc])
    if feature == "c_live":
        dead = ((torch.arange(M) % 40) < 17).to(DEV)
        assert torch.isnan(rc["C"][..., dead, :].float()).all() and torch.isfinite(rc["C"][..., ~dead, :].float()).all()


# kernel id - VLA_KERNEL_NT_SKINNY = the tile of gemm_skinny.hip; (M, N, K, latency hint): 1 and 17 rows under the hint, and the
# shapes at which the plan reaches the larger tiles on a 256-CU chip
SKINNY = [(0, 1, 16, 512, True), (0, 17, 16, 512, True), (1, 1, 4112, 512, True), (2, 17, 4112, 512, True), (3, 33, 4112, 512, True),
          (4, 1538, 192, 128, False), (5, 2823, 192, 128, False), (6, 5650, 192, 128, False)]


@case("vla_gemm_bf16_nt")
@pytest.mark.parametrize("tile,M,Nn,K,hint", SKINNY, ids=[f"tile{t}-{m}x{n}x{k}" for t, m, n, k, _ in SKINNY])
def test_gemm_nt_skinny(tile, M, Nn, K, hint):
    plans = []

    def body(mk):
        a, b = mk.inp(gen(M, K, seed=11), st2(M, K)), mk.inp(gen(Nn, K, seed=12, scale=0.05), st2(Nn, K))
        kw = dict(bias=mk.inp(gen(Nn, seed=13), name="bias"), residual=mk.inp(gen(M, Nn, seed=14), st2(M, Nn), name="R"), act=ops.ACT_GELU)
        out = mk.out((M, Nn), BF, (ld_of(Nn) + 8, 1))        # ldr != ldc
        if hint:
            with ops.latency_hint():
                plans.append(ops.gemm_plan(a, b, out=out, **kw)[0])
                ops.gemm_nt(a, b, out=out, **kw)
        else:
            plans.append(ops.gemm_plan(a, b, out=out, **kw)[0])
            ops.gemm_nt(a, b, out=out, **kw)
        return {"C": out}

    contract(body)
    assert plans == [N.KERNEL_NT_SKINNY + tile] * 2, f"planned on kernel ids {plans}, the case is named for {N.KERNEL_NT_SKINNY + tile}"


# ================================================================================================================ TN GEMM
def tn_plan(a, b, out, **kw):
    d = N.GemmTnDesc()
    d.A, d.B, d.C, d.M, d.N1, d.N2 = a.data_ptr(), b.data_ptr(), out.data_ptr(), kw.get("rows", a.shape[-2]), out.shape[-2], out.shape[-1]
    d.lda, d.ldb, d.ldc, d.batch, d.split = a.stride(-2), b.stride(-2), out.stride(-2), a.shape[0] if a.dim() == 3 else 1, kw.get("split") or 0
    s = C.c_int(0)
    return ops._lib().vla_gemm_tn_plan(C.byref(d), 0, C.byref(s))


@case("vla_gemm_bf16_tn")
@pytest.mark.parametrize("tile,form", [(t, f) for t in (128, 256) for f in ("strided", "batch", "row_groups", "col_groups")] + [(128, "split")])
def test_gemm_tn(tile, form, monkeypatch):
    """Both tiles on N1 / N2 one 8-column chunk past a tile edge, M one past a K-tile; C at its 8-B minimum with ldc % 8 == 4.
    (The contraction split runs on the 128-tile kernel only: plan_tn.)"""
    N1, N2, M = (264, 136, 65) if tile == 256 else (136, 264, 65)
    monkeypatch.setenv("VLA_TN_TILE", str(tile))
    want = N.KERNEL_TN_256 if tile == 256 else N.KERNEL_TN_128

    def body(mk):
        if form == "strided":
            a, b = mk.inp(gen(M, N1, seed=21), st2(M, N1)), mk.inp(gen(M, N2, seed=22), st2(M, N2))
            out = mk.out((N1, N2), BF, (N2 + 4, 1), align=8)
            assert tn_plan(a, b, out) == want
            ops.gemm_tn(a, b, out=out, alpha=0.5, split=0)
        elif form == "batch":
            a, b = mk.inp(gen(2, M, N1, seed=21), st3(2, M, N1)), mk.inp(gen(2, M, N2, seed=22), st3(2, M, N2))
            out = mk.out((2, N1, N2), BF, (N1 * (N2 + 4) + 4, N2 + 4, 1), align=8)
            assert tn_plan(a, b, out) == want
            ops.gemm_tn(a, b, out=out, split=0)
        elif form == "row_groups":                           # the first 64 rows of every sequence of a [B, S, D] tensor, read in place
            nbg, g, S = 2, 64, 70
            a3 = mk.inp(gen(nbg, g, N1, seed=21), (S * ld_of(N1) + 8, ld_of(N1), 1))
            b3 = mk.inp(gen(nbg, g, N2, seed=22), (S * ld_of(N2) + 16, ld_of(N2), 1))
            out = mk.out((N1, N2), BF, (N2 + 4, 1), align=8)
            ops.gemm_tn(flat2d(a3)[:g], flat2d(b3)[:g], out=out, rows=nbg * g, a_group=(g, a3.stride(0)), b_group=(g, b3.stride(0)), split=0)
        elif form == "col_groups":                           # the gate columns of a gate / up interleaved dY: 16 of every 32
            a = mk.inp(gen(M, 2 * N1 + 16, seed=21), st2(M, 2 * N1 + 16))      # (column 16 + 32 (c / 16) + c % 16 for c < N1)
            b = mk.inp(gen(M, N2, seed=22), st2(M, N2))
            out = mk.out((N1, N2), BF, (N2 + 4, 1), align=8)
            ops.gemm_tn(a, b, out=out, a_cols=(N1, 16, 32, 16), split=0)
        else:                                                # two slices of the contraction through the fp32 workspace
            Ms = 129
            a, b = mk.inp(gen(Ms, N1, seed=21), st2(Ms, N1)), mk.inp(gen(Ms, N2, seed=22), st2(Ms, N2))
            out = mk.out((N1, N2), BF, (N2 + 4, 1), align=8)
            ws = mk.out((1, 2, N1, N2), F32, name="workspace [batch, split, N1, N2]")
            monkeypatch.setattr(ARENA, "get", lambda nbytes, device: ws.view(-1).view(U8))
            ops.gemm_tn(a, b, out=out, split=2)
        return {"C": out}

    contract(body)


@case("vla_gemm_bf16_tn_grouped")
@pytest.mark.parametrize("tile", [128, 256])
def test_gemm_tn_grouped(tile, monkeypatch):
    monkeypatch.setenv("VLA_TN_TILE", str(tile))
    shapes = [(65, 136, 264, None), (130, 264, 136, None), (64, 136, 72, (136, 16, 32, 16))]

    def body(mk):
        probs, outs = [], {}
        for i, (M, N1, N2, cols) in enumerate(shapes):
            wa = 2 * N1 + 16 if cols else N1
            a, b = mk.inp(gen(M, wa, seed=30 + i), st2(M, wa)), mk.inp(gen(M, N2, seed=40 + i), st2(M, N2))
            outs[f"C{i}"] = mk.out((N1, N2), BF, (N2 + 4, 1), align=8)
            probs.append(ops.tn_problem(a, b, outs[f"C{i}"], alpha=1.0 + i, a_cols=cols))
        ops.gemm_tn_grouped(probs)
        return outs

    contract(body)


# ================================================================================================================ transpose
@case("vla_transpose_bf16")
@pytest.mark.parametrize("form", ["vector", "element"])
def test_transpose(form):
    """ldi > cols, ldo > rows, batch strides; the columns rows .. ldo of the output are NOT touched (include/vla_native.h)."""
    nb, R, Cc = 2, (72 if form == "vector" else 67), (136 if form == "vector" else 131)
    al, mult = (16, 8) if form == "vector" else (2, 1)

    def body(mk):
        x = mk.inp(gen(nb, R, Cc, seed=50), st3(nb, R, Cc, mult) if mult == 8 else (R * (Cc + 3) + 5, Cc + 3, 1), align=al)
        out = mk.out((nb, Cc, R), BF, st3(nb, Cc, R, mult) if mult == 8 else (Cc * (R + 3) + 7, R + 3, 1), align=al)
        call("vla_transpose_bf16", x, out, R, Cc, x.stride(1), out.stride(1), nb, x.stride(0), out.stride(0))
        return {"out": out}

    rc, _ = contract(body)
    assert torch.equal(rc["out"], gen(nb, R, Cc, seed=50).to(DEV).transpose(1, 2))


# ================================================================================================================ norms, quantisation
ROWS_COLS = [(r, c) for r in (1, 3, 5) for c in (8, 520, 1032)]
EPS = 1e-6


def norm_w(cols, seed):
    return (1 + 0.1 * gen(cols, seed=seed).float()).to(BF)


@case("vla_layernorm_fwd")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_layernorm_fwd(rows, cols):
    def body(mk):
        x = mk.inp(gen(rows, cols, seed=60), st2(rows, cols))
        w, b = mk.inp(norm_w(cols, 61)), mk.inp(gen(cols, seed=62, scale=0.1))
        y, stats = mk.out((rows, cols), BF, (ld_of(cols) + 8, 1)), mk.out((rows, 2), F32, align=4, name="stats")
        call("vla_layernorm_fwd", x, w, b, y, stats, rows, cols, x.stride(0), y.stride(0), EPS)
        return {"y": y, "stats": stats}

    contract(body)


def _ln_stats(x, w, b, rows, cols):
    y, stats = ops.layernorm_fwd(x.to(DEV), w.to(DEV), b.to(DEV), EPS, want_stats=True)
    return stats.cpu()


@case("vla_layernorm_bwd")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_layernorm_bwd_all_four_strides(rows, cols):
    """dx and the aligned (fixed-order) dw / db sums: ldx, lddy, lddx all larger than cols and different."""
    x, w, b, dy = gen(rows, cols, seed=60), norm_w(cols, 61), gen(cols, seed=62, scale=0.1), gen(rows, cols, seed=63)
    st = _ln_stats(x, w, b, rows, cols)

    def body(mk):
        xv, dyv = mk.inp(x, st2(rows, cols)), mk.inp(dy, (ld_of(cols) + 8, 1))
        wv, sv = mk.inp(w), mk.inp(st, align=4, name="stats")
        dx = mk.out((rows, cols), BF, (ld_of(cols) + 16, 1))
        dw, db = mk.out(init=torch.zeros(cols), align=4, name="dw"), mk.out(init=torch.ones(cols), align=4, name="db")
        call("vla_layernorm_bwd", dyv, xv, wv, sv, dx, dw, db, rows, cols, xv.stride(0), dyv.stride(0), dx.stride(0))
        return {"dx": dx, "dw": dw, "db": db}

    contract(body)


@case("vla_layernorm_bwd")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_layernorm_bwd_sums_one_element_off(rows, cols):
    """dy and x one element off a 16-B boundary (dx not requested): the one-thread-per-column sums, rows in order - another fp32
    order than the compact run's workgroup reduction, so dw / db are held to the fp64 bounds of test_kernel_accuracy_gpu.py::
    test_layernorm_bwd (4 sqrt(rows) u32 sum |terms| + the fp32 error of x^) instead of to the compact run's bits."""
    x, w, b, dy = gen(rows, cols, seed=60), norm_w(cols, 61), gen(cols, seed=62, scale=0.1), gen(rows, cols, seed=63)
    st = _ln_stats(x, w, b, rows, cols)

    def body(mk):
        xv, dyv = mk.inp(x, st2(rows, cols), align=2), mk.inp(dy, (ld_of(cols) + 8, 1), align=2)
        wv, sv = mk.inp(w), mk.inp(st, align=4, name="stats")
        dw, db = mk.out(init=torch.zeros(cols), align=4, name="dw"), mk.out(init=torch.zeros(cols), align=4, name="db")
        call("vla_layernorm_bwd", dyv, xv, wv, sv, None, dw, db, rows, cols, xv.stride(0), dyv.stride(0), cols)
        return {"dw": dw, "db": db}

    rc, ra = contract(body, inexact=("dw", "db"))
    x64, dy64 = cpu64(x), cpu64(dy)
    mu = x64.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (x64 - mu) * rstd
    exh = A.norm_floor(xh, torch.ones(cols), None, mu, rstd)
    flw = 4 * math.sqrt(rows) * A.U32 * (dy64.abs() * xh.abs()).sum(0) + (dy64.abs() * exh).sum(0)
    flb = 4 * math.sqrt(rows) * A.U32 * dy64.abs().sum(0)
    for r in (rc, ra):
        assert ((cpu64(r["dw"]) - (dy64 * xh).sum(0)).abs() <= flw + 1e-30).all(), "LN dw"
        assert ((cpu64(r["db"]) - dy64.sum(0)).abs() <= flb + 1e-30).all(), "LN db"


@case("vla_rmsnorm_fwd")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_rmsnorm_fwd(rows, cols):
    def body(mk):
        x, w = mk.inp(gen(rows, cols, seed=64)), mk.inp(norm_w(cols, 65))
        y, rstd = mk.out((rows, cols)), mk.out((rows,), F32, align=4, name="rstd")
        call("vla_rmsnorm_fwd", x, w, y, rstd, rows, cols, EPS)
        return {"y": y, "rstd": rstd}

    contract(body)


@case("vla_rmsnorm_bwd")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_rmsnorm_bwd(rows, cols):
    x, w = gen(rows, cols, seed=64), norm_w(cols, 65)
    rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), EPS, want_rstd=True)[1].cpu()

    def body(mk):
        xv, wv, dy, dres = mk.inp(x), mk.inp(w), mk.inp(gen(rows, cols, seed=66)), mk.inp(gen(rows, cols, seed=67))
        rs, dx = mk.inp(rstd, align=4, name="rstd"), mk.out((rows, cols))
        call("vla_rmsnorm_bwd", dy, xv, wv, rs, dres, dx, rows, cols, 0, 0, 0)
        return {"dx": dx}

    contract(body)


@case("vla_rmsnorm_bwd")
@pytest.mark.parametrize("g,cols", [(1, 520), (3, 8), (5, 1032)])
def test_rmsnorm_bwd_row_window(g, cols):
    """The form of test_rmsnorm_bwd_row_window: x / rstd are the forward's [B, S, .] tensors, the backward visits rows [r0, r0 + g) of
    every sequence.  Only those rows are declared: the rows before and behind the window are poison."""
    nb, S, r0 = 2, 9, 3
    x, w = gen(nb, g, cols, seed=64), norm_w(cols, 65)
    rstd = ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), EPS, want_rstd=True)[1].cpu().view(nb, g)

    def body(mk):
        if mk.arena:
            xv = mk.inp(x, (S * cols, cols, 1))
            rs = mk.inp(rstd, (S, 1), align=4, name="rstd")
            xp, rp = xv.data_ptr() - r0 * cols * 2, rs.data_ptr() - r0 * 4
        else:
            xf, rf = torch.full((nb, S, cols), float("nan"), dtype=BF, device=DEV), torch.full((nb, S), float("nan"), device=DEV)
            xf[:, r0:r0 + g], rf[:, r0:r0 + g] = x.to(DEV), rstd.to(DEV)
            xp, rp = xf.data_ptr(), rf.data_ptr()
        wv, dy, dres = mk.inp(w), mk.inp(gen(nb * g, cols, seed=66)), mk.inp(gen(nb * g, cols, seed=67))
        dx = mk.out((nb * g, cols))
        call("vla_rmsnorm_bwd", dy, C.c_void_p(xp), wv, C.c_void_p(rp), dres, dx, nb * g, cols, g, S, r0)
        torch.cuda.synchronize()                             # (the compact run's full tensors live until here)
        return {"dx": dx}

    rc, _ = contract(body)
    assert torch.isfinite(rc["dx"].float()).all()


@case("vla_rmsnorm_dw")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
@pytest.mark.parametrize("form", ["aligned", "one_element_off"])
def test_rmsnorm_dw(rows, cols, form):
    """aligned: the fixed-order sums, bit for bit.  one_element_off: dy / x one element off a 16-B boundary run one thread per column
    (another fp32 order): held to the fp64 bound of test_kernel_accuracy_gpu.py::test_rmsnorm_bwd_and_dw."""
    x, dy = gen(rows, cols, seed=64), gen(rows, cols, seed=66)
    rstd = ops.rmsnorm_fwd(x.to(DEV), norm_w(cols, 65).to(DEV), EPS, want_rstd=True)[1].cpu()
    al = 16 if form == "aligned" else 2

    def body(mk):
        xv, dyv, rs = mk.inp(x, align=al), mk.inp(dy, align=al), mk.inp(rstd, align=4, name="rstd")
        dw = mk.out(init=torch.zeros(cols), align=4, name="dw")
        call("vla_rmsnorm_dw", dyv, xv, rs, dw, rows, cols)
        return {"dw": dw}

    rc, ra = contract(body, inexact=() if form == "aligned" else ("dw",))
    if form != "aligned":
        n64 = cpu64(x) * cpu64(rstd)[:, None]                # the forward's declared rounding point, from the rstd the entry point is given
        n, fa = A.round_point(n64, 2 * A.U32 * n64.abs())    # (the fp32 product in front of the rounding)
        tw = (cpu64(dy) * n).sum(0)
        flw = 4 * math.sqrt(rows) * A.U32 * (cpu64(dy).abs() * n.abs()).sum(0) + (cpu64(dy).abs() * fa).sum(0)
        for r in (rc, ra):
            assert ((cpu64(r["dw"]) - tw).abs() <= flw + 1e-30).all(), "rmsnorm dw"


@case("vla_quant_fp8_rows")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_quant_fp8_rows(rows, cols):
    def body(mk):
        x = mk.inp(gen(rows, cols, seed=68), st2(rows, cols))
        q, sc = mk.out((rows, cols), U8, st2(rows, cols, 16), cld=-(-cols // 16) * 16), mk.out((rows,), F32, align=4, name="scale")
        call("vla_quant_fp8_rows", x, q, sc, rows, cols, x.stride(0), q.stride(0))
        return {"q": q, "scale": sc}

    contract(body)


@case("vla_rmsnorm_fwd_q8", "vla_layernorm_fwd_q8")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_norms_q8(rows, cols):
    def body(mk):
        x, w, b = mk.inp(gen(rows, cols, seed=64)), mk.inp(norm_w(cols, 65)), mk.inp(gen(cols, seed=62, scale=0.1))
        y, rstd = mk.out((rows, cols)), mk.out((rows,), F32, align=4, name="rstd")
        q, qs = mk.out((rows, cols), U8, st2(rows, cols, 16), cld=-(-cols // 16) * 16), mk.out((rows,), F32, align=4, name="qscale")
        call("vla_rmsnorm_fwd_q8", x, w, y, rstd, q, qs, rows, cols, q.stride(0), EPS)
        xs = mk.inp(gen(rows, cols, seed=60), st2(rows, cols))
        y2, stats = mk.out((rows, cols), BF, (ld_of(cols) + 8, 1)), mk.out((rows, 2), F32, align=4, name="stats")
        q2, qs2 = mk.out((rows, cols), U8, (ld_of(cols, 16) + 16, 1), cld=-(-cols // 16) * 16), mk.out((rows,), F32, align=4, name="qscale2")
        call("vla_layernorm_fwd_q8", xs, w, b, y2, stats, q2, qs2, rows, cols, xs.stride(0), y2.stride(0), q2.stride(0), EPS)
        return {"y": y, "rstd": rstd, "q": q, "qs": qs, "y2": y2, "stats": stats, "q2": q2, "qs2": qs2}

    contract(body)


# ================================================================================================================ attention
def _qkv(mk, nb, Sq, Sk, Hq, Hkv, dh, seed):
    """q, k, v as column windows of wider buffers (the q | k | v columns of one fused projection), a batch stride past the rows."""
    wq, wk = Hq * dh + 64, Hkv * dh + 128
    q = mk.inp(gen(nb, Sq, Hq * dh, seed=seed), (Sq * wq + 8, wq, 1), name="q")
    k = mk.inp(gen(nb, Sk, Hkv * dh, seed=seed + 1), (Sk * wk + 8, wk, 1), name="k")
    v = mk.inp(gen(nb, Sk, Hkv * dh, seed=seed + 2), (Sk * wk + 16, wk, 1), name="v")
    return q, k, v


def _kmask(mk, nb, S, masked):
    if not masked:
        return None
    m = torch.ones(nb, S, dtype=U8)
    m[0, S // 2:] = 0                                        # a padded tail, and for S = 1 a row with no visible key
    m[1, ::3] = 0 if S > 2 else 1
    return mk.inp(m, align=1, poison=1, name="kmask")         # (kmask [B, Sk] is contiguous by contract; poison: key allowed)


@case("vla_attn_fwd", "vla_attn_bwd")
@pytest.mark.parametrize("S", [1, 31, 33, 65])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "kmask"])
def test_attention(S, masked):
    nb, Hq, Hkv, dh = 2, 4, 2, 64

    def body(mk):
        q, k, v = _qkv(mk, nb, S, S, Hq, Hkv, dh, 80)
        km = _kmask(mk, nb, S, masked)
        wo = Hq * dh + 8
        o = mk.out((nb, S, Hq * dh), BF, (S * wo + 8, wo, 1), name="o")
        lse = mk.out((nb, Hq, S), F32, align=4, name="lse")
        ops.attn_fwd(q, k, v, Hq, Hkv, dh, causal=not masked, kmask=km, out=o, lse=lse, want_lse=True)
        do = mk.inp(gen(nb, S, Hq * dh, seed=84), (S * (wo + 8) + 8, wo + 8, 1), name="dout")
        wg, wkg = Hq * dh + 4, Hkv * dh + 4
        dq = mk.out((nb, S, Hq * dh), BF, (S * wg + 4, wg, 1), align=8, name="dq")
        dk = mk.out((nb, S, Hkv * dh), BF, (S * wkg + 4, wkg, 1), align=8, name="dk")
        dv = mk.out((nb, S, Hkv * dh), BF, (S * wkg + 8, wkg, 1), align=8, name="dv")
        delta = mk.out((nb, Hq, S), F32, align=4, name="delta (scratch)")
        ops.attn_bwd(do, q, k, v, o, lse, Hq, Hkv, dh, causal=not masked, kmask=km, dq=dq, dk=dk, dv=dv, delta=delta)
        return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv, "delta": delta}

    rc, _ = contract(body)
    assert torch.isfinite(rc["o"].float()).all()


@case("vla_attn_fwd")
@pytest.mark.parametrize("S", [1, 33, 65])
def test_attention_fwd_minimum_alignment_and_key_split(S):
    """Forward only: o at its 8-B minimum with o_ss % 8 == 4; once plain and once under the latency hint (the key-split kernel:
    fewer workgroups than half the CUs, dh 64)."""
    nb, Hq, Hkv, dh = 2, 4, 2, 64

    def body(mk):
        q, k, v = _qkv(mk, nb, S, S, Hq, Hkv, dh, 80)
        wo, res = Hq * dh + 4, {}
        for name in ("plain", "split"):
            o = mk.out((nb, S, Hq * dh), BF, (S * wo + 4, wo, 1), align=8, name="o " + name)
            lse = mk.out((nb, Hq, S), F32, align=4, name="lse " + name)
            if name == "split":
                with ops.latency_hint():
                    ops.attn_fwd(q, k, v, Hq, Hkv, dh, causal=True, out=o, lse=lse, want_lse=True)
            else:
                ops.attn_fwd(q, k, v, Hq, Hkv, dh, causal=True, out=o, lse=lse, want_lse=True)
            res["o " + name], res["lse " + name] = o, lse
        return res

    contract(body)


@case("vla_attn_bwd")
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "inverse_rope"])
def test_attention_bwd_live_rows(rope):
    """The live-row form at row0 = 32: q / o / dout / dq are the [B, Sk - 32, .] windows, lse the forward's full [B, Hq, Sk], dk / dv
    hold the keys >= 32; with and without the fused inverse RoPE (tables in arenas)."""
    nb, Hq, Hkv, dh, Sk, r0 = 2, 4, 2, 64, 65, 32
    Sq = Sk - r0
    qf, kf, vf = gen(nb, Sk, Hq * dh, seed=90), gen(nb, Sk, Hkv * dh, seed=91), gen(nb, Sk, Hkv * dh, seed=92)
    of, lf = ops.attn_fwd(qf.to(DEV), kf.to(DEV), vf.to(DEV), Hq, Hkv, dh, causal=True, want_lse=True)
    of, lf = of.cpu(), lf.cpu()

    def body(mk):
        wq, wk = Hq * dh + 64, Hkv * dh + 128
        q = mk.inp(qf[:, r0:], (Sk * wq + 8, wq, 1), name="q")           # rows < row0 are not declared: poison
        o = mk.inp(of[:, r0:], (Sk * wq + 8, wq, 1), name="o")
        do = mk.inp(gen(nb, Sq, Hq * dh, seed=93), (Sq * wq + 8, wq, 1), name="dout")
        k, v = mk.inp(kf, (Sk * wk + 8, wk, 1), name="k"), mk.inp(vf, (Sk * wk + 8, wk, 1), name="v")
        lse = mk.inp(lf, align=4, name="lse")
        wg, wkg = Hq * dh + 4, Hkv * dh + 4
        dq = mk.out((nb, Sq, Hq * dh), BF, (Sq * wg + 4, wg, 1), align=8, name="dq")
        dk = mk.out((nb, Sq, Hkv * dh), BF, (Sq * wkg + 4, wkg, 1), align=8, name="dk")
        dv = mk.out((nb, Sq, Hkv * dh), BF, (Sq * wkg + 4, wkg, 1), align=8, name="dv")
        rp = None
        if rope:
            cos, sin = ops.rope_half_tables(Sk, dh, 1e6, "cpu")
            rp = (mk.inp(cos, align=4, name="cos"), mk.inp(sin, align=4, name="sin"))
        delta = mk.out((nb, Hq, Sq), F32, align=4, name="delta (scratch)")
        ops.attn_bwd(do, q, k, v, o, lse, Hq, Hkv, dh, causal=True, dq=dq, dk=dk, dv=dv, rope=rp, row0=r0, delta=delta)
        return {"dq": dq, "dk": dk, "dv": dv, "delta": delta}

    rc, _ = contract(body)
    assert all(torch.isfinite(rc[k].float()).all() for k in ("dq", "dk", "dv"))


# ================================================================================================================ head attention
@case("vla_head_attn_fwd", "vla_head_attn_bwd")
@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_head_attention(path, rope, monkeypatch):
    """Forward and backward, every ld_* larger than H * dh, the backward's workspace in an arena.  T = 8 (the VALU path's only T)."""
    if path == "valu":
        monkeypatch.setenv("VLA_HEAD_ATTN_VALU", "1")
    # (the VALU path adds one gate partial per (sample, head) workgroup with a float atomic: two of them commute, four would not)
    nb, T, Ka, Kt, H, dh = 2, 8, 9, 33, (1 if path == "valu" else 2), 16
    D = H * dh
    ntile = (T + Ka + Kt + 31) // 32
    wsn = nb * H * ntile * (T * dh + 1)

    def body(mk):
        def seg(n, seed, extra, name, f=mk.inp):
            return f(gen(nb, n, D, seed=seed), (n * (D + extra), D + extra, 1), name=name)       # [B, n, D] rows at stride D + extra
        q, ks, vs = seg(T, 100, 8, "q"), seg(T, 101, 16, "k_self"), seg(T, 102, 16, "v_self")
        ka, va, kt, vt = seg(Ka, 103, 24, "k_adp"), seg(Ka, 104, 24, "v_adp"), seg(Kt, 105, 32, "k_task"), seg(Kt, 106, 32, "v_task")
        gate = mk.inp(torch.tensor([0.3], dtype=BF), align=2, name="gate")
        out = mk.out((nb, T, D), BF, (T * (D + 40), D + 40, 1), name="out")
        probs = mk.out((nb, H, T, T + Ka + Kt), F32, name="probs")
        ops.head_attn_fwd(q, ks, vs, ka, va, kt, vt, gate, H=H, out=out, probs=probs)

        def grad(like, name):
            return mk.out(tuple(like.shape), BF, tuple(like.stride()) if mk.arena else None, name=name)
        dout = mk.inp(gen(nb, T, D, seed=107), (T * (D + 40), D + 40, 1), name="dout")
        dq, dks, dvs = grad(q, "dq"), grad(ks, "dk_self"), grad(vs, "dv_self")
        dka, dva, dkt, dvt = grad(ka, "dk_adp"), grad(va, "dv_adp"), grad(kt, "dk_task"), grad(vt, "dv_task")
        dgate = mk.out(init=torch.zeros(1), align=4, name="dgate")
        rp = None
        if rope:
            cos, sin = ops.rope_inter_tables(max(T, Ka, Kt), dh, "cpu")
            rp = (mk.inp(cos, name="cos"), mk.inp(sin, name="sin"))
        ws = mk.out((wsn,), F32, name="workspace")
        monkeypatch.setattr(ARENA, "get", lambda nbytes, device: ws.view(U8))
        ops.head_attn_bwd(dout, out, q, ks, vs, ka, va, kt, vt, gate, probs, dgate, dq, dks, dvs, dka, dva, dkt, dvt, H=H, rope=rp)
        return {"out": out, "dq": dq, "dks": dks, "dvs": dvs, "dka": dka, "dva": dva, "dkt": dkt, "dvt": dvt, "dgate": dgate}

    rc, _ = contract(body)
    assert all(torch.isfinite(t.float()).all() for t in rc.values())


# ================================================================================================================ in-place RoPE
@case("vla_rope_half", "vla_rope_interleaved")
@pytest.mark.parametrize("form", ["vector", "element"])
def test_rope_in_place(form):
    """On a column window of a wider buffer; the interleaved form in its 16-B arm and, one element off, in its element arm."""
    nb, S, H, dh = 2, 5, 3, 16
    al = 16 if form == "vector" else 2

    def body(mk):
        res = {}
        for name, sym, tables, arg in (("half", "vla_rope_half", ops.rope_half_tables(S, dh, 1e6, "cpu"), 1),
                                       ("half_inverse", "vla_rope_half", ops.rope_half_tables(S, dh, 1e6, "cpu"), -1),
                                       ("interleaved", "vla_rope_interleaved", ops.rope_inter_tables(S, dh, "cpu"), 0),
                                       ("interleaved_bwd", "vla_rope_interleaved", ops.rope_inter_tables(S, dh, "cpu"), 1)):
            x = mk.out(init=gen(nb * S, H * dh, seed=110), strides=(H * dh + (8 if form == "vector" else 5), 1), align=al, name=name)
            cos, sin = mk.inp(tables[0], align=al if al == 16 else 4, name="cos"), mk.inp(tables[1], align=al if al == 16 else 4, name="sin")
            call(sym, x, cos, sin, nb * S, S, H, dh, x.stride(0), arg)
            res[name] = x
        return res

    contract(body)


# ================================================================================================================ glue, elementwise
@case("vla_gather_rows", "vla_scatter_add_rows")
def test_gather_scatter_rows():
    R, n, D = 7, 6, 520

    def body(mk):
        src = mk.inp(gen(R, D, seed=120), st2(R, D))
        idx = mk.inp(torch.tensor([3, -1, 0, -2, 6, 3], dtype=I32), align=4, poison=R - 1, name="idx")
        out = mk.out((n, D), BF, (ld_of(D) + 8, 1))
        call("vla_gather_rows", src, idx, out, n, D, src.stride(0), out.stride(0))
        upd = mk.inp(gen(n, D, seed=121), (ld_of(D) + 16, 1))
        sidx = mk.inp(torch.tensor([2, -1, 5, 0, -1, 6], dtype=I32), align=4, poison=1, name="scatter idx")
        acc = mk.out(init=gen(R, D, seed=122), strides=st2(R, D), name="acc")
        call("vla_scatter_add_rows", upd, sidx, acc, n, D, upd.stride(0), acc.stride(0))
        return {"gathered": out, "acc": acc}

    rc, _ = contract(body)
    assert torch.isnan(rc["gathered"][3].float()).all() and (rc["gathered"][1] == 0).all()      # -2: untouched, -1: zeros


@case("vla_colsum_bf16")
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
@pytest.mark.parametrize("form", ["aligned", "one_element_off"])
def test_colsum_batched(rows, cols, form):
    """aligned: bit for bit.  one_element_off: x one element off a 16-B boundary runs one thread per column (rows in order: another
    fp32 order), held to the bound of the kernel's own test (test_kernels_gpu.py: rel-L2 1e-5, max 1e-5 of the largest sum)."""
    nb = 2
    al = 16 if form == "aligned" else 2
    x = gen(nb, rows, cols, seed=130)

    def body(mk):
        xv = mk.inp(x, st3(nb, rows, cols), align=al)
        out = mk.out(init=torch.ones(nb, cols), strides=(cols + 3, 1), align=4, name="sums")
        call("vla_colsum_bf16", xv, out, rows, cols, xv.stride(1), nb, xv.stride(0), out.stride(0))
        return {"sums": out}

    rc, ra = contract(body, inexact=() if form == "aligned" else ("sums",))
    ref = 1 + cpu64(x).sum(1)
    for r in (rc, ra):
        d = cpu64(r["sums"]) - ref
        assert d.norm() <= 1e-5 * ref.norm() and d.abs().max() <= 1e-5 * ref.abs().max() + 1e-6


DT = {"bf16": BF, "f32": F32}


@case("vla_copy2d")
@pytest.mark.parametrize("src_dt,dst_dt", [("bf16", "bf16"), ("f32", "bf16"), ("bf16", "f32"), ("f32", "f32")])
@pytest.mark.parametrize("form", ["vector", "element", "src_mod", "d_group"])
def test_copy2d(src_dt, dst_dt, form):
    sd, dd = DT[src_dt], DT[dst_dt]
    rows, cols = 6, (16 if form == "vector" else 13)
    lds, ldd = (24, 32) if form == "vector" else (15, 17)
    al = (lambda dt: 16) if form == "vector" else (lambda dt: 2 if dt == BF else 4)
    src_rows = 4 if form == "src_mod" else rows
    data = gen(src_rows, cols, seed=140, dtype=sd)

    def body(mk):
        src = mk.inp(data, (lds, 1), align=al(sd))
        if form == "d_group":
            dst = mk.out((2, 3, cols), dd, (5 * ldd + 3, ldd, 1), align=al(dd))
            call("vla_copy2d", src, dst, rows, cols, src.stride(0), dst.stride(1), int(sd == F32), int(dd == F32), 0, 3, dst.stride(0))
        else:
            dst = mk.out((rows, cols), dd, (ldd, 1), align=al(dd))
            call("vla_copy2d", src, dst, rows, cols, src.stride(0), dst.stride(0), int(sd == F32), int(dd == F32), 4 if form == "src_mod" else 0, 0, 0)
        return {"dst": dst}

    rc, _ = contract(body)
    want = data[torch.arange(rows) % src_rows].to(dd).to(DEV)
    assert_bits_equal(rc["dst"].reshape(rows, cols), want, "copy2d")


@case("vla_copy_rows3d")
@pytest.mark.parametrize("form", ["vector", "element"])
def test_copy_rows3d(form):
    G, R, cols = 3, 4, (24 if form == "vector" else 13)
    al, m = (16, 8) if form == "vector" else (2, 1)
    data = gen(G, R, cols, seed=141)

    def body(mk):
        src = mk.inp(data, (R * (cols + 8) + 8, cols + 8, 1) if m == 8 else (R * (cols + 2) + 3, cols + 2, 1), align=al)
        dst = mk.out((G, R, cols), BF, (R * (cols + 16) + 8, cols + 16, 1) if m == 8 else (R * (cols + 4) + 1, cols + 4, 1), align=al)
        call("vla_copy_rows3d", src, dst, G, R, cols, src.stride(0), src.stride(1), dst.stride(0), dst.stride(1))
        return {"dst": dst}

    rc, _ = contract(body)
    assert_bits_equal(rc["dst"], data.to(DEV), "copy_rows3d")


@case("vla_cast_f32_bf16", "vla_cast_bf16_f32")
def test_casts():
    n = 1031
    xf, xb = gen(n, seed=142, dtype=F32), gen(n, seed=143)

    def body(mk):
        a, b = mk.inp(xf, align=4), mk.inp(xb, align=2)
        ya, yb = mk.out((n,), BF, align=2), mk.out((n,), F32, align=4)
        call("vla_cast_f32_bf16", a, ya, n)
        call("vla_cast_bf16_f32", b, yb, n)
        return {"bf16": ya, "f32": yb}

    rc, _ = contract(body)
    assert_bits_equal(rc["bf16"], xf.to(BF).to(DEV), "f32 -> bf16")
    assert_bits_equal(rc["f32"], xb.float().to(DEV), "bf16 -> f32")


@case("vla_fill_zero")
@pytest.mark.parametrize("nbytes", [1, 15, 16, 17, 4097])
def test_zero(nbytes):
    def body(mk):
        t = mk.out((nbytes,), U8)
        ops.zero_(t)
        return {"t": t}

    rc, _ = contract(body)
    assert (rc["t"] == 0).all()


@case("vla_inc_i32", "vla_add_scalar_f32", "vla_add_bf16")
def test_inc_add_scalar_add():
    n = 2072

    def body(mk):
        cnt = mk.out(init=torch.tensor([41], dtype=I32), align=4, poison=7, name="counter")
        ops.inc_i32_(cnt)
        x = mk.out(init=gen(300, seed=150, dtype=F32), align=4, name="x")
        s = mk.inp(torch.tensor([0.375]), align=4, name="scalar")
        ops.add_scalar_f32_(x, s)
        a, b = mk.out(init=gen(n, seed=151), name="a"), mk.inp(gen(n, seed=152), name="b")
        ops.add_(a, b)
        return {"counter": cnt, "x": x, "a": a}

    rc, _ = contract(body)
    assert rc["counter"].item() == 42


@case("vla_gelu_fwd", "vla_gelu_bwd", "vla_relu_bwd", "vla_swiglu_fwd", "vla_swiglu_bwd")
def test_activations():
    n, M, I = 2072, 3, 48

    def body(mk):
        x, dy = mk.inp(gen(n, seed=153), name="x"), mk.inp(gen(n, seed=154), name="dy")
        y, dx, dr = mk.out((n,)), mk.out((n,)), mk.out((n,))
        ops.gelu_fwd(x, out=y)
        ops.gelu_bwd(dy, x, out=dx)
        ops.relu_bwd(dy, x, out=dr)
        gu, dh = mk.inp(gen(M, 2 * I, seed=155), name="gu"), mk.inp(gen(M, I, seed=156), name="dh")
        h, dgu = mk.out((M, I)), mk.out((M, 2 * I))
        ops.swiglu_fwd(gu, out=h)
        ops.swiglu_bwd(dh, gu, out=dgu)
        return {"gelu": y, "gelu_bwd": dx, "relu_bwd": dr, "h": h, "dgu": dgu}

    contract(body)


@case("vla_layerscale_fwd", "vla_layerscale_bwd")
def test_layerscale():
    rows, cols = 5, 520

    def body(mk):
        a, ls, x = mk.inp(gen(rows, cols, seed=160), name="a"), mk.inp(gen(cols, seed=161), name="ls"), mk.inp(gen(rows, cols, seed=162), name="x")
        out = mk.out((rows, cols))
        ops.layerscale_fwd(a, ls, x, out=out)
        dy = mk.inp(gen(rows, cols, seed=163), name="dy")
        da, da2 = mk.out((rows, cols)), mk.out((rows, cols))
        dls = mk.out(init=torch.ones(cols), align=4, name="dls")
        ops.layerscale_bwd(dy, a, ls, dls_f32=dls, out=da)
        ops.layerscale_bwd(dy, None, ls, out=da2)                # the frozen-scale form (LoRA)
        return {"out": out, "da": da, "da_frozen": da2, "dls": dls}

    contract(body)


@case("vla_dropout_bf16", "vla_dropout_bwd_add_bf16")
def test_dropout_strided():
    rows, cols = 5, 24

    def body(mk):
        x, step = mk.inp(gen(rows, cols, seed=164), st2(rows, cols)), mk.inp(torch.tensor([3], dtype=I32), align=4, poison=9, name="step")
        y = mk.out((rows, cols), BF, (ld_of(cols) + 8, 1))
        ops.dropout(x, y, 0.25, seed=1234, step=step)
        dx = mk.out(init=gen(rows, cols, seed=165), strides=(ld_of(cols) + 16, 1), name="dx")
        ops.dropout_bwd_add_(dx, x, 0.25, seed=1234, step=step)
        return {"y": y, "dx": dx}

    rc, _ = contract(body)
    kept = (rc["y"] != 0).float().mean().item()
    assert 0.4 < kept < 0.99


@case("vla_im2col_patch")
@pytest.mark.parametrize("px", ["bf16", "f32"])
def test_im2col(px):
    """Every element of cols [B * (H/P) * (W/P), ldo] is written: the patch, then zeros up to ldo (include/vla_native.h)."""
    B, Ct, c0, H, W, P, ldo = 2, 6, 3, 4, 6, 2, 16

    def body(mk):
        pix = mk.inp(gen(B, Ct, H, W, seed=170, dtype=DT[px]), align=2 if px == "bf16" else 4)
        cols = mk.out((B * (H // P) * (W // P), ldo), BF, align=2)
        call("vla_im2col_patch", pix, cols, B, Ct, c0, H, W, P, ldo, int(px == "f32"))
        return {"cols": cols}

    rc, _ = contract(body)
    assert (rc["cols"][:, 3 * P * P:] == 0).all() and torch.isfinite(rc["cols"].float()).all()


def _labels(B, L):
    lab = torch.full((B, L), -100, dtype=I64)
    lab[0, 5:L - 2] = 151400 + torch.arange(L - 7)          # more than 64 action tokens: two 64-wide passes
    lab[1, 9:20] = 151390
    lab[1, 3] = 1000                                         # a text token among them
    return lab


@case("vla_action_mask", "vla_token_row_class", "vla_head_index_prep")
def test_action_mask_row_class_index_prep():
    B, L = 2, 80

    def body(mk):
        lab = mk.inp(_labels(B, L), align=8, poison=151500, name="labels")      # poison: an id that would be selected
        res = {}
        for shift in (0, 1):
            qidx = mk.out((B, L - shift), I32, align=4, poison=7)
            pos, cnt = mk.out((B, 64), I32, align=4, poison=7), mk.out((B,), I32, align=4, poison=7)
            call("vla_action_mask", lab, qidx, pos, cnt, B, L, shift)
            cls = mk.out((B, L - shift), U8, align=1)
            call("vla_token_row_class", lab, cls, B, L, shift, 151386, 7)
            res.update({f"qidx{shift}": qidx, f"pos{shift}": pos, f"cnt{shift}": cnt, f"cls{shift}": cls})
        S, Np, row0 = L + 5, 5, 8
        p1 = mk.inp(res["pos1"].cpu(), align=4, poison=2, name="pos1")
        p0 = mk.inp(res["pos0"].cpu(), align=4, poison=2, name="pos0")
        c0 = mk.inp(res["cnt0"].cpu(), align=4, poison=2, name="cnt0")
        gather, scatter = mk.out((B, 65), I32, align=4, poison=7), mk.out((B, 65), I32, align=4, poison=7)
        guard = mk.out((1,), F32, align=4)
        call("vla_head_index_prep", p1, p0, c0, gather, scatter, guard, B, S, Np, row0)
        res.update(gather=gather, scatter=scatter, guard=guard)
        return res

    rc, _ = contract(body)
    assert rc["cnt0"].tolist() == [80 - 7, 11] and rc["guard"].item() == 0.0


@case("vla_embed_splice", "vla_embed_grad", "vla_action_query_grad")
def test_embed_splice_and_grads():
    B, L, Np, D, V = 2, 5, 3, 16, 11
    S = L + Np
    ids = torch.tensor([[1, 4, 4, 9, 0], [10, 1, 2, 2, 7]], dtype=I64)
    qidx = torch.tensor([[-1, -1, 0, 1, -1], [-1, 0, -1, -1, 1]], dtype=I32)
    am = torch.tensor([[1, 1, 1, 0, 1], [1, 1, 0, 1, 1]], dtype=U8)

    def body(mk):
        idv, qv = mk.inp(ids, align=8, poison=V - 1, name="ids"), mk.inp(qidx, align=4, poison=5, name="qidx")
        amv = mk.inp(am, align=1, poison=1, name="attention mask")
        table, aq = mk.inp(gen(V, D, seed=180), name="table"), mk.inp(gen(64, D, seed=181), name="action queries")
        out, mm = mk.out((B, S, D)), mk.out((B, S), U8, align=1)
        call("vla_embed_splice", idv, amv, qv, table, aq, out, mm, B, L, Np, D, V)
        dx = mk.inp(gen(B, S, D, seed=182), align=2, name="dx")
        gt = mk.out((V, D), BF, align=2, name="grad table")
        call("vla_embed_grad", dx, idv, qv, gt, B, L, Np, D, V)
        pos = torch.full((B, 64), -1, dtype=I32)
        pos[0, :2], pos[1, :2] = torch.tensor([2, 3]), torch.tensor([1, 4])
        row0 = 2
        dxl = mk.inp(gen(B, S - row0, D, seed=183), align=2, name="live dx")
        dq = mk.out((64, D), F32, align=4, name="dq")
        call("vla_action_query_grad", dxl, mk.inp(pos, align=4, poison=1, name="pos"), dq, B, S - row0, Np, D, row0)
        return {"embeds": out, "mm_mask": mm, "grad_table": gt, "dq": dq}

    rc, _ = contract(body)
    assert torch.isnan(rc["embeds"][:, 1:Np + 1].float()).all(), "rows 1 .. Np belong to the projector GEMM"
    want_mm = torch.ones(B, S, dtype=U8)
    want_mm[:, Np + 1:] = am[:, 1:]
    want_mm[:, 0] = am[:, 0]
    assert torch.equal(rc["mm_mask"].cpu(), want_mm), "every element of mm_mask is written: 1 on the patch rows, the attention mask elsewhere"
    assert torch.isnan(rc["grad_table"][3].float()).all() and torch.isfinite(rc["grad_table"][4].float()).all()   # id 3 never occurs
    assert torch.isfinite(rc["dq"]).all()


# ================================================================================================================ loss, optimiser
@case("vla_token_ce", "vla_token_ce_bwd", "vla_token_ce_metrics", "vla_token_metrics_finish")
@pytest.mark.parametrize("V", [11, 2059])
def test_token_ce(V):
    """ld_logits > V at the smallest V that leaves a vector-loop tail (one 8-chunk + 3), and the same in a thread's second pass
    (2048 + 8 + 3).  Two valid rows: the two atomic adds of a sum commute."""
    rows = 3
    tgt = torch.tensor([V - 2, -100, 3], dtype=I64)

    def body(mk):
        lg = mk.inp(gen(rows, V, seed=190, scale=3.0), st2(rows, V), name="logits", cld=-(-V // 8) * 8)
        t = mk.inp(tgt, align=8, poison=1, name="targets")
        sums = mk.out(init=torch.zeros(2), align=4, name="sums")
        call("vla_token_ce", lg, lg.stride(0), t, rows, V, sums)
        dl = mk.out((rows, V), BF, (ld_of(V) + 8, 1), name="dlogits", cld=-(-V // 8) * 8)
        call("vla_token_ce_bwd", lg, lg.stride(0), t, rows, V, sums, 0.5, dl, dl.stride(0))
        cls = mk.inp(torch.tensor([1, 2, 0], dtype=U8), align=1, poison=1, name="row class")
        sums2 = mk.out(init=torch.zeros(2), align=4, name="sums (metrics)")
        cnt = mk.out(init=torch.zeros(6, dtype=I64), align=8, poison=5, name="counters")
        pred = mk.out((rows,), I32, align=4, poison=7, name="pred ids")
        call("vla_token_ce_metrics", lg, lg.stride(0), t, cls, rows, V, sums2, cnt, pred, V + 1, 8)
        out4 = mk.out((4,), F32, align=4, name="metrics")
        call("vla_token_metrics_finish", cnt, 2.0 / 7, out4)
        return {"sums": sums, "dlogits": dl, "sums2": sums2, "counters": cnt, "pred": pred, "metrics": out4}

    rc, _ = contract(body)
    assert rc["sums"][1].item() == 2 and torch.equal(rc["sums"], rc["sums2"]) and (rc["dlogits"][1] == 0).all()


@case("vla_l1_loss")
def test_l1_loss():
    B, Cc, Da = 2, 3, 7

    def body(mk):
        p, t = mk.inp(gen(B, Cc, Da, seed=200), align=2, name="pred"), mk.inp(gen(B, Cc, Da, seed=201), align=2, name="target")
        loss, dp = mk.out((3,), F32, align=4, name="loss3"), mk.out((B, Cc, Da), BF, align=2, name="dpred")
        call("vla_l1_loss", p, t, loss, dp, B, Cc, Da, 0.5)
        return {"loss": loss, "dpred": dp}

    contract(body)


@case("vla_adamw_bf16", "vla_adamw_clipped_bf16")
@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "clipped"])
@pytest.mark.parametrize("g_f32", [0, 1], ids=["g_bf16", "g_f32"])
@pytest.mark.parametrize("align", [2, 16], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("n", [2056, 2059])
def test_adamw_on_a_range(clipped, g_f32, align, n):
    """A range [off, off + n) of flat p / g / m / v buffers: 16-B aligned (the 8-wide kernel plus its scalar tail for n % 8 = 3) and
    one element off (the scalar kernel throughout); the same arithmetic, bit for bit."""
    def body(mk):
        p, m = mk.out(init=gen(n, seed=210), align=align, name="p"), mk.out(init=gen(n, seed=211, scale=0.1), align=align, name="m")
        v = mk.out(init=gen(n, seed=212, scale=0.1).abs(), align=align, name="v")
        g = mk.inp(gen(n, seed=213, dtype=F32 if g_f32 else BF), align=max(align, 4 if g_f32 else 2), name="g")
        args = (p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, g_f32, 0.5)
        if clipped:
            call("vla_adamw_clipped_bf16", *args, mk.inp(torch.tensor([0.625]), align=4, name="coef"))
        else:
            call("vla_adamw_bf16", *args)
        return {"p": p, "m": m, "v": v}

    contract(body)


@case("vla_grad_sumsq", "vla_grad_norm_finalise")
@pytest.mark.parametrize("g_f32", [0, 1], ids=["g_bf16", "g_f32"])
@pytest.mark.parametrize("align", ["element", 16])
def test_grad_norm(g_f32, align):
    n = 16384 + 2059                                         # two slots; the second with a head, a body and a tail

    def body(mk):
        al = align if align == 16 else (4 if g_f32 else 2)
        g = mk.inp(gen(n, seed=220, dtype=F32 if g_f32 else BF), align=al, name="g")
        slots = mk.out((2,), F32, align=4, name="slots")
        call("vla_grad_sumsq", g, n, g_f32, 0.5, slots)
        out2 = mk.out((2,), F32, align=4, name="norm, coef")
        call("vla_grad_norm_finalise", slots, 2, 1.0, out2)
        return {"slots": slots, "out2": out2}

    rc, ra = contract(body, inexact=() if align == 16 else ("slots", "out2"))
    # one element off, the head / body / tail split of a slot moves, and with it the order of the fp32 adds (vla_native.h says so at
    # vla_grad_sumsq): both runs are held to the bounds of tests/test_grad_clip_gpu.py - the slots (each, and so their sum) within 1e-5
    # of the fp64 sum of squares of the consumed values, the norm within 1e-5, the clip coefficient within 2^-22 of torch's expression
    x = A.r64(cpu64(gen(n, seed=220, dtype=F32 if g_f32 else BF)) * 0.5)
    want = torch.stack([(x[:16384] ** 2).sum(), (x[16384:] ** 2).sum()])
    norm = math.sqrt(want.sum().item())
    for name, r in (("compact", rc), ("view", ra)):
        rel = ((cpu64(r["slots"]) - want).abs() / want).max().item()
        got_norm, got_coef = r["out2"].tolist()
        coef = torch.clamp(1.0 / (r["out2"][0] + 1e-6), max=1.0).item()
        print(f"grad_norm {name}: slots rel err {rel:.3e}, norm rel err {abs(got_norm - norm) / norm:.3e}, coef {got_coef!r} torch {coef!r}")
        assert rel <= 1e-5, (name, r["slots"].tolist(), want.tolist())
        assert abs(got_norm - norm) / norm <= 1e-5, (name, got_norm, norm)
        assert got_coef < 1.0 and abs(got_coef - coef) <= 2.0 ** -22 * coef, (name, got_coef, coef)


# ================================================================================================================ input stage
@case("vla_image_normalize_u8", "vla_resample_u8")
@pytest.mark.parametrize("out_dt", ["bf16", "f32"])
def test_image_normalize_and_resample(out_dt):
    B, H, W, Ct, c0 = 2, 5, 7, 6, 3
    img = torch.randint(0, 256, (B, H, W, 3), dtype=U8, generator=torch.Generator().manual_seed(230))
    mean, std = (C.c_float * 3)(0.5, 0.4, 0.3), (C.c_float * 3)(0.2, 0.25, 0.3)
    in_len, out_len, ks = W, 4, 3
    bounds = torch.tensor([[0, 3], [1, 3], [3, 2], [4, 3]], dtype=I32)
    coefs = torch.tensor([[1 << 20, 1 << 21, 1 << 20]] * out_len, dtype=I32)

    def body(mk):
        im = mk.inp(img, align=1, name="img")
        out = mk.out((B, Ct, H, W), DT[out_dt], align=2 if out_dt == "bf16" else 4)
        call("vla_image_normalize_u8", im, out, B, H, W, Ct, c0, mean, std, int(out_dt == "f32"))
        bd, cf = mk.inp(bounds, align=4, poison=1, name="bounds"), mk.inp(coefs, align=4, poison=1 << 22, name="coefs")
        dst = mk.out((B * H, out_len, 3), U8, align=1, name="resampled")
        call("vla_resample_u8", im, dst, B * H, in_len, out_len, 3, bd, cf, ks)
        return {"pixels": out, "resampled": dst}

    rc, _ = contract(body)
    assert torch.isnan(rc["pixels"][:, :c0].float()).all() and torch.isfinite(rc["pixels"][:, c0:].float()).all()


AUG_CFG = (0.9, 0.2, 0.8, 1.2, 0.8, 1.2, 0.05)


@case("vla_augment_stats", "vla_augment_apply")
@pytest.mark.parametrize("arm", ["eight_byte", "byte"])
@pytest.mark.parametrize("draw", [False, True], ids=["params_given", "params_drawn"])
def test_augment_pair(arm, draw):
    """Both arms of the 8-byte dispatch of augment.hip (frames / frames_out 8-B and out 16-B aligned, or one byte off) against the
    same compact run: they must give the same bits."""
    Ni, H, W, n_img, n_bb = 2, 6, 16, 2, 2
    frames = torch.randint(0, 256, (Ni, H, W, 3), dtype=U8, generator=torch.Generator().manual_seed(240))
    params = torch.tensor([[0.3, 0.05, 0.1, 0.95, 0.9, 0.1, 1.1, 0.9, 0.02], [0.7, 0.0, 0.05, 0.9, 1.0, -0.1, 0.9, 1.1, -0.03]])
    opsmask = 31 | (32 if draw else 0)
    cfg = (C.c_float * 7)(*AUG_CFG)
    mean, std = (C.c_float * 6)(0.5, 0.4, 0.3, 0.45, 0.45, 0.45), (C.c_float * 6)(0.2, 0.25, 0.3, 0.22, 0.22, 0.22)
    nslab = ops._lib().vla_augment_slab_floats(Ni, H, W)
    a8 = arm == "eight_byte"

    def body(mk):
        fr = mk.inp(frames, align=8 if a8 else 1, name="frames")
        pr = mk.out(init=params, align=4, name="params") if draw else mk.inp(params, align=4, name="params")
        slab = mk.out((nslab,), F32, align=4, name="slab")
        call("vla_augment_stats", fr, pr, slab, Ni, H, W, n_img, opsmask, cfg, 77, 1, 5)
        out = mk.out((Ni // n_img, 3 * n_bb * n_img, H, W), BF, align=16 if a8 else 2, name="pixels")
        fo = mk.out((Ni, H, W, 3), U8, align=8 if a8 else 1, name="frames_out")
        call("vla_augment_apply", fr, pr, slab, out, fo, Ni, H, W, n_img, n_bb, mean, std, 0, opsmask, cfg, 77, 1, 5)
        return {"pixels": out, "frames_out": fo, "params": pr}

    rc, _ = contract(body)
    assert torch.isfinite(rc["pixels"].float()).all() and torch.isfinite(rc["params"]).all()


def _bins(nbins=16):
    return torch.linspace(-1, 1, nbins, dtype=F64)


@case("vla_action_tokenize", "vla_normalize_bounds", "vla_collate_tokens")
def test_tokenize_normalize_collate():
    B, n_act, D, L, nbins, tok_len, nt = 3, 6, 7, 24, 16, 1000, 8
    acts = gen(B, n_act, seed=250, dtype=F32).clamp(-1.2, 1.2)
    x = gen(5, D, seed=251, dtype=F32)
    low, high = -gen(D, seed=252, dtype=F32).abs() - 0.1, gen(D, seed=253, dtype=F32).abs() + 0.1
    mask, zmask = torch.tensor([1, 1, 0, 1, 1, 1, 0], dtype=U8), torch.tensor([0, 0, 0, 0, 1, 0, 0], dtype=U8)
    flat = torch.arange(100, 100 + 4 + 9 + 2, dtype=I64)
    off = torch.tensor([0, 4, 13, 15], dtype=I32)

    def body(mk):
        a, bins = mk.inp(acts, align=4, name="actions"), mk.inp(_bins(nbins), align=8, name="bins")
        ids = mk.out((B, n_act), I64, align=8, poison=7)
        call("vla_action_tokenize", a, bins, ids, B * n_act, nbins, -1.0, 1.0, tok_len)
        y = mk.out((5, D), F32, align=4)
        call("vla_normalize_bounds", mk.inp(x, align=4, name="x"), y, 5 * D, D, mk.inp(low, align=4, name="low"), mk.inp(high, align=4, name="high"),
             mk.inp(mask, align=1, poison=0, name="mask"), mk.inp(zmask, align=1, poison=1, name="zero mask"))
        pf, po = mk.inp(flat, align=8, poison=55, name="prompt ids"), mk.inp(off, align=4, poison=1, name="prompt offsets")
        cid, lab = mk.out((B, L), I64, align=8, poison=7, name="input ids"), mk.out((B, L), I64, align=8, poison=7, name="labels")
        am = mk.out((B, L), U8, align=1, name="attention mask")
        call("vla_collate_tokens", pf, po, flat.numel(), a, bins, cid, lab, am, B, n_act, L, nbins, -1.0, 1.0, tok_len, 0, -100, nt, 99, 1, 4)
        return {"token ids": ids, "normalised": y, "input_ids": cid, "labels": lab, "attention_mask": am}

    rc, _ = contract(body)
    assert (rc["normalised"][:, 4] == 0).all() and (rc["attention_mask"][0, :1 + nt] == 1).all()


# ================================================================================================================ aliasing the header allows
@case("vla_token_ce_bwd", "vla_layerscale_fwd", "vla_gemm_bf16_tn")
def test_aliased_runs_equal_unaliased():
    """dlogits = logits, out = x, R = C (gradient accumulation): each aliased run, in arenas, equals the unaliased compact run."""
    rows, V = 3, 2059
    tgt = torch.tensor([5, -100, V - 1], dtype=I64)
    lg = gen(rows, V, seed=190, scale=3.0)
    sums = torch.zeros(2, device=DEV)
    ldl = -(-V // 8) * 8
    lgd, ref = torch.zeros(rows, ldl, dtype=BF, device=DEV)[:, :V].copy_(lg), torch.zeros(rows, ldl, dtype=BF, device=DEV)[:, :V]
    call("vla_token_ce", lgd, ldl, tgt.to(DEV), rows, V, sums)
    call("vla_token_ce_bwd", lgd, ldl, tgt.to(DEV), rows, V, sums, 0.5, ref, ldl)
    mk = Mk(True)
    lv = mk.out(init=lg, strides=st2(rows, V), name="logits = dlogits")
    call("vla_token_ce_bwd", lv, lv.stride(0), mk.inp(tgt, align=8, poison=1), rows, V, mk.inp(sums.cpu(), align=4), 0.5, lv, lv.stride(0))
    assert_bits_equal(lv, ref, "token_ce_bwd in place")

    r2, c2 = 5, 520
    a, ls, x = gen(r2, c2, seed=160), gen(c2, seed=161), gen(r2, c2, seed=162)
    ref = ops.layerscale_fwd(a.to(DEV), ls.to(DEV), x.to(DEV))
    xv = mk.out(init=x, name="x = out")
    ops.layerscale_fwd(mk.inp(a), mk.inp(ls), xv, out=xv)
    assert_bits_equal(xv, ref, "layerscale_fwd in place")

    M, N1, N2 = 65, 136, 72
    dy, xx, acc = gen(M, N1, seed=21), gen(M, N2, seed=22), gen(N1, N2, seed=23)
    d = N.GemmTnDesc()
    cr, dyd, xd, accd = torch.empty(N1, N2, dtype=BF, device=DEV), dy.to(DEV), xx.to(DEV), acc.to(DEV)
    d.A, d.B, d.C, d.R = dyd.data_ptr(), xd.data_ptr(), cr.data_ptr(), accd.data_ptr()
    d.M, d.N1, d.N2, d.lda, d.ldb, d.ldc, d.ldr, d.batch, d.alpha = M, N1, N2, N1, N2, N2, N2, 1, 1.0
    N.check(ops._lib().vla_gemm_bf16_tn(ops._st(), C.byref(d)), "gemm_tn")
    cv = mk.out(init=acc, strides=(N2 + 4, 1), align=8, name="C = R")
    ops.gemm_tn(mk.inp(dy, st2(M, N1)), mk.inp(xx, st2(M, N2)), out=cv, accumulate=True, split=0)
    assert_bits_equal(cv, cr, "gemm_tn accumulating into C")
    mk.check()


# ================================================================================================================ the net has teeth
@case("vla_copy2d", "vla_layernorm_fwd")
def test_overrun_by_one_row_is_caught():
    """copy2d and layernorm_fwd launched with one row more than their output arena was told: the checker must raise.  (The extra row
    lands inside the arena's margin; the inputs hold the extra row.)"""
    rows, cols = 5, 24
    src = Arena((rows + 1, cols), BF, strides=(32, 1), align=16, device=DEV, data=gen(rows + 1, cols, seed=300).to(DEV))
    dst = Arena((rows, cols), BF, strides=(40, 1), align=16, device=DEV)
    call("vla_copy2d", src.view, dst.view, rows + 1, cols, 32, 40, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    src.assert_unchanged()
    with pytest.raises(AssertionError, match="PAST the last element"):
        dst.assert_outside_intact("copy2d, one row too many")

    w, b = gen(cols, seed=301).to(DEV), gen(cols, seed=302).to(DEV)
    y = Arena((rows, cols), BF, strides=(40, 1), align=16, device=DEV)
    call("vla_layernorm_fwd", src.view, w, b, y.view, None, rows + 1, cols, 32, 40, EPS)
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match="PAST the last element"):
        y.assert_outside_intact("layernorm_fwd, one row too many")


@case("vla_colsum_bf16")
def test_overread_by_eight_columns_reaches_the_result():
    """colsum launched with eight columns more than its input arena was told: the poison in the stride gap reaches the sums, which then
    differ from the compact run's."""
    rows, cols = 5, 24
    x = gen(rows, cols + 8, seed=303)
    ref = torch.zeros(cols + 8, device=DEV)
    ops.colsum_(x.to(DEV), ref)
    xa = Arena((rows, cols), BF, strides=(48, 1), align=16, device=DEV, data=x[:, :cols].to(DEV))
    out = torch.zeros(cols + 8, device=DEV)
    call("vla_colsum_bf16", xa.view, out, rows, cols + 8, 48, 1, 0, 0)
    torch.cuda.synchronize()
    assert_bits_equal(out[:cols], ref[:cols], "the declared columns")
    assert torch.isnan(out[cols:]).all() and torch.isfinite(ref).all()
    xa.assert_unchanged()
