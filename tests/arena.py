"""Poisoned arenas for the kernels' memory contract (tests/test_memory_contract_gpu.py; the helper's own tests on CPU tensors:
tests/test_arena_cpu.py).

The training step never hands a kernel a tensor that torch allocated on its own: it passes windows of larger buffers - the q | k | v
columns of a fused projection, the [B, row0:, D] live rows, ranges of the flat parameter buffers.  An ``Arena`` is one such window,
built so that a test can see what a kernel does around it:

 * one allocation, filled with POISON: NaN for bf16 / f32, 0x7f for bytes (a NaN in e4m3; for a u8 mask the caller passes the value
   opposite to the one its case uses), and for integer ids / labels / indices an in-range value of the caller's that would change the
   result.  A read past the declared extent that reaches the result therefore shows in the result;
 * one strided view inside it: ``shape`` with ``strides`` in elements (last stride 1) - a row stride larger than the width, a batch
   or row-group stride that is no multiple of the row stride - whose first element sits at EXACTLY ``align`` bytes (aligned to
   ``align``, not to 2 * ``align``): the minimum a kernel's host check accepts, so the paths chosen by alignment run;
 * the view lies at least max(1 MiB, the bytes it spans) from both ends of the allocation.  That margin is a safety condition, not a
   measurement: an overrun by a buggy kernel, or by a mistaken stride in a test, lands inside the allocation and is REPORTED - a view is
   never placed at the end of an allocation to make a stray access fault;
 * ``assert_outside_intact()`` compares bit patterns (never float equality: NaN != NaN) of every byte of the arena that is not a
   declared element of the view - the margins and the gap between the width and the row stride; ``assert_unchanged()`` compares the
   whole arena, declared elements included (inputs).
"""
from __future__ import annotations

import torch

MIN_MARGIN = 1 << 20
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def default_poison(dtype):
    if dtype.is_floating_point:
        return float("nan")
    if dtype == torch.uint8:
        return 0x7F
    raise ValueError(f"{dtype}: integer ids / labels / indices need a poison of the case's choosing (in range, and changing the result)")


class Arena:
    """One poisoned allocation with one strided view (``.view``) in it."""

    def __init__(self, shape, dtype, *, strides=None, align=None, poison=None, device="cpu", data=None):
        shape = tuple(int(s) for s in shape)
        assert len(shape) >= 1 and all(s > 0 for s in shape), f"bad shape {shape}"
        if strides is None:                                  # compact
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= s
        strides = tuple(int(s) for s in strides)
        assert len(strides) == len(shape) and strides[-1] == 1 and all(s > 0 for s in strides), f"bad strides {strides}"
        self.shape, self.strides, self.dtype = shape, strides, dtype
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.align = int(align) if align is not None else self.esize
        assert self.align >= self.esize and self.align % self.esize == 0 and self.align & (self.align - 1) == 0, f"bad alignment {align}"
        self.span_bytes = (sum((n - 1) * s for n, s in zip(shape, strides)) + 1) * self.esize
        self.margin = max(MIN_MARGIN, self.span_bytes)
        total = 2 * self.margin + self.span_bytes + 4 * self.align
        total = (total + 15) // 16 * 16
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        # first element at an address that is a multiple of `align` and not of 2 * `align`
        base = self.buf.data_ptr()
        assert base % self.esize == 0
        off = self.margin + (-(base + self.margin)) % (2 * self.align) + self.align
        assert (base + off) % (2 * self.align) == self.align
        self.offset = off
        self.buf.view(dtype).fill_(default_poison(dtype) if poison is None else poison)
        self.view = self._strided(self.buf)
        assert self.view.data_ptr() == base + off
        before, after = self.margins()
        assert before >= self.margin and after >= self.margin, "the view must lie a full margin from both ends of its arena"
        # the bytes that are declared elements of the view
        m = torch.zeros(total, dtype=torch.uint8, device=device)
        self._strided(m, _INT_OF_SIZE[self.esize]).fill_(-1 if self.esize > 1 else 255)
        self._declared = m != 0
        self._snap = None
        self.set(data)

    def _strided(self, buf, dtype=None):
        flat = buf[self.offset:self.offset + self.span_bytes].view(dtype or self.dtype)
        return flat.as_strided(self.shape, self.strides)

    def margins(self):
        """(bytes before the view's first element, bytes behind its last) inside the allocation."""
        return self.offset, self.buf.numel() - (self.offset + self.span_bytes)

    def set(self, data=None):
        """Copy ``data`` (the compact operand) into the view, then record the arena's bits as the state to check against."""
        if data is not None:
            assert tuple(data.shape) == self.shape and data.dtype == self.dtype, f"data {tuple(data.shape)} {data.dtype} != view {self.shape} {self.dtype}"
            self.view.copy_(data)
        self._snap = self.buf.clone()
        return self

    def ptr(self, *index):
        """Address of an element of the view (for entry points that take raw pointers)."""
        return self.view.data_ptr() + sum(i * s for i, s in zip(index, self.strides)) * self.esize

    # ---- checks --------------------------------------------------------------------------------------------------------------
    def _where(self, byte):
        rel = byte - self.offset
        if rel < 0:
            return f"{-rel} bytes BEFORE the first element"
        if rel >= self.span_bytes:
            return f"{rel - self.span_bytes} bytes PAST the last element"
        e, idx = rel // self.esize, []
        for s in self.strides:
            idx.append(e // s)
            e %= s
        return f"in a stride gap, at view element offset {tuple(idx)} (shape {self.shape}, strides {self.strides})"

    def _raise(self, bad, what):
        first = int(torch.nonzero(bad)[0])
        last = int(torch.nonzero(bad)[-1])
        raise AssertionError(f"{what}: {int(bad.sum())} bytes changed; first {self._where(first)}, last {self._where(last)}")

    def assert_outside_intact(self, what="arena"):
        """Every byte that is not a declared element of the view still holds the bits it held at set()."""
        bad = (self.buf != self._snap) & ~self._declared
        if bool(bad.any()):
            self._raise(bad, f"{what}: written outside the declared extent")

    def assert_unchanged(self, what="arena"):
        """The whole arena, declared elements included, still holds the bits it held at set() (an input)."""
        bad = self.buf != self._snap
        if bool(bad.any()):
            self._raise(bad, f"{what}: an input arena was written")


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns as integers of the same width (NaNs compare by payload)."""
    return t.contiguous().view(_INT_OF_SIZE[t.element_size()])


def assert_bits_equal(a: torch.Tensor, b: torch.Tensor, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    ne = bits(a) != bits(b)
    if bool(ne.any()):
        i = torch.nonzero(ne)[0].tolist()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ in their bits, first at {tuple(i)}: "
                             f"{a[tuple(i)].item()!r} vs {b[tuple(i)].item()!r}")
