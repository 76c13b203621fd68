"""The kernels' scratch arena (vla_adapter_amd/scratch.py): which buffer a request gets, when one is replaced, retired or reserved.
Host code only: the allocator, the current stream's key and the capture predicate are fakes, no kernel runs."""
import gc
import types
import weakref

import pytest
import torch

from vla_adapter_amd.scratch import ALIGN, ScratchArena

DEV = "cuda:0"


class Fake:
    """An arena over a recording allocator (CPU bytes, ALIGN-aligned), a settable current stream and a settable capture flag."""

    def __init__(self, floor=1024):
        self.stream, self.capturing, self.allocs = 1, False, []      # allocs: (nbytes, device, capturing, weak reference)
        self.arena = ScratchArena(alloc=self.alloc, stream_key=lambda: self.stream, capturing=lambda: self.capturing)
        self.arena.floor = floor

    def alloc(self, nbytes, device):
        raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8)
        buf = raw[(-raw.data_ptr()) % ALIGN:][:nbytes]
        self.allocs.append((nbytes, device, self.capturing, weakref.ref(buf)))
        return buf

    def alive(self):
        gc.collect()
        return [ref() is not None for *_, ref in self.allocs]

    def get(self, nbytes, stream=None, capturing=False):
        self.stream, self.capturing = (self.stream if stream is None else stream), capturing
        try:
            return self.arena.get(nbytes, DEV)
        finally:
            self.capturing = False


def stream(handle):
    return types.SimpleNamespace(cuda_stream=handle, device=DEV)


def test_one_buffer_per_stream_and_repeat_requests_hit():
    f = Fake()
    a, b = f.get(100, stream=1), f.get(100, stream=2)
    assert a is not b and a.data_ptr() != b.data_ptr() and len(f.allocs) == 2
    assert f.get(100, stream=1) is a and f.get(40, stream=1) is a and f.get(1024, stream=1) is a, "up to the capacity: the same object"
    assert f.get(100, stream=2) is b and len(f.allocs) == 2
    assert f.arena.buffers == {(1, DEV): a, (2, DEV): b} and f.arena.high_water == {DEV: 1024}
    assert [n for n, *_ in f.allocs] == [1024, 1024], "a first request gets the floor"


def test_growth_of_an_unheld_buffer_releases_it():
    f = Fake()
    f.get(100)
    big = f.get(5000)
    assert big.numel() >= 5000 and f.arena.buffers[(1, DEV)] is big and f.arena.retired == () and not f.arena.is_held((1, DEV))
    assert f.alive() == [False, True], "nobody captured on the old buffer: the allocator gets it back"


def test_growth_of_a_held_buffer_retires_it():
    f = Fake()
    old = f.get(100)
    f.arena.reserve(stream(1))
    assert f.arena.is_held((1, DEV)) and f.arena.buffers[(1, DEV)] is old and len(f.allocs) == 1, "large enough already: reserve keeps it"
    ptr = old.data_ptr()
    del old
    big = f.get(5000)
    assert f.arena.buffers[(1, DEV)] is big and big.data_ptr() != ptr
    assert [t.data_ptr() for t in f.arena.retired] == [ptr] and f.alive() == [True, True], "an address a graph may hold stays allocated"
    assert f.arena.under_capture == 0


def test_reserve_sizes_to_the_high_water_mark_outside_the_capture():
    f = Fake()
    f.arena.reserve(stream(9))
    assert f.allocs == [] and f.arena.buffers == {}, "nothing on the device has asked: nothing is allocated"
    f.get(100, stream=1)
    f.get(3000, stream=2)
    f.get(200, stream=1)
    assert f.arena.high_water == {DEV: 3000}
    n = len(f.allocs)
    f.capturing = False
    f.arena.reserve(stream(7))
    assert len(f.allocs) == n + 1 and f.allocs[-1][:3] == (4096, DEV, False), "the mark, rounded up to a power of two, not the floor"
    buf = f.arena.buffers[(7, DEV)]
    assert f.arena.is_held((7, DEV))
    assert f.get(3000, stream=7, capturing=True) is buf and f.get(100, stream=7, capturing=True) is buf
    assert len(f.allocs) == n + 1 and f.arena.under_capture == 0, "requests up to the mark allocate nothing under capture"


def test_reserve_grows_a_held_buffer_by_retiring_it():
    f = Fake(floor=256)
    f.get(100, stream=1)
    f.arena.reserve(stream(7))                     # 256 bytes (the mark is 100)
    first = f.arena.buffers[(7, DEV)]
    f.get(2000, stream=1)
    f.arena.reserve(stream(7))
    assert f.arena.buffers[(7, DEV)].numel() == 2048 and [t.data_ptr() for t in f.arena.retired] == [first.data_ptr()]


def test_a_miss_under_capture_falls_back_holds_and_counts():
    f = Fake()
    buf = f.get(100, stream=3, capturing=True)
    assert f.allocs[-1][:3] == (1024, DEV, True) and f.arena.is_held((3, DEV)) and f.arena.under_capture == 1
    assert f.get(100, stream=3, capturing=True) is buf and f.arena.under_capture == 1
    big = f.get(5000, stream=3, capturing=True)    # growth under capture: the graph may already hold the first address
    assert big is not buf and f.arena.under_capture == 2 and [t.data_ptr() for t in f.arena.retired] == [buf.data_ptr()]
    eager = f.get(100, stream=4)                   # growth under capture of a buffer that was not held
    assert f.get(5000, stream=4, capturing=True) is not eager and f.arena.is_held((4, DEV))
    assert eager.data_ptr() in [t.data_ptr() for t in f.arena.retired] and f.arena.under_capture == 3


@pytest.mark.parametrize("nbytes", [1, 4 * 33, 8 * 7, 1025, 4 * (1 << 10) + 4])
def test_dtype_views_are_aligned(nbytes):
    f = Fake(floor=8)
    buf = f.get(nbytes)
    assert buf.dtype == torch.uint8 and buf.numel() >= nbytes and buf.numel() % ALIGN == 0 and buf.data_ptr() % ALIGN == 0
    f32, i64 = buf.view(torch.float32), buf.view(torch.int64)
    assert f32.data_ptr() % 16 == 0 and f32.numel() == buf.numel() // 4 and i64.data_ptr() % 8 == 0 and i64.numel() == buf.numel() // 8


def test_an_unaligned_allocator_is_refused():
    raw = torch.empty(4096, dtype=torch.uint8)
    off = (-raw.data_ptr()) % ALIGN + 8
    arena = ScratchArena(alloc=lambda nbytes, device: raw[off:off + nbytes], stream_key=lambda: 1, capturing=lambda: False)
    with pytest.raises(AssertionError, match="unaligned"):
        arena.get(64, DEV)
