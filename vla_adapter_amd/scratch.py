"""Kernel scratch: one byte buffer per (stream, device) for the fp32 planes of a split product and the digest's partial sums.

THE rule of DESIGN section 13, for scratch: a captured graph holds the address of the scratch it was captured on, so that address stays
allocated.  (A) schedule.graph_capture calls reserve(stream) before it enters a capture: the stream's buffer is allocated outside the
capture, sized to the largest request the device has seen (the warm-up has just run the same calls), and marked held.  (B) a held
buffer that has to grow is retired, not released.  A buffer nobody captured on grows by replacement.
"""
from __future__ import annotations

import torch

ALIGN = 256            # base and capacity of every buffer: a multiple of this, so that every dtype view of one is aligned


def _torch_alloc(nbytes: int, device) -> torch.Tensor:
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def _torch_stream_key() -> int:
    return torch.cuda.current_stream().cuda_stream


class ScratchArena:
    """get(nbytes, device) -> the current stream's uint8 buffer of at least nbytes (streams overlap, so each has its own; the uses on
    one stream are ordered by it).  alloc(nbytes, device), stream_key() -> the current stream's handle and capturing() -> whether
    that stream is being captured are the torch calls unless given (tests)."""

    floor = 16 << 20   # bytes of a buffer on its first request (the smaller of the two floors the split products had)

    def __init__(self, alloc=_torch_alloc, stream_key=_torch_stream_key, capturing=torch.cuda.is_current_stream_capturing):
        self._alloc, self._stream_key, self._capturing = alloc, stream_key, capturing
        self._ents = {}            # (stream handle, device) -> (buffer, largest request it has served)
        self._held = set()         # keys whose buffer a captured graph may address
        self._retired = []         # held buffers that were outgrown: kept for the life of the process
        self._high_water = {}      # device -> largest request in bytes
        self.under_capture = 0     # allocations made while capturing (a capture that went around schedule.graph_capture)

    def get(self, nbytes: int, device) -> torch.Tensor:
        key = (self._stream_key(), str(device))
        ent = self._ents.get(key)
        if ent is None or ent[1] < nbytes:
            ent = self._larger_request(key, nbytes, device)
        return ent[0]

    def _larger_request(self, key, nbytes: int, device):
        self._high_water[key[1]] = max(self._high_water.get(key[1], 0), nbytes)
        ent = self._ents.get(key)
        buf = ent[0] if ent is not None and ent[0].numel() >= nbytes else self._replace(key, max(nbytes, self.floor), device)
        self._ents[key] = (buf, nbytes)
        return self._ents[key]

    def _replace(self, key, nbytes: int, device) -> torch.Tensor:
        if self._capturing():      # the graph being captured records this address, and those the old buffer handed it
            self.under_capture += 1
            self._held.add(key)
        if key in self._held and key in self._ents:
            self._retired.append(self._ents[key][0])
        buf = self._alloc(-(-nbytes // ALIGN) * ALIGN, device)
        assert buf.data_ptr() % ALIGN == 0 and buf.numel() % ALIGN == 0, "scratch: the allocator returned an unaligned buffer"
        return buf

    def reserve(self, stream) -> None:
        """Before ``stream`` captures: its buffer covers the device's high-water mark, was allocated here, and is held from now on.
        Sized to the mark rounded up to a power of two, not to the floor: a capture stream that never asks (vision) costs what the
        largest split product needs and no more, a stream whose captures grow retires less than it ends up holding, and while nothing
        on the device has asked nothing is allocated."""
        dev = str(stream.device)
        key, want = (stream.cuda_stream, dev), self._high_water.get(dev, 0)
        ent = self._ents.get(key)
        if want and (ent is None or ent[0].numel() < want):
            self._ents[key] = (self._replace(key, 1 << (want - 1).bit_length(), dev), want)
        self._held.add(key)

    # ---- read-only views (tests)
    @property
    def buffers(self) -> dict:
        return {key: ent[0] for key, ent in self._ents.items()}

    @property
    def high_water(self) -> dict:
        return dict(self._high_water)

    @property
    def retired(self) -> tuple:
        return tuple(self._retired)

    def is_held(self, key) -> bool:
        return key in self._held


ARENA = ScratchArena()
