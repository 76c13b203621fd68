"""The memory contract of the entry points of include/vla_jpeg_encode.h, by the procedure of tests/test_memory_contract_gpu.py: the two
calls of an encode run on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the
minimum alignment its host check accepts - the frames with a stride between the images that is larger than an image, `out` of exactly
frame_off[N] bytes; the files and offsets must be bit-equal (and Pillow's), the inputs unchanged, and nothing written outside the
declared extents, the workspace included.  Both load arms of the MCU stage run (16-byte words; bytes: a 1-byte aligned base and an odd
stride), and an `out` one byte short of the files keeps the bytes in front and takes no write behind its end."""
import numpy as np
import pytest
import torch

from tests import jpeg_encode_rule_np as E
from tests.test_memory_contract_gpu import U8, call, case_for, contract
from vla_adapter_amd import input_stage as IS
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {"vla_jpeg_encode_workspace_bytes": "host arithmetic only: it takes no pointer"}
I64 = torch.int64

case = case_for(COVERED)


def pillow_store(frames, quality, restart_rows):
    files = [E.pillow(f, quality, restart_rows) for f in frames]
    return np.frombuffer(b"".join(files), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)


@case("vla_jpeg_encode_plan", "vla_jpeg_encode_write")
@pytest.mark.parametrize("short", [0, 1], ids=["whole", "one-byte-short"])
@pytest.mark.parametrize("align_in, pad_in, restart_rows", [(16, 16, 1), (1, 7, 1), (16, 32, 2)], ids=["words", "bytes", "words-r2"])
def test_jpeg_encode_contract(align_in, pad_in, restart_rows, short):
    N, H, W, quality = 3, 48, 32, 100
    imgs = np.stack([E.noise(H, W, seed=3), E.frame("dots", H, W), E.frame("checkerboard", H, W)])
    image = H * W * 3
    n_ws = ops._lib().vla_jpeg_encode_workspace_bytes(N, H, W, restart_rows)
    qtab = torch.from_numpy(IS.jpeg_quant_tables(quality).view(np.int16).copy())
    want, want_off = pillow_store(imgs, quality, restart_rows)
    total = int(want_off[-1]) - short

    def body(mk):
        fr = mk.inp(torch.from_numpy(imgs).view(N, image), strides=(image + pad_in, 1), align=align_in, name="frames")
        q = mk.inp(qtab, align=2, poison=1, name="qtab")
        ws = mk.out((n_ws,), U8, align=16, name="workspace")
        off = mk.out((N + 1,), I64, align=8, poison=1 << 40, name="frame_off")
        out = mk.out((total,), U8, align=1, name="out")
        call("vla_jpeg_encode_plan", fr, fr.stride(0), N, H, W, q, restart_rows, ws, n_ws, off)
        call("vla_jpeg_encode_write", N, H, W, q, restart_rows, ws, n_ws, off, out, total)
        return {"frame_off": off, "out": out}

    rc, _ = contract(body)
    assert rc["frame_off"].cpu().tolist() == want_off.tolist()
    assert np.array_equal(rc["out"].cpu().numpy(), want[:total])
