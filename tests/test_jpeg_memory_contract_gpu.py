"""The memory contract of the JPEG entry points (include/vla_jpeg.h), by the procedure of tests/test_memory_contract_gpu.py: the decode
runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum alignment
its host check accepts - out_frames with a stride between its images that is larger than an image; outputs must be bit-equal, inputs
unchanged, and nothing written outside the declared extent.  Both store arms of the pixel kernel run: words (out_frames 4-byte
aligned, stride a multiple of 4) and bytes (a 1-byte aligned base, an odd stride); both lane mappings; both samplings."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests.test_memory_contract_gpu import DEV, I32, I64, U8, call, case_for, contract
from vla_adapter_amd import jpeg_store as JS
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {"vla_jpeg_workspace_bytes": "host arithmetic only: it takes no pointer"}


case = case_for(COVERED)


@case("vla_jpeg_decode_rows")
@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("h2v2, align, pad", [(1, 4, 8), (1, 1, 7), (0, 1, 1)], ids=["420-words", "420-bytes", "444-bytes"])
def test_jpeg_decode_rows_contract(h2v2, align, pad, mapping):
    H, W, n_img, lengths = 32, 48, 2, (1, 3)
    cases = JC.stores_of_the_matrix()[(H, W, h2v2)]
    T, B = sum(lengths), 5
    files = [c[3] for c in cases][:T * n_img]
    want = np.stack([c[4] for c in cases][:T * n_img]).reshape(T, n_img, H, W, 3)
    ix = JS.parse_frames(*(JC.pack(files, n_img, H, W)[k] for k in JS.JPEG_KEYS))
    data = torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy())
    image = H * W * 3
    n_ws = ops.jpeg_workspace_bytes(B * n_img, H, W, h2v2)
    eps, rows = [0, 1, 1, 0, 1], [0, 3, 2, -3, 99]              # (two of them out of range: clamped to rows 0 and 3)

    def body(mk):
        by = mk.inp(data, align=1, name="bytes")
        img_seg, seg_tab = mk.inp(torch.from_numpy(ix.img_seg), align=8, poison=0, name="img_seg"), mk.inp(torch.from_numpy(ix.seg_tab), align=8, poison=5, name="seg_tab")
        img_tab = mk.inp(torch.from_numpy(ix.img_tab), align=4, poison=1, name="img_tab")
        qt = mk.inp(torch.from_numpy(ix.qt_pool.view(np.int16)), align=2, poison=3, name="qt_pool")
        ht = mk.inp(torch.from_numpy(ix.ht_pool), align=4, poison=0x101, name="ht_pool")
        eo = mk.inp(torch.tensor(np.cumsum((0,) + lengths), dtype=I64), align=8, poison=1, name="episode_off")
        ep, row = mk.inp(torch.tensor(eps, dtype=I32), align=4, poison=0, name="ep"), mk.inp(torch.tensor(rows, dtype=I64), align=8, poison=0, name="row")
        ws = mk.out((n_ws,), U8, align=16, name="workspace")
        out = mk.out((B * n_img, image), U8, strides=(image + pad, 1), align=align, name="out_frames")
        status = mk.out((B, n_img, ix.max_seg), U8, align=1, name="status")
        stride = out.stride(0)
        call("vla_jpeg_decode_rows", by, data.numel(), img_seg, seg_tab, ix.seg_tab.shape[0], img_tab, qt, ix.qt_pool.shape[0], ht, ix.ht_pool.shape[0],
             eo, len(lengths), T, ep, row, B, n_img, H, W, h2v2, ix.max_seg, mapping, ws, n_ws, out, stride, status)
        return {"frames_u8": out, "status": status}

    rc, _ = contract(body)
    assert not rc["status"].any()
    got = rc["frames_u8"].cpu().numpy().reshape(B, n_img, H, W, 3)
    assert np.array_equal(got, want[[0, 3, 2, 0, 3]])
