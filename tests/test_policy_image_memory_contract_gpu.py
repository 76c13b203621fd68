"""The memory contract of the entry points of include/vla_policy_image.h, by the procedure of tests/test_memory_contract_gpu.py: each
call runs on compact operands and then with every device operand a view inside a poisoned arena (tests/arena.py) at the minimum
alignment its host check accepts - the frames with a stride between the images that is larger than an image; outputs must be
bit-equal (and equal to the numpy rule), inputs unchanged, and nothing written outside the declared extents, the workspace
included.  Both load arms of the forward kernel run (16-byte words: frames 16-byte aligned with a stride that is a multiple of 16;
bytes: a 1-byte aligned base and an odd stride), both store arms of stage B's pixel kernel, and all three shapes of the resize (two
passes through the float32 intermediate, the horizontal pass alone, the vertical pass alone)."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import policy_image_rule_np as P
from tests.test_memory_contract_gpu import F32, I32, U8, call, case_for, contract
from vla_adapter_amd import input_stage as IS
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {"vla_policy_image_workspace_bytes": "host arithmetic only: it takes no pointer"}
I16 = torch.int16


case = case_for(COVERED)


def frames_of(N, H, W):
    return np.stack([JC.content("noise", H, W, seed=s) for s in range(N - 1)] + [JC.content("saturated", H, W)])


@case("vla_policy_jpeg_round_trip")
@pytest.mark.parametrize("align_in, pad_in, align_out, pad_out", [(16, 16, 4, 8), (1, 7, 1, 5), (16, 32, 1, 1)], ids=["words", "bytes", "words-in-bytes-out"])
def test_policy_jpeg_round_trip_contract(align_in, pad_in, align_out, pad_out):
    N, H, W, quality = 3, 32, 48, 95
    imgs = frames_of(N, H, W)
    image = H * W * 3
    n_ws = ops._lib().vla_policy_image_workspace_bytes(N, H, W, 0, 0, 1)
    qtab = torch.from_numpy(IS.jpeg_quant_tables(quality).view(np.int16).copy())

    def body(mk):
        fr = mk.inp(torch.from_numpy(imgs).view(N, image), strides=(image + pad_in, 1), align=align_in, name="frames")
        q = mk.inp(qtab, align=2, poison=1, name="qtab")
        ws = mk.out((n_ws,), U8, align=16, name="workspace")
        out = mk.out((N, image), U8, strides=(image + pad_out, 1), align=align_out, name="out_frames")
        call("vla_policy_jpeg_round_trip", fr, fr.stride(0), N, H, W, q, ws, n_ws, out, out.stride(0))
        return {"out_frames": out}

    rc, _ = contract(body)
    want = np.stack([P.jpeg_round_trip(a, quality) for a in imgs])
    assert np.array_equal(rc["out_frames"].cpu().numpy().reshape(N, H, W, 3), want)


@case("vla_policy_lanczos3_resize")
@pytest.mark.parametrize("H, W, oh, ow", [(32, 48, 24, 40), (48, 32, 48, 24), (32, 48, 40, 48), (5, 7, 3, 4)],
                         ids=["two-passes", "horizontal-only", "vertical-only", "5x7-to-3x4"])
def test_policy_lanczos3_resize_contract(H, W, oh, ow):
    N = 3
    imgs = frames_of(N, H, W)
    image = H * W * 3
    n_ws = ops._lib().vla_policy_image_workspace_bytes(N, H, W, oh, ow, 0)
    assert n_ws == (N * oh * W * 3 * 4 if (H != oh and W != ow) else 0)
    sv, sh = (IS.tf_lanczos3_spans(H, oh) if H != oh else None), (IS.tf_lanczos3_spans(W, ow) if W != ow else None)

    def body(mk):
        fr = mk.inp(torch.from_numpy(imgs).view(N, image), strides=(image + 5, 1), align=1, name="frames")
        tabs = []
        for tag, sp in (("v", sv), ("h", sh)):
            if sp is None:
                tabs += [None, None, 0]
            else:                                           # (poison: a start far outside the source, a weight that would show)
                tabs += [mk.inp(torch.from_numpy(sp[0].copy()), align=4, poison=1 << 20, name=f"starts_{tag}"),
                         mk.inp(torch.from_numpy(sp[1].copy()), align=4, poison=1e6, name=f"weights_{tag}"), sp[1].shape[1]]
        ws = mk.out((max(n_ws, 4),), U8, align=4, name="workspace")
        out = mk.out((N, oh, ow, 3), U8, align=1, name="out")
        call("vla_policy_lanczos3_resize", fr, fr.stride(0), N, H, W, oh, ow, *tabs, ws, n_ws, out)
        return {"out": out} if n_ws else {"out": out, "workspace_untouched": ws}

    rc, _ = contract(body)
    want = np.stack([P.tf_lanczos3_resize(a, oh, ow) for a in imgs])
    assert np.array_equal(rc["out"].cpu().numpy(), want)
    if not n_ws:
        assert (rc["workspace_untouched"] == 0x7F).all(), "a single pass goes from u8 to u8: the workspace is not written"
