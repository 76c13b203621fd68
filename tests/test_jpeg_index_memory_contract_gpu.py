"""The memory contract of the scan-index entry points (include/vla_jpeg_index.h), by the procedure of
tests/test_jpeg_memory_contract_gpu.py: each runs on compact operands and then with every device operand a view inside a poisoned
arena (tests/arena.py) at the minimum alignment its host check accepts - out_frames with a stride between its images that is larger
than an image; outputs must be bit-equal, inputs unchanged, and nothing written outside the declared extent.  The build writes
exactly the rows and the status of its slice; the decode exactly out_frames and status.  Then the hostile tables that passed the
sanitized host program (tests/test_jpeg_index_cpu.py) go through both kernels inside arenas: nothing outside is touched and every
word written lies inside the store."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as JC
from tests import jpeg_index_cases as IC
from tests.test_memory_contract_gpu import I32, I64, U8, call, case_for, contract
from vla_adapter_amd import jpeg_store as JS
from vla_adapter_amd import ops

COVERED = {}
EXEMPT = {}                      # both entry points have a device footprint
H, W, N_IMG, LENGTHS = 32, 48, 2, (1, 3)
SEG_POISON, ENT_POISON, ST_POISON = 5, 0x01010101, 0x7F


case = case_for(COVERED)


def store(h2v2):
    """Eight files of the matrix (with and without restart markers, four table sets) as a store of two images per step."""
    cases = JC.stores_of_the_matrix()[(H, W, h2v2)]
    T = sum(LENGTHS)
    files = [c[3] for c in cases][:T * N_IMG]
    want = np.stack([c[4] for c in cases][:T * N_IMG]).reshape(T, N_IMG, H, W, 3)
    ix = JS.parse_frames(*(JC.pack(files, N_IMG, H, W)[k] for k in JS.JPEG_KEYS))
    return files, want, ix, torch.from_numpy(np.frombuffer(b"".join(files), dtype=np.uint8).copy())


def store_inputs(mk, ix, data):
    return (mk.inp(data, align=1, name="bytes"), mk.inp(torch.from_numpy(ix.img_seg), align=8, poison=0, name="img_seg"),
            mk.inp(torch.from_numpy(ix.seg_tab), align=8, poison=5, name="seg_tab"), mk.inp(torch.from_numpy(ix.img_tab), align=4, poison=1, name="img_tab"),
            mk.inp(torch.from_numpy(ix.qt_pool.view(np.int16)), align=2, poison=3, name="qt_pool"), mk.inp(torch.from_numpy(ix.ht_pool), align=4, poison=0x101, name="ht_pool"))


def build_call(mk, ix, data, plan, pm, s0, s1, mapping):
    piece_off, _, S2, _ = plan
    S = ix.seg_tab.shape[0]
    by, img_seg, seg_tab, img_tab, qt, ht = store_inputs(mk, ix, data)
    po = mk.inp(torch.from_numpy(np.ascontiguousarray(piece_off)), align=8, poison=0, name="piece_off")
    seg2 = mk.out((S2, 4), I64, align=8, poison=SEG_POISON, name="out_seg_tab")
    ent2 = mk.out((S2, 4), I32, align=4, poison=ENT_POISON, name="out_seg_ent")
    st = mk.out((S,), U8, align=1, poison=ST_POISON, name="out_status")
    call("vla_jpeg_index_build", by, data.numel(), img_seg, seg_tab, S, img_tab, qt, ix.qt_pool.shape[0], ht, ix.ht_pool.shape[0], ix.N, H, W, ix.h2v2, pm,
         po, s0, s1, mapping, seg2, ent2, S2, st)
    return (by, img_seg, seg_tab, img_tab, qt, ht), seg2, ent2, st


@case("vla_jpeg_index_build")
@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("h2v2", [1, 0], ids=["420", "444"])
def test_jpeg_index_build_contract(h2v2, mapping):
    files, _, ix, data = store(h2v2)
    S, pm = ix.seg_tab.shape[0], 2
    plan = JS.plan_pieces(ix, pm)
    piece_off, S2 = plan[0], plan[2]
    s0, s1 = 1, S - 2                                           # a slice strictly inside the store
    assert S2 > S >= 8

    def body(mk):
        _, seg2, ent2, st = build_call(mk, ix, data, plan, pm, s0, s1, mapping)
        return {"out_seg_tab": seg2, "out_seg_ent": ent2, "out_status": st}

    rc, _ = contract(body)
    seg2, ent2, st = (rc[k].cpu().numpy() for k in ("out_seg_tab", "out_seg_ent", "out_status"))
    r0, r1 = int(piece_off[s0]), int(piece_off[s1])
    want_seg, want_ent = IC.rule_tables(files, ix, pm)
    assert np.array_equal(seg2[r0:r1], want_seg[r0:r1]) and np.array_equal(ent2[r0:r1], want_ent[r0:r1]) and not st[s0:s1].any()
    for rows in (slice(0, r0), slice(r1, S2)):                  # exactly the slice's rows and status
        assert (seg2[rows] == SEG_POISON).all() and (ent2[rows] == ENT_POISON).all()
    assert (st[:s0] == ST_POISON).all() and (st[s1:] == ST_POISON).all()


@case("vla_jpeg_decode_rows_at")
@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
@pytest.mark.parametrize("h2v2, align, pad", [(1, 4, 8), (1, 1, 7), (0, 1, 1)], ids=["420-words", "420-bytes", "444-bytes"])
def test_jpeg_decode_rows_at_contract(h2v2, align, pad, mapping):
    files, want, ix, data = store(h2v2)
    pm = 2
    _, img_seg2, S2, max_seg2 = JS.plan_pieces(ix, pm)
    seg2, ent2 = IC.rule_tables(files, ix, pm)
    T, B, image = sum(LENGTHS), 5, H * W * 3
    n_ws = ops.jpeg_workspace_bytes(B * N_IMG, H, W, h2v2)
    eps, rows = [0, 1, 1, 0, 1], [0, 3, 2, -3, 99]              # (two of them out of range: clamped to rows 0 and 3)

    def body(mk):
        by, _, _, img_tab, qt, ht = store_inputs(mk, ix, data)
        img_seg = mk.inp(torch.from_numpy(np.ascontiguousarray(img_seg2)), align=8, poison=0, name="img_seg")
        seg_tab = mk.inp(torch.from_numpy(seg2), align=8, poison=5, name="seg_tab")
        seg_ent = mk.inp(torch.from_numpy(ent2), align=4, poison=3, name="seg_ent")
        eo = mk.inp(torch.tensor(np.cumsum((0,) + LENGTHS), dtype=I64), align=8, poison=1, name="episode_off")
        ep, row = mk.inp(torch.tensor(eps, dtype=I32), align=4, poison=0, name="ep"), mk.inp(torch.tensor(rows, dtype=I64), align=8, poison=0, name="row")
        ws = mk.out((n_ws,), U8, align=16, name="workspace")
        out = mk.out((B * N_IMG, image), U8, strides=(image + pad, 1), align=align, name="out_frames")
        status = mk.out((B, N_IMG, max_seg2), U8, align=1, name="status")
        call("vla_jpeg_decode_rows_at", by, data.numel(), img_seg, seg_tab, seg_ent, S2, img_tab, qt, ix.qt_pool.shape[0], ht, ix.ht_pool.shape[0],
             eo, len(LENGTHS), T, ep, row, B, N_IMG, H, W, h2v2, max_seg2, mapping, ws, n_ws, out, out.stride(0), status)
        return {"frames_u8": out, "status": status}

    rc, _ = contract(body)
    assert not rc["status"].any() and S2 > ix.seg_tab.shape[0] and ent2.any()
    got = rc["frames_u8"].cpu().numpy().reshape(B, N_IMG, H, W, 3)
    assert np.array_equal(got, want[[0, 3, 2, 0, 3]])


@case("vla_jpeg_index_build", "vla_jpeg_decode_rows_at")
@pytest.mark.parametrize("mapping", [0, 1], ids=["lane-per-segment", "wave-per-segment"])
def test_hostile_tables_give_in_range_results(mapping):
    """The variants of tests/jpeg_index_cases.py: hostile_variants - lo / hi / MCU ranges / pool ids / img_seg out of range, piece_off
    non-monotone and past S' - through the build, and what it wrote, under an entry table of bit 255 and predictors at the int32
    extremes, through the decode.  Inputs unchanged, nothing outside the outputs written, every table word written inside the store
    and the image.  (Rows that two segments both own under a non-monotone piece_off hold either one's words: the two runs are not
    compared.)"""
    files, _, ix, data = store(1)
    pm, n_bytes = 1, int(data.numel())
    B, T, image = 4, sum(LENGTHS), H * W * 3
    n_ws = ops.jpeg_workspace_bytes(B * N_IMG, H, W, 1)
    variants = IC.hostile_variants(ix, pm)
    assert len(variants) >= 7
    for name, v, plan in variants:
        _, img_seg2, S2, max_seg2 = plan

        def body(mk):
            (by, _, _, img_tab, qt, ht), seg2, ent2, st = build_call(mk, v, data, plan, pm, 0, v.seg_tab.shape[0], mapping)
            seg_w = seg2.clone()
            ent_h = torch.empty_like(ent2)                      # the entry table the decode gets: hostile
            ent_h[:, 0], ent_h[:, 1], ent_h[:, 2], ent_h[:, 3] = 255, -2 ** 31, 2 ** 31 - 1, -2 ** 31
            ent_h[1::2, 1] = 2 ** 31 - 1
            ent_in = mk.inp(ent_h, align=4, poison=3, name="seg_ent")
            img_seg = mk.inp(torch.from_numpy(np.ascontiguousarray(img_seg2)), align=8, poison=0, name="img_seg (pieces)")
            seg_in = mk.inp(seg_w, align=8, poison=5, name="seg_tab (pieces)")
            eo = mk.inp(torch.tensor(np.cumsum((0,) + LENGTHS), dtype=I64), align=8, poison=1, name="episode_off")
            ep, row = mk.inp(torch.tensor([0, 1, 1, 1], dtype=I32), align=4, poison=0, name="ep"), mk.inp(torch.tensor([0, 1, 2, 3], dtype=I64), align=8, poison=0, name="row")
            ws = mk.out((n_ws,), U8, align=16, name="workspace")
            out = mk.out((B * N_IMG, image), U8, strides=(image + 8, 1), align=4, name="out_frames")
            status = mk.out((B, N_IMG, max_seg2), U8, align=1, name="status")
            call("vla_jpeg_decode_rows_at", by, data.numel(), img_seg, seg_in, ent_in, S2, img_tab, qt, v.qt_pool.shape[0], ht, v.ht_pool.shape[0],
                 eo, len(LENGTHS), T, ep, row, B, N_IMG, H, W, 1, max_seg2, mapping, ws, n_ws, out, out.stride(0), status)
            return {"out_seg_tab": seg2, "out_seg_ent": ent2, "out_status": st, "frames_u8": out, "status": status}

        rc, ra = contract(body, inexact=("out_seg_tab", "out_seg_ent", "out_status", "frames_u8", "status"))
        for r in (rc, ra):
            seg, ent, st, status = (r[k].cpu().numpy() for k in ("out_seg_tab", "out_seg_ent", "out_status", "status"))
            w = seg[(seg != SEG_POISON).any(1) | (ent != ENT_POISON).any(1)]
            assert w.shape[0] >= 1, name
            assert (w[:, 0] >= 0).all() and (w[:, 0] <= w[:, 1]).all() and (w[:, 1] <= n_bytes).all(), f"{name}: byte ranges inside the store"
            assert (w[:, 2] >= 0).all() and (w[:, 2] <= w[:, 3]).all() and (w[:, 3] <= v.mcus).all(), f"{name}: MCU ranges inside the image"
            e = ent[(ent != ENT_POISON).any(1)]
            assert (e[:, 0] >= 0).all() and (e[:, 0] <= 7).all(), f"{name}: entry bits inside a byte"
            assert (st <= 3).all() and (status <= 3).all(), f"{name}: every status is one of the four"
