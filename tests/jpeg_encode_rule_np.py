"""The JPEG encoder as a numpy rule: encode(frame, quality, restart_rows) -> the bytes of the baseline 4:2:0 file, the truth the host
program around csrc/jpeg_encode_core.h and the device (include/vla_jpeg_encode.h) are compared with - and itself compared, whole, with
the file Pillow saves (tests/test_jpeg_encode_cpu.py).

It is the quantised coefficients of tests/policy_image_rule_np.py coded with the helpers of tests/jpeg_writer.py - block_symbols,
code_table, _BitWriter, _header with an explicit layout - and the four standard Huffman tables (T.81 Annex K.3), which are read from a
file Pillow wrote.  jpeg_writer.write is not called: its BOUND is about decode truth and refuses noise.

corpus() is the set of frames the encoder is pinned on, and statistics() what the rule's own symbols say about a frame: the conditions
the corpus must meet (a category-11 DC difference, ZRL, a block without EOB, ten MCU rows, a stuffed byte) are asserted from them."""
import functools
import io

import numpy as np
from PIL import Image

from tests import jpeg_rule_np as R
from tests import jpeg_writer as JW
from tests import policy_image_rule_np as P

QUALITIES = (1, 50, 95, 100)
LAYOUT = [("JFIF",), ("DQT", [0]), ("DQT", [1]), ("SOF",), ("DHT", [(0, 0)]), ("DHT", [(1, 0)]), ("DHT", [(0, 1)]), ("DHT", [(1, 1)]), ("DRI",)]


def pillow(frame: np.ndarray, quality: int, restart_rows: int = 1) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=int(quality), subsampling=2, restart_marker_rows=int(restart_rows))
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def standard_tables():
    """({id: (counts, vals)} DC, the same AC) of the tables Pillow writes by default, read from a file of its own."""
    p = R.parse(pillow(np.zeros((16, 16, 3), np.uint8), 75))
    dc = {i: JW.tables_from_codes(p["ht"][i]) for i in (0, 1)}
    ac = {i: JW.tables_from_codes(p["ht"][0x10 | i]) for i in (0, 1)}
    return dc, ac


def spec_of(H: int, W: int, quality: int, restart_rows: int) -> JW.Spec:
    dc, ac = standard_tables()
    q = {0: P.quant_table(P.LUMA, quality).reshape(64)[R.ZIGZAG].tolist(), 1: P.quant_table(P.CHROMA, quality).reshape(64)[R.ZIGZAG].tolist()}
    return JW.Spec(H=H, W=W, h2v2=True, qtables=q, dc_tables=dc, ac_tables=ac, restart=restart_rows * (W // 16), layout=LAYOUT)


def quantised(frame: np.ndarray, quality: int):
    st = {}
    P.jpeg_round_trip(frame, quality, st)
    return st["quantised"]


def encode(frame: np.ndarray, quality: int = 95, restart_rows: int = 1, stats: dict = None) -> bytes:
    """uint8 [H, W, 3], H and W multiples of 16 -> the file.  ``stats``, when given, receives what statistics() reports."""
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and restart_rows >= 1
    H, W = frame.shape[:2]
    spec, blocks = spec_of(H, W, quality, restart_rows), quantised(frame, quality)
    dc = [JW.code_table(*spec.dc_tables[spec.comp_td[c]]) for c in range(3)]
    ac = [JW.code_table(*spec.ac_tables[spec.comp_ta[c]]) for c in range(3)]
    total, per = JW.n_mcus(spec), spec.restart
    scan, st = b"", dict(max_dc_category=0, zrl=0, blocks=0, blocks_without_eob=0, stuffed=0, mcu_rows=H // 16, intervals=0, max_mcu_bytes=0.0)
    for i, m0 in enumerate(range(0, total, per)):
        if i:
            scan += bytes([0xFF, 0xD0 + (i - 1) % 8])
        w, pred = JW._BitWriter(), [0, 0, 0]
        m1 = min(m0 + per, total)
        for mcu in range(m0, m1):
            for c, blk, _ in JW.mcu_blocks(spec, blocks, mcu):
                syms, pred[c] = JW.block_symbols(blk, pred[c])
                st["blocks"] += 1
                st["max_dc_category"] = max(st["max_dc_category"], syms[0][1])
                st["zrl"] += sum(1 for a, s, _, _ in syms if a and s == 0xF0)
                st["blocks_without_eob"] += int(not (syms[-1][0] and syms[-1][1] == 0))
                for is_ac, s, extra, nbits in syms:
                    length, code = (ac if is_ac else dc)[c][s]
                    w.put(code, length)
                    w.put(extra, nbits)
        data = w.flush()
        st["stuffed"] += data.count(b"\xff\x00")
        st["intervals"] += 1
        st["max_mcu_bytes"] = max(st["max_mcu_bytes"], len(data) / (m1 - m0))
        scan += data
    if stats is not None:
        stats.update(st)
    return JW._header(spec) + scan + JW.EOI


def statistics(frame: np.ndarray, quality: int, restart_rows: int = 1) -> dict:
    st = {}
    encode(frame, quality, restart_rows, st)
    return st


# ---------------------------------------------------------------------------------------------------------------- the corpus
def noise(H: int, W: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 * seed + 7 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def checkerboard(H: int, W: int) -> np.ndarray:
    """Black and white 8 x 8 squares: the DC value swings between the two ends of its range from block to block."""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((y // 8 + x // 8) % 2) * 255).astype(np.uint8)[..., None], 3, -1)


def dots(H: int, W: int) -> np.ndarray:
    """The highest frequency in both directions: one white pixel in four."""
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((y % 2) * (x % 2)) * 255).astype(np.uint8)[..., None], 3, -1)


def gradient(H: int, W: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], -1).astype(np.uint8)


def band_limited(H: int, W: int) -> np.ndarray:
    return np.ascontiguousarray(P.band_limited(3, max(H, W))[:H, :W])


KINDS = {"noise": noise, "checkerboard": checkerboard, "dots": dots, "gradient": gradient, "band_limited": band_limited}


def frame(kind: str, H: int, W: int) -> np.ndarray:
    return KINDS[kind](H, W)


@functools.lru_cache(maxsize=None)
def corpus():
    """{name: uint8 [H, W, 3]}: noise at 32 x 48, 160 x 16 and 224 x 224, and one frame of every other kind."""
    out = {f"noise-{H}x{W}": noise(H, W, seed) for H, W, seed in ((32, 48, 0), (160, 16, 1), (224, 224, 0))}       # (seed 1: no block has an EOB)
    out.update({"checkerboard-32x48": checkerboard(32, 48), "dots-32x48": dots(32, 48), "gradient-64x32": gradient(64, 32),
                "band_limited-64x64": band_limited(64, 64)})
    return out


def mixed_frames(N: int, H: int, W: int) -> np.ndarray:
    """uint8 [N, H, W, 3]: the kinds of the corpus in turn at one shape (the device tests take N = 5: one of each)."""
    kinds = list(KINDS)
    return np.stack([noise(H, W, seed=n) if kinds[n % len(kinds)] == "noise" else frame(kinds[n % len(kinds)], H, W) for n in range(N)])
