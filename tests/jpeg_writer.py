"""A coefficient-level writer of baseline JPEG files for the tests (plain Python / numpy; not part of the package): it takes the
quantised coefficient blocks of the three components, in zigzag order, and a description of the file - tables, table and component
ids, sampling, restart interval, the layout of the header segments, fill and pad bytes - and writes a SOF0 file with byte stuffing and
1-bit padding as T.81 prescribes.  It makes the files no encoder writes (tests/jpeg_cases.py: crafted_corpus): Huffman tables of any
legal shape, blocks of any structure, headers in any order.

The truth for every file is Pillow's decode of it, and that is only unambiguous while libjpeg's C and SIMD inverse DCTs agree: while
no IDCT output leaves [-512, 511], where the range-limit table clamps without wrapping.  An output is at most a quarter of the sum of
|coefficient x quantiser| of its block, so ``write`` asserts that sum <= BOUND = 2000 for every block: a condition on the inputs, not
a tolerance.

tests/test_jpeg_cpu.py pins the writer: every crafted file decodes under tests/jpeg_rule_np.py to Pillow's pixels, and a Pillow file's
coefficients rewritten with its own tables decode to the same pixels."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.jpeg_rule_np import ZIGZAG

BOUND = 2000
SOI, EOI = b"\xff\xd8", b"\xff\xd9"
JFIF = b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"


# ---------------------------------------------------------------------------------------------------------------- helpers
def _dct_matrix() -> np.ndarray:
    k, n = np.mgrid[0:8, 0:8]
    m = np.cos((2 * n + 1) * k * np.pi / 16) * 0.5
    m[0] /= np.sqrt(2)
    return m


def blocks_from_pixels(plane: np.ndarray, qtable) -> np.ndarray:
    """uint8 (or any integer) samples [h, w], h and w multiples of 8 -> int64 [h / 8, w / 8, 64]: the float64 forward DCT of the
    level-shifted 8 x 8 blocks, divided by the table (zigzag order) and rounded, in zigzag order."""
    h, w = plane.shape
    assert h % 8 == 0 and w % 8 == 0
    x = (plane.astype(np.float64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    m = _dct_matrix()
    f = (m @ x @ m.T).reshape(h // 8, w // 8, 64)[..., ZIGZAG]
    return np.rint(f / np.asarray(qtable, dtype=np.float64)).astype(np.int64)


def huffman_from_lengths(pairs: Sequence[Tuple[int, int]]):
    """[(symbol, code length 1 .. 16)] -> (counts [16], vals): a valid DHT table in which every symbol has the requested length;
    symbols of one length keep the order they are given in (the later, the larger the code).  Asserts that the lengths are
    Kraft-feasible with room to spare, which is what keeps the all-ones code of every length unused (T.81 Annex C)."""
    assert len({s for s, _ in pairs}) == len(pairs) and all(0 <= s <= 255 and 1 <= l <= 16 for s, l in pairs)
    assert sum(1 << (16 - l) for _, l in pairs) <= (1 << 16) - 1, "these code lengths do not fit a prefix code that leaves all-ones free"
    counts = [sum(1 for _, l in pairs if l == n) for n in range(1, 17)]
    vals = [s for n in range(1, 17) for s, l in pairs if l == n]
    return counts, vals


def code_table(counts, vals) -> Dict[int, Tuple[int, int]]:
    """{symbol: (length, code)} - the canonical codes of Annex C."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[vals[k]] = (l, code)
            code, k = code + 1, k + 1
        assert code <= 1 << l, "the counts overflow the code space"
        code <<= 1
    for s, (l, c) in out.items():
        assert c != (1 << l) - 1, f"symbol {s} has the all-ones code of length {l}"
    return out


def category(v: int) -> int:
    return int(abs(int(v))).bit_length()


def block_symbols(blk, pred: int, zrl_eob: bool = False):
    """One block (64 zigzag coefficients) -> ([(is_ac, symbol, extra bits, their count)], the new predictor): the DC difference,
    then runs and values with ZRL (0xF0) for every 16 zeros in front of a value and EOB (0x00) when zeros end the block.  zrl_eob:
    16 or more zeros at the end are coded as ZRL, EOB - legal, and what no encoder writes."""
    d = int(blk[0]) - pred
    s = category(d)
    assert s <= 11, "baseline DC differences have at most 11 bits"
    out = [(0, s, d if d >= 0 else d + (1 << s) - 1, s)]
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        s = category(v)
        assert 1 <= s <= 10, "baseline AC coefficients have at most 10 bits"
        out.append((1, (run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
        run = 0
    if run:
        out += [(1, 0xF0, 0, 0)] * bool(zrl_eob and run > 15) + [(1, 0x00, 0, 0)]
    return out, int(blk[0])


# ---------------------------------------------------------------------------------------------------------------- the description
@dataclass
class Spec:
    """What a file looks like apart from its coefficients.  ``layout`` lists what stands between SOI and SOS, in order:
         ("JFIF",)  ("ADOBE", transform)  ("APP", n, payload)  ("COM", payload)  ("FILL", n): n 0xFF bytes in front of the next marker
         ("DQT", [id, ...]) or ("DQT", [(id, table), ...])         one segment with these tables (an id alone: the spec's table)
         ("DHT", [(cls, id), ...]) or ("DHT", [(cls, id, counts, vals), ...])        cls 0: DC, 1: AC
         ("SOF",)  ("DRI",)
       None: JFIF, one DQT segment per table, SOF, one DHT segment per table, DRI when ``restart`` is not None."""
    H: int
    W: int
    h2v2: bool
    qtables: Dict[int, Sequence[int]]                   # id 0 .. 3 -> 64 values in zigzag order
    dc_tables: Dict[int, tuple]                         # id 0 .. 3 -> (counts, vals)
    ac_tables: Dict[int, tuple]
    comp_ids: Sequence[int] = (1, 2, 3)
    comp_tq: Sequence[int] = (0, 1, 1)
    comp_td: Sequence[int] = (0, 1, 1)
    comp_ta: Sequence[int] = (0, 1, 1)
    restart: Optional[int] = None                       # MCUs per restart interval; 0 writes DRI 0, None writes no DRI segment
    layout: Optional[List[tuple]] = None
    rst_fill: int = 0                                   # 0xFF fill bytes in front of every RSTn marker
    eoi_fill: int = 0                                   # and in front of EOI
    pad: bytes = b""                                    # between the last entropy-coded byte and EOI
    trailer: bytes = b""                                # behind EOI
    zrl_eob: tuple = ()                                 # (component, block row, block column) of blocks that end ZRL, EOB

    def default_layout(self):
        out = [("JFIF",)] + [("DQT", [i]) for i in sorted(self.qtables)] + [("SOF",)]
        out += [("DHT", [(0, i)]) for i in sorted(self.dc_tables)] + [("DHT", [(1, i)]) for i in sorted(self.ac_tables)]
        return out + ([("DRI",)] if self.restart is not None else [])


def _segment(marker: int, payload: bytes) -> bytes:
    assert len(payload) + 2 <= 0xFFFF
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _header(spec: Spec) -> bytes:
    out = SOI
    for item in (spec.layout if spec.layout is not None else spec.default_layout()):
        kind = item[0]
        if kind == "JFIF":
            out += _segment(0xE0, JFIF)
        elif kind == "ADOBE":
            out += _segment(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([item[1]]))
        elif kind == "APP":
            out += _segment(0xE0 + item[1], bytes(item[2]))
        elif kind == "COM":
            out += _segment(0xFE, bytes(item[1]))
        elif kind == "FILL":
            out += b"\xff" * item[1]
        elif kind == "DQT":
            body = b""
            for t in item[1]:
                i, tab = (t, spec.qtables[t]) if isinstance(t, int) else t
                assert 0 <= i <= 3 and len(tab) == 64 and all(1 <= int(q) <= 255 for q in tab)
                body += bytes([i]) + bytes(int(q) for q in tab)
            out += _segment(0xDB, body)
        elif kind == "DHT":
            body = b""
            for t in item[1]:
                cls, i = t[0], t[1]
                counts, vals = (t[2], t[3]) if len(t) == 4 else (spec.dc_tables, spec.ac_tables)[cls][i]
                assert 0 <= i <= 3 and len(counts) == 16 and sum(counts) == len(vals)
                body += bytes([(cls << 4) | i]) + bytes(counts) + bytes(vals)
            out += _segment(0xC4, body)
        elif kind == "SOF":
            samp = [0x22 if spec.h2v2 else 0x11, 0x11, 0x11]
            body = bytes([8]) + spec.H.to_bytes(2, "big") + spec.W.to_bytes(2, "big") + bytes([3])
            out += _segment(0xC0, body + b"".join(bytes([spec.comp_ids[c], samp[c], spec.comp_tq[c]]) for c in range(3)))
        elif kind == "DRI":
            out += _segment(0xDD, int(spec.restart or 0).to_bytes(2, "big"))
        else:
            raise ValueError(kind)
    sos = bytes([3]) + b"".join(bytes([spec.comp_ids[c], (spec.comp_td[c] << 4) | spec.comp_ta[c]]) for c in range(3)) + bytes([0, 63, 0])
    return out + _segment(0xDA, sos)


class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, bits: int):
        if bits:
            assert 0 <= value < (1 << bits)
            self.acc, self.n = (self.acc << bits) | value, self.n + bits
            while self.n >= 8:
                self.n -= 8
                b = (self.acc >> self.n) & 0xFF
                self.out.append(b)
                if b == 0xFF:
                    self.out.append(0)                  # byte stuffing (F.1.2.3)
            self.acc &= (1 << self.n) - 1

    def flush(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)           # 1-bit padding
        return bytes(self.out)


def mcu_blocks(spec: Spec, blocks, mcu: int):
    """[(component, its block, whether it ends ZRL, EOB)] of MCU `mcu` in coding order."""
    if spec.h2v2:
        my, mx = divmod(mcu, spec.W // 16)
        at = [(0, 2 * my + dy, 2 * mx + dx) for dy in (0, 1) for dx in (0, 1)] + [(1, my, mx), (2, my, mx)]
    else:
        my, mx = divmod(mcu, spec.W // 8)
        at = [(c, my, mx) for c in range(3)]
    return [(c, blocks[c][y, x], (c, y, x) in spec.zrl_eob) for c, y, x in at]


def n_mcus(spec: Spec) -> int:
    return (spec.H // 16) * (spec.W // 16) if spec.h2v2 else (spec.H // 8) * (spec.W // 8)


def symbols_used(spec: Spec, blocks):
    """({DC symbol: count}, {AC symbol: count}) per component, [3] each - what the file's tables must hold."""
    dc, ac = [dict() for _ in range(3)], [dict() for _ in range(3)]
    per, pred = spec.restart or n_mcus(spec), [0, 0, 0]
    for mcu in range(n_mcus(spec)):
        if mcu % per == 0:
            pred = [0, 0, 0]
        for c, blk, ze in mcu_blocks(spec, blocks, mcu):
            syms, pred[c] = block_symbols(blk, pred[c], ze)
            for is_ac, s, _, _ in syms:
                d = (ac if is_ac else dc)[c]
                d[s] = d.get(s, 0) + 1
    return dc, ac


def write(spec: Spec, blocks) -> bytes:
    """blocks: [Y, Cb, Cr], integer arrays [block rows, block columns, 64] of quantised coefficients in zigzag order -> the file."""
    assert spec.H % 16 == 0 and spec.W % 16 == 0 and len(blocks) == 3
    bh, bw = spec.H // 8, spec.W // 8
    want = [(bh, bw, 64)] + [((bh // 2, bw // 2, 64) if spec.h2v2 else (bh, bw, 64))] * 2
    assert [tuple(b.shape) for b in blocks] == want, f"blocks of shapes {[b.shape for b in blocks]}, the frame needs {want}"
    for c in range(3):
        q = np.asarray(spec.qtables[spec.comp_tq[c]], dtype=np.int64)
        load = np.abs(np.asarray(blocks[c], dtype=np.int64) * q).sum(-1)
        assert load.max() <= BOUND, (f"component {c}: a block with sum |coefficient x quantiser| = {load.max()} > {BOUND}: libjpeg's C and SIMD "
                                     "inverse DCTs may disagree on it, so Pillow is no truth for it")
    dc = [code_table(*spec.dc_tables[spec.comp_td[c]]) for c in range(3)]
    ac = [code_table(*spec.ac_tables[spec.comp_ta[c]]) for c in range(3)]
    total, per = n_mcus(spec), spec.restart or n_mcus(spec)
    scan = b""
    for i, m0 in enumerate(range(0, total, per)):
        if i:
            scan += b"\xff" * spec.rst_fill + bytes([0xFF, 0xD0 + (i - 1) % 8])
        w, pred = _BitWriter(), [0, 0, 0]
        for mcu in range(m0, min(m0 + per, total)):
            for c, blk, ze in mcu_blocks(spec, blocks, mcu):
                syms, pred[c] = block_symbols(blk, pred[c], ze)
                for is_ac, s, extra, nbits in syms:
                    tab = (ac if is_ac else dc)[c]
                    assert s in tab, f"component {c}: {'AC' if is_ac else 'DC'} symbol 0x{s:02X} is coded and has no code in its table"
                    w.put(tab[s][1], tab[s][0])
                    w.put(extra, nbits)
        scan += w.flush()
    return _header(spec) + scan + spec.pad + b"\xff" * spec.eoi_fill + EOI + spec.trailer


def tables_from_codes(codes: dict):
    """{(length, code): symbol}, as tests/jpeg_rule_np.py reads a DHT table -> (counts, vals)."""
    keys = sorted(codes)
    return [sum(1 for l, _ in keys if l == n) for n in range(1, 17)], [codes[k] for k in keys]
