"""The baseline JPEG decode restated in plain Python and numpy, independently of the product's parser (vla_adapter_amd/jpeg_store.py)
and of its decode core (csrc/jpeg_core.h): a marker walk, canonical Huffman decode with byte stuffing and restart markers, the islow
inverse DCT of libjpeg's jidctint.c, h2v2 fancy upsampling (jdsample.c) and the fixed-point colour conversion (jdcolor.c).  It is the
written-down rule the product is pinned to, and is itself tested against Pillow bit for bit (tests/test_jpeg_cpu.py).  Slow: a
224 x 224 file takes about a second."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def huffman_codes(counts, vals):
    """{(length, code): symbol} of a DHT table: codes of a length are consecutive, the first of length l + 1 is twice the one
    behind the last of length l (JPEG Annex C)."""
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            table[(l, code)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


class Bits:
    """The bits of an entropy-coded segment, 0xFF 0x00 unstuffed."""

    def __init__(self, data: bytes):
        self.data = data
        self.bits = "".join(f"{b:08b}" for b in data.replace(b"\xff\x00", b"\xff"))
        self.pos = 0
        self.by_length = [0] * 17          # symbols decoded so far, by the length of their code

    def bytes_consumed(self) -> int:
        """How many bytes of the segment, stuffed zeros included, hold the bits taken so far."""
        left, i = (self.pos + 7) // 8, 0
        while left:
            i += 2 if self.data[i] == 0xFF else 1
            left -= 1
        return i

    def take(self, n: int) -> int:
        if n == 0:
            return 0
        if self.pos + n > len(self.bits):
            raise EOFError("the segment runs out of bits")
        v = int(self.bits[self.pos:self.pos + n], 2)
        self.pos += n
        return v

    def symbol(self, table) -> int:
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.take(1)
            if (l, code) in table:
                self.by_length[l] += 1
                return table[(l, code)]
        raise ValueError("a code that is in no table")


def extend(v: int, s: int) -> int:
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def parse(data: bytes) -> dict:
    """The markers of a baseline file -> dict(H, W, comps [(id, h, v, tq)], qt, ht, dri, scan [(td, ta)], segments [bytes])."""
    assert data[:2] == b"\xff\xd8"
    out, pos = dict(qt={}, ht={}, dri=0), 2
    while True:
        assert data[pos] == 0xFF
        while data[pos + 1] == 0xFF:             # fill bytes in front of a marker
            pos += 1
        m, L = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + L]
        if m == 0xDB:
            for i in range(0, len(seg), 65):
                assert seg[i] >> 4 == 0
                out["qt"][seg[i] & 15] = np.frombuffer(seg[i + 1:i + 65], dtype=np.uint8).astype(np.int64)
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                counts = list(seg[i + 1:i + 17])
                out["ht"][seg[i]] = huffman_codes(counts, list(seg[i + 17:i + 17 + sum(counts)]))
                i += 17 + sum(counts)
        elif m == 0xC0:
            assert seg[0] == 8 and seg[5] == 3
            out["H"], out["W"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            out["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
        elif m == 0xDD:
            out["dri"] = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            out["scan"] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(3)]
            pos += 2 + L
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA, 0xCB), "baseline files only"
        pos += 2 + L
    segs, start, i = [], pos, pos
    while True:                                  # 0xFF 0x00 is data, 0xFF RSTn splits, any other marker (EOI) ends the scan;
        i = j = data.index(b"\xff", i)           # a marker may have 0xFF fill bytes in front of it
        while data[j + 1] == 0xFF:
            j += 1
        nxt = data[j + 1]
        if nxt == 0:
            assert j == i, "fill bytes in front of a stuffed byte"
            i += 2
        elif 0xD0 <= nxt <= 0xD7:
            segs.append(data[start:i])
            start = i = j + 2
        else:
            segs.append(data[start:i])
            break
    out["segments"] = segs
    return out


def idct_1d(x):
    """One pass of jpeg_idct_islow over the last axis of an int64 array [..., 8] (before its descale)."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 + z3 * -15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3], -1)


def idct_islow(blocks):
    """int64 [..., 8, 8] dequantised coefficients -> uint8 [..., 8, 8]: columns first (descale 11), then rows (descale 18), + 128,
    clamped."""
    ws = (idct_1d(np.swapaxes(blocks, -1, -2)) + (1 << 10)) >> 11            # [..., column, row]
    out = (idct_1d(np.swapaxes(ws, -1, -2)) + (1 << 17)) >> 18
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def upsample_h2v2(c):
    """uint8 [h, w] -> int64 [2 h, 2 w], libjpeg's h2v2_fancy_upsample."""
    c = c.astype(np.int64)
    h, w = c.shape
    up, down = np.vstack([c[:1], c[:-1]]), np.vstack([c[1:], c[-1:]])
    s = np.empty((2 * h, w), dtype=np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = np.hstack([s[:, :1], s[:, :-1]]), np.hstack([s[:, 1:], s[:, -1:]])
    out = np.empty((2 * h, 2 * w), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    out[:, 0], out[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes, stats: dict = None) -> np.ndarray:
    """A baseline 4:2:0 or 4:4:4 file whose sides are multiples of 16 -> uint8 [H, W, 3].  ``stats``, when given, receives what only
    a decode can count: "by_length" [17], the symbols decoded by the length of their code, and "consumed", per segment the bytes that
    hold the bits its MCUs took, "blocks" [(component, [the DC symbol, the AC symbols ...])] in coding order, and "quantised", the
    coefficients before dequantisation."""
    p = parse(data)
    H, W, comps = p["H"], p["W"], p["comps"]
    h2v2 = (comps[0][1], comps[0][2]) == (2, 2)
    assert all((c[1], c[2]) == (1, 1) for c in comps[1:]) and ((comps[0][1], comps[0][2]) in ((1, 1), (2, 2))) and H % 16 == 0 and W % 16 == 0
    mw, mh = (W // 16, H // 16) if h2v2 else (W // 8, H // 8)
    planes = [np.zeros((H // 8, W // 8, 64), dtype=np.int64)] + [np.zeros((mh, mw, 64), dtype=np.int64) for _ in range(2)]
    layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)] if h2v2 else [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    per = p["dri"] or mw * mh
    for si, seg in enumerate(p["segments"]):
        bits, pred = Bits(seg), [0, 0, 0]
        for mcu in range(si * per, min((si + 1) * per, mw * mh)):
            my, mx = divmod(mcu, mw)
            for c, dy, dx in layout:
                q, (td, ta) = p["qt"][comps[c][3]], p["scan"][c]
                blk = planes[c][(2 * my + dy, 2 * mx + dx) if (h2v2 and c == 0) else (my, mx)]
                s = bits.symbol(p["ht"][td])
                syms = [s]
                pred[c] += extend(bits.take(s), s)
                blk[0] = pred[c] * q[0]
                k = 1
                while k < 64:
                    rs = bits.symbol(p["ht"][0x10 | ta])
                    syms.append(rs)
                    r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        blk[ZIGZAG[k]] = extend(bits.take(s), s) * q[k]
                    elif r == 15:
                        k += 15
                    else:
                        break
                    k += 1
                if stats is not None:
                    stats.setdefault("blocks", []).append((c, syms))
        if stats is not None:
            stats.setdefault("consumed", []).append(bits.bytes_consumed())
            stats["by_length"] = [a + b for a, b in zip(stats.get("by_length", [0] * 17), bits.by_length)]
    if stats is not None:                        # the quantised coefficients as the file codes them: [Y, Cb, Cr], zigzag order
        stats["quantised"] = [pl[..., ZIGZAG] // p["qt"][comps[c][3]] for c, pl in enumerate(planes)]
    pix = []
    for pl in planes:
        bh, bw = pl.shape[:2]
        pix.append(idct_islow(pl.reshape(bh, bw, 8, 8)).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    cb, cr = (upsample_h2v2(pix[1]), upsample_h2v2(pix[2])) if h2v2 else (pix[1], pix[2])
    return ycc_to_rgb(pix[0], cb, cr)
