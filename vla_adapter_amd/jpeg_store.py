"""Episodes whose frames are JPEG files: the second storage form of an episode file, and what is done with it once, at load.

In place of ``frames_u8`` an episode dict may carry

  frames_jpeg   uint8  [n_bytes]          complete baseline JPEG files back to back, frame (t, cam) at index t * n_img + cam
  frame_off     int64  [T * n_img + 1]    byte offsets of the files, rising from 0 to n_bytes
  frame_shape   int64  [3]                (n_img, H, W)

and every batch's frames are then decoded on the device (csrc/jpeg.hip, include/vla_jpeg.h) into the same ``frames_u8
[B, n_img, H, W, 3]`` buffer the raw store fills: bit for bit what Pillow - libjpeg-turbo with its defaults - decodes (DESIGN.md
section 18).

Accepted: baseline sequential (SOF0), 8 bit, the three components Y, Cb, Cr in one scan, sampled 4:2:0 or 4:4:4, one sampling per
store, H and W multiples of 16 and equal to ``frame_shape``.  Everything else is refused at load by a ValueError that names the frame:
other codings (extended, progressive, lossless, hierarchical, arithmetic), 12-bit samples, one or four components, other samplings,
16-bit quantisation tables, a table that is used and never defined, a second scan or a missing EOI, a size mismatch, Huffman counts
that overflow their code space, and three components that store RGB.  Whether they do is libjpeg's rule (``_stores_rgb``): a JFIF
marker says YCbCr; without one an Adobe marker says RGB with transform 0; without either the ids 'R', 'G', 'B' say RGB.  0xFF fill
bytes are accepted in front of every marker, RSTn and EOI included; in front of a stuffed 0xFF 0x00 they are refused (T.81 has
none there; libjpeg reads them as one data byte, the decode core as the end of the segment).

``parse_frames`` walks the markers of every file once: it pools the quantisation and Huffman tables by content (the latter in the
derived form the kernel reads), finds the entropy-coded segments - one per image, or one per restart interval - and writes the small
per-image and per-segment tables that ``JpegFrames`` uploads beside the bytes.  Only the scan is validated structurally (its markers);
whether its bits decode is the kernel's ``status``, and ``EpisodeStore.verify_frames`` reads it for the whole store.

The decode is serial per segment, and a file without restart markers is one segment.  ``JpegFrames.build_scan_index`` (asked for by
``jpeg_scan_index=True`` of the stores, ``--jpeg_scan_index`` of ``finetune``) walks such segments once on the device and cuts them
into pieces of one MCU row, each with the byte, the bit and the DC predictors at which it begins (``plan_pieces``,
include/vla_jpeg_index.h): the files stay as they are, the pixels too, and the decode gets a work item per row.
A piece is a segment in every respect - in ``seg_tab``, in ``max_seg``, in ``status`` and in what ``verify_frames`` names.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch

JPEG_KEYS = ("frames_jpeg", "frame_off", "frame_shape")
# csrc/jpeg_core.h: the layout of a derived Huffman table, of a per-image row and of a per-segment row
HT_MAXCODE, HT_VALOFF, HT_LOOK, HT_VAL, HT_WORDS = 0, 18, 36, 36 + 256, 36 + 512
IMG_Q, IMG_DC, IMG_AC, IMG_RESTART, IMG_H2V2, IMG_WORDS = 0, 3, 6, 9, 10, 12
SEG_WORDS = 4
STATUS_TEXT = {1: "the segment runs out of bytes", 2: "a code that is in no Huffman table", 3: "a zero run past the end of its block"}

_SOF_REFUSED = {0xC1: "extended sequential coding (SOF1)", 0xC2: "progressive coding (SOF2)", 0xC3: "lossless coding (SOF3)",
                0xC5: "hierarchical coding (SOF5)", 0xC6: "hierarchical progressive coding (SOF6)", 0xC7: "hierarchical lossless coding (SOF7)",
                0xC9: "arithmetic coding (SOF9)", 0xCA: "progressive arithmetic coding (SOF10)", 0xCB: "lossless arithmetic coding (SOF11)",
                0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def storage_form(d: dict, where: str) -> str:
    """"raw" or "jpeg"; ValueError naming the keys for a dict that carries both forms, or a part of the JPEG form."""
    raw, jpeg = "frames_u8" in d, [k for k in JPEG_KEYS if k in d]
    if raw and jpeg:
        raise ValueError(f"{where}: carries both frames_u8 and {tuple(jpeg)}: an episode file stores its frames in one form, frames_u8 or {JPEG_KEYS}")
    if jpeg and len(jpeg) != len(JPEG_KEYS):
        raise ValueError(f"{where}: {tuple(k for k in JPEG_KEYS if k not in d)} missing (the JPEG form carries {JPEG_KEYS})")
    return "jpeg" if jpeg else "raw"


def check_jpeg_shard(d: dict, T: int, where: str) -> None:
    """ValueError naming the key for JPEG tables that do not fit each other or the T rows of the shard (the files themselves are
    looked at by parse_frames)."""
    fj, fo, fs = (d[k] for k in JPEG_KEYS)
    for k, t in zip(JPEG_KEYS, (fj, fo, fs)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{where}: {k} must be a tensor")
    if fs.dtype != torch.int64 or tuple(fs.shape) != (3,) or int(fs.min()) < 1:
        raise ValueError(f"{where}: frame_shape must be int64 [3] = (n_img, H, W), all >= 1, got {fs.dtype} {fs.tolist() if fs.numel() < 8 else tuple(fs.shape)}")
    n_img = int(fs[0])
    if fj.dtype != torch.uint8 or fj.dim() != 1 or fj.numel() < 1:
        raise ValueError(f"{where}: frames_jpeg must be uint8 [n_bytes], got {fj.dtype} {tuple(fj.shape)}")
    if fo.dtype != torch.int64 or fo.dim() != 1 or fo.numel() != T * n_img + 1:
        raise ValueError(f"{where}: frame_off must be int64 [T * n_img + 1 = {T * n_img + 1}], got {fo.dtype} {tuple(fo.shape)}")
    if int(fo[0]) != 0 or int(fo[-1]) != fj.numel() or bool((fo.diff() < 0).any()):
        raise ValueError(f"{where}: frame_off must rise from 0 to len(frames_jpeg) = {fj.numel()} without a step back")


# ---------------------------------------------------------------------------------------------------------------- Huffman tables
def derive_huffman(counts, vals) -> np.ndarray:
    """The derived form of a DHT table (counts of the 16 code lengths, the symbols in code order), int32 [HT_WORDS] as csrc/jpeg_core.h
    reads it: canonical codes (JPEG Annex C), maxcode per length, valptr - mincode, and the 8-bit lookahead.  ValueError when the
    counts overflow the code space of some length, or count more symbols than are given / than 256."""
    counts = [int(c) for c in counts]
    if len(counts) != 16 or sum(counts) > 256 or sum(counts) > len(vals):
        raise ValueError(f"a Huffman table of {sum(counts)} codes with {len(vals)} symbols")
    t = np.zeros(HT_WORDS, dtype=np.int32)
    t[HT_MAXCODE:HT_MAXCODE + 18] = -1
    code = k = 0
    for l in range(1, 17):
        n = counts[l - 1]
        if n:
            t[HT_VALOFF + l] = k - code
            if code + n > (1 << l):
                raise ValueError(f"a Huffman table whose code counts overflow the {l}-bit code space")
            if l <= 8:
                for i in range(n):
                    lo = (code + i) << (8 - l)
                    t[HT_LOOK + lo:HT_LOOK + lo + (1 << (8 - l))] = (l << 8) | int(vals[k + i])
            t[HT_VAL + k:HT_VAL + k + n] = [int(v) for v in vals[k:k + n]]
            code, k = code + n, k + n
            t[HT_MAXCODE + l] = code - 1
        code <<= 1
    t[HT_MAXCODE + 17] = 0x7FFFFFFF
    return t


# ---------------------------------------------------------------------------------------------------------------- the parser
@dataclass
class JpegIndex:
    """What parse_frames makes of N files (host arrays; JpegFrames uploads them)."""
    n_img: int
    H: int
    W: int
    h2v2: int                   # 1: 4:2:0, 0: 4:4:4 - one sampling per store
    img_seg: np.ndarray         # int64 [N + 1]
    seg_tab: np.ndarray         # int64 [S, 4]: lo, hi (absolute byte offsets), mcu0, mcu1
    img_tab: np.ndarray         # int32 [N, 12]
    qt_pool: np.ndarray         # uint16 [nQ, 64], zigzag order
    ht_pool: np.ndarray         # int32 [nH, HT_WORDS]
    max_seg: int                # the largest segment count of an image: sizes the decode grid

    @property
    def N(self) -> int:
        return int(self.img_tab.shape[0])

    @property
    def mcus(self) -> int:
        return (self.H // 16) * (self.W // 16) if self.h2v2 else (self.H // 8) * (self.W // 8)


class _Pools:
    def __init__(self):
        self.q: Dict[bytes, int] = {}
        self.h: Dict[bytes, int] = {}
        self.q_rows: List[np.ndarray] = []
        self.h_rows: List[np.ndarray] = []

    def quant(self, table: bytes) -> int:
        if table not in self.q:
            self.q[table] = len(self.q_rows)
            self.q_rows.append(np.frombuffer(table, dtype=np.uint8).astype(np.uint16))
        return self.q[table]

    def huffman(self, counts: bytes, vals: bytes) -> int:
        key = counts + vals
        if key not in self.h:
            row = derive_huffman(counts, vals)          # (ValueError: the caller names the frame)
            self.h[key] = len(self.h_rows)
            self.h_rows.append(row)
        return self.h[key]


def _stores_rgb(jfif: bool, adobe, ids) -> str:
    """libjpeg's rule for the colour coding of three components (jdapimin.c, default_decompress_parms): a JFIF marker says YCbCr;
    without one an Adobe marker says RGB with transform 0 and YCbCr with any other; without either the component ids 'R', 'G', 'B'
    say RGB and any others YCbCr.  -> what says RGB, or "" for YCbCr."""
    if jfif:
        return ""
    if adobe is not None:
        return "Adobe transform 0" if adobe == 0 else ""
    return "component ids 'R', 'G', 'B' and neither a JFIF nor an Adobe marker" if list(ids) == [0x52, 0x47, 0x42] else ""


def _parse_one(buf: np.ndarray, base: int, H: int, W: int, pools: _Pools):
    """One file (buf: its bytes; base: its offset in the store) -> (img row, [segment rows]); ValueError with the reason alone."""
    n = int(buf.shape[0])
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        raise ValueError("no SOI marker at its start: not a JPEG file")
    qt, ht, sof, dri, pos = {}, {}, None, 0, 2
    jfif, adobe = False, None                           # a JFIF APP0 marker was seen; the transform flag of an Adobe APP14 marker
    while True:
        if pos + 2 > n:
            raise ValueError("the header is truncated: no SOS marker (the file ends inside its header)")
        if buf[pos] != 0xFF:
            raise ValueError(f"byte {pos}: a marker was expected in the header")
        m = int(buf[pos + 1])
        if m == 0xFF:                                   # a fill byte
            pos += 1
            continue
        if m == 0xD9:
            raise ValueError("EOI before any SOS marker: the file has no scan")
        if m == 0x01 or 0xD0 <= m <= 0xD8:
            pos += 2
            continue
        if pos + 4 > n:
            raise ValueError("the header is truncated: no SOS marker (the file ends inside its header)")
        L = (int(buf[pos + 2]) << 8) | int(buf[pos + 3])
        if L < 2 or pos + 2 + L > n:
            raise ValueError(f"the header is truncated: the segment of marker 0xFF{m:02X} runs past the end of the file")
        seg = buf[pos + 4:pos + 2 + L].tobytes()
        if m in _SOF_REFUSED:
            raise ValueError(f"{_SOF_REFUSED[m]} is not supported: baseline sequential (SOF0) files only")
        if m == 0xE0 and len(seg) >= 14 and seg[:5] == b"JFIF\0":          # (jdmarker.c: 14 and 12 bytes are what it examines)
            jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                if seg[i] >> 4:
                    raise ValueError("16-bit quantisation tables are not supported")
                if i + 65 > len(seg):
                    raise ValueError("a truncated DQT segment")
                qt[seg[i] & 15] = pools.quant(seg[i + 1:i + 65])
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise ValueError("a truncated DHT segment")
                counts = seg[i + 1:i + 17]
                nv = sum(counts)
                if i + 17 + nv > len(seg):
                    raise ValueError("a truncated DHT segment")
                ht[seg[i]] = pools.huffman(counts, seg[i + 17:i + 17 + nv])          # key: (class << 4) | id
                i += 17 + nv
        elif m == 0xC0:
            if len(seg) < 6:
                raise ValueError("a truncated SOF0 segment")
            P, fh, fw, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if P != 8:
                raise ValueError(f"{P}-bit precision is not supported: 8-bit samples only")
            if nf != 3 or len(seg) < 6 + 3 * nf:
                raise ValueError(f"{nf} component(s) ({'grayscale' if nf == 1 else 'CMYK / YCCK' if nf == 4 else 'unknown'}) are not supported: "
                                 "the three components Y, Cb, Cr only")
            if (fh, fw) != (H, W):
                raise ValueError(f"size mismatch: the file is {fh} x {fw}, frame_shape says {H} x {W}")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)]
            samp = [(h, v) for _, h, v, _ in comps]
            if samp == [(2, 2), (1, 1), (1, 1)]:
                h2v2 = 1
            elif samp == [(1, 1), (1, 1), (1, 1)]:
                h2v2 = 0
            else:
                raise ValueError(f"sampling factors {samp} are not supported: 4:2:0 (2x2, 1x1, 1x1) or 4:4:4 only")
            sof = (comps, h2v2)
        elif m == 0xDD:
            if len(seg) < 2:
                raise ValueError("a truncated DRI segment")
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if sof is None:
                raise ValueError("SOS before any SOF0 marker")
            comps, h2v2 = sof
            if len(seg) < 1 or seg[0] != 3 or len(seg) < 10:
                raise ValueError(f"a scan of {seg[0] if seg else 0} component(s): one scan that lists the three components is needed")
            if [seg[1 + 2 * c] for c in range(3)] != [c[0] for c in comps]:
                raise ValueError("the scan does not list the three components in the frame's order")
            if (seg[7], seg[8], seg[9]) != (0, 63, 0):
                raise ValueError("a scan with spectral selection or successive approximation: sequential scans only")
            rgb = _stores_rgb(jfif, adobe, [c[0] for c in comps])
            if rgb:
                raise ValueError(f"the file stores RGB ({rgb}), not YCbCr: not supported")
            rec = np.zeros(IMG_WORDS, dtype=np.int32)
            for c in range(3):
                td, ta, tq = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15, comps[c][3]
                if tq not in qt:
                    raise ValueError(f"quantisation table {tq} is used and never defined")
                if td not in ht or (0x10 | ta) not in ht:
                    raise ValueError(f"Huffman table DC {td} / AC {ta} is used and never defined")
                rec[IMG_Q + c], rec[IMG_DC + c], rec[IMG_AC + c] = qt[tq], ht[td], ht[0x10 | ta]
            rec[IMG_RESTART], rec[IMG_H2V2] = dri, h2v2
            start = pos + 2 + L
            break
        pos += 2 + L
    # the scan: entropy-coded bytes, in which 0xFF is followed by 0x00 (a data byte 0xFF) or, with DRI, by RSTn; anything else ends it.
    # A marker may have 0xFF fill bytes in front of it (T.81 B.1.1.2), so the scan is walked run of 0xFF by run: `s` the first byte of
    # a run, `e` the byte behind it, which is the marker code (a run at the very end of the file has none and marks nothing).
    data = buf[start:]
    isff = data == 0xFF
    prev = np.concatenate([[False], isff])[:-1]
    s, e = np.flatnonzero(isff & ~prev), np.flatnonzero(~isff & prev)
    s = s[:e.shape[0]]
    code = data[e]
    keep = ~((code == 0) & (e - s == 1))                          # a single 0xFF and 0x00: a stuffed data byte
    s, e, code = s[keep], e[keep], code[keep]
    is_rst = (code >= 0xD0) & (code <= 0xD7) if dri else np.zeros(code.shape, dtype=bool)
    ends = np.flatnonzero(~is_rst)
    if ends.size == 0:
        raise ValueError("missing EOI: the scan runs to the end of the file")
    j = int(ends[0])
    if code[j] == 0:
        raise ValueError(f"{int(e[j] - s[j] - 1)} 0xFF fill byte(s) in front of a stuffed 0xFF 0x00 inside the entropy-coded data (scan byte "
                         f"{int(s[j])}): fill bytes are accepted in front of markers only")
    if code[j] != 0xD9:
        raise ValueError(f"missing EOI: the scan is followed by marker 0xFF{int(code[j]):02X} (a second scan, or stray bytes)")
    end = int(s[j])
    los = np.concatenate([[0], e[:j] + 1]).astype(np.int64)       # a segment starts behind the code of its RSTn marker
    his = np.concatenate([s[:j], [end]]).astype(np.int64)         # and ends at the first 0xFF - a fill byte, if there are any - of the next
    n_mcu = (H // 16) * (W // 16) if h2v2 else (H // 8) * (W // 8)
    segs = np.zeros((los.shape[0], SEG_WORDS), dtype=np.int64)
    segs[:, 0], segs[:, 1] = los + (base + start), his + (base + start)
    if dri:
        i = np.arange(los.shape[0], dtype=np.int64)
        segs[:, 2], segs[:, 3] = np.minimum(i * dri, n_mcu), np.minimum((i + 1) * dri, n_mcu)
    segs[-1, 3] = n_mcu                 # (fewer markers than intervals - a damaged file: the last segment is asked for the rest and
    return rec, segs                    #  reports that it ran out of bytes)


def parse_frames(frames_jpeg, frame_off, frame_shape, where: str = "episode store") -> JpegIndex:
    """Walk every file once -> JpegIndex.  ValueError ``{where}: frame i (step t, image cam): reason`` for the first file that is
    refused."""
    data = frames_jpeg.cpu().numpy() if isinstance(frames_jpeg, torch.Tensor) else np.asarray(frames_jpeg, dtype=np.uint8)
    off = [int(o) for o in (frame_off.tolist() if isinstance(frame_off, torch.Tensor) else frame_off)]
    n_img, H, W = (int(x) for x in (frame_shape.tolist() if isinstance(frame_shape, torch.Tensor) else frame_shape))
    N = len(off) - 1

    def refuse(i, why):
        return ValueError(f"{where}: frame {i} (step {i // n_img}, image {i % n_img}): {why}")
    if H % 16 or W % 16:
        raise refuse(0, f"size {H} x {W}: height and width must be multiples of 16 (whole MCUs of either sampling)")
    pools, recs, segs, counts, h2v2 = _Pools(), [], [], [], None
    for i in range(N):
        try:
            rec, sg = _parse_one(data[off[i]:off[i + 1]], off[i], H, W, pools)
        except ValueError as e:
            raise refuse(i, str(e)) from None
        if h2v2 is None:
            h2v2 = int(rec[IMG_H2V2])
        elif int(rec[IMG_H2V2]) != h2v2:
            raise refuse(i, f"sampling {'4:2:0' if rec[IMG_H2V2] else '4:4:4'} differs from frame 0's: a store keeps one sampling")
        recs.append(rec)
        segs.append(sg)
        counts.append(sg.shape[0])
    img_seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return JpegIndex(n_img=n_img, H=H, W=W, h2v2=int(h2v2), img_seg=img_seg, seg_tab=np.concatenate(segs), img_tab=np.stack(recs),
                     qt_pool=np.stack(pools.q_rows), ht_pool=np.stack(pools.h_rows), max_seg=int(max(counts)))


# ---------------------------------------------------------------------------------------------------------------- the scan index
def plan_pieces(index: JpegIndex, piece_mcus: int):
    """How the segments of a store are cut into pieces of ``piece_mcus`` MCUs (include/vla_jpeg_index.h; numpy only): segment
    [m0, m1) gets max(1, ceil((m1 - m0) / piece_mcus)) pieces that tile it without gap or overlap, the last one shorter.
    -> (piece_off int64 [S + 1]: the pieces of segment s are rows piece_off[s] .. piece_off[s + 1] of the new tables, the new img_seg
    int64 [N + 1] = piece_off[img_seg], S' = the number of pieces, the new max_seg)."""
    piece_mcus = int(piece_mcus)
    if piece_mcus < 1:
        raise ValueError(f"piece_mcus must be >= 1, got {piece_mcus}")
    n = np.maximum(index.seg_tab[:, 3] - index.seg_tab[:, 2], 0)
    pieces = np.maximum(1, (n + piece_mcus - 1) // piece_mcus)
    piece_off = np.concatenate([[0], np.cumsum(pieces)]).astype(np.int64)
    img_seg = piece_off[index.img_seg]
    return piece_off, img_seg, int(piece_off[-1]), int(np.diff(img_seg).max())


# vla_jpeg_index_build walks segments serially, a lane a 224 x 224 scan in 12 - 25 ms.  4096 segments are 64
# waves of the lane mapping - fewer than the device has compute units - so a launch of one slice lasts about as long as one walk, tens
# of milliseconds, however large the store: no single launch holds a shared device for long.
BUILD_SLICE = 4096


# ---------------------------------------------------------------------------------------------------------------- on the device
class JpegFrames:
    """The JPEG frames of a store on the device: the bytes, the tables parse_frames wrote, and the decode of a batch's frames."""

    mapping = 1                 # vla_jpeg_decode_rows: 0 one lane per segment, 1 one wave per segment
    build_mapping = 0           # vla_jpeg_index_build: likewise; the build is bound by throughput, and a lane per scan is the faster
                                # one for a store of more than one slice

    def __init__(self, tables: dict, device, where: str = "episode store"):
        self.device = device
        self.index = ix = parse_frames(tables["frames_jpeg"], tables["frame_off"], tables["frame_shape"], where)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.bytes = tables["frames_jpeg"].to(device).contiguous()
        self.img_seg, self.seg_tab, self.img_tab = up(ix.img_seg), up(ix.seg_tab), up(ix.img_tab)
        self.qt_pool, self.ht_pool = up(ix.qt_pool.view(np.int16)), up(ix.ht_pool)          # (torch has no uint16 arithmetic: same bits)
        self.n_img, self.H, self.W, self.h2v2, self.max_seg, self.N = ix.n_img, ix.H, ix.W, ix.h2v2, ix.max_seg, ix.N
        self._ws: Dict[int, torch.Tensor] = {}
        self.seg_ent, self.index_status, self.piece_mcus = None, None, None        # (set by build_scan_index)

    def build_scan_index(self, piece_mcus: int = None, mapping: int = None, slice_segments: int = BUILD_SLICE) -> int:
        """Cut every segment longer than ``piece_mcus`` MCUs (default: one MCU row) into pieces the decode starts in parallel
        (include/vla_jpeg_index.h): one serial walk per segment on the device, ``slice_segments`` segments per launch.  Swaps in the
        new img_seg / seg_tab / max_seg and the entry table seg_ent, drops the buffers sized by the old max_seg, and keeps
        ``index_status`` u8 [S] (the walk's status of every original segment) on the device - nothing is read back; how many walks
        stopped early is ``(index_status != 0).sum()`` for whoever logs it.  -> the number of pieces, or 0 when no segment is longer
        than piece_mcus and the store stays as it is."""
        from . import ops
        ix = self.index
        if piece_mcus is None:
            piece_mcus = ix.W // 16 if ix.h2v2 else ix.W // 8
        if self.seg_ent is not None:
            raise ValueError("build_scan_index: the store already has a scan index")
        piece_off, img_seg, S2, max_seg = plan_pieces(ix, piece_mcus)
        S = int(ix.seg_tab.shape[0])
        if S2 == S:
            return 0
        dev = self.device
        po = torch.from_numpy(piece_off).to(dev)
        seg_tab = torch.empty(S2, SEG_WORDS, dtype=torch.int64, device=dev)
        seg_ent = torch.empty(S2, 4, dtype=torch.int32, device=dev)
        status = torch.empty(S, dtype=torch.uint8, device=dev)
        step = max(1, int(slice_segments))
        for s0 in range(0, S, step):
            ops.jpeg_index_build(self.bytes, self.img_seg, self.seg_tab, self.img_tab, self.qt_pool, self.ht_pool, self.H, self.W, self.h2v2,
                                 int(piece_mcus), po, s0, min(s0 + step, S), self.build_mapping if mapping is None else mapping,
                                 seg_tab, seg_ent, status)
        self.img_seg, self.seg_tab, self.seg_ent, self.max_seg = torch.from_numpy(img_seg).to(dev), seg_tab, seg_ent, max_seg
        self.index_status, self.piece_mcus = status, int(piece_mcus)
        self._ws = {}
        return S2

    def index_bytes(self) -> int:
        """The bytes of the scan index on the device: a row of seg_tab (32) and one of seg_ent (16) per piece."""
        return 0 if self.seg_ent is None else int(self.seg_tab.shape[0]) * (SEG_WORDS * 8 + 16)

    def buffers(self, B: int) -> dict:
        """workspace and status for batches of B samples, and the zero-length frame rows the store's gather writes (allocated once
        per batch size)."""
        from . import ops
        if B not in self._ws:
            n = ops.jpeg_workspace_bytes(B * self.n_img, self.H, self.W, self.h2v2)
            self._ws[B] = dict(workspace=torch.empty(n, dtype=torch.uint8, device=self.device),
                               status=torch.zeros(B, self.n_img, self.max_seg, dtype=torch.uint8, device=self.device),
                               no_frames=torch.empty(B, 0, dtype=torch.uint8, device=self.device))
        return self._ws[B]

    def decode(self, episode_off: torch.Tensor, T: int, ep: torch.Tensor, row: torch.Tensor, out_frames: torch.Tensor, buf: dict = None,
               mapping: int = None) -> torch.Tensor:
        """vla_jpeg_decode_rows (vla_jpeg_decode_rows_at for a store with a scan index) of the windows (ep, row) into out_frames u8
        [B, n_img, H, W, 3]; -> status u8 [B, n_img, max_seg]."""
        from . import ops
        buf = buf or self.buffers(int(ep.numel()))
        ops.jpeg_decode_rows(self.bytes, self.img_seg, self.seg_tab, self.img_tab, self.qt_pool, self.ht_pool, episode_off, T, ep, row,
                             self.n_img, self.H, self.W, self.h2v2, self.max_seg, self.mapping if mapping is None else mapping,
                             buf["workspace"], out_frames, buf["status"], self.seg_ent)
        return buf["status"]


def concat_jpeg(shards: List[dict], names: List[str], device) -> dict:
    """frames_jpeg / frame_off / frame_shape of the shards back to back: the bytes concatenated (assembled on ``device`` shard by
    shard), the offsets rebased."""
    first = shards[0]["frame_shape"]
    for d, n in zip(shards[1:], names[1:]):
        if not torch.equal(d["frame_shape"], first):
            raise ValueError(f"{n}: frame_shape {d['frame_shape'].tolist()} differs from {names[0]}'s {first.tolist()}")
    total = sum(int(d["frames_jpeg"].numel()) for d in shards)
    out = dict(frames_jpeg=torch.empty(total, dtype=torch.uint8, device=device), frame_shape=first)
    offs, b0 = [shards[0]["frame_off"][:1]], 0
    for d in shards:
        nb = int(d["frames_jpeg"].numel())
        out["frames_jpeg"][b0:b0 + nb].copy_(d["frames_jpeg"])
        offs.append(d["frame_off"][1:] + b0)
        b0 += nb
    out["frame_off"] = torch.cat(offs)
    return out


# ---------------------------------------------------------------------------------------------------------------- raw frames -> files
ENCODE_SLICE = 1024             # steps per encode: at 256 x 256 and one camera 201 MB of raw frames and as many bytes of workspace at a time


def check_encode_quality(quality, restart_rows=1) -> int:
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quality must be an int inside 1 .. 100, got {quality!r}")
    if isinstance(restart_rows, bool) or not isinstance(restart_rows, int) or restart_rows < 1:
        raise ValueError(f"restart_rows must be >= 1 on the device (0, one segment per file, is coded serially: tools/pack_episodes_jpeg.py "
                         f"writes those with Pillow), got {restart_rows!r}")
    return quality


def encode_tables(tables: dict, device, quality: int = 95, restart_rows: int = 1, slice_frames: int = ENCODE_SLICE, where: str = "episode store") -> dict:
    """The episode dict ``tables`` with its frames_u8 [T, n_img, H, W, 3] replaced by frames_jpeg / frame_off / frame_shape - what
    tools/pack_episodes_jpeg.pack returns for the same quality and restart_rows, byte for byte - coded on ``device``
    (ops.jpeg_encode).  The frames go up ``slice_frames`` steps at a time and only their files stay, so neither the host nor the device
    ever holds the raw frames twice; frames_jpeg is on the device, the small tables stay where they were.  LOSSY.  ValueError naming
    ``where`` for frames whose sides are no multiples of 16; a dict already in the JPEG form comes back as it is."""
    from . import ops
    check_encode_quality(quality, restart_rows)
    if storage_form(tables, where) == "jpeg":
        return tables
    fr = tables["frames_u8"]
    T, n_img, H, W, _ = fr.shape
    if H % 16 or W % 16:
        name = tables.get("dataset_name")
        raise ValueError(f"{where}{f' (dataset {name!r})' if isinstance(name, str) and name else ''}: frames of {H} x {W}: the JPEG form needs "
                         "sides that are multiples of 16 (resize or pad the frames first)")
    step = max(1, int(slice_frames))
    pieces, offs, b0 = [], [torch.zeros(1, dtype=torch.int64)], 0
    for t0 in range(0, T, step):
        part = fr[t0:t0 + step].to(device, non_blocking=False)
        data, off = ops.jpeg_encode(part, quality, restart_rows)
        pieces.append(data)
        offs.append(off[1:].cpu() + b0)
        b0 += int(data.numel())
        del part
    out = {k: v for k, v in tables.items() if k != "frames_u8"}
    out["frames_jpeg"] = pieces[0] if len(pieces) == 1 else torch.cat(pieces)
    out["frame_off"] = torch.cat(offs)
    out["frame_shape"] = torch.tensor([n_img, H, W], dtype=torch.int64)
    return out
