// The baseline JPEG decode, stated once for the device (csrc/jpeg.hip, csrc/jpeg_index.hip) and for the host (the stand-alone program of
// tests/test_jpeg_core_cpu.py, which runs it under the sanitizers): bit reader, symbol decode, block decode, IDCT, chroma upsample and
// colour conversion.  Every function is plain integer C++ and compiles with hipcc for both sides and with any host compiler.
//
// The arithmetic is libjpeg's defaults, which is what Pillow decodes with: the JDCT_ISLOW inverse DCT
// (CONST_BITS 13, PASS1_BITS 2, its range-limit table included), h2v2 "fancy" triangle upsampling, and the 16-bit fixed-point
// YCbCr -> RGB tables.
//
// Memory safety does not depend on the stream or on the tables: every byte read lies inside [lo, hi) of the segment, every table
// index is checked or masked, and the callers bound the blocks a segment may write.  A segment that runs out of bytes or meets a code
// that is in no table stops there, reports a non-zero status and leaves its remaining coefficients zero.
#pragma once

#if defined(__HIPCC__)
#define VLA_JPEG_HD __host__ __device__ __forceinline__
#else
#define VLA_JPEG_HD inline
#endif

namespace vlajpeg {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned char u8;

// status of a segment (0: every block decoded)
enum { ST_OK = 0, ST_TRUNCATED = 1, ST_BAD_CODE = 2, ST_BAD_RUN = 3 };

// A Huffman table in derived form, HT_WORDS int32 (vla_adapter_amd/jpeg_store.py: derive_huffman writes it):
//   [HT_MAXCODE + l]  l = 1 .. 16: the largest code of length l, -1 when there is none; [HT_MAXCODE + 17] = 0x7fffffff (sentinel)
//   [HT_VALOFF + l]   valptr[l] - mincode[l]: huffval index of a code of length l is code + valoff
//   [HT_LOOK + i]     i = the next 8 bits: (length << 8) | symbol when a code of length <= 8 starts them, else 0
//   [HT_VAL + j]      huffval[j], j < 256
constexpr int HT_MAXCODE = 0, HT_VALOFF = 18, HT_LOOK = 36, HT_VAL = 36 + 256, HT_WORDS = 36 + 512;
// a row of the per-image table (int32 [N, IMG_WORDS]): quantisation table, DC table and AC table of Y, Cb, Cr, then the restart
// interval in MCUs (0: none) and the sampling (1: 4:2:0, 0: 4:4:4)
constexpr int IMG_Q = 0, IMG_DC = 3, IMG_AC = 6, IMG_RESTART = 9, IMG_H2V2 = 10, IMG_WORDS = 12;
// a row of the segment table (int64 [S, SEG_WORDS]): the entropy-coded bytes [lo, hi) and the MCUs [mcu0, mcu1) they hold
constexpr int SEG_LO = 0, SEG_HI = 1, SEG_MCU0 = 2, SEG_MCU1 = 3, SEG_WORDS = 4;
// a row of the optional entry table (int32 [S, ENT_WORDS], include/vla_jpeg_index.h): how many bits of the byte at `lo` are already
// consumed, and the DC predictors of Y, Cb, Cr there
constexpr int ENT_BIT = 0, ENT_P0 = 1, ENT_P1 = 2, ENT_P2 = 3, ENT_WORDS = 4;

VLA_JPEG_HD int natural_order(int k) {
  // jpeg_natural_order: zigzag position -> position in the 8 x 8 block
  constexpr u8 ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return ZZ[k & 63];
}

// ---------------------------------------------------------------------------------------------------------------- the bit reader
// Bits of bytes[lo, hi), most significant first, with the 0xFF 0x00 byte stuffing removed.  Behind the last byte - or a 0xFF that is
// followed by anything but 0x00, which ends the data - the reader supplies zero bits, so that a lookahead past the end reads nothing;
// CONSUMING one of them sets `truncated`.
struct BitReader {
  const u8* bytes;
  i64 pos, end;
  i64 fed;          // bytes pushed into `acc` so far, supplied ones included: 8 * fed - n bits are consumed.  Only the index walk reads
                    // it; in the per-batch decode it is a dead store, which the compiler drops once the reader is inlined
  u64 acc;          // the low `n` bits are unread, the oldest on top
  int n, pad;       // `pad` of them, the youngest, are supplied zeros
  int truncated;
};

VLA_JPEG_HD void br_init(BitReader& br, const u8* bytes, i64 lo, i64 hi) {
  br.bytes = bytes;
  br.pos = lo;
  br.end = hi > lo ? hi : lo;
  br.acc = 0;
  br.fed = 0;
  br.n = br.pad = br.truncated = 0;
}

VLA_JPEG_HD void br_fill(BitReader& br) {
  while (br.n <= 56) {
    unsigned b = 0;
    if (br.pos < br.end) {
      b = br.bytes[br.pos++];
      if (b == 0xFF) {
        if (br.pos < br.end && br.bytes[br.pos] == 0) {
          ++br.pos;
        } else {                // a marker, or a lone 0xFF at the end: the data ends here
          br.pos = br.end;
          b = 0;
          br.pad += 8;
        }
      }
    } else {
      br.pad += 8;
    }
    br.acc = (br.acc << 8) | b;
    br.n += 8;
    ++br.fed;
  }
}

// the next k bits (1 <= k <= 16) without consuming them; needs br.n >= k, which br_fill() guarantees for k <= 57
VLA_JPEG_HD unsigned br_peek(const BitReader& br, int k) { return (unsigned)(br.acc >> (br.n - k)) & ((1u << k) - 1u); }

VLA_JPEG_HD void br_skip(BitReader& br, int k) {
  br.n -= k;
  if (br.n < br.pad) {
    br.truncated = 1;
    br.pad = br.n;
  }
}

// ---------------------------------------------------------------------------------------------------------------- symbols
// The next Huffman symbol (0 .. 255), or -1 for a code that is in no table.  Call with br.n >= 16 (after br_fill).
VLA_JPEG_HD int decode_symbol(BitReader& br, const int* __restrict ht) {
  const int look = ht[HT_LOOK + (int)br_peek(br, 8)];
  if (look) {
    br_skip(br, look >> 8);
    return look & 255;
  }
  const int code16 = (int)br_peek(br, 16);
  for (int l = 9; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= ht[HT_MAXCODE + l]) {
      const int j = code + ht[HT_VALOFF + l];
      if (j < 0 || j > 255) return -1;
      br_skip(br, l);
      return ht[HT_VAL + j] & 255;
    }
  }
  return -1;
}

// s more bits as the signed value of category s (jdhuff.c HUFF_EXTEND); 1 <= s <= 15
VLA_JPEG_HD int receive_extend(BitReader& br, int s) {
  const int r = (int)br_peek(br, s);
  br_skip(br, s);
  return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

VLA_JPEG_HD short saturate16(i64 v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// One 8 x 8 block: 64 dequantised coefficients in natural order into out[0 .. 64), every one of them written (zero where the stream
// codes none).  `q`: the quantisation table in zigzag order; `pred`: the component's DC predictor.  -> ST_*; after a non-zero status
// the block holds what was decoded before it.
VLA_JPEG_HD int decode_block(BitReader& br, const int* __restrict dc, const int* __restrict ac, const unsigned short* __restrict q,
                             int& pred, short* __restrict out) {
  for (int i = 0; i < 64; ++i) out[i] = 0;
  br_fill(br);
  int s = decode_symbol(br, dc);
  if (s < 0 || s > 15) return ST_BAD_CODE;
  if (s) {
    br_fill(br);
    pred = (int)((unsigned)pred + (unsigned)receive_extend(br, s));          // (wraps: an entry table may hand in any predictor)
  }
  if (br.truncated) return ST_TRUNCATED;
  out[0] = saturate16((i64)pred * q[0]);
  for (int k = 1; k < 64; ++k) {
    br_fill(br);
    const int rs = decode_symbol(br, ac);
    if (rs < 0) return ST_BAD_CODE;
    if (br.truncated) return ST_TRUNCATED;
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return ST_BAD_RUN;
      const int v = receive_extend(br, s);            // (br.n >= 57 - 16 after the symbol: no refill needed)
      if (br.truncated) return ST_TRUNCATED;
      out[natural_order(k)] = saturate16((i64)v * q[k]);
    } else if (r == 15) {
      k += 15;
      if (k > 63) return ST_BAD_RUN;
    } else {
      break;
    }
  }
  return ST_OK;
}

// Where block `blk` of MCU `mcu` stands in an image's coefficient (and plane) layout: the Y blocks in raster order, then Cb, then Cr.
// bw = W / 8 blocks per Y row, bh = H / 8.  4:2:0: blk 0 .. 3 are the MCU's Y blocks (raster), 4 Cb, 5 Cr; 4:4:4: Y, Cb, Cr.
VLA_JPEG_HD int block_component(int blk, int h2v2) { return h2v2 ? (blk < 4 ? 0 : blk - 3) : blk; }

VLA_JPEG_HD int block_index(int mcu, int blk, int bw, int bh, int h2v2, int& comp) {
  comp = block_component(blk, h2v2);
  if (h2v2) {
    const int mw = bw >> 1, my = mcu / mw, mx = mcu - my * mw;
    if (blk < 4) return (2 * my + (blk >> 1)) * bw + 2 * mx + (blk & 1);
    return bw * bh + (comp - 1) * (mw * (bh >> 1)) + my * mw + mx;
  }
  return blk * bw * bh + mcu;
}

VLA_JPEG_HD int blocks_per_mcu(int h2v2) { return h2v2 ? 6 : 3; }
VLA_JPEG_HD int mcus_per_image(int H, int W, int h2v2) { return h2v2 ? (H >> 4) * (W >> 4) : (H >> 3) * (W >> 3); }
VLA_JPEG_HD i64 blocks_per_image(int H, int W, int h2v2) { return (i64)mcus_per_image(H, W, h2v2) * blocks_per_mcu(h2v2); }

// The nine tables of an image - quantisation (zigzag order), DC and AC Huffman tables of Y, Cb, Cr - as element offsets into one
// array of quantisation tables and one of Huffman tables (the store's pools, or a copy in LDS).  Named fields and selects, not arrays:
// a component index that is only known at run time would put an array into scratch memory on the device.
struct Tables {
  const unsigned short* q;
  const int* ht;
  i64 q0, q1, q2, dc0, dc1, dc2, ac0, ac1, ac2;
};
VLA_JPEG_HD const unsigned short* table_q(const Tables& t, int c) { return t.q + (c == 0 ? t.q0 : (c == 1 ? t.q1 : t.q2)); }
VLA_JPEG_HD const int* table_dc(const Tables& t, int c) { return t.ht + (c == 0 ? t.dc0 : (c == 1 ? t.dc1 : t.dc2)); }
VLA_JPEG_HD const int* table_ac(const Tables& t, int c) { return t.ht + (c == 0 ? t.ac0 : (c == 1 ? t.ac1 : t.ac2)); }

// Where a segment's decode begins: `bit` (0 .. 7) bits of the byte at `lo` are already consumed, and the DC predictors of Y, Cb, Cr
// are p0, p1, p2.  Behind a marker - the start of every segment the parser finds - it is all zero; index_segment() records the state
// at MCUs inside a segment, which makes a piece of a segment a segment of its own.
struct Entry {
  int bit, p0, p1, p2;
};

VLA_JPEG_HD Entry entry_at(const int* ent) {          // (null: no entry table; the row as it stands: decode_segment masks the bit)
  return ent ? Entry{ent[ENT_BIT], ent[ENT_P0], ent[ENT_P1], ent[ENT_P2]} : Entry{0, 0, 0, 0};
}

// One segment: the MCUs [mcu0, mcu1) of an image from bytes[lo, hi), begun in state `e`, into the image's coefficient blocks `coef`
// (64 shorts each, laid out by block_index).  The caller has clamped lo <= hi into the byte array and mcu0 <= mcu1 into the image's
// MCUs.  `img`: the image's row of the per-image table, its table ids already clamped into the pools.  Every block of the range is
// written; -> ST_*.  The entry's bit is masked to 0 .. 7 here, the one place every caller - the kernels and the host program - passes
// through; the predictors feed arithmetic only (a wrapping add, a saturating product): any value is safe.
VLA_JPEG_HD int decode_segment(const u8* bytes, i64 lo, i64 hi, const Entry& e, int mcu0, int mcu1, int H, int W, int h2v2,
                               const Tables& t, short* __restrict coef) {
  BitReader br;
  br_init(br, bytes, lo, hi);
  const int bit = e.bit & 7;
  if (bit) {                                            // (the bits of the byte at `lo` that the piece in front consumed)
    br_fill(br);
    br_skip(br, bit);
  }
  int p0 = e.p0, p1 = e.p1, p2 = e.p2;                  // the DC predictors of Y, Cb, Cr
  int status = ST_OK;
  const int bw = W >> 3, bh = H >> 3, nb = blocks_per_mcu(h2v2);
  for (int mcu = mcu0; mcu < mcu1; ++mcu) {
    for (int blk = 0; blk < nb; ++blk) {
      int comp;
      short* out = coef + (i64)block_index(mcu, blk, bw, bh, h2v2, comp) * 64;
      if (status != ST_OK) {
        for (int i = 0; i < 64; ++i) out[i] = 0;
        continue;
      }
      int& pred = comp == 0 ? p0 : (comp == 1 ? p1 : p2);
      status = decode_block(br, table_dc(t, comp), table_ac(t, comp), table_q(t, comp), pred, out);
    }
  }
  return status;
}

// The store's tables as include/vla_jpeg.h describes them; N images, S segments, nQ and nH pool entries.
struct Store {
  const u8* bytes;
  i64 n_bytes;
  const i64* img_seg;
  const i64* seg_tab;
  i64 S;
  const int* img_tab;
  const unsigned short* qt_pool;
  int nQ;
  const int* ht_pool;
  int nH;
  const int* seg_ent = nullptr;     // int32 [S, ENT_WORDS]: the entry state of every segment, or null when every segment starts behind a marker
};

VLA_JPEG_HD i64 clamp_i64(i64 v, i64 lo, i64 hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Work item (image img, segment k) of the decode, resolved from the tables: the segment's bytes and MCUs and the image's nine tables.
struct Item {
  i64 lo, hi;
  int mcu0, mcu1;
  Entry e;
  Tables t;
};

// Row s of the segment table (0 <= s < S, the caller's duty) as a segment of image img (0 <= img < N, likewise).  Every value read
// from a table is clamped before it is used: byte ranges into [0, n_bytes], MCU ranges into the image, ids into the pools (the entry
// bit is masked where it is used, in decode_segment).
VLA_JPEG_HD void resolve_segment(const Store& st, i64 img, i64 s, int H, int W, int h2v2, Item& it) {
  const i64* seg = st.seg_tab + s * SEG_WORDS;
  it.e = entry_at(st.seg_ent ? st.seg_ent + s * ENT_WORDS : nullptr);
  const int n_mcu = mcus_per_image(H, W, h2v2);
  it.lo = clamp_i64(seg[SEG_LO], 0, st.n_bytes);
  it.hi = clamp_i64(seg[SEG_HI], it.lo, st.n_bytes);
  it.mcu0 = (int)clamp_i64(seg[SEG_MCU0], 0, n_mcu);
  it.mcu1 = (int)clamp_i64(seg[SEG_MCU1], it.mcu0, n_mcu);
  const int* rec = st.img_tab + img * IMG_WORDS;
  i64 q[3], dc[3], ac[3];
  for (int c = 0; c < 3; ++c) {
    q[c] = clamp_i64(rec[IMG_Q + c], 0, st.nQ - 1) * 64;
    dc[c] = clamp_i64(rec[IMG_DC + c], 0, st.nH - 1) * HT_WORDS;
    ac[c] = clamp_i64(rec[IMG_AC + c], 0, st.nH - 1) * HT_WORDS;
  }
  it.t = Tables{st.qt_pool, st.ht_pool, q[0], q[1], q[2], dc[0], dc[1], dc[2], ac[0], ac[1], ac[2]};
}

// -> false when image img (0 <= img < N, the caller's duty) has no segment k; the image's segment rows are clamped into [0, S].
VLA_JPEG_HD bool resolve_item(const Store& st, i64 img, int k, int H, int W, int h2v2, Item& it) {
  const i64 s0 = clamp_i64(st.img_seg[img], 0, st.S), s1 = clamp_i64(st.img_seg[img + 1], s0, st.S);
  if (k < 0 || k >= s1 - s0) return false;
  resolve_segment(st, img, s0 + k, H, W, h2v2, it);
  return true;
}

// Segment k of image img into the image's coefficient blocks.  -> ST_*, or -1 when the image has no segment k (nothing is written).
VLA_JPEG_HD int decode_item(const Store& st, i64 img, int k, int H, int W, int h2v2, short* __restrict coef) {
  Item it;
  if (!resolve_item(st, img, k, H, W, h2v2, it)) return -1;
  return decode_segment(st.bytes, it.lo, it.hi, it.e, it.mcu0, it.mcu1, H, W, h2v2, it.t, coef);
}

// ---------------------------------------------------------------------------------------------------------------- the scan index
// The walk that makes pieces of a segment (include/vla_jpeg_index.h): the Huffman decode of the MCUs [mcu0, mcu1) from bytes[lo, hi),
// coefficients discarded, and at every MCU whose distance from mcu0 is a multiple of piece_mcus (>= 1) a record of where the reader
// stands - a row of the segment table (`seg`: lo, hi, mcu0, mcu1) and one of the entry table (`ent`: bit, p0, p1, p2), `rows` of
// each, every word of them written, and no more whatever the stream holds.  `base` is added to the byte positions written (the
// caller may hand in a copy of the segment's bytes that starts at 0).  -> the walk's ST_*.
//
// Position: the reader refills up to 8 bytes ahead, so `pos` is not where the next bit lies.  8 * fed - n bits are consumed, and at
// a record all of them are bits of the data (no MCU in front ended truncated), so the next bit is bit c & 7 of data byte c >> 3; a
// cursor steps from byte to byte, over a stuffed 0x00 together with its 0xFF, and so never rests on one.  The cursor only moves
// forward: the whole walk reads every byte twice.
//
// hi: piece j ends where piece j + 1 begins - at its lo; one byte later when it begins inside a byte, which the two share; two when
// that byte is 0xFF, whose stuffed 0x00 must be inside the range or the reader takes the pair for a marker.  The last piece keeps the
// segment's hi.  A piece's decode consumes exactly the bits in front of the next piece's entry, all of them inside its range; what the
// reader supplies behind the range is zero bits that only a lookahead sees.  decode_symbol() settles on a code of length l by
// its first l bits alone (the lookup table has one entry for every continuation of a short code, and the search compares l-bit
// prefixes), and those l bits are bits of the data, so every symbol is the one the whole segment's decode reads there.
//
// A walk that stops with a non-zero status inside piece j has written pieces 0 .. j; piece j keeps the segment's hi, so its decode
// meets the same bits and fails at the same block.  Every later piece gets lo = hi = the segment's hi and a zero entry: its decode
// runs out of bytes at once, reports it and writes zero coefficients, which is what the whole segment's decode leaves behind a failure.
VLA_JPEG_HD int index_segment(const u8* bytes, i64 lo, i64 hi, i64 base, int mcu0, int mcu1, int h2v2, const Tables& t, int piece_mcus,
                              i64 rows, i64* __restrict seg, int* __restrict ent) {
  BitReader br;
  br_init(br, bytes, lo, hi);
  hi = br.end;
  int p0 = 0, p1 = 0, p2 = 0, status = ST_OK, left = 0;
  i64 j = 0, at = lo, at_byte = 0;                      // rows written; the cursor: data byte `at_byte` of the segment is bytes[at]
  short blk[64];
  const int nb = blocks_per_mcu(h2v2);
  for (int mcu = mcu0; (mcu < mcu1 || mcu == mcu0) && status == ST_OK; ++mcu) {         // (an empty segment is one empty piece)
    if (left == 0) {
      if (j >= rows) break;
      const i64 c = 8 * br.fed - br.n, bit = c & 7;
      for (; at_byte < (c >> 3) && at < hi; ++at_byte) at += (bytes[at] == 0xFF && at + 1 < hi) ? 2 : 1;
      if (j) seg[(j - 1) * SEG_WORDS + SEG_HI] = base + clamp_i64(at + (bit ? (at < hi && bytes[at] == 0xFF ? 2 : 1) : 0), lo, hi);
      const i64 m1 = clamp_i64((i64)mcu + piece_mcus, mcu0, mcu1);
      seg[j * SEG_WORDS + SEG_LO] = base + at;
      seg[j * SEG_WORDS + SEG_HI] = base + hi;
      seg[j * SEG_WORDS + SEG_MCU0] = mcu;
      seg[j * SEG_WORDS + SEG_MCU1] = m1;
      ent[j * ENT_WORDS + ENT_BIT] = (int)bit;
      ent[j * ENT_WORDS + ENT_P0] = p0;
      ent[j * ENT_WORDS + ENT_P1] = p1;
      ent[j * ENT_WORDS + ENT_P2] = p2;
      ++j;
      left = piece_mcus;
    }
    --left;
    for (int b = 0; b < nb && mcu < mcu1 && status == ST_OK; ++b) {
      const int comp = block_component(b, h2v2);
      int& pred = comp == 0 ? p0 : (comp == 1 ? p1 : p2);
      status = decode_block(br, table_dc(t, comp), table_ac(t, comp), table_q(t, comp), pred, blk);
    }
  }
  for (; j < rows; ++j) {                               // pieces behind a failure (or rows the segment has no MCUs for): nothing to read
    const i64 m0 = clamp_i64((i64)mcu0 + j * piece_mcus, mcu0, mcu1), m1 = clamp_i64(m0 + piece_mcus, mcu0, mcu1);
    seg[j * SEG_WORDS + SEG_LO] = seg[j * SEG_WORDS + SEG_HI] = base + hi;
    seg[j * SEG_WORDS + SEG_MCU0] = m0;
    seg[j * SEG_WORDS + SEG_MCU1] = m1;
    ent[j * ENT_WORDS + ENT_BIT] = ent[j * ENT_WORDS + ENT_P0] = ent[j * ENT_WORDS + ENT_P1] = ent[j * ENT_WORDS + ENT_P2] = 0;
  }
  return status;
}

// Work item s of the index build (0 <= s < S, the caller's duty), resolved from the tables: the segment as a segment of its image -
// the last image whose first segment row is not behind s, by a binary search that ends whatever img_seg holds - and the rows of the
// output it owns, piece_off[s] .. piece_off[s + 1] clamped into [0, S_out] and made monotone.
struct IndexItem {
  Item it;
  i64 r0, rows;
};

VLA_JPEG_HD IndexItem resolve_index_item(const Store& st, i64 N, i64 s, int H, int W, int h2v2, const i64* __restrict piece_off, i64 S_out) {
  i64 a = 0, b = N - 1;                                 // the answer lies in [a, b]
  while (a < b) {
    const i64 m = a + (b - a + 1) / 2;
    if (clamp_i64(st.img_seg[m], 0, st.S) <= s) a = m; else b = m - 1;
  }
  IndexItem w;
  resolve_segment(st, a, s, H, W, h2v2, w.it);
  w.r0 = clamp_i64(piece_off[s], 0, S_out);
  w.rows = clamp_i64(piece_off[s + 1], w.r0, S_out) - w.r0;
  return w;
}

// Segment s of the store walked and cut: -> the walk's ST_*
VLA_JPEG_HD int index_item(const Store& st, i64 N, i64 s, int H, int W, int h2v2, int piece_mcus, const i64* __restrict piece_off, i64 S_out,
                           i64* __restrict out_seg_tab, int* __restrict out_seg_ent) {
  const IndexItem w = resolve_index_item(st, N, s, H, W, h2v2, piece_off, S_out);
  return index_segment(st.bytes, w.it.lo, w.it.hi, 0, w.it.mcu0, w.it.mcu1, h2v2, w.it.t, piece_mcus, w.rows, out_seg_tab + w.r0 * SEG_WORDS,
                       out_seg_ent + w.r0 * ENT_WORDS);
}

// ---------------------------------------------------------------------------------------------------------------- the inverse DCT
// jidctint.c, jpeg_idct_islow, on dequantised coefficients: 64-bit intermediates as libjpeg's JLONG on LP64, an int workspace, the
// zero-column / zero-row shortcuts left out (they give the same bits).
VLA_JPEG_HD i64 descale(i64 x, int n) { return (x + ((i64)1 << (n - 1))) >> n; }

// libjpeg's IDCT range-limit table: index (x & 1023) -> clamp(x + 128) for |x| < 512, and what the table wraps to beyond
VLA_JPEG_HD u8 range_limit_idct(i64 x) {
  const int v = (int)(x & 1023);
  return (u8)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}

VLA_JPEG_HD void idct_1d(const i64 in[8], i64 out[8]) {
  // even part
  i64 z2 = in[2], z3 = in[6];
  i64 z1 = (z2 + z3) * 4433;
  i64 tmp2 = z1 + z3 * (-15137);
  i64 tmp3 = z1 + z2 * 6270;
  z2 = in[0];
  z3 = in[4];
  i64 tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;             // << CONST_BITS
  const i64 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  // odd part
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  i64 z4 = tmp1 + tmp3;
  const i64 z5 = (z3 + z4) * 9633;
  tmp0 *= 2446;
  tmp1 *= 16819;
  tmp2 *= 25172;
  tmp3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 *= -16069;
  z4 *= -3196;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  out[0] = tmp10 + tmp3;
  out[7] = tmp10 - tmp3;
  out[1] = tmp11 + tmp2;
  out[6] = tmp11 - tmp2;
  out[2] = tmp12 + tmp1;
  out[5] = tmp12 - tmp1;
  out[3] = tmp13 + tmp0;
  out[4] = tmp13 - tmp0;
}

// coef: 64 dequantised coefficients; out: 8 rows of 8 samples, `stride` bytes apart
VLA_JPEG_HD void idct_islow(const short* __restrict coef, u8* __restrict out, i64 stride) {
  int ws[64];
  for (int c = 0; c < 8; ++c) {                         // pass 1: columns, descaled by CONST_BITS - PASS1_BITS
    i64 in[8], o[8];
    for (int r = 0; r < 8; ++r) in[r] = coef[r * 8 + c];
    idct_1d(in, o);
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = (int)descale(o[r], 11);
  }
  for (int r = 0; r < 8; ++r) {                         // pass 2: rows, descaled by CONST_BITS + PASS1_BITS + 3
    i64 in[8], o[8];
    for (int c = 0; c < 8; ++c) in[c] = ws[r * 8 + c];
    idct_1d(in, o);
    for (int c = 0; c < 8; ++c) out[r * stride + c] = range_limit_idct(descale(o[c], 18));
  }
}

// ---------------------------------------------------------------------------------------------------------------- upsample, colour
// jdsample.c h2v2_fancy_upsample: the chroma sample of output pixel (y, x) from the (H / 2) x (W / 2) plane `c`.  Vertically the
// nearer row weighs 3 and the farther 1 (the row above for an even y, below for an odd one; replicated at the image's edge);
// horizontally the same with the roundings 8 (even x) and 7 (odd x), and 4 s at the first and last column.
VLA_JPEG_HD int upsample_h2v2(const u8* __restrict c, int ch, int cw, int y, int x) {
  const int cy = y >> 1, cx = x >> 1;
  int fy = (y & 1) ? cy + 1 : cy - 1;
  fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
  const u8* near = c + (i64)cy * cw;
  const u8* far = c + (i64)fy * cw;
  const int s = 3 * near[cx] + far[cx];
  if (x & 1) {
    if (cx == cw - 1) return (4 * s + 7) >> 4;
    return (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
  }
  if (cx == 0) return (4 * s + 8) >> 4;
  return (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

VLA_JPEG_HD u8 clamp_u8(int v) { return (u8)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// jdcolor.c ycc_rgb_convert: SCALEBITS 16, FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554
VLA_JPEG_HD void ycc_to_rgb(int yv, int cb, int cr, u8* __restrict rgb) {
  cb -= 128;
  cr -= 128;
  rgb[0] = clamp_u8(yv + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp_u8(yv + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = clamp_u8(yv + ((116130 * cb + 32768) >> 16));
}

// Pixel (y, x) of an image from its planes: Y [H, W], then Cb and Cr, [H / 2, W / 2] each (4:2:0) or [H, W] each (4:4:4)
VLA_JPEG_HD void plane_pixel(const u8* __restrict planes, int H, int W, int h2v2, int y, int x, u8* __restrict rgb) {
  const i64 hw = (i64)H * W;
  const int yv = planes[(i64)y * W + x];
  int cb, cr;
  if (h2v2) {
    const int ch = H >> 1, cw = W >> 1;
    cb = upsample_h2v2(planes + hw, ch, cw, y, x);
    cr = upsample_h2v2(planes + hw + (i64)ch * cw, ch, cw, y, x);
  } else {
    cb = planes[hw + (i64)y * W + x];
    cr = planes[2 * hw + (i64)y * W + x];
  }
  ycc_to_rgb(yv, cb, cr, rgb);
}

// Where the 8 x 8 samples of block `b` of an image (block_index's numbering) go in its planes: -> offset of the top-left sample, and
// the row stride
VLA_JPEG_HD i64 plane_offset(i64 b, int H, int W, int h2v2, i64& stride) {
  const int bw = W >> 3, bh = H >> 3;
  const i64 ny = (i64)bw * bh;
  if (b < ny || !h2v2) {
    const i64 comp = b / ny, r = b - comp * ny;
    stride = W;
    return comp * (i64)H * W + (r / bw) * 8 * W + (r % bw) * 8;
  }
  const int cbw = bw >> 1, cbh = bh >> 1, cw = W >> 1;
  const i64 nc = (i64)cbw * cbh, c = (b - ny) / nc, r = (b - ny) - c * nc;
  stride = cw;
  return (i64)H * W + c * (i64)(H >> 1) * cw + (r / cbw) * 8 * cw + (r % cbw) * 8;
}

}  // namespace vlajpeg
