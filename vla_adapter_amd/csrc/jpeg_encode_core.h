// The entropy coder of a baseline JPEG file, stated once for the device (csrc/jpeg_encode.hip) and for the host (the stand-alone program
// of tests/test_jpeg_encode_cpu.py, which runs it under the sanitizers): the standard Huffman tables in derived form, the symbol rule of
// one block, byte stuffing, the 1-bit padding at the end of a restart interval and the header.  Behind the forward half of
// csrc/jpeg_forward.h it writes, byte for byte, the file Pillow - libjpeg-turbo with its defaults - saves for quality q, 4:2:0 and
// restart_marker_rows r.  Every function is plain integer C++ and compiles with hipcc for both sides and with any
// host compiler.
//
// Accepted: 4:2:0, H and W multiples of 16 inside [16, 4096], a restart interval of restart_rows >= 1 rows of MCUs.  Optimised Huffman
// tables are not built: the four tables are the ones libjpeg installs by default (T.81 Annex K.3).
#pragma once

#include "jpeg_core.h"

namespace vlajpeg {

// ---------------------------------------------------------------------------------------------------------------- the standard tables
// Table t: 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance - the order in which the header writes them.
constexpr int ENC_TABLES = 4;

// how many codes of length l + 1 table t has (the BITS list of its DHT segment)
VLA_JPEG_HD int std_count(int t, int l) {
  constexpr u8 BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                              {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                              {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                              {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
  return BITS[t & 3][l & 15];
}

VLA_JPEG_HD int std_symbols(int t) { return (t & 1) ? 162 : 12; }

// symbol j of table t in code order (the HUFFVAL list); j < std_symbols(t)
VLA_JPEG_HD int std_value(int t, int j) {
  constexpr u8 AC_LUMA[162] = {
      0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa};
  constexpr u8 AC_CHROMA[162] = {
      0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
      0xfa};
  if (!(t & 1)) return j;                               // both DC tables: the categories 0 .. 11 in order
  j = j < 0 ? 0 : (j > 161 ? 161 : j);
  return (t & 2) ? AC_CHROMA[j] : AC_LUMA[j];
}

// The inverse of natural_order: where position p of the 8 x 8 block stands in zigzag order.
VLA_JPEG_HD int zigzag_of(int p) {
  constexpr u8 INV[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                          10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
  return INV[p & 63];
}

// The derived form of a table, ENC_WORDS words: [symbol] = (code length << 16) | code, 0 for a symbol the table does not hold.  The codes
// are the canonical ones of T.81 Annex C: symbols in HUFFVAL order, a code one larger than the one before, doubled at every length.
constexpr int ENC_WORDS = 256;

VLA_JPEG_HD void derive_codes(int t, unsigned* __restrict tab) {
  for (int s = 0; s < ENC_WORDS; ++s) tab[s] = 0;
  unsigned code = 0;
  int j = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < std_count(t, l - 1); ++i, ++j, ++code) tab[std_value(t, j) & 255] = ((unsigned)l << 16) | code;
    code <<= 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------- one block
// The category of a value: how many bits its magnitude has (jchuff.c nbits).
VLA_JPEG_HD int category(int v) {
  unsigned a = (unsigned)(v < 0 ? -v : v);
  int n = 0;
  while (a) {
    ++n;
    a >>= 1;
  }
  return n;
}

// What one coded value costs at most.  A Huffman code has at most 16 bits, the extra bits of a DC difference at most 11, those of an AC
// coefficient at most 10: no emission is longer than 27 bits, and a block emits at most 64 of them (a ZRL stands for 16 coefficients and
// EOB for at least one, so neither adds to the count) - 64 * 27 = 1728 bits = 216 bytes a block before stuffing, twice that behind it.
constexpr int MAX_EMIT_BITS = 27, MAX_BLOCK_BITS = 64 * MAX_EMIT_BITS, MAX_BLOCK_BYTES = MAX_BLOCK_BITS / 8;

// The symbol rule of one block (T.81 F.1.2; jchuff.c encode_one_block).  zz: its 64 quantised coefficients in zigzag order; pred: the
// DC value of the previous block of the same component inside the restart interval, 0 for the first; dc, ac: the component's tables in
// derived form.  Calls emit(bits, n) once per coded value with the Huffman code and the extra bits joined, n <= MAX_EMIT_BITS, most
// significant bit first, and returns the sum of the n.  A negative value's extra bits are the low bits of value - 1 (one's complement).
// Values no baseline file holds - a DC difference past 11 bits, an AC coefficient past 10 - are coded as the largest category: the
// forward half cannot produce them, and the bound above holds for any input.
template <typename Emit>
VLA_JPEG_HD int code_block(const short* __restrict zz, int pred, const unsigned* __restrict dc, const unsigned* __restrict ac, Emit& emit) {
  int total = 0;
  {
    const int d = (int)zz[0] - pred;
    int s = category(d);
    s = s > 11 ? 11 : s;
    const unsigned extra = (unsigned)(d < 0 ? d - 1 : d) & ((1u << s) - 1u);
    const unsigned e = dc[s];
    emit(((e & 0xffffu) << s) | extra, (int)(e >> 16) + s);
    total += (int)(e >> 16) + s;
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    while (run > 15) {                                  // ZRL: sixteen zeros
      const unsigned e = ac[0xF0];
      emit(e & 0xffffu, (int)(e >> 16));
      total += (int)(e >> 16);
      run -= 16;
    }
    int s = category(v);
    s = s > 10 ? 10 : s;
    const unsigned extra = (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
    const unsigned e = ac[(run << 4) | s];
    emit(((e & 0xffffu) << s) | extra, (int)(e >> 16) + s);
    total += (int)(e >> 16) + s;
    run = 0;
  }
  if (run) {                                            // EOB: zeros to the end of the block
    const unsigned e = ac[0x00];
    emit(e & 0xffffu, (int)(e >> 16));
    total += (int)(e >> 16);
  }
  return total;
}

// Which block of a restart interval carries the DC predictor of block b of it (blocks in coding order, six per MCU: Y Y Y Y Cb Cr):
// the previous block of the same component, -1 when b is the first of its component in the interval.
VLA_JPEG_HD int predictor_block(int b) {
  const int blk = b % 6;
  const int p = blk == 0 ? b - 3 : (blk < 4 ? b - 1 : b - 6);
  return p < 0 ? -1 : p;
}

// ---------------------------------------------------------------------------------------------------------------- bytes
// Byte stuffing (T.81 F.1.2.3): a data byte 0xFF is followed by a zero byte.
VLA_JPEG_HD int stuffed_size(unsigned byte) { return byte == 0xFF ? 2 : 1; }

// Padding (F.1.2.3): the bits behind the last code of an interval, up to the byte's end, are ones; `bits` of the last byte are used.
VLA_JPEG_HD unsigned pad_ones(unsigned byte, int bits) { return bits ? (byte | (0xFFu >> bits)) & 0xFFu : byte; }

// The serial bit writer of the host: put() as emit() calls it, flush() at the end of an interval.  `cap`: the bytes `out` holds; a
// writer that runs out of them sets `overflow` and writes no further.
struct BitWriter {
  u8* out;
  i64 pos, cap;
  u64 acc;
  int n, overflow;
  VLA_JPEG_HD void byte(unsigned b) {
    if (pos + stuffed_size(b) > cap) {
      overflow = 1;
      return;
    }
    out[pos++] = (u8)b;
    if (b == 0xFF) out[pos++] = 0;
  }
  VLA_JPEG_HD void operator()(unsigned bits, int k) {
    acc = (acc << k) | bits;
    n += k;
    while (n >= 8) {
      n -= 8;
      byte((unsigned)(acc >> n) & 0xFFu);
    }
  }
  VLA_JPEG_HD void flush() {
    if (n) byte(pad_ones((unsigned)(acc << (8 - n)) & 0xFFu, n));
    n = 0;
    acc = 0;
  }
};

VLA_JPEG_HD void bw_init(BitWriter& w, u8* out, i64 cap) {
  w.out = out;
  w.pos = 0;
  w.cap = cap;
  w.acc = 0;
  w.n = w.overflow = 0;
}

// ---------------------------------------------------------------------------------------------------------------- the file
VLA_JPEG_HD bool encode_shape_ok(int H, int W, int restart_rows) {
  return H >= 16 && W >= 16 && H <= 4096 && W <= 4096 && H % 16 == 0 && W % 16 == 0 && restart_rows >= 1 &&
         (long long)restart_rows * (W >> 4) <= 65535;      // (the DRI segment counts the interval's MCUs in 16 bits)
}
VLA_JPEG_HD int intervals_per_image(int H, int restart_rows) { return ((H >> 4) + restart_rows - 1) / restart_rows; }
// the marker between interval i - 1 and interval i, i >= 1: RSTn with n = (i - 1) mod 8
VLA_JPEG_HD unsigned restart_marker(int i) { return 0xD0u + (unsigned)((i - 1) & 7); }

// SOI, JFIF APP0, DQT 0, DQT 1, SOF0, DHT DC0, DHT AC0, DHT DC1, DHT AC1, DRI, SOS: 615 bytes up to the SOS marker, 14 of SOS.
constexpr int HEADER_BYTES = 629;

// The header of an H x W 4:2:0 file into out[0 .. HEADER_BYTES).  qtab: the luminance and the chrominance quantisation table, 64
// entries each in natural order (the file lists them in zigzag order).  The restart interval it declares is restart_rows rows of MCUs.
VLA_JPEG_HD int write_header(u8* __restrict out, int H, int W, const unsigned short* __restrict qtab, int restart_rows) {
  int p = 0;
  auto put = [&](unsigned b) { out[p++] = (u8)b; };
  auto put16 = [&](unsigned v) { put(v >> 8); put(v & 255); };
  put(0xFF), put(0xD8);
  put(0xFF), put(0xE0), put16(16);                      // JFIF 1.01, no units, aspect 1 : 1, no thumbnail
  constexpr u8 JFIF[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 14; ++i) put(JFIF[i]);
  for (int t = 0; t < 2; ++t) {
    put(0xFF), put(0xDB), put16(67), put(t);
    for (int k = 0; k < 64; ++k) {
      const unsigned q = qtab[t * 64 + natural_order(k)];
      put(q < 1 ? 1 : (q > 255 ? 255 : q));
    }
  }
  put(0xFF), put(0xC0), put16(17), put(8), put16(H), put16(W), put(3);
  put(1), put(0x22), put(0), put(2), put(0x11), put(1), put(3), put(0x11), put(1);
  for (int t = 0; t < ENC_TABLES; ++t) {
    put(0xFF), put(0xC4), put16(19 + std_symbols(t)), put(((t & 1) << 4) | (t >> 1));
    for (int l = 0; l < 16; ++l) put(std_count(t, l));
    for (int j = 0; j < std_symbols(t); ++j) put(std_value(t, j));
  }
  put(0xFF), put(0xDD), put16(4), put16(restart_rows * (W >> 4));
  put(0xFF), put(0xDA), put16(12), put(3), put(1), put(0x00), put(2), put(0x11), put(3), put(0x11), put(0), put(63), put(0);
  return p;
}

// The 64 quantised coefficients of block `blk` of MCU `mcu` in zigzag order, from an image's quantised values in the decode's block
// layout (block_index, natural order: what forward_mcu's `quant` holds).  The device keeps them in this order from the start.
VLA_JPEG_HD void block_zigzag(const short* __restrict quant, int mcu, int blk, int H, int W, short* __restrict zz) {
  int comp;
  const short* s = quant + (i64)block_index(mcu, blk, W >> 3, H >> 3, 1, comp) * 64;
  for (int k = 0; k < 64; ++k) zz[k] = s[natural_order(k)];
}

// One whole file on the host, serially: header, the intervals with RSTn between them, EOI.  quant: the image's quantised values as
// forward_mcu leaves them.  -> the bytes written, or -1 when `cap` does not hold them.
inline i64 encode_image_serial(const short* quant, int H, int W, const unsigned short* qtab, int restart_rows, u8* out, i64 cap) {
  if (!encode_shape_ok(H, W, restart_rows) || cap < HEADER_BYTES + 2) return -1;
  unsigned tabs[ENC_TABLES][ENC_WORDS];
  for (int t = 0; t < ENC_TABLES; ++t) derive_codes(t, tabs[t]);
  i64 p = write_header(out, H, W, qtab, restart_rows);
  const int n_mcu = mcus_per_image(H, W, 1), per = restart_rows * (W >> 4);
  for (int i = 0, m0 = 0; m0 < n_mcu; ++i, m0 += per) {
    if (i) {
      if (p + 2 > cap) return -1;
      out[p++] = 0xFF;
      out[p++] = (u8)restart_marker(i);
    }
    BitWriter w;
    bw_init(w, out + p, cap - p);
    const int m1 = m0 + per < n_mcu ? m0 + per : n_mcu;
    int pred[3] = {0, 0, 0};
    for (int mcu = m0; mcu < m1; ++mcu)
      for (int blk = 0; blk < 6; ++blk) {
        short zz[64];
        block_zigzag(quant, mcu, blk, H, W, zz);
        const int c = block_component(blk, 1);
        code_block(zz, pred[c], tabs[c ? 2 : 0], tabs[c ? 3 : 1], w);
        pred[c] = zz[0];
      }
    w.flush();
    if (w.overflow) return -1;
    p += w.pos;
  }
  if (p + 2 > cap) return -1;
  out[p++] = 0xFF;
  out[p++] = 0xD9;
  return p;
}

}  // namespace vlajpeg
