// The forward half of a baseline JPEG file, stated once for the device (csrc/policy_image.hip) and for the host (the stand-alone
// program of tests/test_policy_image_cpu.py, which runs it under the sanitizers): colour conversion, h2v2 chroma downsampling, the
// islow forward DCT, quantisation and dequantisation.  Joined to the inverse half of csrc/jpeg_core.h it is what writing a frame as a
// 4:2:0 file and decoding it again does to the pixels: the entropy coding between the two halves is lossless and
// is left out.  Every function is plain integer C++ and compiles with hipcc for both sides and with any host compiler.
//
// The arithmetic is libjpeg's defaults, which is what Pillow encodes with: jccolor.c rgb_ycc_convert (SCALEBITS 16), jcsample.c
// h2v2_downsample with its alternating bias, jfdctint.c jpeg_fdct_islow (CONST_BITS 13, PASS1_BITS 2) and the quantisation by division
// of jcdctmgr.c, whose divisors are the table's entries times 8.
#pragma once

#include "jpeg_core.h"

namespace vlajpeg {

// jccolor.c: FIX(x) = (int)(x * 65536 + 0.5); ONE_HALF = 32768; CBCR_OFFSET = 128 << 16.  The chroma terms carry ONE_HALF - 1, the
// luma term ONE_HALF.
VLA_JPEG_HD int rgb_to_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
VLA_JPEG_HD int rgb_to_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
VLA_JPEG_HD int rgb_to_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// jcsample.c h2v2_downsample: the chroma sample of output column cx from the sum of its four full-size samples; the bias alternates
// 1, 2, 1, 2 ... along a row so that the roundings do not all go one way.
VLA_JPEG_HD int downsample_h2v2(int sum4, int cx) { return (sum4 + 1 + (cx & 1)) >> 2; }

// One pass of jpeg_fdct_islow over eight values: `first` = the row pass (outputs scaled up by PASS1_BITS), else the column pass
// (PASS1_BITS and the factor of 8 of the unnormalised transform stay in: the quantiser divides them out).  64-bit intermediates, as
// the inverse transform of the core has them.
VLA_JPEG_HD void fdct_1d(const i64 d[8], i64 out[8], bool first) {
  const i64 tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const i64 tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const i64 tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int n = first ? 11 : 15;                        // CONST_BITS - PASS1_BITS, CONST_BITS + PASS1_BITS
  out[0] = first ? (tmp10 + tmp11) * 4 : descale(tmp10 + tmp11, 2);
  out[4] = first ? (tmp10 - tmp11) * 4 : descale(tmp10 - tmp11, 2);
  i64 z1 = (tmp12 + tmp13) * 4433;
  out[2] = descale(z1 + tmp13 * 6270, n);
  out[6] = descale(z1 + tmp12 * (-15137), n);
  z1 = tmp4 + tmp7;
  i64 z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const i64 z5 = (z3 + z4) * 9633;
  const i64 t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * (-16069) + z5;
  z4 = z4 * (-3196) + z5;
  out[7] = descale(t4 + z1 + z3, n);
  out[5] = descale(t5 + z2 + z4, n);
  out[3] = descale(t6 + z2 + z3, n);
  out[1] = descale(t7 + z1 + z4, n);
}

// jcdctmgr.c quantize: divisor q << 3, rounded half away from zero; then the decoder's product with q, as decode_block() stores it.
// q: an entry of the quantisation table, 1 .. 255 (a zero is taken as 1: no table makes the division fault).
VLA_JPEG_HD int quantise(int c, int q) {
  const int qv = (q < 1 ? 1 : q) << 3;
  const int t = ((c < 0 ? -c : c) + (qv >> 1)) / qv;
  return c < 0 ? -t : t;
}
VLA_JPEG_HD short requantise(int c, int q) { return saturate16((i64)quantise(c, q) * (q < 1 ? 1 : q)); }

// One 8 x 8 block: samples (0 .. 255, rows `stride` apart) -> 64 dequantised coefficients in natural order, as stage B of the decode
// reads them.  q: the block's quantisation table in natural order.  `quant` (optional): the quantised values, for the host's checks.
VLA_JPEG_HD void forward_block(const u8* __restrict s, i64 stride, const unsigned short* __restrict q, short* __restrict out, short* quant = nullptr) {
  int ws[64];
  for (int r = 0; r < 8; ++r) {                         // pass 1: rows
    i64 in[8], o[8];
    for (int c = 0; c < 8; ++c) in[c] = (int)s[r * stride + c] - 128;
    fdct_1d(in, o, true);
    for (int c = 0; c < 8; ++c) ws[r * 8 + c] = (int)o[c];
  }
  for (int c = 0; c < 8; ++c) {                         // pass 2: columns
    i64 in[8], o[8];
    for (int r = 0; r < 8; ++r) in[r] = ws[r * 8 + c];
    fdct_1d(in, o, false);
    for (int r = 0; r < 8; ++r) {
      out[r * 8 + c] = requantise((int)o[r], q[r * 8 + c]);
      if (quant) quant[r * 8 + c] = (short)quantise((int)o[r], q[r * 8 + c]);
    }
  }
}

// One 16 x 16 MCU of a 4:2:0 image on the host, the whole chain: RGB rows (`row_stride` bytes apart) -> its six coefficient blocks at
// their places (block_index) in the image's layout `coef`.  qtab: the luma table, then the chroma table, 64 entries each in natural
// order.  The device does the same with the work spread over a wave (csrc/policy_image.hip).
VLA_JPEG_HD void forward_mcu(const u8* __restrict rgb, i64 row_stride, int mcu, int H, int W, const unsigned short* __restrict qtab,
                             short* __restrict coef, short* quant = nullptr) {
  u8 y[256], cb[64], cr[64];
  for (int cy = 0; cy < 8; ++cy)
    for (int cx = 0; cx < 8; ++cx) {
      int sb = 0, sr = 0;
      for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
          const u8* p = rgb + (2 * cy + dy) * row_stride + (2 * cx + dx) * 3;
          y[(2 * cy + dy) * 16 + 2 * cx + dx] = (u8)rgb_to_y(p[0], p[1], p[2]);
          sb += rgb_to_cb(p[0], p[1], p[2]);
          sr += rgb_to_cr(p[0], p[1], p[2]);
        }
      cb[cy * 8 + cx] = (u8)downsample_h2v2(sb, cx);    // (an MCU is 8 chroma columns wide: the column's parity in the image is cx's)
      cr[cy * 8 + cx] = (u8)downsample_h2v2(sr, cx);
    }
  for (int blk = 0; blk < 6; ++blk) {
    int comp;
    const i64 at = (i64)block_index(mcu, blk, W >> 3, H >> 3, 1, comp) * 64;
    const u8* s = blk < 4 ? y + (blk >> 1) * 128 + (blk & 1) * 8 : (blk == 4 ? cb : cr);
    forward_block(s, blk < 4 ? 16 : 8, qtab + (comp ? 64 : 0), coef + at, quant ? quant + at : nullptr);
  }
}

}  // namespace vlajpeg
