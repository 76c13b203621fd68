// The scan index of a JPEG frame store, built once at load: every segment longer than piece_mcus MCUs is walked serially - Huffman
// decode with the coefficients discarded, csrc/jpeg_core.h: index_segment - and cut into pieces, each with the byte, the bit and the
// DC predictors at which it begins.  Declared in include/vla_jpeg_index.h; the per-batch decode that begins every piece from its
// record is vla_jpeg_decode_rows_at in csrc/jpeg.hip.  One launch on the caller's stream, nothing allocated or read back.
//
// One work item per segment of the slice [s_begin, s_end).  As in the decode the mapping of items to lanes is a launch argument: one
// lane per segment (64 walks share a wave) or one wave per segment (its first lane walks, from LDS).  The build is bound by throughput
// over the whole store, not by the latency of one walk: measured, a store of two slices builds in 0.07 s per
// 10 000 frames of 224 x 224 with a lane per segment and in 0.16 s with a wave per segment, so the caller's default is the lane mapping;
// only a store smaller than a slice, whose build is one walk long either way, builds faster with waves.
//
// A walk of a 224 x 224 scan takes a lane 12 - 25 ms (the one-segment rows of table (a)), and a launch lasts as
// long as its slowest wave times the rounds of waves the device needs.  The caller (jpeg_store.py: BUILD_SLICE) therefore hands in
// slices of a few thousand segments: 4096 lanes are 64 waves, fewer than the compute units, so a launch is one walk long - tens of
// milliseconds (29 measured) - whatever the size of the store, and a shared device is never held by one launch for longer.
#include "common.h"
#include "jpeg_core.h"
#include "../../include/vla_jpeg_index.h"

namespace {

using namespace vlajpeg;

constexpr int INDEX_THREADS = 64;               // one wave per workgroup
constexpr int INDEX_STAGE_BYTES = 32 * 1024;    // the wave mapping walks a segment of up to this many bytes from a copy in LDS

// One lane per segment: grid ceil((s_end - s_begin) / 64) workgroups of one wave; every lane walks its own segment from global memory.
__global__ void __launch_bounds__(INDEX_THREADS)
jpeg_index_lane_kernel(const u8* __restrict__ bytes, i64 n_bytes, const i64* __restrict__ img_seg, const i64* __restrict__ seg_tab, i64 S,
                       const int* __restrict__ img_tab, const unsigned short* __restrict__ qt_pool, int nQ, const int* __restrict__ ht_pool, int nH,
                       i64 N, int H, int W, int h2v2, int piece_mcus, const i64* __restrict__ piece_off, i64 s_begin, i64 s_end,
                       i64* __restrict__ out_seg_tab, int* __restrict__ out_seg_ent, i64 S_out, u8* __restrict__ out_status) {
  const i64 s = s_begin + (i64)blockIdx.x * INDEX_THREADS + threadIdx.x;
  if (s >= s_end) return;
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH};
  out_status[s] = (u8)index_item(st, N, s, H, W, h2v2, piece_mcus, piece_off, S_out, out_seg_tab, out_seg_ent);
}

// One wave per segment: grid s_end - s_begin workgroups of one wave.  The wave copies the image's six Huffman tables and, when they
// fit, the segment's bytes into LDS; then its first lane walks.  (The quantisation tables stay where they are: the walk multiplies
// by them and discards the product.)
__global__ void __launch_bounds__(INDEX_THREADS)
jpeg_index_wave_kernel(const u8* __restrict__ bytes, i64 n_bytes, const i64* __restrict__ img_seg, const i64* __restrict__ seg_tab, i64 S,
                       const int* __restrict__ img_tab, const unsigned short* __restrict__ qt_pool, int nQ, const int* __restrict__ ht_pool, int nH,
                       i64 N, int H, int W, int h2v2, int piece_mcus, const i64* __restrict__ piece_off, i64 s_begin, i64 s_end,
                       i64* __restrict__ out_seg_tab, int* __restrict__ out_seg_ent, i64 S_out, u8* __restrict__ out_status) {
  __shared__ int s_ht[6 * HT_WORDS];
  __shared__ u8 s_bytes[INDEX_STAGE_BYTES];
  const i64 s = s_begin + blockIdx.x;                   // (the grid is exactly the slice)
  const int lane = threadIdx.x;
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH};
  const IndexItem w = resolve_index_item(st, N, s, H, W, h2v2, piece_off, S_out);         // (uniform over the wave)
  const i64 len = w.it.hi - w.it.lo;
  const bool staged = len <= INDEX_STAGE_BYTES;
  for (int c = 0; c < 3; ++c)
    for (int i = lane; i < HT_WORDS; i += INDEX_THREADS) {
      s_ht[c * HT_WORDS + i] = table_dc(w.it.t, c)[i];
      s_ht[(3 + c) * HT_WORDS + i] = table_ac(w.it.t, c)[i];
    }
  if (staged)
    for (int i = lane; i < (int)len; i += INDEX_THREADS) s_bytes[i] = bytes[w.it.lo + i];
  __syncthreads();
  if (lane != 0) return;
  Tables t = w.it.t;
  t.ht = s_ht;
  t.dc0 = 0, t.dc1 = HT_WORDS, t.dc2 = 2 * HT_WORDS;
  t.ac0 = 3 * HT_WORDS, t.ac1 = 4 * HT_WORDS, t.ac2 = 5 * HT_WORDS;
  i64* __restrict__ seg = out_seg_tab + w.r0 * SEG_WORDS;
  int* __restrict__ ent = out_seg_ent + w.r0 * ENT_WORDS;
  int rc;
  if (staged)
    rc = index_segment(s_bytes, 0, len, w.it.lo, w.it.mcu0, w.it.mcu1, h2v2, t, piece_mcus, w.rows, seg, ent);
  else
    rc = index_segment(bytes, w.it.lo, w.it.hi, 0, w.it.mcu0, w.it.mcu1, h2v2, t, piece_mcus, w.rows, seg, ent);
  out_status[s] = (u8)rc;
}

}  // namespace

extern "C" int vla_jpeg_index_build(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg,
                                    const long long* seg_tab, long long S, const int* img_tab, const unsigned short* qt_pool, int nQ,
                                    const int* ht_pool, int nH, long long N, int H, int W, int h2v2, int piece_mcus,
                                    const long long* piece_off, long long s_begin, long long s_end, int mapping, long long* out_seg_tab,
                                    int* out_seg_ent, long long S_out, unsigned char* out_status) {
  VLA_REQUIRE(bytes && img_seg && seg_tab && img_tab && qt_pool && ht_pool && piece_off, "jpeg_index_build: null input pointer");
  VLA_REQUIRE(out_seg_tab && out_seg_ent && out_status, "jpeg_index_build: null output pointer");
  VLA_REQUIRE(H >= 16 && W >= 16 && H <= 4096 && W <= 4096 && H % 16 == 0 && W % 16 == 0 && (h2v2 == 0 || h2v2 == 1),
              "jpeg_index_build: H and W must be multiples of 16 inside [16, 4096], h2v2 0 or 1");
  VLA_REQUIRE(n_bytes >= 1 && S >= 1 && nQ >= 1 && nH >= 1 && N >= 1 && S_out >= 1, "jpeg_index_build: n_bytes, S, nQ, nH, N, S_out >= 1");
  VLA_REQUIRE(piece_mcus >= 1 && piece_mcus <= (1 << 20) && (mapping == 0 || mapping == 1), "jpeg_index_build: 1 <= piece_mcus <= 2^20, mapping 0 or 1");
  VLA_REQUIRE(s_begin >= 0 && s_begin <= s_end && s_end <= S, "jpeg_index_build: 0 <= s_begin <= s_end <= S");
  const long long items = s_end - s_begin;
  if (items == 0) return VLA_OK;
  VLA_REQUIRE(items <= 0x7fffffffll, "jpeg_index_build: the slice is too large for one grid");
  const hipStream_t st = (hipStream_t)stream;
  if (mapping)
    hipLaunchKernelGGL(jpeg_index_wave_kernel, dim3((unsigned)items), dim3(INDEX_THREADS), 0, st, bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt_pool,
                       nQ, ht_pool, nH, N, H, W, h2v2, piece_mcus, piece_off, s_begin, s_end, out_seg_tab, out_seg_ent, S_out, out_status);
  else
    hipLaunchKernelGGL(jpeg_index_lane_kernel, dim3((unsigned)((items + INDEX_THREADS - 1) / INDEX_THREADS)), dim3(INDEX_THREADS), 0, st, bytes,
                       n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH, N, H, W, h2v2, piece_mcus, piece_off, s_begin, s_end,
                       out_seg_tab, out_seg_ent, S_out, out_status);
  VLA_CHECK_LAUNCH("jpeg_index_build");
  return VLA_OK;
}
