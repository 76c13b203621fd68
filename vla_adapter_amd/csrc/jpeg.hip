// Training from JPEG-compressed episodes: the frames of a batch decoded where the data lives.  Declared in include/vla_jpeg.h (and
// include/vla_jpeg_index.h: the same decode with an entry state per segment, for stores that carry a scan index); the
// decode itself - bit reader, Huffman symbols, blocks, inverse DCT, upsampling, colour - is csrc/jpeg_core.h, which the host compiles
// too (tests/test_jpeg_core_cpu.py runs it under the sanitizers).  Three launches on the caller's stream, nothing allocated or read
// back: a captured graph may hold them.
//   jpeg_entropy_*_kernel one work item per (image of the batch, segment): Huffman decode -> dequantised int16 blocks in workspace
//   jpeg_idct_kernel      one thread per 8 x 8 block: islow inverse DCT -> the u8 planes Y, Cb, Cr in workspace
//   jpeg_pixels_kernel    one thread per 4 pixels of a row: fancy upsampling, YCbCr -> RGB -> out_frames
// The last two are stage B, launched through vlajpeg::stage_b (jpeg_stage_b.h): the JPEG round trip of csrc/policy_image.hip puts its
// own coefficient blocks in front of the same two kernels.
// Entropy decode is serial per segment and lanes diverge (every lane follows its own stream), so the mapping of items to lanes is a
// launch argument: one lane per item (64 segments share a wave and its instruction stream) or one wave per item (the first lane
// decodes; no divergence, 64 times the waves).  DESIGN.md section 18 has the measurements of both.
#include "common.h"
#include "episode_row.h"                        // episode_row: the row a sample reads, shared with episodes.hip
#include "jpeg_core.h"
#include "jpeg_stage_b.h"
#include "../../include/vla_jpeg.h"
#include "../../include/vla_jpeg_index.h"

namespace {

using namespace vlajpeg;

constexpr int ENTROPY_THREADS = 64;             // one wave per workgroup: the items spread over the CUs
constexpr int IDCT_THREADS = 256;
constexpr int PIXEL_THREADS = 256;

// Item (slot, k) of the entropy stage - segment k of the image in slot b * n_img + cam - and the store's image it decodes.
struct ItemId {
  int slot, k;
  i64 img;                                      // inside [0, T * n_img)
};

__device__ __forceinline__ ItemId item_id(i64 item, int max_seg, int n_img, const i64* __restrict__ episode_off, int E, i64 T,
                                          const int* __restrict__ ep, const i64* __restrict__ row) {
  ItemId id;
  id.slot = (int)(item / max_seg);
  id.k = (int)(item - (i64)id.slot * max_seg);
  const int b = id.slot / n_img, cam = id.slot - b * n_img;
  id.img = episode_row(episode_off, ep, row, b, E, T).r * n_img + cam;
  return id;
}

constexpr int STAGE_BYTES = 32 * 1024;           // a wave stages a segment of up to this many bytes in LDS (a 256 x 256 q95 frame fits)

// One lane per item: grid ceil(B * n_img * max_seg / 64) workgroups of one wave.  Item = (slot, k): segment k of the image in slot
// b * n_img + cam.  Every lane reads its own stream and its own image's tables from global memory.  seg_ent: the entry state of every
// segment (include/vla_jpeg_index.h), or null - every segment starts behind a marker, with no bit consumed and zero predictors.
__global__ void __launch_bounds__(ENTROPY_THREADS)
jpeg_entropy_lane_kernel(const u8* __restrict__ bytes, i64 n_bytes, const i64* __restrict__ img_seg, const i64* __restrict__ seg_tab, i64 S,
                         const int* __restrict__ img_tab, const unsigned short* __restrict__ qt_pool, int nQ, const int* __restrict__ ht_pool,
                         int nH, const i64* __restrict__ episode_off, int E, i64 T, const int* __restrict__ ep, const i64* __restrict__ row,
                         int B, int n_img, int H, int W, int h2v2, int max_seg, const int* __restrict__ seg_ent, short* __restrict__ coef,
                         u8* __restrict__ status) {
  const i64 item = (i64)blockIdx.x * ENTROPY_THREADS + threadIdx.x;
  if (item >= (i64)B * n_img * max_seg) return;
  const ItemId id = item_id(item, max_seg, n_img, episode_off, E, T, ep, row);
  const int slot = id.slot, k = id.k;
  const i64 img = id.img;
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH, seg_ent};
  const int rc = decode_item(st, img, k, H, W, h2v2, coef + (i64)slot * blocks_per_image(H, W, h2v2) * 64);
  status[item] = (u8)(rc < 0 ? ST_OK : rc);             // (no segment k in this image: nothing to decode)
}

// One wave per item: grid B * n_img * max_seg workgroups of one wave.  The decode is a chain of dependent loads - stream byte, table
// entry, quantiser - so the wave first copies what its segment reads into LDS, all 64 lanes side by side: the image's six Huffman
// tables, its three quantisation tables and the segment's bytes (the first STAGE_BYTES of them: a longer segment is read from global
// memory).  Then its first lane decodes; nothing diverges.
__global__ void __launch_bounds__(ENTROPY_THREADS)
jpeg_entropy_wave_kernel(const u8* __restrict__ bytes, i64 n_bytes, const i64* __restrict__ img_seg, const i64* __restrict__ seg_tab, i64 S,
                         const int* __restrict__ img_tab, const unsigned short* __restrict__ qt_pool, int nQ, const int* __restrict__ ht_pool,
                         int nH, const i64* __restrict__ episode_off, int E, i64 T, const int* __restrict__ ep, const i64* __restrict__ row,
                         int B, int n_img, int H, int W, int h2v2, int max_seg, const int* __restrict__ seg_ent, short* __restrict__ coef,
                         u8* __restrict__ status) {
  __shared__ int s_ht[6 * HT_WORDS];
  __shared__ unsigned short s_q[3 * 64];
  __shared__ u8 s_bytes[STAGE_BYTES];
  const i64 item = blockIdx.x;                          // (the grid is exactly the items)
  const int lane = threadIdx.x;
  const ItemId id = item_id(item, max_seg, n_img, episode_off, E, T, ep, row);
  const int slot = id.slot, k = id.k;
  const i64 img = id.img;
  const Store st{bytes, n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH, seg_ent};
  Item it;
  if (!resolve_item(st, img, k, H, W, h2v2, it)) {      // (uniform over the wave: no segment k in this image)
    if (lane == 0) status[item] = ST_OK;
    return;
  }
  const i64 len = it.hi - it.lo;
  const bool staged = len <= STAGE_BYTES;
  for (int c = 0; c < 3; ++c) {
    for (int i = lane; i < HT_WORDS; i += ENTROPY_THREADS) {
      s_ht[c * HT_WORDS + i] = table_dc(it.t, c)[i];
      s_ht[(3 + c) * HT_WORDS + i] = table_ac(it.t, c)[i];
    }
    s_q[c * 64 + lane] = table_q(it.t, c)[lane];
  }
  if (staged)
    for (int i = lane; i < (int)len; i += ENTROPY_THREADS) s_bytes[i] = bytes[it.lo + i];
  __syncthreads();
  if (lane != 0) return;
  Tables t = it.t;                                      // the same tables, now at their places in LDS
  t.q = s_q;
  t.ht = s_ht;
  t.q0 = 0, t.q1 = 64, t.q2 = 128;
  t.dc0 = 0, t.dc1 = HT_WORDS, t.dc2 = 2 * HT_WORDS;
  t.ac0 = 3 * HT_WORDS, t.ac1 = 4 * HT_WORDS, t.ac2 = 5 * HT_WORDS;
  short* __restrict__ out = coef + (i64)slot * blocks_per_image(H, W, h2v2) * 64;
  int rc;
  if (staged)
    rc = decode_segment(s_bytes, 0, len, it.e, it.mcu0, it.mcu1, H, W, h2v2, t, out);
  else
    rc = decode_segment(bytes, it.lo, it.hi, it.e, it.mcu0, it.mcu1, H, W, h2v2, t, out);
  status[item] = (u8)rc;
}

// one thread per block of the batch: coef [slots, blocks, 64] -> planes [slots, plane_bytes]
__global__ void __launch_bounds__(IDCT_THREADS)
jpeg_idct_kernel(const short* __restrict__ coef, u8* __restrict__ planes, i64 n_blocks, i64 per_image, i64 plane_bytes, int H, int W, int h2v2) {
  const i64 i = (i64)blockIdx.x * IDCT_THREADS + threadIdx.x;
  if (i >= n_blocks) return;
  const i64 slot = i / per_image, blk = i - slot * per_image;
  alignas(16) short c[64];
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(coef + i * 64);            // (workspace is 16-byte aligned)
#pragma unroll
  for (int j = 0; j < 8; ++j) reinterpret_cast<uint4*>(c)[j] = src[j];
  i64 stride;
  u8* __restrict__ dst = planes + slot * plane_bytes + plane_offset(blk, H, W, h2v2, stride);
  idct_islow(c, dst, stride);
}

// one thread per 4 consecutive pixels of a row (W is a multiple of 16): 12 bytes, as three words when out_frames allows
template <bool WIDE>
__global__ void __launch_bounds__(PIXEL_THREADS)
jpeg_pixels_kernel(const u8* __restrict__ planes, u8* __restrict__ out_frames, i64 n_quads, i64 plane_bytes, i64 out_stride, int H, int W, int h2v2) {
  const i64 i = (i64)blockIdx.x * PIXEL_THREADS + threadIdx.x;
  if (i >= n_quads) return;
  const int qw = W >> 2;
  const i64 per_image = (i64)H * qw, slot = i / per_image, rem = i - slot * per_image;
  const int y = (int)(rem / qw), x = (int)(rem - (i64)y * qw) * 4;
  const u8* __restrict__ src = planes + slot * plane_bytes;
  union { u8 b[12]; unsigned w[3]; } px;
#pragma unroll
  for (int j = 0; j < 4; ++j) plane_pixel(src, H, W, h2v2, y, x + j, px.b + 3 * j);
  u8* __restrict__ dst = out_frames + slot * out_stride + ((i64)y * W + x) * 3;
  if (WIDE) {
#pragma unroll
    for (int j = 0; j < 3; ++j) reinterpret_cast<unsigned*>(dst)[j] = px.w[j];
  } else {
#pragma unroll
    for (int j = 0; j < 12; ++j) dst[j] = px.b[j];
  }
}

bool shape_ok(long long slots, int H, int W, int h2v2) {
  return slots >= 1 && slots <= (1 << 20) && H >= 16 && W >= 16 && H <= 4096 && W <= 4096 && H % 16 == 0 && W % 16 == 0 && (h2v2 == 0 || h2v2 == 1);
}

long long coef_bytes(long long slots, int H, int W, int h2v2) { return slots * blocks_per_image(H, W, h2v2) * 128; }
long long plane_bytes_of(int H, int W, int h2v2) { return blocks_per_image(H, W, h2v2) * 64; }

}  // namespace

extern "C" long long vla_jpeg_workspace_bytes(long long slots, int H, int W, int h2v2) {
  if (!shape_ok(slots, H, W, h2v2)) return -1;
  return coef_bytes(slots, H, W, h2v2) + slots * plane_bytes_of(H, W, h2v2);
}

bool vlajpeg::stage_b_fits(long long slots, int H, int W) { return slots * H * (W / 4) <= 0x7fffffffll * PIXEL_THREADS; }

// Stage B (jpeg_stage_b.h): coefficient blocks -> planes -> pixels, two launches.  The callers have checked the shape (shape_ok's rule),
// the pointers and that the grids fit.
int vlajpeg::stage_b(hipStream_t st, const short* coef, unsigned char* planes, long long slots, int H, int W, int h2v2, unsigned char* out_frames,
                     long long out_stride) {
  const long long per_image = blocks_per_image(H, W, h2v2), plane_bytes = plane_bytes_of(H, W, h2v2);
  const long long n_blocks = slots * per_image;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((n_blocks + IDCT_THREADS - 1) / IDCT_THREADS)), dim3(IDCT_THREADS), 0, st, coef, planes,
                     n_blocks, per_image, plane_bytes, H, W, h2v2);
  VLA_CHECK_LAUNCH("jpeg stage B (idct)");
  const long long n_quads = slots * H * (W / 4);
  const dim3 grid_c((unsigned)((n_quads + PIXEL_THREADS - 1) / PIXEL_THREADS));
  if ((uintptr_t)out_frames % 4 == 0 && out_stride % 4 == 0)
    hipLaunchKernelGGL(jpeg_pixels_kernel<true>, grid_c, dim3(PIXEL_THREADS), 0, st, planes, out_frames, n_quads, plane_bytes, out_stride, H, W, h2v2);
  else
    hipLaunchKernelGGL(jpeg_pixels_kernel<false>, grid_c, dim3(PIXEL_THREADS), 0, st, planes, out_frames, n_quads, plane_bytes, out_stride, H, W, h2v2);
  VLA_CHECK_LAUNCH("jpeg stage B (pixels)");
  return VLA_OK;
}

// vla_jpeg_decode_rows and vla_jpeg_decode_rows_at: the same three launches, the entropy stage with or without an entry table
static int decode_rows(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg, const long long* seg_tab,
                       long long S, const int* seg_ent, const int* img_tab, const unsigned short* qt_pool, int nQ, const int* ht_pool, int nH,
                       const long long* episode_off, int E, long long T, const int* ep, const long long* row, int B, int n_img, int H, int W,
                       int h2v2, int max_seg, int mapping, void* workspace, long long workspace_bytes, unsigned char* out_frames,
                       long long out_stride, unsigned char* status) {
  VLA_REQUIRE(bytes && img_seg && seg_tab && img_tab && qt_pool && ht_pool && episode_off && ep && row, "jpeg_decode_rows: null input pointer");
  VLA_REQUIRE(workspace && out_frames && status, "jpeg_decode_rows: null output pointer");
  VLA_REQUIRE(B >= 1 && B <= 65535 && n_img >= 1 && n_img <= 16 && E >= 1 && T >= 1, "jpeg_decode_rows: 1 <= B <= 65535, 1 <= n_img <= 16, E, T >= 1");
  VLA_REQUIRE(shape_ok((long long)B * n_img, H, W, h2v2), "jpeg_decode_rows: H and W must be multiples of 16 inside [16, 4096], h2v2 0 or 1");
  VLA_REQUIRE(n_bytes >= 1 && S >= 1 && nQ >= 1 && nH >= 1, "jpeg_decode_rows: n_bytes, S, nQ, nH >= 1");
  VLA_REQUIRE(max_seg >= 1 && max_seg <= 65536 && (mapping == 0 || mapping == 1), "jpeg_decode_rows: 1 <= max_seg <= 65536, mapping 0 or 1");
  VLA_REQUIRE(out_stride >= (long long)H * W * 3, "jpeg_decode_rows: out_stride must be at least H * W * 3");
  const long long slots = (long long)B * n_img;
  VLA_REQUIRE((uintptr_t)workspace % 16 == 0 && workspace_bytes >= vla_jpeg_workspace_bytes(slots, H, W, h2v2),
              "jpeg_decode_rows: workspace must be 16-byte aligned and hold vla_jpeg_workspace_bytes");
  const long long items = slots * max_seg;
  VLA_REQUIRE(items <= 0x7fffffffll && vlajpeg::stage_b_fits(slots, H, W),
              "jpeg_decode_rows: B * n_img * max_seg or B * n_img * H * W is too large for one grid");
  short* coef = (short*)workspace;
  unsigned char* planes = (unsigned char*)workspace + coef_bytes(slots, H, W, h2v2);
  const hipStream_t st = (hipStream_t)stream;
  if (mapping)
    hipLaunchKernelGGL(jpeg_entropy_wave_kernel, dim3((unsigned)items), dim3(ENTROPY_THREADS), 0, st, bytes, n_bytes, img_seg, seg_tab, S, img_tab,
                       qt_pool, nQ, ht_pool, nH, episode_off, E, T, ep, row, B, n_img, H, W, h2v2, max_seg, seg_ent, coef, status);
  else
    hipLaunchKernelGGL(jpeg_entropy_lane_kernel, dim3((unsigned)((items + ENTROPY_THREADS - 1) / ENTROPY_THREADS)), dim3(ENTROPY_THREADS), 0, st, bytes,
                       n_bytes, img_seg, seg_tab, S, img_tab, qt_pool, nQ, ht_pool, nH, episode_off, E, T, ep, row, B, n_img, H, W, h2v2, max_seg,
                       seg_ent, coef, status);
  VLA_CHECK_LAUNCH("jpeg_decode_rows (entropy)");
  return vlajpeg::stage_b(st, coef, planes, slots, H, W, h2v2, out_frames, out_stride);
}

extern "C" int vla_jpeg_decode_rows(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg,
                                    const long long* seg_tab, long long S, const int* img_tab, const unsigned short* qt_pool, int nQ,
                                    const int* ht_pool, int nH, const long long* episode_off, int E, long long T, const int* ep,
                                    const long long* row, int B, int n_img, int H, int W, int h2v2, int max_seg, int mapping,
                                    void* workspace, long long workspace_bytes, unsigned char* out_frames, long long out_stride,
                                    unsigned char* status) {
  return decode_rows(stream, bytes, n_bytes, img_seg, seg_tab, S, nullptr, img_tab, qt_pool, nQ, ht_pool, nH, episode_off, E, T, ep, row, B, n_img,
                     H, W, h2v2, max_seg, mapping, workspace, workspace_bytes, out_frames, out_stride, status);
}

extern "C" int vla_jpeg_decode_rows_at(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg,
                                       const long long* seg_tab, const int* seg_ent, long long S, const int* img_tab,
                                       const unsigned short* qt_pool, int nQ, const int* ht_pool, int nH, const long long* episode_off, int E,
                                       long long T, const int* ep, const long long* row, int B, int n_img, int H, int W, int h2v2,
                                       int max_seg, int mapping, void* workspace, long long workspace_bytes, unsigned char* out_frames,
                                       long long out_stride, unsigned char* status) {
  VLA_REQUIRE(seg_ent, "jpeg_decode_rows_at: null entry table");
  return decode_rows(stream, bytes, n_bytes, img_seg, seg_tab, S, seg_ent, img_tab, qt_pool, nQ, ht_pool, nH, episode_off, E, T, ep, row, B, n_img,
                     H, W, h2v2, max_seg, mapping, workspace, workspace_bytes, out_frames, out_stride, status);
}
