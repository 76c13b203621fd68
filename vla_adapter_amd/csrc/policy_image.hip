// The evaluator's frame pipeline (the reference's resize_image_for_policy, experiments/robot/openvla_utils.py:542-565) where the frames
// are: a JPEG round trip without an entropy coder, then TF's lanczos3 resize with antialiasing.  Declared in
// include/vla_policy_image.h; DESIGN.md section 20.
//   policy_forward_kernel   one wave per 16 x 16 MCU: RGB -> YCbCr, h2v2 downsampling, islow forward DCT, quantisation and
//                           dequantisation (csrc/jpeg_forward.h) -> int16 blocks in the decode's coefficient layout
//   stage B                 csrc/jpeg.hip's two kernels through vlajpeg::stage_b: inverse DCT -> planes -> fancy upsampling, colour
//   policy_resample_kernel  one thread per 1, 3 or 4 output values of one 1-D pass: float32 sums over the span's taps, in source order
// The forward kernel is integer only; the resize sums in float32 with no contraction, as the numpy rule does
// (tests/policy_image_rule_np.py).  Nothing is allocated, read back or synchronised.
#include "common.h"
#include "jpeg_encode_core.h"
#include "jpeg_forward.h"
#include "jpeg_stage_a.h"
#include "jpeg_stage_b.h"
#include "../../include/vla_jpeg.h"
#include "../../include/vla_policy_image.h"

// No FMA contraction anywhere in this file: every product and sum rounds on its own, as in the float32 restatement.
#pragma clang fp contract(off)

namespace {

using namespace vlajpeg;

constexpr int FWD_WAVES = 4;                    // MCUs per workgroup, one wave each
constexpr int FWD_THREADS = 64 * FWD_WAVES;
constexpr int RESAMPLE_THREADS = 256;

// What one wave keeps in LDS for its MCU.  The row and column passes of the DCT exchange through `ws`; nothing goes to scratch.
struct McuLds {
  uint4 raw[48];                                // 16 rows of 48 bytes: the MCU's RGB as loaded
  u8 y[256], cb[64], cr[64];                    // the samples: Y 16 x 16, Cb and Cr 8 x 8
  int ws[6 * 64];                               // the six blocks behind the row pass
  alignas(16) short out[6 * 64];                // the six blocks, dequantised
};

// WIDE: frames and in_stride are multiples of 16, so every 16 bytes of an MCU's row (48 bytes, at a multiple of 48 inside an image
// whose rows are multiples of 48) load as one uint4.  QUANT (the encoder's stage 1, jpeg_stage_a.h): the quantised values, not the
// dequantised ones, every block in zigzag order, the MCUs one behind the other in coding order.
template <bool WIDE, bool QUANT = false>
__global__ void __launch_bounds__(FWD_THREADS)
policy_forward_kernel(const u8* __restrict__ frames, i64 in_stride, i64 n_mcus, int H, int W, const unsigned short* __restrict__ qtab,
                      short* __restrict__ coef) {
  __shared__ McuLds s_all[FWD_WAVES];
  __shared__ unsigned short s_q[128];
  const int lane = threadIdx.x & 63;
  McuLds& s = s_all[threadIdx.x >> 6];
  if (threadIdx.x < 128) s_q[threadIdx.x] = qtab[threadIdx.x];
  const i64 g = (i64)blockIdx.x * FWD_WAVES + (threadIdx.x >> 6);
  const bool live = g < n_mcus;                 // (uniform over a wave; a dead wave only joins the barriers)
  const int per_image = (H >> 4) * (W >> 4), mw = W >> 4;
  const i64 img = live ? g / per_image : 0;
  const int mcu = live ? (int)(g - img * per_image) : 0;
  const int my = mcu / mw, mx = mcu - my * mw;

  // the MCU's 16 rows of 48 bytes, 16 bytes a lane
  if (live && lane < 48) {
    const int row = lane / 3, part = lane - row * 3;
    const u8* __restrict__ src = frames + img * in_stride + ((i64)(my * 16 + row) * W + mx * 16) * 3 + part * 16;
    if (WIDE) {
      s.raw[lane] = *reinterpret_cast<const uint4*>(src);
    } else {
      union { u8 b[16]; uint4 v; } t;
#pragma unroll
      for (int j = 0; j < 16; ++j) t.b[j] = src[j];
      s.raw[lane] = t.v;
    }
  }
  __syncthreads();

  // colour conversion and chroma downsampling: a lane per 2 x 2 pixels = one chroma sample
  {
    const u8* raw = reinterpret_cast<const u8*>(s.raw);
    const int cy = lane >> 3, cx = lane & 7;
    int sb = 0, sr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const u8* p = raw + (2 * cy + dy) * 48 + (2 * cx + dx) * 3;
        const int r = p[0], gg = p[1], b = p[2];
        s.y[(2 * cy + dy) * 16 + 2 * cx + dx] = (u8)rgb_to_y(r, gg, b);
        sb += rgb_to_cb(r, gg, b);
        sr += rgb_to_cr(r, gg, b);
      }
    s.cb[lane] = (u8)downsample_h2v2(sb, cx);   // (an MCU is 8 chroma columns wide: the column's parity in the image is cx's)
    s.cr[lane] = (u8)downsample_h2v2(sr, cx);
  }
  __syncthreads();

  // forward DCT: 6 blocks x 8 rows, then 6 blocks x 8 columns, a lane each
  const int blk = lane >> 3, k = lane & 7;
  if (lane < 48) {
    const u8* src = blk < 4 ? s.y + ((blk >> 1) * 8 + k) * 16 + (blk & 1) * 8 : (blk == 4 ? s.cb : s.cr) + k * 8;
    i64 in[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = (int)src[c] - 128;
    fdct_1d(in, o, true);
#pragma unroll
    for (int c = 0; c < 8; ++c) s.ws[blk * 64 + k * 8 + c] = (int)o[c];
  }
  __syncthreads();
  if (lane < 48) {
    i64 in[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = s.ws[blk * 64 + r * 8 + k];
    fdct_1d(in, o, false);
    const unsigned short* q = s_q + (blk < 4 ? 0 : 64);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (QUANT)
        s.out[blk * 64 + zigzag_of(r * 8 + k)] = (short)quantise((int)o[r], q[r * 8 + k]);
      else
        s.out[blk * 64 + r * 8 + k] = requantise((int)o[r], q[r * 8 + k]);
    }
  }
  __syncthreads();

  // the six blocks to their places in the image's coefficient layout, 16 bytes a lane (the workspace is 16-byte aligned)
  if (live && lane < 48) {
    int comp;
    const i64 at = QUANT ? (g * 6 + blk) * 64 + k * 8 : (img * (i64)per_image * 6 + block_index(mcu, blk, W >> 3, H >> 3, 1, comp)) * 64 + k * 8;
    *reinterpret_cast<uint4*>(coef + at) = *reinterpret_cast<const uint4*>(s.out + blk * 64 + k * 8);
  }
}

__device__ __forceinline__ float store_as(float v, float*) { return v; }
__device__ __forceinline__ u8 store_as(float v, u8*) { return (u8)fminf(fmaxf(rintf(v), 0.f), 255.f); }    // tf.round: half to even

// V consecutive elements of a row: one 4-byte or 16-byte access for V == 4 (the caller has checked the alignment), else one by one
template <int V>
__device__ __forceinline__ void load_v(const u8* __restrict__ p, float* x) {
  if constexpr (V == 4) {
    const uchar4 v = *reinterpret_cast<const uchar4*>(p);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = p[j];
  }
}
template <int V>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float* x) {
#pragma unroll
  for (int j = 0; j < V; ++j) x[j] = p[j];
}
template <int V>
__device__ __forceinline__ void store_v(u8* __restrict__ p, const float* acc) {
  if constexpr (V == 4) {
    *reinterpret_cast<uchar4*>(p) = make_uchar4(store_as(acc[0], p), store_as(acc[1], p), store_as(acc[2], p), store_as(acc[3], p));
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = store_as(acc[j], p);
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float* acc) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = acc[j];
  }
}

// One 1-D pass on a [rows, in_len, inner] -> [rows, out_len, inner] layout: out[o, p, i] = sum_k w[p, k] * in[o, min(start_p + k,
// in_len - 1), i], acc = 0; acc += w * v in source order.  Row o of the input stands at (o / rows_per_img) * img_stride +
// (o % rows_per_img) * in_len * inner (elements), the output is contiguous.  Vertical pass: rows = N, inner = W * 3; horizontal pass:
// rows = N * out_h, inner = 3.  TIn u8 or float, TOut float or u8 (rounded half to even, clamped).  A thread owns V consecutive
// values of `inner` (V divides it): 4 where the operands allow 4-element accesses, the 3 channels of a pixel in the horizontal pass,
// else 1.  Every value's sum is its own, whatever V: the bits do not depend on it.
template <typename TIn, typename TOut, int V>
__global__ void __launch_bounds__(RESAMPLE_THREADS)
policy_resample_kernel(const TIn* __restrict__ src, TOut* __restrict__ dst, i64 total, i64 rows_per_img, i64 img_stride, int in_len, int out_len,
                       int inner, const int* __restrict__ starts, const float* __restrict__ weights, int span) {
  const i64 idx = (i64)blockIdx.x * RESAMPLE_THREADS + threadIdx.x;         // which group of V values
  if (idx >= total) return;
  const int groups = inner / V;
  const int i = (int)(idx % groups) * V;
  const i64 op = idx / groups;
  const int p = (int)(op % out_len);
  const i64 o = op / out_len;
  const i64 im = o / rows_per_img;
  const TIn* __restrict__ row = src + im * img_stride + (o - im * rows_per_img) * (i64)in_len * inner + i;
  int start = starts[p];
  start = start < 0 ? 0 : (start > in_len - 1 ? in_len - 1 : start);
  const float* __restrict__ w = weights + (i64)p * span;
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  for (int k = 0; k < span; ++k) {
    const int at = start + k < in_len - 1 ? start + k : in_len - 1;
    float x[V];
    load_v<V>(row + (i64)at * inner, x);
    const float wk = w[k];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] += wk * x[j];
  }
  store_v<V>(dst + idx * V, acc);
}

template <typename TIn, typename TOut, int V>
int resample_v(hipStream_t st, const TIn* src, TOut* dst, i64 rows, i64 rows_per_img, i64 img_stride, int in_len, int out_len, int inner,
               const int* starts, const float* weights, int span) {
  const i64 total = rows * out_len * (inner / V);
  hipLaunchKernelGGL((policy_resample_kernel<TIn, TOut, V>), dim3((unsigned)((total + RESAMPLE_THREADS - 1) / RESAMPLE_THREADS)),
                     dim3(RESAMPLE_THREADS), 0, st, src, dst, total, rows_per_img, img_stride, in_len, out_len, inner, starts, weights, span);
  VLA_CHECK_LAUNCH("policy_lanczos3_resize");
  return VLA_OK;
}

// the pass with the widest accesses its operands allow: 4 values a thread when every row of the input and every group of the output
// starts at a multiple of 4 elements; else a pixel a thread in the horizontal pass (inner == 3), a value a thread in the vertical one
template <typename TIn, typename TOut>
int resample(hipStream_t st, const TIn* src, TOut* dst, i64 rows, i64 rows_per_img, i64 img_stride, int in_len, int out_len, int inner,
             const int* starts, const float* weights, int span) {
  const bool wide = inner % 4 == 0 && img_stride % 4 == 0 && (uintptr_t)src % (4 * sizeof(TIn)) == 0 && (uintptr_t)dst % (4 * sizeof(TOut)) == 0;
  if (wide) return resample_v<TIn, TOut, 4>(st, src, dst, rows, rows_per_img, img_stride, in_len, out_len, inner, starts, weights, span);
  if (inner == 3) return resample_v<TIn, TOut, 3>(st, src, dst, rows, rows_per_img, img_stride, in_len, out_len, inner, starts, weights, span);
  return resample_v<TIn, TOut, 1>(st, src, dst, rows, rows_per_img, img_stride, in_len, out_len, inner, starts, weights, span);
}

bool resize_shape_ok(long long N, int H, int W, int out_h, int out_w) {
  return N >= 1 && N <= (1 << 20) && H >= 1 && W >= 1 && out_h >= 1 && out_w >= 1 && H <= 4096 && W <= 4096 && out_h <= 4096 && out_w <= 4096 &&
         (H != out_h || W != out_w);
}

long long intermediate_bytes(long long N, int H, int W, int out_h, int out_w) { return (H != out_h && W != out_w) ? N * out_h * W * 3 * 4 : 0; }

}  // namespace

int vlajpeg::stage_a_quantised(hipStream_t st, const unsigned char* frames, long long in_stride, long long N, int H, int W,
                               const unsigned short* qtab, short* quant) {
  const long long n_mcus = N * mcus_per_image(H, W, 1), grid = (n_mcus + FWD_WAVES - 1) / FWD_WAVES;
  VLA_REQUIRE(grid <= 0x7fffffffll, "jpeg_encode: N * H * W is too large for one grid");
  if ((uintptr_t)frames % 16 == 0 && in_stride % 16 == 0)
    hipLaunchKernelGGL((policy_forward_kernel<true, true>), dim3((unsigned)grid), dim3(FWD_THREADS), 0, st, frames, in_stride, n_mcus, H, W, qtab, quant);
  else
    hipLaunchKernelGGL((policy_forward_kernel<false, true>), dim3((unsigned)grid), dim3(FWD_THREADS), 0, st, frames, in_stride, n_mcus, H, W, qtab, quant);
  VLA_CHECK_LAUNCH("jpeg_encode (forward)");
  return VLA_OK;
}

extern "C" long long vla_policy_image_workspace_bytes(long long N, int H, int W, int out_h, int out_w, int round_trip) {
  if (round_trip) return vla_jpeg_workspace_bytes(N, H, W, 1);
  if (!resize_shape_ok(N, H, W, out_h, out_w)) return -1;
  return intermediate_bytes(N, H, W, out_h, out_w);
}

extern "C" int vla_policy_jpeg_round_trip(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W,
                                          const unsigned short* qtab, void* workspace, long long workspace_bytes, unsigned char* out_frames,
                                          long long out_stride) {
  VLA_REQUIRE(frames && qtab && workspace && out_frames, "policy_jpeg_round_trip: null pointer");
  const long long need = vla_jpeg_workspace_bytes(N, H, W, 1);
  VLA_REQUIRE(need >= 0, "policy_jpeg_round_trip: H and W must be multiples of 16 inside [16, 4096] (edge MCUs are not built), 1 <= N <= 2^20");
  VLA_REQUIRE(in_stride >= (long long)H * W * 3 && out_stride >= (long long)H * W * 3, "policy_jpeg_round_trip: strides must be at least H * W * 3");
  VLA_REQUIRE((uintptr_t)workspace % 16 == 0 && workspace_bytes >= need,
              "policy_jpeg_round_trip: workspace must be 16-byte aligned and hold vla_policy_image_workspace_bytes");
  const long long n_mcus = N * mcus_per_image(H, W, 1), grid = (n_mcus + FWD_WAVES - 1) / FWD_WAVES;
  VLA_REQUIRE(grid <= 0x7fffffffll && stage_b_fits(N, H, W), "policy_jpeg_round_trip: N * H * W is too large for one grid");
  short* coef = (short*)workspace;
  unsigned char* planes = (unsigned char*)workspace + N * blocks_per_image(H, W, 1) * 128;
  const hipStream_t st = (hipStream_t)stream;
  if ((uintptr_t)frames % 16 == 0 && in_stride % 16 == 0)
    hipLaunchKernelGGL(policy_forward_kernel<true>, dim3((unsigned)grid), dim3(FWD_THREADS), 0, st, frames, in_stride, n_mcus, H, W, qtab, coef);
  else
    hipLaunchKernelGGL(policy_forward_kernel<false>, dim3((unsigned)grid), dim3(FWD_THREADS), 0, st, frames, in_stride, n_mcus, H, W, qtab, coef);
  VLA_CHECK_LAUNCH("policy_jpeg_round_trip (forward)");
  return stage_b(st, coef, planes, N, H, W, 1, out_frames, out_stride);
}

extern "C" int vla_policy_lanczos3_resize(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W, int out_h,
                                          int out_w, const int* starts_v, const float* weights_v, int span_v, const int* starts_h,
                                          const float* weights_h, int span_h, void* workspace, long long workspace_bytes, unsigned char* out) {
  VLA_REQUIRE(frames && out, "policy_lanczos3_resize: null pointer");
  VLA_REQUIRE(resize_shape_ok(N, H, W, out_h, out_w),
              "policy_lanczos3_resize: 1 <= N <= 2^20, sides inside [1, 4096], and at least one side must change (equal sizes: nothing to do)");
  VLA_REQUIRE(in_stride >= (long long)H * W * 3, "policy_lanczos3_resize: in_stride must be at least H * W * 3");
  const bool vert = H != out_h, horz = W != out_w;
  VLA_REQUIRE((!vert || (starts_v && weights_v && span_v >= 1 && span_v <= H)) && (!horz || (starts_h && weights_h && span_h >= 1 && span_h <= W)),
              "policy_lanczos3_resize: a pass that runs needs its starts, its weights and 1 <= span <= the side it reads");
  const long long need = intermediate_bytes(N, H, W, out_h, out_w);
  VLA_REQUIRE(need == 0 || (workspace && (uintptr_t)workspace % 4 == 0 && workspace_bytes >= need),
              "policy_lanczos3_resize: workspace must be 4-byte aligned and hold vla_policy_image_workspace_bytes");
  const long long biggest = N * (long long)out_h * (W > out_w ? W : out_w) * 3;
  VLA_REQUIRE(biggest <= 0x7fffffffll * RESAMPLE_THREADS, "policy_lanczos3_resize: N * out_h * W is too large for one grid");
  const hipStream_t st = (hipStream_t)stream;
  // THE PASS ORDER: vertical first, then horizontal (tests/policy_image_rule_np.py: PASS_ORDER states the same for the rule)
  if (vert && horz) {
    float* mid = (float*)workspace;
    const int rc = resample<u8, float>(st, frames, mid, N, 1, in_stride, H, out_h, W * 3, starts_v, weights_v, span_v);
    if (rc != VLA_OK) return rc;
    return resample<float, u8>(st, mid, out, N * out_h, out_h, (i64)out_h * W * 3, W, out_w, 3, starts_h, weights_h, span_h);
  }
  if (vert) return resample<u8, u8>(st, frames, out, N, 1, in_stride, H, out_h, W * 3, starts_v, weights_v, span_v);
  return resample<u8, u8>(st, frames, out, N * H, H, in_stride, W, out_w, 3, starts_h, weights_h, span_h);
}
