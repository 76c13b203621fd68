// Training-time image augmentation of the reference's RLDS pipeline and the evaluator's center crop, fused with the
// processor's ToTensor + Normalize.  The chain, per image of a uint8 [N, H, W, 3] batch, in f32:
//   x = q * (1/255)                                                  tf.image.convert_image_dtype
//   crop    tf.image.crop_and_resize(box, size = (H, W)), bilinear   random_resized_crop / center_crop_image
//   bright  x + delta                                                random_brightness
//   contr.  (x - mean_c) * f + mean_c   (mean over H x W per channel) random_contrast
//   sat.    RGB -> HSV, s = clamp(s * f, 0, 1), HSV -> RGB            random_saturation
//   hue     RGB -> HSV, h = wrap(h + delta), HSV -> RGB               random_hue
//   each followed by clip(0, 1); then q' = min(255, floor(x * 255.5)) (convert_image_dtype(saturate=True)) and, per backbone,
//   ((q' / 255) - mean_b) / std_b into the channel-stacked pixel tensor (image_normalize_kernel's order and layout).
// Two passes: the statistics pass runs crop + brightness and writes per-chunk channel sums into a caller-owned slab; the
// apply pass recomputes them (same code, same rounding), reduces the slab in a fixed order (no float atomics: bitwise
// reproducible) and runs the rest.  A chunk = 256 thread units of 8 consecutive pixels of one row of one image.
#include "common.h"
#include "../../include/vla_native.h"

// No FMA contraction anywhere in this file: every product and sum rounds on its own, as in the float32 restatement.
#pragma clang fp contract(off)

namespace {

constexpr int AUG_NP = VLA_AUG_NPARAM;
constexpr int AUG_THREADS = 256;
constexpr int AUG_PIX = 8;                 // pixels of one row per thread unit
constexpr int AUG_MAX_BB = 4;
constexpr float INV255 = (float)(1.0 / 255.0);

struct AugArgs {
  int N, H, W, n_img, G, P;               // G = units per row, P = chunks per image
  unsigned ops;
  float side, bright, c_lo, c_hi, s_lo, s_hi, hue;
  unsigned long long seed;
  long long rank, step;
  int n_bb, out_f32;
  float mean[3 * AUG_MAX_BB], std[3 * AUG_MAX_BB];
};

// the scheme of the LoRA dropout mask (common.h splitmix64_key)
__device__ __forceinline__ unsigned long long aug_mix(unsigned long long seed, unsigned long long idx) { return splitmix64_key(seed, idx); }

// tf.random.uniform's affine map of a unit variate: (hi - lo) * u + lo
__device__ __forceinline__ float aug_uniform(float lo, float hi, float u) { return (hi - lo) * u + lo; }

// The draw mapping: ONE variate u per image drives all five ops, as dlimp passes the same seed to each.
// Switching to independent draws is a change of this function alone.
__device__ void aug_params_from_u(float u, const AugArgs& a, float* p) {
  const float off = aug_uniform(0.f, 1.f - a.side, u);
  p[VLA_AUG_P_U] = u;
  p[VLA_AUG_P_Y1] = off;
  p[VLA_AUG_P_X1] = off;
  p[VLA_AUG_P_Y2] = off + a.side;
  p[VLA_AUG_P_X2] = off + a.side;
  p[VLA_AUG_P_BRIGHT] = aug_uniform(-a.bright, a.bright, u);
  p[VLA_AUG_P_CONTRAST] = aug_uniform(a.c_lo, a.c_hi, u);
  p[VLA_AUG_P_SAT] = aug_uniform(a.s_lo, a.s_hi, u);
  p[VLA_AUG_P_HUE] = aug_uniform(-a.hue, a.hue, u);
}

// Parameters of image n: drawn from the key (seed, rank, micro-step, sample, image), or read from the caller's buffer.
__device__ __forceinline__ void aug_load_params(const AugArgs& a, const float* __restrict__ params, int n, float* p) {
  if (a.ops & VLA_AUG_DRAW) {
    const unsigned long long h =
        aug_mix(aug_mix(aug_mix(aug_mix(a.seed, (unsigned long long)a.rank), (unsigned long long)a.step), (unsigned long long)(n / a.n_img)),
                (unsigned long long)(n % a.n_img));
    aug_params_from_u((float)(h >> 40) * (1.f / 16777216.f), a, p);      // 24 bits: exact in f32
  } else {
#pragma unroll
    for (int k = 0; k < AUG_NP; ++k) p[k] = params[(long long)n * AUG_NP + k];
  }
}

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// Crop + brightness (+ clips) of the 8 pixels (y, x0 .. x0+7) of image `img`: the part both passes compute.
template <bool VEC>
__device__ void aug_stage1(const unsigned char* __restrict__ img, const AugArgs& a, const float* p, int y, int x0, float (&v)[AUG_PIX][3]) {
  const int H = a.H, W = a.W;
  if (a.ops & VLA_AUG_CROP) {
    // tensorflow/core/kernels/image/crop_and_resize_op.cc, crop size = image size
    const float hs = (p[VLA_AUG_P_Y2] - p[VLA_AUG_P_Y1]) * (float)(H - 1) / (float)(H - 1);
    const float ws = (p[VLA_AUG_P_X2] - p[VLA_AUG_P_X1]) * (float)(W - 1) / (float)(W - 1);
    const float in_y = p[VLA_AUG_P_Y1] * (float)(H - 1) + (float)y * hs;
    const bool row_in = in_y >= 0.f && in_y <= (float)(H - 1);
    const int ty = row_in ? (int)floorf(in_y) : 0, by = row_in ? min((int)ceilf(in_y), H - 1) : 0;
    const float yl = in_y - floorf(in_y);
    const unsigned char* rt = img + (long long)ty * W * 3;
    const unsigned char* rb = img + (long long)by * W * 3;
#pragma unroll
    for (int i = 0; i < AUG_PIX; ++i) {
      const float in_x = p[VLA_AUG_P_X1] * (float)(W - 1) + (float)(x0 + i) * ws;
      const bool in = row_in && x0 + i < W && in_x >= 0.f && in_x <= (float)(W - 1);      // outside: extrapolation value 0
      const int lx = in ? (int)floorf(in_x) : 0, rx = in ? min((int)ceilf(in_x), W - 1) : 0;
      const float xl = in_x - floorf(in_x);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float tl = (float)rt[lx * 3 + c] * INV255, tr = (float)rt[rx * 3 + c] * INV255;
        const float bl = (float)rb[lx * 3 + c] * INV255, br = (float)rb[rx * 3 + c] * INV255;
        const float top = tl + (tr - tl) * xl, bot = bl + (br - bl) * xl;
        v[i][c] = in ? clip01(top + (bot - top) * yl) : 0.f;
      }
    }
  } else {
    const unsigned char* src = img + ((long long)y * W + x0) * 3;
    unsigned char q[AUG_PIX * 3];
    if (VEC) {                                   // 24 bytes, 8-B aligned (W % 8 == 0)
      const uint2 w0 = reinterpret_cast<const uint2*>(src)[0], w1 = reinterpret_cast<const uint2*>(src)[1],
                  w2 = reinterpret_cast<const uint2*>(src)[2];
      const unsigned w[6] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y};
#pragma unroll
      for (int k = 0; k < AUG_PIX * 3; ++k) q[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
      for (int k = 0; k < AUG_PIX * 3; ++k) q[k] = x0 + k / 3 < W ? src[k] : 0;
    }
#pragma unroll
    for (int i = 0; i < AUG_PIX; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[i][c] = (float)q[i * 3 + c] * INV255;
  }
  if (a.ops & VLA_AUG_BRIGHTNESS) {
#pragma unroll
    for (int i = 0; i < AUG_PIX; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) v[i][c] = clip01(v[i][c] + p[VLA_AUG_P_BRIGHT]);
  }
}

// TF's fused AdjustSaturation / AdjustHue per-pixel conversions
__device__ __forceinline__ void rgb_to_hsv(float r, float g, float b, float& h, float& s, float& v) {
  const float vv = fmaxf(r, fmaxf(g, b));
  const float range = vv - fminf(r, fminf(g, b));
  s = vv > 0.f ? range / vv : 0.f;
  float hh = 0.f;
  if (range > 0.f) {
    const float n = 1.f / (6.f * range);
    if (r == vv) hh = n * (g - b);
    else if (g == vv) hh = n * (b - r) + 2.f / 6.f;
    else hh = n * (r - g) + 4.f / 6.f;
  }
  if (hh < 0.f) hh = hh + 1.f;
  h = hh;
  v = vv;
}

__device__ __forceinline__ void hsv_to_rgb(float h, float s, float v, float& r, float& g, float& b) {
  const float c = s * v, m = v - c, dh = h * 6.f;
  const int k = min(max((int)floorf(dh), 0), 5);          // h rounded up to 1.0 (h < 0 wrapped) lands in sector 5
  const float x = c * (1.f - fabsf(fmodf(dh, 2.f) - 1.f));
  float rr, gg, bb;
  switch (k) {
    case 0: rr = c; gg = x; bb = 0.f; break;
    case 1: rr = x; gg = c; bb = 0.f; break;
    case 2: rr = 0.f; gg = c; bb = x; break;
    case 3: rr = 0.f; gg = x; bb = c; break;
    case 4: rr = x; gg = 0.f; bb = c; break;
    default: rr = c; gg = 0.f; bb = x; break;
  }
  r = rr + m;
  g = gg + m;
  b = bb + m;
}

// chunk -> (image, first unit); unit -> (row, first column)
__device__ __forceinline__ void aug_unit(const AugArgs& a, long long chunk, int& n, int& y, int& x0, bool& live) {
  n = (int)(chunk / a.P);
  const int u = (int)(chunk - (long long)n * a.P) * AUG_THREADS + (int)threadIdx.x;
  live = u < a.H * a.G;
  y = live ? u / a.G : 0;
  x0 = live ? (u - y * a.G) * AUG_PIX : 0;
}

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) augment_stats_kernel(const unsigned char* __restrict__ frames, const float* __restrict__ params,
                                                                    float* __restrict__ slab, AugArgs a) {
  __shared__ float red[AUG_THREADS / 64][3];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (long long chunk = blockIdx.x; chunk < (long long)a.N * a.P; chunk += gridDim.x) {
    int n, y, x0;
    bool live;
    aug_unit(a, chunk, n, y, x0, live);
    float p[AUG_NP];
    aug_load_params(a, params, n, p);
    float s[3] = {0.f, 0.f, 0.f};
    if (live) {
      float v[AUG_PIX][3];
      aug_stage1<VEC>(frames + (long long)n * a.H * a.W * 3, a, p, y, x0, v);
#pragma unroll
      for (int i = 0; i < AUG_PIX; ++i)
        if (x0 + i < a.W)
#pragma unroll
          for (int c = 0; c < 3; ++c) s[c] += v[i][c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
    __syncthreads();                              // red[] of the previous chunk has been read
    if (lane == 0)
#pragma unroll
      for (int c = 0; c < 3; ++c) red[wid][c] = s[c];
    __syncthreads();
    if (threadIdx.x < 3) {
      float t = red[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < AUG_THREADS / 64; ++w) t += red[w][threadIdx.x];
      slab[chunk * 3 + threadIdx.x] = t;
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) augment_apply_kernel(const unsigned char* __restrict__ frames, float* __restrict__ params,
                                                                    const float* __restrict__ slab, void* __restrict__ out,
                                                                    unsigned char* __restrict__ frames_out, AugArgs a) {
  __shared__ float mean_s[3];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool contrast = a.ops & VLA_AUG_CONTRAST;
  for (long long chunk = blockIdx.x; chunk < (long long)a.N * a.P; chunk += gridDim.x) {
    int n, y, x0;
    bool live;
    aug_unit(a, chunk, n, y, x0, live);
    float p[AUG_NP];
    aug_load_params(a, params, n, p);
    if ((a.ops & VLA_AUG_DRAW) && chunk % a.P == 0 && threadIdx.x < AUG_NP) params[(long long)n * AUG_NP + threadIdx.x] = p[threadIdx.x];
    if (contrast) {                               // image mean per channel: the slab's chunk sums in a fixed order
      __syncthreads();
      if (wid < 3) {
        float t = 0.f;
        for (int q = lane; q < a.P; q += 64) t += slab[((long long)n * a.P + q) * 3 + wid];
        t = wave_sum(t);
        if (lane == 0) mean_s[wid] = t / (float)(a.H * a.W);
      }
      __syncthreads();
    }
    if (!live) continue;
    float v[AUG_PIX][3];
    aug_stage1<VEC>(frames + (long long)n * a.H * a.W * 3, a, p, y, x0, v);
    if (contrast) {
      const float m[3] = {mean_s[0], mean_s[1], mean_s[2]}, f = p[VLA_AUG_P_CONTRAST];
#pragma unroll
      for (int i = 0; i < AUG_PIX; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = clip01((v[i][c] - m[c]) * f + m[c]);
    }
    if (a.ops & VLA_AUG_SATURATION) {
      const float f = p[VLA_AUG_P_SAT];
#pragma unroll
      for (int i = 0; i < AUG_PIX; ++i) {
        float h, s, vv;
        rgb_to_hsv(v[i][0], v[i][1], v[i][2], h, s, vv);
        hsv_to_rgb(h, fminf(fmaxf(s * f, 0.f), 1.f), vv, v[i][0], v[i][1], v[i][2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = clip01(v[i][c]);
      }
    }
    if (a.ops & VLA_AUG_HUE) {
      const float d = p[VLA_AUG_P_HUE];
#pragma unroll
      for (int i = 0; i < AUG_PIX; ++i) {
        float h, s, vv;
        rgb_to_hsv(v[i][0], v[i][1], v[i][2], h, s, vv);
        float t = h + d;
        if (t < 0.f) t = t + 1.f;
        else if (t >= 1.f) t = t - 1.f;
        hsv_to_rgb(t, s, vv, v[i][0], v[i][1], v[i][2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[i][c] = clip01(v[i][c]);
      }
    }
    unsigned char q[AUG_PIX][3];
#pragma unroll
    for (int i = 0; i < AUG_PIX; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) q[i][c] = (unsigned char)fminf(v[i][c] * 255.5f, 255.f);      // x >= 0: truncation = floor
    if (frames_out) {
      unsigned char* dst = frames_out + ((long long)n * a.H * a.W + (long long)y * a.W + x0) * 3;
      if (VEC) {
        unsigned w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < AUG_PIX * 3; ++k) w[k >> 2] |= (unsigned)q[k / 3][k % 3] << (8 * (k & 3));
        reinterpret_cast<uint2*>(dst)[0] = uint2{w[0], w[1]};
        reinterpret_cast<uint2*>(dst)[1] = uint2{w[2], w[3]};
        reinterpret_cast<uint2*>(dst)[2] = uint2{w[4], w[5]};
      } else {
#pragma unroll
        for (int k = 0; k < AUG_PIX * 3; ++k)
          if (x0 + k / 3 < a.W) dst[k] = q[k / 3][k % 3];
      }
    }
    // ToTensor + Normalize per backbone (image_normalize_kernel): image im of sample b -> channels 3 * (im * n_bb + j) + c
    const int b = n / a.n_img, im = n % a.n_img, Ctot = 3 * a.n_bb * a.n_img;
    for (int j = 0; j < a.n_bb; ++j) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float mu = a.mean[3 * j + c], sd = a.std[3 * j + c];
        float o[AUG_PIX];
#pragma unroll
        for (int i = 0; i < AUG_PIX; ++i) o[i] = ((float)q[i][c] / 255.0f - mu) / sd;
        const long long off = (((long long)b * Ctot + 3 * (im * a.n_bb + j) + c) * a.H + y) * a.W + x0;
        if (VEC) {
          if (a.out_f32) {
            float4* d = reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + off);
            d[0] = float4{o[0], o[1], o[2], o[3]};
            d[1] = float4{o[4], o[5], o[6], o[7]};
          } else {
            *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(out) + off) = uint4{pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])};
          }
        } else {
#pragma unroll
          for (int i = 0; i < AUG_PIX; ++i) {
            if (x0 + i >= a.W) break;
            if (a.out_f32) reinterpret_cast<float*>(out)[off + i] = o[i];
            else reinterpret_cast<bf16_t*>(out)[off + i] = f2bf(o[i]);
          }
        }
      }
    }
  }
}

int aug_setup(AugArgs& a, int N, int H, int W, int n_img, unsigned ops, const float* cfg, unsigned long long seed, long long rank, long long step) {
  VLA_REQUIRE(N > 0 && H >= 2 && W >= 2 && n_img > 0 && N % n_img == 0, "augment: N > 0, H, W >= 2, N a multiple of n_img");
  VLA_REQUIRE((long long)N * H * W * 3 < (1ll << 40), "augment: batch too large");
  VLA_REQUIRE((ops & ~(unsigned)VLA_AUG_ALL) == 0, "augment: unknown op bits");
  VLA_REQUIRE(cfg, "augment: null cfg");
  a = AugArgs{};
  a.N = N; a.H = H; a.W = W; a.n_img = n_img;
  a.G = (W + AUG_PIX - 1) / AUG_PIX;
  a.P = (H * a.G + AUG_THREADS - 1) / AUG_THREADS;
  a.ops = ops;
  a.side = cfg[0]; a.bright = cfg[1]; a.c_lo = cfg[2]; a.c_hi = cfg[3]; a.s_lo = cfg[4]; a.s_hi = cfg[5]; a.hue = cfg[6];
  VLA_REQUIRE(a.side > 0.f && a.side <= 1.f && a.bright >= 0.f && a.c_lo <= a.c_hi && a.s_lo <= a.s_hi && a.hue >= 0.f && a.hue <= 0.5f,
              "augment: cfg = {crop side in (0, 1], brightness >= 0, contrast lo <= hi, saturation lo <= hi, hue in [0, 0.5]}");
  a.seed = seed; a.rank = rank; a.step = step;
  return VLA_OK;
}

dim3 aug_grid(const AugArgs& a) { return dim3((unsigned)min((long long)a.N * a.P, 2048ll)); }

}  // namespace

extern "C" long long vla_augment_slab_floats(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return -1;
  const long long P = ((long long)H * ((W + AUG_PIX - 1) / AUG_PIX) + AUG_THREADS - 1) / AUG_THREADS;
  return (long long)N * P * 3;
}

extern "C" int vla_augment_stats(void* stream, const void* frames, const float* params, float* slab, int N, int H, int W, int n_img,
                                 unsigned ops, const float* cfg, unsigned long long seed, long long rank, long long step) {
  AugArgs a;
  const int rc = aug_setup(a, N, H, W, n_img, ops, cfg, seed, rank, step);
  if (rc) return rc;
  VLA_REQUIRE(frames && slab && (params || (ops & VLA_AUG_DRAW)), "augment_stats: null frames / slab / params");
  const bool vec = W % AUG_PIX == 0 && ((uintptr_t)frames & 7) == 0;
  if (vec) hipLaunchKernelGGL(augment_stats_kernel<true>, aug_grid(a), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const unsigned char*)frames, params, slab, a);
  else hipLaunchKernelGGL(augment_stats_kernel<false>, aug_grid(a), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const unsigned char*)frames, params, slab, a);
  VLA_CHECK_LAUNCH("augment_stats");
  return VLA_OK;
}

extern "C" int vla_augment_apply(void* stream, const void* frames, float* params, const float* slab, void* out, void* frames_out, int N,
                                 int H, int W, int n_img, int n_bb, const float* mean, const float* std, int out_f32, unsigned ops,
                                 const float* cfg, unsigned long long seed, long long rank, long long step) {
  AugArgs a;
  const int rc = aug_setup(a, N, H, W, n_img, ops, cfg, seed, rank, step);
  if (rc) return rc;
  VLA_REQUIRE(frames && params && out && mean && std, "augment_apply: null frames / params / out / mean / std");
  VLA_REQUIRE(slab || !(ops & VLA_AUG_CONTRAST), "augment_apply: contrast needs the statistics slab");
  VLA_REQUIRE(n_bb >= 1 && n_bb <= AUG_MAX_BB, "augment_apply: 1 to 4 backbones");
  for (int k = 0; k < 3 * n_bb; ++k) {
    VLA_REQUIRE(std[k] != 0.f, "augment_apply: zero std");
    a.mean[k] = mean[k];
    a.std[k] = std[k];
  }
  a.n_bb = n_bb;
  a.out_f32 = out_f32 ? 1 : 0;
  const bool vec = W % AUG_PIX == 0 && (((uintptr_t)frames | (uintptr_t)frames_out) & 7) == 0 && ((uintptr_t)out & 15) == 0;
  if (vec) hipLaunchKernelGGL(augment_apply_kernel<true>, aug_grid(a), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const unsigned char*)frames, params, slab, out, (unsigned char*)frames_out, a);
  else hipLaunchKernelGGL(augment_apply_kernel<false>, aug_grid(a), dim3(AUG_THREADS), 0, (hipStream_t)stream, (const unsigned char*)frames, params, slab, out, (unsigned char*)frames_out, a);
  VLA_CHECK_LAUNCH("augment_apply");
  return VLA_OK;
}
