// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels.  One wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

typedef unsigned short bf16_t;  // raw bf16 storage
typedef __attribute__((ext_vector_type(8))) short bf16x8;     // MFMA A/B fragment (8 bf16 = 4 VGPR)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;      // 16x16 accumulator
typedef __attribute__((ext_vector_type(16))) float f32x16;    // 32x32 accumulator
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // 16 B of packed bf16 that stay four plain registers
typedef __attribute__((ext_vector_type(8))) int v8i_f8;       // the 32-byte fp8 MFMA operand

#define VLA_OK 0
#define VLA_ERR_ARG (-1)       // bad shape / alignment / null pointer
#define VLA_ERR_LAUNCH (-2)    // hipGetLastError() after launch
#define VLA_ERR_UNSUPPORTED (-3)

extern "C" void vla_set_error(const char* msg);

#define VLA_REQUIRE(cond, msg)            \
  do {                                    \
    if (!(cond)) {                        \
      vla_set_error(msg);                 \
      return VLA_ERR_ARG;                 \
    }                                     \
  } while (0)

// Lift KERNEL's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to `bytes`, once per kernel: the call runs in a
// thread-safe static initialiser, and its refusal is returned (VLA_ERR_LAUNCH, the kernel named in vla_last_error) on every launch.
template <auto KERNEL>
int vla_lds_limit(int bytes, const char* name) {
  static const hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) return VLA_OK;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: setting %d bytes of dynamic LDS failed (%s)", name, bytes, hipGetErrorString(e));
  vla_set_error(msg);
  return VLA_ERR_LAUNCH;
}

#define VLA_CHECK_LAUNCH(name)                          \
  do {                                                  \
    hipError_t e__ = hipGetLastError();                 \
    if (e__ != hipSuccess) {                            \
      vla_set_error(name ": launch failed");            \
      return VLA_ERR_LAUNCH;                            \
    }                                                   \
  } while (0)

__device__ __forceinline__ float bf2f(bf16_t x) { return __uint_as_float(((unsigned)x) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }  // bf16 rounding point
__device__ __forceinline__ unsigned pack2(float lo, float hi) {   // ONE v_cvt_pk_bf16_f32 (two RNE conversions, lo in bits 0..15)
  typedef float f32x2_v __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_v __attribute__((ext_vector_type(2)));
  const bf16x2_v b = __builtin_convertvector(f32x2_v{lo, hi}, bf16x2_v);
  return __builtin_bit_cast(unsigned, b);
}

// ---- packed bf16: a 32-bit word holds two values, the lower-indexed one in bits 0..15.  The ONE spelling of the unpack.
__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ void unpack4(const uint2& u, float (&f)[4]) {
  f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
}
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = bf_lo(w[k]);
    f[2 * k + 1] = bf_hi(w[k]);
  }
}
template <class V>   // four floats behind operator[] (float[4], f32x4)
__device__ __forceinline__ uint2 pack4(const V& f) { return uint2{pack2(f[0], f[1]), pack2(f[2], f[3])}; }
__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return uint4{pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])};
}

// splitmix64 finaliser of (seed + idx * golden ratio): the ONE counter-based generator of the device-side draws (LoRA dropout mask,
// image augmentation, the collator's filler tokens).  Keys chain: mix(mix(seed, a), b) ...
__device__ __forceinline__ unsigned long long splitmix64_key(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + idx * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ActionTokenizer.__call__ (action_tokenizer.py:60-74, use_minivlm branch) of one value: clip to [lo, hi], np.digitize against the
// caller's bin edges (count of edges <= x, compared in f64 like numpy; bins increasing), token id = tokenizer_len - bin index.
__device__ __forceinline__ long long action_token_id(float v, const double* __restrict__ bins, int nbins, float lo, float hi,
                                                     long long tokenizer_len) {
  const double x = (double)fminf(fmaxf(v, lo), hi);
  int a = 0, b = nbins;                       // first edge index with bins[idx] > x  (== np.digitize(x, bins))
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (bins[mid] <= x) a = mid + 1;
    else b = mid;
  }
  return tokenizer_len - a;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// erf by Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, far below a bf16 ulp): one v_exp + one v_rcp instead of the
// ~25-instruction libm erff - the GELU epilogue of the ViT fc1 GEMM evaluates it 64x per thread per tile.
__device__ __forceinline__ float fast_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float r = 1.0f - poly * __expf(-ax * ax);
  return copysignf(r, x);
}
// gelu(x) = x * Phi(x) with Phi through the same A&S erf, folded: for z = |x|/sqrt2, t = 1/(1 + p z),
// erf(z) = 1 - poly(t) exp(-z^2)  =>  gelu(x) = max(x, 0) - |x| * (poly(t)/2) * exp(-x^2/2)   (both signs of x; no
// 1 - (1 - eps) cancellation on the negative side).  11 VALU + v_rcp + v_exp per element - the fc1 epilogue of the ViT
// evaluates it 32x per thread per tile, right on the tile's tail.
__device__ __forceinline__ float gelu_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(ax, 0.3275911f * 0.70710678118654752440f, 1.0f));
  const float poly = t * (0.127414796f + t * (-0.142248368f + t * (0.7107068705f + t * (-0.7265760135f + t * 0.5307027145f))));
  const float e = __builtin_amdgcn_exp2f(x * x * -0.72134752044448170368f);       // exp(-x^2/2)
  return __builtin_fmaf(-ax * poly, e, fmaxf(x, 0.f));
}
__device__ __forceinline__ float gelu_erf_grad(float x) {
  const float c = 0.3989422804014327f;  // 1/sqrt(2 pi)
  return 0.5f * (1.0f + fast_erf(x * 0.70710678118654752440f)) + x * c * __expf(-0.5f * x * x);
}
// 0.5 x (1 + tanh u) = x * sigmoid(2u), u = k (x + 0.044715 x^3): one v_exp + one v_rcp instead of libm tanhf
__device__ __forceinline__ float gelu_tanh(float x) {
  const float u2 = x * __builtin_fmaf(x * x, 0.044715f * 1.5957691216057308f, 1.5957691216057308f);   // 2u
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u2 * -1.4426950408889634f));
}

// Zero `bytes` (a multiple of 16, 16-B aligned) of LDS with 16-B stores, strided over `n` threads.  The attention kernels cleared
// their tile images with one ds_write_b16 per element: 136 stores per lane and tile pair in the head kernels - 8.3k of
// head_fwd_mfma's 32k cycles (tools/diag/hf_stamps.py, round 3).
__device__ __forceinline__ void lds_zero16(void* p, int bytes, int idx, int n) {
  for (int i = idx * 16; i < bytes; i += n * 16) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(p) + i) = uint4{0, 0, 0, 0};
}

// async global -> LDS copy, 16 B per lane; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* gptr, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gptr,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// The same copy issued from inline asm: 16 B per lane from (wave-uniform base + per-lane 32-bit byte offset) to LDS address `dst`
// (+ lane * 16).  Hidden from hipcc on purpose: beside a builtin global_load_lds it drains vmcnt(0) before every ordinary
// load, every ds_write that might alias the DMA target and every reuse of a loaded register - i.e. all through an epilogue
// that runs under the next tile's K-tile 0.  Its completion is counted by hand (the s_waitcnt statements of the callers); M0 is
// saved and restored in the same statement (it is compiler-reserved).
__device__ __forceinline__ void glds16s(const char* base, unsigned voff, unsigned dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}

// two 16-B fragment reads -> the 32-byte fp8 MFMA operand
__device__ __forceinline__ v8i_f8 cat8(bf16x8 lo, bf16x8 hi) {
  typedef float f32x8 __attribute__((ext_vector_type(8)));
  const f32x4 l = __builtin_bit_cast(f32x4, lo), h = __builtin_bit_cast(f32x4, hi);
  return __builtin_bit_cast(v8i_f8, f32x8{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]});
}

// raw s_barrier that the scheduler moves nothing across (the hand-scheduled phases of the 256-row kernels)
#define VLA_BARRIER()                      \
  do {                                     \
    __builtin_amdgcn_sched_barrier(0);     \
    __builtin_amdgcn_s_barrier();          \
    asm volatile("" ::: "memory");         \
    __builtin_amdgcn_sched_barrier(0);     \
  } while (0)

// XCD-aware bijective order over `nwg` workgroups: workgroups b and b + 8 share an XCD (round-robin dispatch); every XCD gets a
// contiguous run of the tile list, so neighbouring tiles (same operand panel) hit the same L2
__device__ __forceinline__ int xcd_order(int bid, int nwg) {
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// ---------------------------------------------------------------- column reductions with a fixed summation order
// Weight / bias gradients summed over rows (norm dw / db, bias colsums, LayerScale) are reproducible bit for bit: one
// 1024-thread workgroup owns a slice of columns over ALL rows - LPR lanes x 8 columns per row segment, 1024 / LPR row groups
// (row r goes to group r % groups) - and sums in a fixed order: the row groups of a wave by a lane butterfly, then the 16 waves
// in index order.  Its total is added with one atomic per column; no two workgroups of a launch add to the same column, so the
// result does not depend on which workgroup finishes first (cross-workgroup f32 atomics did).
// LPR 8: 64 columns and 128 row groups per workgroup (narrower slices for tall inputs measured slower: 32-B row segments).
constexpr int CR_THREADS = 1024;

template <int LPR>
struct CR {
  static constexpr int COLS = 8 * LPR, GROUPS = CR_THREADS / LPR;
  // thread -> (first of its 8 columns, first row): columns blockIdx.x * COLS + [0, COLS), rows row0, row0 + GROUPS, ...
  static __device__ __forceinline__ int col() { return blockIdx.x * COLS + (threadIdx.x % LPR) * 8; }
  static __device__ __forceinline__ int row0() { return threadIdx.x / LPR; }
  static int blocks(int cols) { return (cols + COLS - 1) / COLS; }

  // out[c] += sum over the workgroup of a[] (every thread of the workgroup must call it)
  static __device__ __forceinline__ void add(float (&a)[8], float* __restrict__ out, int cols, float (*sm)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) a[k] += __shfl_xor(a[k], o, 64);
    if (lane < LPR)
#pragma unroll
      for (int k = 0; k < 8; ++k) sm[w][lane * 8 + k] = a[k];
    __syncthreads();
    const int c = blockIdx.x * COLS + threadIdx.x;
    if (threadIdx.x < COLS && c < cols) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CR_THREADS / 64; ++i) s += sm[i][threadIdx.x];
      atomicAdd(out + c, s);
    }
    __syncthreads();                                       // sm may be reused by the next call
  }
};

// launch KERNEL<8> over `cols` columns (grid y = 1, z = batch)
#define CR_LAUNCH(KERNEL, rows, cols, batch, stream, ...) \
  hipLaunchKernelGGL(KERNEL<8>, dim3(CR<8>::blocks(cols), 1, (batch)), dim3(CR_THREADS), 0, (hipStream_t)(stream), __VA_ARGS__)
