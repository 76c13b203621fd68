// The epilogue arithmetic of a Linear, stated ONCE for every GEMM kernel (gemm.hip, gemm256.hip, gemm_skinny.hip, gemm_tn.hip,
// the split-K finalize passes) and for the stand-alone SwiGLU kernels of elementwise.hip.  Under bf16 autocast the chain is
//
//   acc * alpha (+ bias) -> bf16 -> activation -> bf16 -> RoPE (every product rounded) -> (+ residual) -> bf16
//
// with SwiGLU forward and backward as variants.  Everything here is value-level: what ONE lane holds (a value, four or eight of
// them), in and out by value or in small fixed arrays.  Staging layouts, load / store order and scheduling pins stay with the
// kernels; a change to a rounding point is made here and nowhere else (tests/test_epilogue_single_definition.py).
#pragma once
#include "common.h"
#include "../../include/vla_native.h"

// ---------------------------------------------------------------- linear
// x = alpha acc + bias (one FMA, not yet rounded); post-round form bf16(alpha acc) + bias: torch CPU Linear on a strided input
template <bool POST = false>
__device__ __forceinline__ float epi_linear(float acc, float alpha, float bias) {
  return POST ? rbf(acc * alpha) + bias : acc * alpha + bias;
}

// ---------------------------------------------------------------- activation
// Functors on the UNROUNDED linear value: the reference's Linear emits bf16 before the activation module (the rbf below); the
// activation's own bf16 rounding is the caller's pack or rbf.  (ReLU commutes with the rounding.)
struct ActNone { __device__ __forceinline__ float operator()(float v) const { return v; } };
struct ActGelu { __device__ __forceinline__ float operator()(float v) const { return gelu_erf(rbf(v)); } };
struct ActRelu { __device__ __forceinline__ float operator()(float v) const { return fmaxf(v, 0.f); } };
struct ActGeluTanh { __device__ __forceinline__ float operator()(float v) const { return gelu_tanh(rbf(v)); } };
// body(functor) with the functor of `act`: the choice is made HERE, outside the caller's element loops (a per-element switch cost
// 5 us on the ViT fc1 GEMM even for ReLU)
template <class Body>
__device__ __forceinline__ void epi_with_act(int act, Body&& body) {
  if (act == VLA_ACT_GELU) body(ActGelu{});
  else if (act == VLA_ACT_RELU) body(ActRelu{});
  else if (act == VLA_ACT_GELU_TANH) body(ActGeluTanh{});
  else body(ActNone{});
}

// ---------------------------------------------------------------- RoPE, on bf16-rounded values, every product rounded
// the pair rotation (a, b, c, s) -> (a c - b s, b c + a s), one output each
__device__ __forceinline__ float rope_rot_a(float a, float b, float c, float s) { return rbf(a * c) + rbf(-b * s); }
__device__ __forceinline__ float rope_rot_b(float a, float b, float c, float s) { return rbf(b * c) + rbf(a * s); }
// HF rotate_half: a[j] is column d + j of a head, b[j] its partner d + j + dh / 2; c / s the table segment at d (N values)
template <int N, class X, class T>
__device__ __forceinline__ void rope_half(X& a, X& b, const T& c, const T& s) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const float x = rbf(a[j]), y = rbf(b[j]);
    a[j] = rope_rot_a(x, y, c[j], s[j]);
    b[j] = rope_rot_b(x, y, c[j], s[j]);
  }
}
// interleaved (action_heads.py:125-146): the partners are neighbours (2i, 2i + 1) and the tables are cat([f, f]) - a table value per
// column: x[2i] = rope_rot_a(x0, x1, c[2i], s[2i]), x[2i + 1] = rope_rot_b(x0, x1, c[2i + 1], s[2i + 1]), written at the call sites

// ---------------------------------------------------------------- SwiGLU, on bf16-rounded g, u (and d)
__device__ __forceinline__ float sigmoid_rcp(float g) { return __builtin_amdgcn_rcpf(1.0f + __expf(-g)); }
__device__ __forceinline__ float silu_grad(float g, float sg) { return sg * (1.0f + g * (1.0f - sg)); }   // d silu / dg, sg = sigmoid(g)
// forward: h = bf16(silu(g)) u (the caller's pack rounds h)
__device__ __forceinline__ float swiglu_h(float g, float u) { return rbf(g * sigmoid_rcp(g)) * u; }
// backward: (d, g, u) -> (dg, du) = (d u silu'(g), d silu(g))
__device__ __forceinline__ void swiglu_bwd(float d, float g, float u, float& dg, float& du) {
  const float sg = sigmoid_rcp(g);
  du = d * g * sg;
  dg = d * u * silu_grad(g, sg);
}

// ---------------------------------------------------------------- residual add on packed bf16: bf16(a + r) per element
__device__ __forceinline__ unsigned add_packed2(unsigned a, unsigned r) { return pack2(bf_lo(a) + bf_lo(r), bf_hi(a) + bf_hi(r)); }
template <class R>   // a 16-byte segment; r: uint4 or u32x4
__device__ __forceinline__ uint4 add_packed8(const uint4& a, const R& r) {
  if constexpr (__is_same(R, uint4)) return uint4{add_packed2(a.x, r.x), add_packed2(a.y, r.y), add_packed2(a.z, r.z), add_packed2(a.w, r.w)};
  else return uint4{add_packed2(a.x, r[0]), add_packed2(a.y, r[1]), add_packed2(a.z, r[2]), add_packed2(a.w, r[3])};
}
// a rounded (not yet packed) value plus its residual: bf16(v) + r, packed by the caller
__device__ __forceinline__ void add_residual4(float (&v)[4], const uint2& r) {
  float rr[4];
  unpack4(r, rr);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = rbf(v[j]) + rr[j];
}
// ragged tail: the elements n + k < N of the staged segment v (columns n .. n + 7) one at a time into the row at c + crow, plus
// those of the residual row at r + roff (r == nullptr: none)
__device__ __forceinline__ void store_tail8(bf16_t* c, long long crow, const bf16_t* r, long long roff, const uint4& v, int n, int N) {
  const unsigned wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (n + k < N) {
      float f = (k & 1) ? bf_hi(wv[k >> 1]) : bf_lo(wv[k >> 1]);
      if (r) f += bf2f(r[roff + n + k]);
      c[crow + n + k] = f2bf(f);
    }
  }
}

// ---------------------------------------------------------------- row offsets (elements)
// row-group addressing: row m at (m / g) * stride + (m % g) * ld; g == 0: plain rows
__device__ __forceinline__ long long grouped_row(int m, int g, long long stride, int ld) {
  return g > 0 ? (long long)(m / g) * stride + (long long)(m % g) * ld : (long long)m * ld;
}
// residual row: broadcast over blocks of res_mod rows (m % res_mod), else grouped, else plain
__device__ __forceinline__ long long residual_row(int m, int res_mod, int g, long long stride, int ld) {
  return res_mod > 0 ? (long long)(m % res_mod) * ld : grouped_row(m, g, stride, ld);
}
// live-row filter: rows with (m % mod) < from are never read again and not stored (mod == 0: every row is live)
__device__ __forceinline__ bool row_live(int m, int mod, int from) { return !(mod > 0 && (m % mod) < from); }
