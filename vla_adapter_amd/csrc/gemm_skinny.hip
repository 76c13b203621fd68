// Small-output NT products for gfx950:  C[M, N] = epilogue(alpha * A[M, K] . B[N, K]^T)  whose OUTPUT is too small to give every CU a
// 128 x 128 tile: (a) tall-skinny, N = 64 / 128 / 192 with M in the thousands; (b) short, M <= 512 (any N % 16 == 0).
//
// (a) replaces, for the LoRA fine-tune (vla-scripts/finetune.py:832-844, peft Linear.forward / its autograd), the two low-rank
// products on every wrapped Linear's forward / dX chain:  t = 2 x A_cat^T  (lora_A of all pairs that share the input) and
// dt = 2 dy B_blk  (the transpose of lora_B); (b) the action head's per-block Linears on its 8 x B query rows (action_heads.py:337-410:
// q | k | v, o_proj, ffn and their dX products) and the batch-1 pass's products (modeling_prismatic.py:892-972).  On the 128 x 128
// tiles of gemm.hip such a product is 7-44 workgroups, each pulling (128 + 128) K-rows through ONE CU's L1 (~50 GB/s per CU whatever
// the ring depth): ~20 us per launch in the step, 120 (head) + 280 (LoRA) launches per step.
//
// Here a workgroup owns a (16 MT) x (16 NT) output tile - 16 x 16 ... 64 x 96, picked per shape so that every CU gets a workgroup and
// pulls as few operand rows as possible - and its four waves split the contraction four ways (wave w: k in [w K/4, (w+1) K/4)); they read
// their operand fragments straight from global memory into registers in the MFMA layout (lane l: row l % 16, eight consecutive k at
// 8 (l / 16): 16 B per lane, 64 B per row and k-step) - no LDS staging, no barrier in the loop, U k-steps of loads in flight per wave.
// The four partial accumulators meet in LDS and are summed in wave order (deterministic); the epilogue runs on 8-column row chunks.
//
// Rounding: fp32 accumulation as four K-quarter partial sums added in order 0..3, then gemm.hip's epilogue at gemm.hip's rounding points
// (alpha, bias, activation on the bf16-rounded value, rotate_half or interleaved RoPE, bf16, + residual, bf16): the arithmetic of vla_gemm_bf16_nt
// with split_k = 4 (bit-identical to it when K % 256 == 0: test_gemm_skinny / test_gemm_small_rows).
#include "gemm_epilogue.h"
#include "gemm_params.h"

namespace {

template <int MT, int NT, int U>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmP p) {
  constexpr int TM = 16 * MT, TN = 16 * NT, LDP = TN + 4;          // partial rows padded by 16 B
  extern __shared__ __attribute__((aligned(16))) float part[];      // [4 waves][TM rows][LDP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const int kq = p.K >> 2, nks = kq >> 5;                           // this wave's K range: nks k-steps of 32
  const int k0 = wid * kq + lq * 8;
  const bf16_t* ap[MT];
  const bf16_t* bp[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) ap[i] = p.A + (long long)min(m0 + 16 * i + lr, p.M - 1) * p.lda + k0;
#pragma unroll
  for (int j = 0; j < NT; ++j) bp[j] = p.B + (long long)min(n0 + 16 * j + lr, p.N - 1) * p.ldb + k0;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[U][MT], fb[U][NT];
  auto load = [&](int u, int ks) {
#pragma unroll
    for (int i = 0; i < MT; ++i) fa[u][i] = *reinterpret_cast<const bf16x8*>(ap[i] + ks * 32);
#pragma unroll
    for (int j = 0; j < NT; ++j) fb[u][j] = *reinterpret_cast<const bf16x8*>(bp[j] + ks * 32);
  };
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < nks) load(u, u);
  for (int ks = 0; ks < nks; ks += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (ks + u < nks) {
        // operands swapped as in gemm.hip (first operand := B rows): lane owns row m = 16 i + lr and four consecutive n
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[u][j], fa[u][i], acc[i][j], 0, 0, 0);
        if (ks + u + U < nks) load(u, ks + u + U);
      }
    }
  }
  float* pw = part + wid * TM * LDP;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) *reinterpret_cast<f32x4*>(pw + (16 * i + lr) * LDP + 16 * j + 4 * lq) = acc[i][j];
  __syncthreads();
  constexpr int CPR = TN / 8;                                        // 16-byte output chunks per row
  const int act = p.act;
  for (int c = tid; c < TM * CPR; c += 256) {
    const int row = c / CPR, col = (c - row * CPR) * 8;
    const int m = m0 + row, n = n0 + col;
    if (m >= p.M || n >= p.N) continue;                              // (N % 8 == 0: a chunk is inside or outside)
    // the eight values of chunk (row, cc) after alpha / bias / activation (fp32, not yet rounded)
    auto chunk = [&](int cc, float* v) {
      const float* s = part + row * LDP + cc;
      f32x4 a0 = *reinterpret_cast<const f32x4*>(s), a1 = *reinterpret_cast<const f32x4*>(s + 4);
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        a0 += *reinterpret_cast<const f32x4*>(s + w * TM * LDP);
        a1 += *reinterpret_cast<const f32x4*>(s + w * TM * LDP + 4);
      }
      const float r[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
      float bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (p.bias) unpack8(*reinterpret_cast<const uint4*>(p.bias + n0 + cc), bb);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float x = p.bias_post ? epi_linear<true>(r[k], p.alpha, bb[k]) : epi_linear(r[k], p.alpha, bb[k]);
        epi_with_act(act, [&](auto fn) { v[k] = fn(x); });
      }
    };
    float v[8];
    chunk(col, v);
    if (p.rope_mode == 1 && n < p.rope_cols) {                       // HF rotate_half, head dim 64: the partner d +- 32 is another chunk of this row (TN == 64)
      const int d0 = n & 63, lo = d0 < 32;
      float q[8];
      chunk(lo ? col + 32 : col - 32, q);
      const int pos = m % p.rope_T, d = d0 & 31;
      const float* cp = p.rope_cos + (long long)pos * 32 + d;
      const float* sp = p.rope_sin + (long long)pos * 32 + d;
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
      const float cc[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]}, ss[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float own = rbf(v[k]), oth = rbf(q[k]);                  // this chunk holds the first (a) or the second (b) half of the pair
        v[k] = lo ? rope_rot_a(own, oth, cc[k], ss[k]) : rope_rot_b(oth, own, cc[k], ss[k]);
      }
    }
    if (p.rope_mode == 2 && n < p.rope_cols) {                       // action_heads.py:125-146: pairs (2i, 2i+1), tables of cat([f, f])
      const int pos = m % p.rope_T, d = n % p.rope_dh;
      const float* cp = p.rope_cos + (long long)pos * p.rope_dh + d;
      const float* sp = p.rope_sin + (long long)pos * p.rope_dh + d;
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
      const float cc[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]}, ss[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const float x0 = rbf(v[k]), x1 = rbf(v[k + 1]);
        v[k] = rope_rot_a(x0, x1, cc[k], ss[k]);
        v[k + 1] = rope_rot_b(x0, x1, cc[k + 1], ss[k + 1]);
      }
    }
    unsigned o[4] = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
    if (p.R) {
      const uint4 r4 = *reinterpret_cast<const uint4*>(p.R + (long long)m * p.ldr + n);
      const unsigned rw[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = add_packed2(o[k], rw[k]);
    }
    *reinterpret_cast<uint4*>(p.C + (long long)m * p.ldc + n) = uint4{o[0], o[1], o[2], o[3]};
  }
}

template <int MT, int NT, int U>
int launch_skinny(const GemmP& p, hipStream_t st) {
  constexpr int LDS = 4 * 16 * MT * (16 * NT + 4) * 4;
  if (int rc = vla_lds_limit<gemm_skinny_kernel<MT, NT, U>>(LDS, "gemm_skinny_kernel")) return rc;
  hipLaunchKernelGGL((gemm_skinny_kernel<MT, NT, U>), dim3((p.M + 16 * MT - 1) / (16 * MT), (p.N + 16 * NT - 1) / (16 * NT)), dim3(256), LDS, st, p);
  return VLA_OK;
}

}  // namespace

// Launch on SKINNY_TILE[tile] (called from vla_gemm_bf16_nt after its argument checks; the eligibility is gemm.hip's skinny_tile).
int vla_gemm_skinny_launch(const GemmP& p, int tile, hipStream_t st) {
  switch (tile) {
    case 0: return launch_skinny<1, 1, 8>(p, st);
    case 1: return launch_skinny<1, 2, 6>(p, st);
    case 2: return launch_skinny<2, 2, 6>(p, st);
    case 3: return launch_skinny<1, 4, 4>(p, st);
    case 4: return launch_skinny<2, 4, 4>(p, st);
    case 5: return launch_skinny<4, 4, 3>(p, st);
    default: return launch_skinny<4, 6, 2>(p, st);
  }
}
