// Greedy action-token decoding with a key/value cache (VLAEngine.generate): what one cached single-token step needs beside the norms
// and GEMMs it shares with the full-sequence forward.  Declared in include/vla_decode.h.
//   vla_decode_prompt           ids, mask and per-row positions of the prompt-only batch
//   vla_decode_rope_append      RoPE of the new token's q and k at pos[b]; k and v into row pos[b] of the layer's cache
//   vla_decode_attn             one query row per (b, head) against keys 0 .. pos[b] of the cache
//   vla_decode_lm_head_argmax   logits in one stream of the lm_head, argmax, and the hand-over to the next step
// Positions are read from device memory, so one captured step graph serves every token of a ragged batch.  No atomics: every
// output element is written by one thread and every reduction has a fixed order.
#include "gemm_epilogue.h"
#include "argmax_order.h"
#include "decode_advance.h"
#include "../../include/vla_decode.h"
#include <limits.h>

namespace {

constexpr int DEC_THREADS = 256;

// ---------------------------------------------------------------- prompt assembly: one workgroup per sample
__global__ void __launch_bounds__(DEC_THREADS)
decode_prompt_kernel(const long long* __restrict__ prompt_flat, const int* __restrict__ prompt_off, long long n_flat,
                     long long* __restrict__ ids, unsigned char* __restrict__ attn, int* __restrict__ pos, int* __restrict__ last_row,
                     unsigned char* __restrict__ row_ok, int L, int Np, long long pad_id) {
  const int b = blockIdx.x;
  const long long o0 = min(max((long long)prompt_off[b], 0ll), n_flat);
  const long long o1 = min(max((long long)prompt_off[b + 1], o0), n_flat);
  const long long len = o1 - o0;
  const bool ok = len >= 1 && len <= (long long)L;
  const long long P = ok ? len : 1;                    // not ok: the row of the one-id prompt [pad_id]
  for (int j = threadIdx.x; j < L; j += DEC_THREADS) {
    const long long o = (long long)b * L + j;
    ids[o] = (ok && j < P) ? prompt_flat[o0 + j] : pad_id;
    attn[o] = j < P;
  }
  if (threadIdx.x == 0) {
    const int p = Np + (int)P - 1;
    pos[b] = p;
    last_row[b] = b * (Np + L) + p;
    row_ok[b] = ok;
  }
}

// ---------------------------------------------------------------- RoPE of the new token and append
// One thread per (b, head of q|k|v, pair d / d + dh/2): q rotated in place, k rotated into the cache, v copied into the cache.
__global__ void decode_rope_append_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ ct, const float* __restrict__ st,
                                          const int* __restrict__ pos, bf16_t* __restrict__ kc, bf16_t* __restrict__ vc, int B, int Hq,
                                          int Hkv, int dh, int ld_qkv, int S_cap, long long sb, int ss) {
  const int half = dh / 2, heads = Hq + 2 * Hkv;
  const long long total = (long long)B * heads * half;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % half);
    const long long t = i / half;
    const int hh = (int)(t % heads), b = (int)(t / heads);
    const int p = pos[b];
    if (p < 0 || p >= S_cap) continue;                 // a position outside the cache: nothing of this row is touched
    bf16_t* x = qkv + (long long)b * ld_qkv + hh * dh + d;
    if (hh < Hq + Hkv) {
      const float a = bf2f(x[0]), bb = bf2f(x[half]);
      const float c = ct[p * half + d], s = st[p * half + d];
      const bf16_t ra = f2bf(rope_rot_a(a, bb, c, s)), rb = f2bf(rope_rot_b(a, bb, c, s));
      if (hh < Hq) {
        x[0] = ra;
        x[half] = rb;
      } else {
        bf16_t* k = kc + (long long)b * sb + (long long)p * ss + (hh - Hq) * dh + d;
        k[0] = ra;
        k[half] = rb;
      }
    } else {
      bf16_t* v = vc + (long long)b * sb + (long long)p * ss + (hh - Hq - Hkv) * dh + d;
      v[0] = x[0];
      v[half] = x[half];
    }
  }
}

// ---------------------------------------------------------------- single-query attention over the cache
// One workgroup per (kv head, b): the G = Hq / Hkv query heads of the group are its rows, so the cache is read once per group.  Keys
// go to the four waves in tiles of ATT_TILE (tile t -> wave t % 4): a lane owns one key for the scores (its row against the G
// queries held in LDS), then one (or two) columns of dh for the weighted sum, the probabilities passing through the wave's own LDS
// rows.  Each wave keeps a running (max, sum, accumulator) per query; the four are merged in LDS in wave order.
constexpr int ATT_TILE = 64, ATT_WAVES = DEC_THREADS / 64, ATT_MAXG = 8;

template <int DH>
__global__ void __launch_bounds__(DEC_THREADS)
decode_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                   const int* __restrict__ pos, bf16_t* __restrict__ out, int G, int ld_q, int ld_out, int S_cap, long long sb, int ss,
                   float scale) {
  constexpr int E = DH / 64;                           // columns of dh per lane in the weighted sum
  __shared__ __attribute__((aligned(16))) float qs[ATT_MAXG][DH];
  __shared__ float ps[ATT_WAVES][ATT_MAXG][ATT_TILE];
  __shared__ float acc_s[ATT_WAVES][ATT_MAXG][DH];
  __shared__ float red_m[ATT_WAVES][ATT_MAXG], red_l[ATT_WAVES][ATT_MAXG];
  const int kvh = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = min(max(pos[b], 0), S_cap - 1) + 1;    // keys 0 .. pos[b]
  const bf16_t* qb = q + (long long)b * ld_q + (long long)kvh * G * DH;
  for (int i = tid; i < G * DH; i += DEC_THREADS) qs[i / DH][i % DH] = bf2f(qb[i]);
  __syncthreads();

  const bf16_t* kb = kc + (long long)b * sb + kvh * DH;
  const bf16_t* vb = vc + (long long)b * sb + kvh * DH;
  float m[ATT_MAXG], l[ATT_MAXG], acc[ATT_MAXG][E];
#pragma unroll
  for (int g = 0; g < ATT_MAXG; ++g) {
    m[g] = -__builtin_inff();
    l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) acc[g][e] = 0.f;
  }
  const int ntiles = (n + ATT_TILE - 1) / ATT_TILE;
  for (int tile = w; tile < ntiles; tile += ATT_WAVES) {
    const int j = tile * ATT_TILE + lane;
    const bool valid = j < n;
    float s[ATT_MAXG];
#pragma unroll
    for (int g = 0; g < ATT_MAXG; ++g) s[g] = 0.f;
    if (valid) {
      const bf16_t* kp = kb + (long long)j * ss;
#pragma unroll 2
      for (int c = 0; c < DH; c += 8) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(kp + c), f);
#pragma unroll
        for (int g = 0; g < ATT_MAXG; ++g)
          if (g < G) {
            const float4 q0 = *reinterpret_cast<const float4*>(&qs[g][c]), q1 = *reinterpret_cast<const float4*>(&qs[g][c + 4]);
            s[g] += f[0] * q0.x + f[1] * q0.y + f[2] * q0.z + f[3] * q0.w + f[4] * q1.x + f[5] * q1.y + f[6] * q1.z + f[7] * q1.w;
          }
      }
    }
#pragma unroll
    for (int g = 0; g < ATT_MAXG; ++g)
      if (g < G) {
        const float sg = valid ? s[g] * scale : -__builtin_inff();
        const float mn = fmaxf(m[g], wave_max(sg));    // (the tile holds at least one key: mn is finite unless a score is not)
        const float corr = __expf(m[g] - mn);
        const float p = valid ? __expf(sg - mn) : 0.f;
        l[g] = l[g] * corr + wave_sum(p);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[g][e] *= corr;
        m[g] = mn;
        ps[w][g][lane] = p;
      }
    __builtin_amdgcn_wave_barrier();                   // ps[w] is this wave's own: written above, read below by its other lanes
    const int cnt = min(ATT_TILE, n - tile * ATT_TILE);
    const bf16_t* vp = vb + (long long)tile * ATT_TILE * ss + lane * E;
    for (int jj = 0; jj < cnt; ++jj) {
      float v[E];
      if constexpr (E == 2) {
        const unsigned u = *reinterpret_cast<const unsigned*>(vp + (long long)jj * ss);
        v[0] = bf_lo(u);
        v[1] = bf_hi(u);
      } else {
        v[0] = bf2f(vp[(long long)jj * ss]);
      }
#pragma unroll
      for (int g = 0; g < ATT_MAXG; ++g)
        if (g < G) {
          const float p = ps[w][g][jj];
#pragma unroll
          for (int e = 0; e < E; ++e) acc[g][e] += p * v[e];
        }
    }
    __builtin_amdgcn_wave_barrier();
  }
#pragma unroll
  for (int g = 0; g < ATT_MAXG; ++g)
    if (g < G) {
      if (lane == 0) {
        red_m[w][g] = m[g];
        red_l[w][g] = l[g];
      }
#pragma unroll
      for (int e = 0; e < E; ++e) acc_s[w][g][lane * E + e] = acc[g][e];
    }
  __syncthreads();
  bf16_t* ob = out + (long long)b * ld_out + (long long)kvh * G * DH;
  for (int i = tid; i < G * DH; i += DEC_THREADS) {
    const int g = i / DH, d = i % DH;
    float M = red_m[0][g];                             // wave 0 always holds key 0: M is finite
#pragma unroll
    for (int k = 1; k < ATT_WAVES; ++k) M = fmaxf(M, red_m[k][g]);
    float L = 0.f, o = 0.f;
#pragma unroll
    for (int k = 0; k < ATT_WAVES; ++k) {              // a wave without a tile holds (-inf, 0, 0): weight exp(-inf) = 0
      const float e = __expf(red_m[k][g] - M);
      L += red_l[k][g] * e;
      o += acc_s[k][g][d] * e;
    }
    ob[i] = f2bf(o / L);                               // one key: (v * 1) / 1, the v row bit for bit
  }
}

// ---------------------------------------------------------------- lm_head argmax
// Pass 1: workgroup (slab, chunk of LM_NB samples) streams LM_SLAB rows of W once and holds the chunk's x rows in LDS.  A group of 16
// lanes owns a row of W (8 columns per lane and round), so a wave works on four rows and the workgroup on sixteen at a time; the
// partial sums of a row meet in a 16-lane butterfly.  The rounded logit is the value stored AND the value compared.  Each group
// keeps its best pair per sample; groups, then waves (in index order) merge in the order of argmax_order.h into one pair per
// (sample, slab).  Pass 2: one workgroup walks the slabs of every sample in a fixed order and performs the advance.
constexpr int LM_SLAB = 128, LM_NB = 8, LM_MAX_D = 4096, LM_MAX_B = 64;

__global__ void __launch_bounds__(DEC_THREADS)
lm_head_slab_kernel(const bf16_t* __restrict__ x, int ld_x, const bf16_t* __restrict__ W, int ld_w, int B, int D, int V,
                    float* __restrict__ part_val, int* __restrict__ part_idx, int n_slab, bf16_t* __restrict__ logits_out,
                    long long ld_logits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lm_smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(lm_smem);     // [nb][D]
  __shared__ float red_v[DEC_THREADS / 64][LM_NB];
  __shared__ int red_i[DEC_THREADS / 64][LM_NB];
  const int slab = blockIdx.x, b0 = blockIdx.y * LM_NB, nb = min(LM_NB, B - b0);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, sub = lane & 15, rg = lane >> 4;
  const int D8 = D / 8;
  for (int i = tid; i < nb * D8; i += DEC_THREADS) {
    const int r = i / D8, c = i % D8;
    reinterpret_cast<uint4*>(xs)[i] = *reinterpret_cast<const uint4*>(x + (long long)(b0 + r) * ld_x + c * 8);
  }
  __syncthreads();
  float bv[LM_NB];
  int bi[LM_NB];
#pragma unroll
  for (int k = 0; k < LM_NB; ++k) {
    bv[k] = -__builtin_inff();
    bi[k] = INT_MAX;                                   // (no row seen yet: loses to every real pair, -inf included)
  }
  for (int it = 0; it < LM_SLAB / 16; ++it) {
    const int row = slab * LM_SLAB + it * 16 + w * 4 + rg;
    const bool valid = row < V;
    float acc[LM_NB];
#pragma unroll
    for (int k = 0; k < LM_NB; ++k) acc[k] = 0.f;
    if (valid) {
      const bf16_t* wr = W + (long long)row * ld_w;
      for (int c = sub * 8; c < D; c += 128) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(wr + c), f);
#pragma unroll
        for (int k = 0; k < LM_NB; ++k)
          if (k < nb) {
            float g[8];
            unpack8(*reinterpret_cast<const uint4*>(xs + k * D + c), g);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[k] = __builtin_fmaf(f[e], g[e], acc[k]);
          }
      }
    }
#pragma unroll
    for (int k = 0; k < LM_NB; ++k)
      if (k < nb) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
      }
    if (valid) {
#pragma unroll
      for (int k = 0; k < LM_NB; ++k)
        if (k < nb) {
          const bf16_t r16 = f2bf(acc[k]);
          const float r = bf2f(r16);
          if (logits_out && sub == 0) logits_out[(long long)(b0 + k) * ld_logits + row] = r16;
          if (argmax_before(r, row, bv[k], bi[k])) { bv[k] = r; bi[k] = row; }
        }
    }
  }
#pragma unroll
  for (int k = 0; k < LM_NB; ++k)
    if (k < nb) {
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {              // the four row groups of the wave; the order is total
        const float ov = __shfl_xor(bv[k], o, 64);
        const int oi = __shfl_xor(bi[k], o, 64);
        if (argmax_before(ov, oi, bv[k], bi[k])) { bv[k] = ov; bi[k] = oi; }
      }
      if (lane == 0) {
        red_v[w][k] = bv[k];
        red_i[w][k] = bi[k];
      }
    }
  __syncthreads();
  if (tid < nb) {
    float v = red_v[0][tid];
    int i = red_i[0][tid];
    for (int k = 1; k < DEC_THREADS / 64; ++k)
      if (argmax_before(red_v[k][tid], red_i[k][tid], v, i)) { v = red_v[k][tid]; i = red_i[k][tid]; }
    part_val[(long long)(b0 + tid) * n_slab + slab] = v;
    part_idx[(long long)(b0 + tid) * n_slab + slab] = i;
  }
}

__global__ void __launch_bounds__(DEC_THREADS)
lm_head_finish_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx, int n_slab, int B, int D, int V,
                      long long* __restrict__ id, long long* __restrict__ out_ids, int T, int* __restrict__ step, int* __restrict__ pos,
                      const int* __restrict__ pos_from,
                      const bf16_t* __restrict__ embed, int vocab_e, int ld_embed, bf16_t* __restrict__ x_next, int ld_next) {
  __shared__ float red_v[DEC_THREADS / 64];
  __shared__ int red_i[DEC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int t = decode_step_index(out_ids, pos_from, step);   // (read by every thread before thread 0 advances it behind the last barrier)
  for (int b = 0; b < B; ++b) {
    float bv = -__builtin_inff();
    int bi = INT_MAX;
    for (int s = tid; s < n_slab; s += DEC_THREADS) {
      const float v = part_val[(long long)b * n_slab + s];
      const int i = part_idx[(long long)b * n_slab + s];
      if (argmax_before(v, i, bv, bi)) { bv = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (argmax_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
      red_v[w] = bv;
      red_i[w] = bi;
    }
    __syncthreads();
    bv = red_v[0];
    bi = red_i[0];
    for (int k = 1; k < DEC_THREADS / 64; ++k)
      if (argmax_before(red_v[k], red_i[k], bv, bi)) { bv = red_v[k]; bi = red_i[k]; }
    bi = min(max(bi, 0), V - 1);                       // (every slab holds a row: bi is one already)
    if (tid == 0) id[b] = bi;
    if (out_ids) decode_advance_row(b, bi, t, tid, DEC_THREADS, out_ids, T, embed, vocab_e, ld_embed, x_next, ld_next, D);
    __syncthreads();                                   // red_v / red_i are reused by the next sample
  }
  if (out_ids) decode_advance_counters(B, t, tid, DEC_THREADS, step, pos, pos_from);
}

inline unsigned grid_for(long long n) {
  const long long blocks = (n + DEC_THREADS - 1) / DEC_THREADS;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int vla_decode_prompt(void* stream, const long long* prompt_flat, const int* prompt_off, long long n_flat, long long* ids,
                                 unsigned char* attention_mask, int* pos, int* last_row, unsigned char* row_ok, int B, int L, int Np,
                                 long long pad_id) {
  VLA_REQUIRE(prompt_off && ids && attention_mask && pos && last_row && row_ok, "decode_prompt: null pointer");
  VLA_REQUIRE(prompt_flat || n_flat == 0, "decode_prompt: null prompt_flat with n_flat > 0");
  VLA_REQUIRE(B > 0 && n_flat >= 0 && L >= 1 && Np >= 0, "decode_prompt: B > 0, n_flat >= 0, L >= 1, Np >= 0");
  VLA_REQUIRE((long long)B * ((long long)Np + L) <= (long long)INT_MAX, "decode_prompt: B * (Np + L) must fit an int32 row index");
  hipLaunchKernelGGL(decode_prompt_kernel, dim3(B), dim3(DEC_THREADS), 0, (hipStream_t)stream, prompt_flat, prompt_off, n_flat, ids,
                     attention_mask, pos, last_row, row_ok, L, Np, pad_id);
  VLA_CHECK_LAUNCH("decode_prompt");
  return VLA_OK;
}

// the cache view both cache kernels take
#define DEC_REQUIRE_CACHE(name, k, v, Hkv, dh, S_cap, sb, ss)                                                                        \
  do {                                                                                                                                \
    VLA_REQUIRE((k) && (v) && aligned16(k) && aligned16(v), name ": k_cache / v_cache must be 16-B aligned and not null");              \
    VLA_REQUIRE((S_cap) >= 1 && (ss) % 8 == 0 && (sb) % 8 == 0 && (ss) >= (Hkv) * (dh) && (sb) >= (long long)(S_cap) * (ss),            \
                name ": S_cap >= 1, cache_ss >= Hkv * dh, cache_sb >= S_cap * cache_ss, both multiples of 8");                         \
  } while (0)

extern "C" int vla_decode_rope_append(void* stream, void* qkv, const float* cos_t, const float* sin_t, const int* pos, void* k_cache,
                                      void* v_cache, int B, int Hq, int Hkv, int dh, int ld_qkv, int S_cap, long long cache_sb,
                                      int cache_ss) {
  VLA_REQUIRE(qkv && cos_t && sin_t && pos, "decode_rope_append: null pointer");
  VLA_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && dh > 0 && dh % 2 == 0, "decode_rope_append: B, Hq, Hkv > 0, dh even");
  VLA_REQUIRE(ld_qkv >= (Hq + 2 * Hkv) * dh, "decode_rope_append: ld_qkv below (Hq + 2 Hkv) dh");
  DEC_REQUIRE_CACHE("decode_rope_append", k_cache, v_cache, Hkv, dh, S_cap, cache_sb, cache_ss);
  const long long total = (long long)B * (Hq + 2 * Hkv) * (dh / 2);
  hipLaunchKernelGGL(decode_rope_append_kernel, dim3(grid_for(total)), dim3(DEC_THREADS), 0, (hipStream_t)stream, (bf16_t*)qkv, cos_t,
                     sin_t, pos, (bf16_t*)k_cache, (bf16_t*)v_cache, B, Hq, Hkv, dh, ld_qkv, S_cap, cache_sb, cache_ss);
  VLA_CHECK_LAUNCH("decode_rope_append");
  return VLA_OK;
}

extern "C" int vla_decode_attn(void* stream, const void* q, const void* k_cache, const void* v_cache, const int* pos, void* out, int B,
                               int Hq, int Hkv, int dh, int ld_q, int ld_out, int S_cap, long long cache_sb, int cache_ss, float scale) {
  VLA_REQUIRE(q && pos && out, "decode_attn: null pointer");
  VLA_REQUIRE(B > 0 && B <= 65535 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Hq / Hkv <= ATT_MAXG,
              "decode_attn: B in [1, 65535], Hq a multiple of Hkv with at most 8 query heads per kv head");
  VLA_REQUIRE(dh == 64 || dh == 128, "decode_attn: head dim 64 or 128");
  VLA_REQUIRE(ld_q >= Hq * dh && ld_out >= Hq * dh, "decode_attn: row strides below Hq * dh");
  DEC_REQUIRE_CACHE("decode_attn", k_cache, v_cache, Hkv, dh, S_cap, cache_sb, cache_ss);
  const dim3 grid(Hkv, B);
  if (dh == 64)
    hipLaunchKernelGGL(decode_attn_kernel<64>, grid, dim3(DEC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k_cache,
                       (const bf16_t*)v_cache, pos, (bf16_t*)out, Hq / Hkv, ld_q, ld_out, S_cap, cache_sb, cache_ss, scale);
  else
    hipLaunchKernelGGL(decode_attn_kernel<128>, grid, dim3(DEC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)q, (const bf16_t*)k_cache,
                       (const bf16_t*)v_cache, pos, (bf16_t*)out, Hq / Hkv, ld_q, ld_out, S_cap, cache_sb, cache_ss, scale);
  VLA_CHECK_LAUNCH("decode_attn");
  return VLA_OK;
}

extern "C" int vla_decode_argmax_slabs(int V) { return V > 0 ? (V + LM_SLAB - 1) / LM_SLAB : 0; }

extern "C" int vla_decode_lm_head_argmax(void* stream, const void* x, int ld_x, const void* W, int ld_w, int B, int D, int V,
                                         float* part_val, int* part_idx, long long* id, void* logits_out, long long ld_logits,
                                         long long* out_ids, int T, int* step, int* pos, const int* pos_from, const void* embed,
                                         int vocab_e, int ld_embed, void* x_next, int ld_next) {
  VLA_REQUIRE(x && W && part_val && part_idx && id, "decode_lm_head_argmax: null pointer");
  VLA_REQUIRE(B > 0 && B <= LM_MAX_B && V > 0 && D > 0 && D % 8 == 0 && D <= LM_MAX_D,
              "decode_lm_head_argmax: B in [1, 64], V > 0, D a multiple of 8 up to 4096");
  VLA_REQUIRE(ld_x >= D && ld_w >= D && ld_x % 8 == 0 && ld_w % 8 == 0 && aligned16(x) && aligned16(W),
              "decode_lm_head_argmax: x / W 16-B aligned, row strides multiples of 8 and at least D");
  VLA_REQUIRE(!logits_out || ld_logits >= V, "decode_lm_head_argmax: ld_logits below V");
  if (out_ids) {
    VLA_REQUIRE(T >= 1 && step && pos && embed && x_next, "decode_lm_head_argmax: the advance needs T >= 1, step, pos, embed and x_next");
    VLA_REQUIRE(vocab_e >= 1 && ld_embed >= D && ld_next >= D && ld_embed % 8 == 0 && ld_next % 8 == 0 && aligned16(embed) && aligned16(x_next),
                "decode_lm_head_argmax: embed / x_next 16-B aligned, row strides multiples of 8 and at least D");
  }
  const int n_slab = vla_decode_argmax_slabs(V);
  const int lds = LM_NB * D * (int)sizeof(bf16_t);
  if (lds > 48 * 1024) {
    const int rc = vla_lds_limit<lm_head_slab_kernel>(LM_NB * LM_MAX_D * (int)sizeof(bf16_t), "decode_lm_head_argmax");
    if (rc != VLA_OK) return rc;
  }
  hipLaunchKernelGGL(lm_head_slab_kernel, dim3(n_slab, (B + LM_NB - 1) / LM_NB), dim3(DEC_THREADS), lds, (hipStream_t)stream,
                     (const bf16_t*)x, ld_x, (const bf16_t*)W, ld_w, B, D, V, part_val, part_idx, n_slab, (bf16_t*)logits_out, ld_logits);
  VLA_CHECK_LAUNCH("decode_lm_head_argmax (slabs)");
  hipLaunchKernelGGL(lm_head_finish_kernel, dim3(1), dim3(DEC_THREADS), 0, (hipStream_t)stream, part_val, part_idx, n_slab, B, D, V, id,
                     out_ids, T, step, pos, pos_from, (const bf16_t*)embed, vocab_e, ld_embed, (bf16_t*)x_next, ld_next);
  VLA_CHECK_LAUNCH("decode_lm_head_argmax (finish)");
  return VLA_OK;
}
