// Sampling of action tokens (VLAEngine.generate with sample= / return_logprobs).  Declared in include/vla_sample.h; the rule is
// restated in float64 by tests/sample_rule_np.py and written out in DESIGN section 23.
//   vla_sample_tokens   temperature, top-k, top-p, Gumbel-max draw and log-probability of one decoding step - or the greedy token with
//                       its log-probability - and the advance of include/vla_decode.h
// One workgroup of 1024 threads per row; the row (V bf16 logits, L2-resident behind the lm_head pass that wrote it) is walked once per
// phase.  A bf16 logit has 65 536 possible values, so both thresholds are order statistics of an order-preserving 16-bit key and are
// found EXACTLY by two rounds of a 256-bin histogram each (high byte, then low byte inside the chosen bin): counts for top-k, and for
// top-p the probability mass in 2^-40 fixed point.  The histograms are integer sums in LDS, which commute; every floating-point sum
// runs in a fixed order (a thread's elements in ascending order, the lanes of a wave by a butterfly, the waves in index order) and in
// double.  No float atomics: the same inputs give the same bits.
#include "common.h"
#include "argmax_order.h"
#include "decode_advance.h"
#include "../../include/vla_sample.h"
#include <limits.h>

namespace {

constexpr int SMP_THREADS = 1024, SMP_WAVES = SMP_THREADS / 64, SMP_MAX_B = 64, ADV_THREADS = 256, BINS = 256;
constexpr unsigned long long SAMPLE_STREAM = 0x5A3D1E70C0DE5ull;   // keeps these draws apart from the dropout's, the augmentation's, the collator's and the shuffles'
constexpr float MASS_ONE = 1099511627776.f;                        // 2^40: the fixed-point unit of the top-p mass (exp(z - zmax) <= 1)

struct SampleParams {                                              // include/vla_sample.h: 24 bytes in device memory
  float temperature, top_p;
  int top_k, greedy;
  unsigned long long seed;
};
static_assert(sizeof(SampleParams) == 24, "the parameter block of include/vla_sample.h");

// bf16 bits -> a 16-bit key in the order of the values (-0 and +0 are one value); NaNs never reach it
__device__ __forceinline__ unsigned sample_key(bf16_t u) {
  if (u == 0x8000u) u = 0;
  return (u & 0x8000u) ? (~(unsigned)u & 0xffffu) : ((unsigned)u | 0x8000u);
}
__device__ __forceinline__ float sample_key_value(unsigned key) {
  const unsigned bits = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);      // the bf16 bit pattern of the key
  return __uint_as_float(bits << 16);
}
__device__ __forceinline__ float scaled(bf16_t u, float temperature) { return __fdiv_rn(bf2f(u), temperature); }

// Bins walked from the top: sel[0] = the bin in which the running count first reaches `target` (1 <= target <= the total),
// sel[1] = the count above that bin.  Integer sums: every thread below BINS adds up the bins above its own.
__device__ __forceinline__ void select_from_top(const unsigned* cnt, unsigned target, unsigned* sel) {
  const int t = threadIdx.x;
  if (t < BINS) {
    unsigned above = 0;
    for (int j = BINS - 1; j > t; --j) above += cnt[j];
    if (above < target && above + cnt[t] >= target) {
      sel[0] = (unsigned)t;
      sel[1] = above;
    }
  }
  __syncthreads();
}
// Bins walked from the bottom: sel[0] = the first bin through which the running mass exceeds x (x < the total), sel[1] = the mass below.
__device__ __forceinline__ void select_from_bottom(const unsigned long long* mass, unsigned long long x, unsigned long long* sel) {
  const int t = threadIdx.x;
  if (t < BINS) {
    unsigned long long below = 0;
    for (int j = 0; j < t; ++j) below += mass[j];
    if (below <= x && below + mass[t] > x) {
      sel[0] = (unsigned long long)t;
      sel[1] = below;
    }
  }
  __syncthreads();
}

// The best (value, index) pair of the workgroup in the order of argmax_order.h (a total order: any grouping gives the same pair).
__device__ __forceinline__ void block_argmax(float& v, int& i, float* red_v, int* red_i) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (argmax_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
  __syncthreads();                                     // red_* may still be read from the previous call
  if (lane == 0) {
    red_v[w] = v;
    red_i[w] = i;
  }
  __syncthreads();
  v = red_v[0];
  i = red_i[0];
  for (int k = 1; k < SMP_WAVES; ++k)
    if (argmax_before(red_v[k], red_i[k], v, i)) { v = red_v[k]; i = red_i[k]; }
}

__global__ void __launch_bounds__(SMP_THREADS)
sample_kernel(const bf16_t* __restrict__ logits, long long ld_logits, int V, const SampleParams* __restrict__ params,
              const long long* __restrict__ streams, long long* __restrict__ id, float* __restrict__ logprob_out,
              float* __restrict__ probs_out, long long ld_probs, int T, const int* __restrict__ step, const int* __restrict__ pos_from) {
  __shared__ unsigned cnt[BINS];
  __shared__ unsigned long long mass[BINS];
  __shared__ float red_v[SMP_WAVES];
  __shared__ int red_i[SMP_WAVES];
  __shared__ double red_d[SMP_WAVES];
  __shared__ unsigned sel_c[2];
  __shared__ unsigned long long sel_m[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* row = logits + (long long)b * ld_logits;
  const SampleParams P = *params;
  const int t = pos_from ? 0 : *step;
  const bool greedy = P.greedy != 0;
  const bool params_ok = greedy || (P.temperature > 0.f && P.top_p > 0.f && P.top_p <= 1.f && P.top_k >= 0);   // (a NaN fails every comparison)
  const float temperature = greedy ? 1.f : P.temperature;       // l / 1 = l: the greedy log-probability is log_softmax(l)
  const bool use_k = !greedy && params_ok && P.top_k >= 1 && P.top_k < V;
  const bool use_p = !greedy && params_ok && P.top_p < 1.f;
  const float ninf = -__builtin_inff();

  // ---- phase 0: the greedy pair, the non-finite test, and the high-byte counts of top-k
  if (tid < BINS) cnt[tid] = 0;
  __syncthreads();
  float gv = ninf;
  int gi = INT_MAX;
  int bad = 0;
  for (int v = tid; v < V; v += SMP_THREADS) {
    const bf16_t u = row[v];
    const float l = bf2f(u);
    if (argmax_before(l, v, gv, gi)) { gv = l; gi = v; }       // (INT_MAX loses to every column, a -inf one included)
    bad |= (l != l) || (l == __builtin_inff());
    if (use_k) atomicAdd(&cnt[sample_key(u) >> 8], 1u);
  }
  block_argmax(gv, gi, red_v, red_i);
  gi = min(max(gi, 0), V - 1);                                 // (thread 0 holds column 0: gi is a column already)
  bad = __syncthreads_or(bad);
  float* prow = probs_out ? probs_out + (long long)b * ld_probs : nullptr;
  if (bad || !params_ok || gv == ninf) {                       // a non-finite row: the greedy token, NaN everywhere else
    const float nan = __builtin_nanf("");
    if (tid == 0) {
      id[b] = gi;
      if (logprob_out && t >= 0 && t < T) logprob_out[(long long)b * T + t] = nan;
    }
    if (prow)
      for (int v = tid; v < V; v += SMP_THREADS) prow[v] = nan;
    return;
  }
  const float zmax = __fdiv_rn(gv, temperature);

  // ---- top-k: the k-th largest key, exactly, from the high-byte counts and the low-byte counts inside the chosen bin
  float z_thr = ninf;
  if (use_k) {
    select_from_top(cnt, (unsigned)P.top_k, sel_c);
    const unsigned h1 = sel_c[0], want = (unsigned)P.top_k - sel_c[1];
    __syncthreads();
    if (tid < BINS) cnt[tid] = 0;
    __syncthreads();
    for (int v = tid; v < V; v += SMP_THREADS) {
      const unsigned key = sample_key(row[v]);
      if ((key >> 8) == h1) atomicAdd(&cnt[key & 255u], 1u);
    }
    __syncthreads();
    select_from_top(cnt, want, sel_c);
    z_thr = __fdiv_rn(sample_key_value((h1 << 8) | sel_c[0]), temperature);
  }

  // ---- top-p over what top-k kept: the first class, from the bottom, through which the cumulative mass exceeds (1 - top_p) of the total
  if (use_p) {
    if (tid < BINS) mass[tid] = 0;
    __syncthreads();
    for (int v = tid; v < V; v += SMP_THREADS) {
      const bf16_t u = row[v];
      const float z = scaled(u, temperature);
      if (z >= z_thr) atomicAdd(&mass[sample_key(u) >> 8], (unsigned long long)(expf(z - zmax) * MASS_ONE));
    }
    __syncthreads();
    unsigned long long total = 0;
    for (int j = 0; j < BINS; ++j) total += mass[j];           // (every thread the same integer sum; the largest token alone adds 2^40)
    const unsigned long long x = (unsigned long long)((1.0 - (double)P.top_p) * (double)total);   // floor: mass > x as integers <=> as reals
    select_from_bottom(mass, x, sel_m);
    const unsigned hp = (unsigned)sel_m[0];
    const unsigned long long rest = x - sel_m[1];
    __syncthreads();
    if (tid < BINS) mass[tid] = 0;
    __syncthreads();
    for (int v = tid; v < V; v += SMP_THREADS) {
      const bf16_t u = row[v];
      const unsigned key = sample_key(u);
      const float z = scaled(u, temperature);
      if (z >= z_thr && (key >> 8) == hp) atomicAdd(&mass[key & 255u], (unsigned long long)(expf(z - zmax) * MASS_ONE));
    }
    __syncthreads();
    select_from_bottom(mass, rest, sel_m);
    z_thr = fmaxf(z_thr, __fdiv_rn(sample_key_value((hp << 8) | (unsigned)sel_m[0]), temperature));
  }

  // ---- the kept tokens (z >= z_thr): their sum of exp(z - zmax) and the Gumbel-max draw
  const unsigned long long s = streams ? (unsigned long long)streams[b] : (unsigned long long)b;
  const unsigned long long base = splitmix64_key(splitmix64_key(P.seed ^ SAMPLE_STREAM, s), (unsigned long long)(long long)t);
  double sum = 0.0;
  float bs = ninf;
  int bidx = INT_MAX;
  for (int v = tid; v < V; v += SMP_THREADS) {
    const float z = scaled(row[v], temperature);
    if (z >= z_thr) {
      sum += (double)expf(z - zmax);
      if (!greedy) {
        const unsigned long long r = splitmix64_key(base, (unsigned long long)v);
        const float u01 = ((float)(unsigned)(r >> 41) + 0.5f) * 1.1920928955078125e-07f;     // ((r >> 41) + 0.5) / 2^23: exact, inside (0, 1)
        const float sc = z - logf(-logf(u01));
        if (sc > bs) { bs = sc; bidx = v; }                    // ascending columns: the lowest id among equal sums
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (!greedy) block_argmax(bs, bidx, red_v, red_i);           // (the largest token is kept and its sum is finite: bidx is a column)
  if (lane == 0) red_d[w] = sum;
  __syncthreads();
  sum = 0.0;
  for (int k = 0; k < SMP_WAVES; ++k) sum += red_d[k];
  const int tok = greedy ? gi : min(max(bidx, 0), V - 1);
  if (tid == 0) {
    id[b] = tok;
    if (logprob_out && t >= 0 && t < T)
      logprob_out[(long long)b * T + t] = (float)(((double)scaled(row[tok], temperature) - (double)zmax) - log(sum));
  }
  if (prow)
    for (int v = tid; v < V; v += SMP_THREADS) {
      const float z = scaled(row[v], temperature);
      prow[v] = z >= z_thr ? (float)((double)expf(z - zmax) / sum) : 0.f;
    }
}

// The advance for every row, by one workgroup, behind the launch that chose the tokens.
__global__ void __launch_bounds__(ADV_THREADS)
sample_advance_kernel(const long long* __restrict__ id, int B, int D, long long* __restrict__ out_ids, int T, int* __restrict__ step,
                      int* __restrict__ pos, const int* __restrict__ pos_from, const bf16_t* __restrict__ embed, int vocab_e, int ld_embed,
                      bf16_t* __restrict__ x_next, int ld_next) {
  const int tid = threadIdx.x;
  const int t = decode_step_index(out_ids, pos_from, step);
  for (int b = 0; b < B; ++b) decode_advance_row(b, (int)id[b], t, tid, ADV_THREADS, out_ids, T, embed, vocab_e, ld_embed, x_next, ld_next, D);
  __syncthreads();                                             // every thread has read *step
  decode_advance_counters(B, t, tid, ADV_THREADS, step, pos, pos_from);
}

inline bool aligned_to(const void* p, unsigned n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" int vla_sample_tokens(void* stream, const void* logits, long long ld_logits, int B, int V, const void* params,
                                 const long long* streams, long long* id, float* logprob_out, float* probs_out, long long ld_probs,
                                 long long* out_ids, int T, int* step, int* pos, const int* pos_from, const void* embed, int vocab_e,
                                 int ld_embed, void* x_next, int ld_next, int D) {
  VLA_REQUIRE(logits && params && id && step, "sample_tokens: null pointer (logits, params, id and step are required)");
  VLA_REQUIRE(B > 0 && B <= SMP_MAX_B && V > 0, "sample_tokens: B in [1, 64], V >= 1");
  VLA_REQUIRE(ld_logits >= V && aligned_to(logits, 2), "sample_tokens: ld_logits below V, or logits not 2-B aligned");
  VLA_REQUIRE(aligned_to(params, 8), "sample_tokens: the parameter block must be 8-B aligned");
  VLA_REQUIRE(!logprob_out || T >= 1, "sample_tokens: logprob_out needs T >= 1");
  VLA_REQUIRE(!probs_out || ld_probs >= V, "sample_tokens: ld_probs below V");
  if (out_ids) {
    VLA_REQUIRE(T >= 1 && pos && embed && x_next, "sample_tokens: the advance needs T >= 1, pos, embed and x_next");
    VLA_REQUIRE(D > 0 && D % 8 == 0 && vocab_e >= 1 && ld_embed >= D && ld_next >= D && ld_embed % 8 == 0 && ld_next % 8 == 0 &&
                    aligned_to(embed, 16) && aligned_to(x_next, 16),
                "sample_tokens: D a multiple of 8; embed / x_next 16-B aligned, row strides multiples of 8 and at least D");
  }
  hipLaunchKernelGGL(sample_kernel, dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld_logits, V,
                     (const SampleParams*)params, streams, id, logprob_out, probs_out, ld_probs, T, (const int*)step, pos_from);
  VLA_CHECK_LAUNCH("sample_tokens");
  if (out_ids) {
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(ADV_THREADS), 0, (hipStream_t)stream, (const long long*)id, B, D, out_ids, T,
                       step, pos, pos_from, (const bf16_t*)embed, vocab_e, ld_embed, (bf16_t*)x_next, ld_next);
    VLA_CHECK_LAUNCH("sample_tokens (advance)");
  }
  return VLA_OK;
}
