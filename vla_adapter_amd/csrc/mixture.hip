// Training on a weighted mixture of device-resident datasets: the part of the reference's make_interleaved_dataset
// (prismatic/vla/datasets/rlds/dataset.py:490-585) that decides which dataset the next frame comes from and normalises every frame
// with its own dataset's statistics.  Declared in include/vla_mixture.h.
//   vla_mixture_sample          (seed, rank, world, step) -> the B windows of this rank's batch: dataset, episode, first row, prompt offsets
//   vla_normalize_bounds_rows   vla_normalize_bounds with one statistics set per row
// Both launch on the caller's stream, allocate nothing and read nothing back: a captured graph may hold them.  Every output element is
// written by exactly one thread (plain stores, no atomics).  The sampling rule is restated in Python (vla_adapter_amd/mixture.py:
// sample_windows), which is what the kernel is tested against, bit for bit.
#include "common.h"
#include "permute.h"
#include "windows.h"
#include "../../include/vla_mixture.h"

// Every product, quotient and difference of the normalisation rounds on its own, as in collate.hip.
#pragma clang fp contract(off)

namespace {

constexpr int SAMPLE_MAX_B = 1024;
constexpr int NORMALIZE_THREADS = 256;
constexpr u64 MIX_STREAM = 0x313D0DA7A5E75ull;       // keeps the period shuffle apart from the window shuffle, the augmentation and the collator

// One workgroup; thread b < B draws sample b, then all threads scan the prompt lengths (emit_windows).
__global__ void __launch_bounds__(SAMPLE_MAX_B)
mixture_sample_kernel(const long long* __restrict__ valid_off, const long long* __restrict__ episode_off,
                      const int* __restrict__ prompt_off, const int* __restrict__ dataset_off, const long long* __restrict__ quota_off,
                      int E, int D, u64 seed, u64 rank, u64 world, u64 step, int B, int Pmax, int* __restrict__ ds,
                      int* __restrict__ ep, long long* __restrict__ row, int* __restrict__ out_off) {
  __shared__ int scan[SAMPLE_MAX_B];
  const int b = threadIdx.x;
  int e = 0;
  long long t = 0;
  if (b < B) {
    const long long q_tab = quota_off[D];
    const u64 pos = (step * world + rank) * (u64)B + (u64)b;
    int d = 0;
    u64 c = pos;                                     // Q < 1 (a bad table): dataset 0, its draws in position order
    if (q_tab >= 1) {
      const u64 q = (u64)q_tab;
      const u64 k = pos / q, s = pos % q;
      const long long s2 = (long long)permute_index(s, q, splitmix64_key(seed ^ MIX_STREAM, k));
      d = last_not_above(quota_off, 0, D - 1, s2);
      c = k * (u64)(quota_off[d + 1] - quota_off[d]) + (u64)(s2 - quota_off[d]);
    }
    const int e_lo = min(max(dataset_off[d], 0), E - 1);             // dataset d's episodes [e_lo, e_hi), kept inside [0, E)
    const int e_hi = min(max(dataset_off[d + 1], e_lo + 1), E);
    const long long v0 = valid_off[e_lo], n_tab = valid_off[e_hi] - v0;
    e = e_lo;
    if (n_tab >= 1) {
      const u64 n = (u64)n_tab;
      const u64 epoch = c / n, i = c % n;
      const u64 key = splitmix64_key(splitmix64_key(seed ^ EPISODE_STREAM, epoch), (u64)d + 1ull);
      const long long j = v0 + (long long)permute_index(i, n, key);
      e = last_not_above(valid_off, e_lo, e_hi - 1, j);
      t = j - valid_off[e];
    }
    ds[b] = d;
  }
  emit_windows(b, B, e, t, episode_off, prompt_off, Pmax, scan, ep, row, out_off);
}

// x [R, row_len] f32 -> y; element (r, i) with column d = i % D of set s = clamp(sel[r]): normalize_bounds_kernel of collate.hip
// (data_utils.py:79-89) with the statistics row chosen per sample, same operations in the same order.
__global__ void normalize_bounds_rows_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, int row_len, int D,
                                             const int* __restrict__ sel, int n_sets, const float* __restrict__ low,
                                             const float* __restrict__ high, const unsigned char* __restrict__ mask,
                                             const unsigned char* __restrict__ zero) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / row_len;
    const int d = (int)((i - r * row_len) % D);
    const long long s = (long long)min(max(sel[r], 0), n_sets - 1) * D + d;
    const float v = x[i];
    float o = v;
    if (!mask || mask[s]) {
      const float num = 2.0f * (v - low[s]);
      const float den = (high[s] - low[s]) + 1e-8f;
      const float t = num / den - 1.0f;
      o = fminf(fmaxf(t, -1.0f), 1.0f);              // tf.clip_by_value: minimum(maximum(t, lo), hi)
    }
    if (zero && zero[s]) o = 0.0f;
    y[i] = o;
  }
}

}  // namespace

extern "C" int vla_mixture_sample(void* stream, const long long* valid_off, const long long* episode_off, const int* prompt_off,
                                  const int* dataset_off, const long long* quota_off, int E, int D, unsigned long long seed,
                                  long long rank, long long world, long long step, int B, int Pmax, int* ds, int* ep, long long* row,
                                  int* out_off) {
  VLA_REQUIRE(valid_off && episode_off && prompt_off && dataset_off && quota_off && ds && ep && row && out_off, "mixture_sample: null pointer");
  VLA_REQUIRE(E >= 1 && D >= 1 && D <= E, "mixture_sample: E >= 1, 1 <= D <= E (every dataset holds an episode)");
  VLA_REQUIRE(B >= 1 && B <= SAMPLE_MAX_B && Pmax >= 0, "mixture_sample: 1 <= B <= 1024 (one workgroup), Pmax >= 0");
  VLA_REQUIRE(world >= 1 && rank >= 0 && rank < world && step >= 0, "mixture_sample: 0 <= rank < world, step >= 0");
  // (step * world + rank) * B + (B - 1), the position of the batch's last sample, stays below 2^63: the kernel forms it in u64
  const long long most = (0x7fffffffffffffffll - (B - 1)) / B;
  VLA_REQUIRE(rank <= most && step <= (most - rank) / world, "mixture_sample: the stream position overflows 63 bits");
  VLA_REQUIRE((long long)B * Pmax <= 0x7fffffffll, "mixture_sample: B * Pmax must fit int32 offsets");
  const int threads = (B + 63) / 64 * 64;
  hipLaunchKernelGGL(mixture_sample_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, valid_off, episode_off, prompt_off, dataset_off,
                     quota_off, E, D, (u64)seed, (u64)rank, (u64)world, (u64)step, B, Pmax, ds, ep, row, out_off);
  VLA_CHECK_LAUNCH("mixture_sample");
  return VLA_OK;
}

extern "C" int vla_normalize_bounds_rows(void* stream, const float* x, float* y, long long R, int row_len, int Dim, const int* sel,
                                         int n_sets, const float* low, const float* high, const unsigned char* mask,
                                         const unsigned char* zero_mask) {
  VLA_REQUIRE(x && y && sel && low && high, "normalize_bounds_rows: null pointer");
  VLA_REQUIRE(R > 0 && row_len > 0 && Dim > 0 && n_sets > 0 && row_len % Dim == 0,
              "normalize_bounds_rows: empty / row_len is not a multiple of Dim");
  VLA_REQUIRE((long long)n_sets * Dim <= 0x7fffffffll && R <= 0x7fffffffffffffffll / row_len, "normalize_bounds_rows: extents overflow");
  const long long n = R * row_len;
  const long long blocks = (n + NORMALIZE_THREADS - 1) / NORMALIZE_THREADS;
  hipLaunchKernelGGL(normalize_bounds_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(NORMALIZE_THREADS), 0,
                     (hipStream_t)stream, x, y, n, row_len, Dim, sel, n_sets, low, high, mask, zero_mask);
  VLA_CHECK_LAUNCH("normalize_bounds_rows");
  return VLA_OK;
}
