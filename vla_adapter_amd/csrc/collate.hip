// The batch producer's integer bookkeeping on the device (third part): raw transitions -> the collated token tensors.
//   vla_normalize_bounds   normalize_action_and_proprio, BOUNDS / BOUNDS_Q99 (prismatic/vla/datasets/rlds/utils/data_utils.py:67-90)
//   vla_collate_tokens     RLDSBatchTransform.__call__, use_minivlm branch (prismatic/vla/datasets/datasets.py:76-89, 124) and
//                          PaddedCollatorForActionPrediction's right padding / attention mask (prismatic/util/data_utils.py:114-134)
// Both launch on the caller's stream, allocate nothing and read nothing back: a captured graph may hold them.
#include "common.h"
#include "../../include/vla_native.h"

// Every product, quotient and difference of the normalisation rounds on its own, as TF's float32 ops do.
#pragma clang fp contract(off)

namespace {

constexpr int COLLATE_THREADS = 256;
constexpr int COLLATE_MAX_TOKENS = 256;            // action-block slots held in LDS (the reference's NUM_TOKENS is 64)
constexpr unsigned long long COLLATE_STREAM = 0xC011A7E5EEDull;      // keeps these draws apart from the augmentation's under equal seed words

// x [n / D, D] f32 -> y, per element of column d (f32 throughout, TF's op order):
//   data_utils.py:79-83  y = mask[d] ? clip_by_value(2 * (x - low[d]) / (high[d] - low[d] + 1e-8) - 1, -1, 1) : x
//                        (low / high: min / max for BOUNDS, q01 / q99 for BOUNDS_Q99, :69-74; mask defaults to all ones, :75)
//   data_utils.py:87-89  y = zero[d] ? 0 : y      (zero = the stats' min == max, for both types)
__global__ void normalize_bounds_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, int D,
                                        const float* __restrict__ low, const float* __restrict__ high,
                                        const unsigned char* __restrict__ mask, const unsigned char* __restrict__ zero) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    const float v = x[i];
    float r = v;
    if (!mask || mask[d]) {
      const float num = 2.0f * (v - low[d]);
      const float den = (high[d] - low[d]) + 1e-8f;
      const float t = num / den - 1.0f;
      r = fminf(fmaxf(t, -1.0f), 1.0f);              // tf.clip_by_value: minimum(maximum(t, lo), hi)
    }
    if (zero && zero[d]) r = 0.0f;
    y[i] = r;
  }
}

// One workgroup per sample.  Row b = kept prompt ids | action block of num_tokens ids | pad, cut at L:
//   datasets.py:76-79   the prompt loses its last three ids when it has at least three
//   datasets.py:81-87   the block = the first min(n_act, num_tokens) binned action ids; n_act < num_tokens: every further slot is a
//                       uniform draw from the sample's own n_act ids (random.choices; here flat[r % n_act], r from the counter-based
//                       generator keyed by (seed, rank, step, sample, slot) - the reference's stream is not reproduced)
//   datasets.py:88,124  labels = ids with every position below row_len - (num_tokens + 1) set to ignore_index (row_len: the
//                       untruncated length)
//   data_utils.py:114-134  right padding: ids pad_id, labels ignore_index, attention_mask = ids != pad_id
// Offsets are clamped into [0, n_flat]: a bad offset table cannot make the kernel read outside prompt_flat.
__global__ void __launch_bounds__(COLLATE_THREADS)
collate_tokens_kernel(const long long* __restrict__ prompt_flat, const int* __restrict__ prompt_off, long long n_flat,
                      const float* __restrict__ actions, const double* __restrict__ bins, long long* __restrict__ ids,
                      long long* __restrict__ labels, unsigned char* __restrict__ attn, int n_act, int L, int nbins, float lo, float hi,
                      long long tokenizer_len, long long pad_id, long long ignore_index, int num_tokens, unsigned long long seed,
                      long long rank, long long step) {
  __shared__ long long tok[COLLATE_MAX_TOKENS];
  const int b = blockIdx.x;
  const int n_bin = min(n_act, num_tokens);
  for (int k = threadIdx.x; k < n_bin; k += COLLATE_THREADS)
    tok[k] = action_token_id(actions[(long long)b * n_act + k], bins, nbins, lo, hi, tokenizer_len);
  __syncthreads();
  if (n_bin < num_tokens) {                             // only when n_act < num_tokens: every draw indexes a binned id
    const unsigned long long key = splitmix64_key(
        splitmix64_key(splitmix64_key(seed ^ COLLATE_STREAM, (unsigned long long)rank), (unsigned long long)step), (unsigned long long)b);
    for (int k = n_bin + threadIdx.x; k < num_tokens; k += COLLATE_THREADS)
      tok[k] = tok[(unsigned)(splitmix64_key(key, (unsigned long long)k) >> 32) % (unsigned)n_act];
    __syncthreads();
  }
  const long long o0 = min(max((long long)prompt_off[b], 0ll), n_flat);
  const long long o1 = min(max((long long)prompt_off[b + 1], o0), n_flat);
  const long long len = o1 - o0;
  const long long p = len >= 3 ? len - 3 : len;
  const long long row_len = p + num_tokens, first_label = row_len - (num_tokens + 1);
  for (int j = threadIdx.x; j < L; j += COLLATE_THREADS) {
    const long long id = j < p ? prompt_flat[o0 + j] : j < row_len ? tok[j - p] : pad_id;
    const long long o = (long long)b * L + j;
    ids[o] = id;
    labels[o] = (j < first_label || j >= row_len) ? ignore_index : id;
    attn[o] = id != pad_id;
  }
}

}  // namespace

extern "C" int vla_normalize_bounds(void* stream, const float* x, float* y, long long n, int D, const float* low, const float* high,
                                    const unsigned char* mask, const unsigned char* zero_mask) {
  VLA_REQUIRE(x && y && low && high && n > 0 && D > 0 && n % D == 0, "normalize_bounds: null / empty / n is not a multiple of D");
  const long long blocks = (n + COLLATE_THREADS - 1) / COLLATE_THREADS;
  hipLaunchKernelGGL(normalize_bounds_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(COLLATE_THREADS), 0, (hipStream_t)stream,
                     x, y, n, D, low, high, mask, zero_mask);
  VLA_CHECK_LAUNCH("normalize_bounds");
  return VLA_OK;
}

extern "C" int vla_collate_tokens(void* stream, const long long* prompt_flat, const int* prompt_off, long long n_flat,
                                  const float* actions, const double* bins, long long* ids, long long* labels,
                                  unsigned char* attention_mask, int B, int n_act, int L, int nbins, float lo, float hi,
                                  long long tokenizer_len, long long pad_id, long long ignore_index, int num_tokens,
                                  unsigned long long seed, long long rank, long long step) {
  VLA_REQUIRE(prompt_off && actions && bins && ids && labels && attention_mask, "collate_tokens: null pointer");
  VLA_REQUIRE(prompt_flat || n_flat == 0, "collate_tokens: null prompt_flat with n_flat > 0");
  VLA_REQUIRE(B > 0 && n_act > 0 && L > 0 && n_flat >= 0 && nbins > 1 && lo < hi, "collate_tokens: B, n_act, L > 0, n_flat >= 0, nbins > 1, lo < hi");
  VLA_REQUIRE(num_tokens > 0 && num_tokens <= COLLATE_MAX_TOKENS, "collate_tokens: num_tokens in [1, 256]");
  hipLaunchKernelGGL(collate_tokens_kernel, dim3(B), dim3(COLLATE_THREADS), 0, (hipStream_t)stream, prompt_flat, prompt_off, n_flat, actions,
                     bins, ids, labels, attention_mask, n_act, L, nbins, lo, hi, tokenizer_len, pad_id, ignore_index, num_tokens, seed, rank, step);
  VLA_CHECK_LAUNCH("collate_tokens");
  return VLA_OK;
}
