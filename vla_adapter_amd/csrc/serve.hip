// Serving a batch of observations (predict_actions): everything between "B prompts of different lengths" and the batch dict the
// engine runs, and between the head's bf16 output and the un-normalised chunk.  Declared in include/vla_serve.h.
//   vla_serve_tokens             _prepare_input_for_action_prediction + _prepare_labels_for_action_prediction
//                                (prismatic/extern/hf/modeling_prismatic.py:747-782) for a ragged batch, right-padded
//   vla_normalize_proprio_serve  the evaluator's normalize_proprio (experiments/robot/openvla_utils.py:671-701)
//   vla_unnormalize_actions      _unnormalize_actions (modeling_prismatic.py:784-805)
//   vla_serve_gather_hidden      the returned action hidden states (modeling_prismatic.py:855, 927)
// All four launch on the caller's stream, allocate nothing and read nothing back: a captured graph may hold them.  Every output
// element is written by exactly one thread (plain stores, no atomics).
#include "common.h"
#include "../../include/vla_serve.h"

// numpy rounds every product, quotient, sum and difference on its own; hipcc would contract a * b + c into one fused operation.
#pragma clang fp contract(off)

namespace {

constexpr int SERVE_THREADS = 256;

// One workgroup per sample (see vla_serve.h for the row layout).
__global__ void __launch_bounds__(SERVE_THREADS)
serve_tokens_kernel(const long long* __restrict__ prompt_flat, const int* __restrict__ prompt_off, long long n_flat,
                    long long* __restrict__ ids, long long* __restrict__ labels, unsigned char* __restrict__ attn,
                    int* __restrict__ hid_row, unsigned char* __restrict__ row_ok, int L, int num_tokens, long long fill_id,
                    long long stop_id, long long action_label, long long pad_id, long long ignore_index) {
  const int b = blockIdx.x;
  const long long o0 = min(max((long long)prompt_off[b], 0ll), n_flat);
  const long long o1 = min(max((long long)prompt_off[b + 1], o0), n_flat);
  const long long len = o1 - o0;
  const bool ok = len >= 1 && len + num_tokens + 1 <= (long long)L;
  const long long P = ok ? len : 1;                    // not ok: the row of the one-id prompt [pad_id] (L >= num_tokens + 2: it fits)
  const long long stop_at = P + num_tokens, n = stop_at + 1;
  for (int j = threadIdx.x; j < L; j += SERVE_THREADS) {
    long long id, lab;
    if (j < P) {
      id = ok ? prompt_flat[o0 + j] : pad_id;
      lab = ignore_index;
    } else if (j < stop_at) {
      id = fill_id;
      lab = action_label;
    } else if (j == stop_at) {
      id = lab = stop_id;
    } else {
      id = pad_id;
      lab = ignore_index;
    }
    const long long o = (long long)b * L + j;
    ids[o] = id;
    labels[o] = lab;
    attn[o] = j < n;
  }
  if (threadIdx.x == 0) {
    hid_row[b] = (int)(P - 1);
    row_ok[b] = ok;
  }
}

// np.clip(v, -1, 1): NaN stays NaN (fmin / fmax would drop it)
__device__ __forceinline__ double clip1(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

template <class T>
__global__ void normalize_proprio_serve_kernel(const T* __restrict__ x, float* __restrict__ y, long long n, int D,
                                               const double* __restrict__ low, const double* __restrict__ high,
                                               const unsigned char* __restrict__ mask) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    double v = (double)x[i];
    if (!mask || mask[d]) {
      const double num = 2.0 * (v - low[d]);
      const double den = (high[d] - low[d]) + 1e-8;
      v = num / den - 1.0;
    }
    y[i] = (float)clip1(v);
  }
}

__global__ void unnormalize_actions_kernel(const bf16_t* __restrict__ pred, double* __restrict__ out, int B, int row, int Da,
                                           int ld_pred, int ld_out, const double* __restrict__ low, const double* __restrict__ high,
                                           const unsigned char* __restrict__ mask, const unsigned char* __restrict__ row_ok) {
  const long long n = (long long)B * row;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / row), c = (int)(i % row), d = c % Da;
    const float a = bf2f(pred[(long long)b * ld_pred + c]);
    double r = (double)a;
    if (!mask || mask[d]) {
      const float h = 0.5f * (a + 1.0f);               // f32: numpy keeps the float32 array's type against Python scalars
      const double span = (high[d] - low[d]) + 1e-8;
      r = (double)h * span + low[d];                   // (contraction is off: product and sum round separately)
    }
    if (row_ok && !row_ok[b]) r = __longlong_as_double(0x7ff8000000000000ll);
    out[(long long)b * ld_out + c] = r;
  }
}

// 16 B per thread and step: chunk q of sample b's T x D block
__global__ void serve_gather_hidden_kernel(const uint4* __restrict__ hs, const int* __restrict__ hid_row, uint4* __restrict__ out,
                                           int B, int S, int Np, int T, int D8, long long s_batch8, int ld8) {
  const long long per = (long long)T * D8, n = (long long)B * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const long long q = i % per;
    const int t = (int)(q / D8), c = (int)(q % D8);
    const int r0 = min(max(Np + hid_row[b], 0), S - T);
    out[i] = hs[(long long)b * s_batch8 + (long long)(r0 + t) * ld8 + c];
  }
}

inline unsigned grid_for(long long n) {
  const long long blocks = (n + SERVE_THREADS - 1) / SERVE_THREADS;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}

}  // namespace

extern "C" int vla_serve_tokens(void* stream, const long long* prompt_flat, const int* prompt_off, long long n_flat, long long* ids,
                                long long* labels, unsigned char* attention_mask, int* hid_row, unsigned char* row_ok, int B, int L,
                                int num_tokens, long long fill_id, long long stop_id, long long action_label, long long pad_id,
                                long long ignore_index) {
  VLA_REQUIRE(prompt_off && ids && labels && attention_mask && hid_row && row_ok, "serve_tokens: null pointer");
  VLA_REQUIRE(prompt_flat || n_flat == 0, "serve_tokens: null prompt_flat with n_flat > 0");
  VLA_REQUIRE(B > 0 && n_flat >= 0 && num_tokens >= 1, "serve_tokens: B > 0, n_flat >= 0, num_tokens >= 1");
  VLA_REQUIRE((long long)L >= (long long)num_tokens + 2, "serve_tokens: L >= num_tokens + 2 (the substitute row of a bad sample must fit)");
  hipLaunchKernelGGL(serve_tokens_kernel, dim3(B), dim3(SERVE_THREADS), 0, (hipStream_t)stream, prompt_flat, prompt_off, n_flat, ids,
                     labels, attention_mask, hid_row, row_ok, L, num_tokens, fill_id, stop_id, action_label, pad_id, ignore_index);
  VLA_CHECK_LAUNCH("serve_tokens");
  return VLA_OK;
}

extern "C" int vla_normalize_proprio_serve(void* stream, const void* x, int x_is_f64, float* y, long long n, int D, const double* low,
                                           const double* high, const unsigned char* mask) {
  VLA_REQUIRE(x && y && low && high && n > 0 && D > 0 && n % D == 0, "normalize_proprio_serve: null / empty / n is not a multiple of D");
  if (x_is_f64)
    hipLaunchKernelGGL(normalize_proprio_serve_kernel<double>, dim3(grid_for(n)), dim3(SERVE_THREADS), 0, (hipStream_t)stream,
                       (const double*)x, y, n, D, low, high, mask);
  else
    hipLaunchKernelGGL(normalize_proprio_serve_kernel<float>, dim3(grid_for(n)), dim3(SERVE_THREADS), 0, (hipStream_t)stream,
                       (const float*)x, y, n, D, low, high, mask);
  VLA_CHECK_LAUNCH("normalize_proprio_serve");
  return VLA_OK;
}

extern "C" int vla_unnormalize_actions(void* stream, const void* pred, double* out, int B, int row, int Da, int ld_pred, int ld_out,
                                       const double* low, const double* high, const unsigned char* mask, const unsigned char* row_ok) {
  VLA_REQUIRE(pred && out && low && high, "unnormalize_actions: null pointer");
  VLA_REQUIRE(B > 0 && row > 0 && Da > 0 && row % Da == 0, "unnormalize_actions: B, row, Da > 0 and row a multiple of Da");
  VLA_REQUIRE(ld_pred >= row && ld_out >= row, "unnormalize_actions: row strides below the row length");
  hipLaunchKernelGGL(unnormalize_actions_kernel, dim3(grid_for((long long)B * row)), dim3(SERVE_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)pred, out, B, row, Da, ld_pred, ld_out, low, high, mask, row_ok);
  VLA_CHECK_LAUNCH("unnormalize_actions");
  return VLA_OK;
}

extern "C" int vla_serve_gather_hidden(void* stream, const void* hs, const int* hid_row, void* out, int B, int S, int Np, int T, int D,
                                       long long s_batch, int ld) {
  VLA_REQUIRE(hs && hid_row && out, "serve_gather_hidden: null pointer");
  VLA_REQUIRE(B > 0 && T > 0 && S >= T && Np >= 0 && D > 0, "serve_gather_hidden: B, T, D > 0, S >= T, Np >= 0");
  VLA_REQUIRE(D % 8 == 0 && ld % 8 == 0 && s_batch % 8 == 0 && ld >= D && s_batch >= 0, "serve_gather_hidden: D, ld, s_batch multiples of 8, ld >= D");
  VLA_REQUIRE(((uintptr_t)hs | (uintptr_t)out) % 16 == 0, "serve_gather_hidden: hs / out must be 16-B aligned");
  hipLaunchKernelGGL(serve_gather_hidden_kernel, dim3(grid_for((long long)B * T * (D / 8))), dim3(SERVE_THREADS), 0, (hipStream_t)stream,
                     (const uint4*)hs, hid_row, (uint4*)out, B, S, Np, T, D / 8, s_batch / 8, ld / 8);
  VLA_CHECK_LAUNCH("serve_gather_hidden");
  return VLA_OK;
}
