// The ONE statement of the hand-over from a chosen token to the next cached step (include/vla_decode.h: "the advance"), for the greedy
// finish of decode.hip and the sampler of sample.hip:
//   out_ids[b, t] = id[b] (when 0 <= t < T);  x_next[b, :] = embed[min(id[b], vocab_e - 1), :];  pos[b] = (pos_from ? pos_from[b] : pos[b]) + 1;
//   *step = t + 1, with t = *step - or 0 behind the prefill (pos_from given), whatever *step holds.
// One workgroup performs it for every row: the three parts below are called by all of its threads, the counters last and behind a
// barrier that follows every thread's read of *step.
#pragma once
#include "common.h"

// The step index of this launch.  Every thread reads it before any thread writes *step.
__device__ __forceinline__ int decode_step_index(const void* out_ids, const int* pos_from, const int* step) {
  return (out_ids && !pos_from) ? *step : 0;
}

// Row b: the token into out_ids (one thread) and its embedding row into x_next (16-B words strided over the workgroup).
__device__ __forceinline__ void decode_advance_row(int b, int id, int t, int tid, int nthreads, long long* __restrict__ out_ids, int T,
                                                   const bf16_t* __restrict__ embed, int vocab_e, int ld_embed, bf16_t* __restrict__ x_next,
                                                   int ld_next, int D) {
  if (tid == 0 && t >= 0 && t < T) out_ids[(long long)b * T + t] = id;
  const uint4* src = reinterpret_cast<const uint4*>(embed + (long long)min(id, vocab_e - 1) * ld_embed);
  uint4* dst = reinterpret_cast<uint4*>(x_next + (long long)b * ld_next);
  for (int c = tid; c < D / 8; c += nthreads) dst[c] = src[c];
}

// The counters the next step reads.
__device__ __forceinline__ void decode_advance_counters(int B, int t, int tid, int nthreads, int* __restrict__ step, int* __restrict__ pos,
                                                        const int* __restrict__ pos_from) {
  for (int b = tid; b < B; b += nthreads) pos[b] = (pos_from ? pos_from[b] : pos[b]) + 1;
  if (tid == 0) *step = t + 1;
}
