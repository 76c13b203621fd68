// The ONE order of an argmax over bf16 logits, for the token-accuracy metric (elementwise.hip: token_row_max<true>) and for the
// token the server emits (decode.hip): torch.argmax's rule on the CPU - the lowest index among equal values, a NaN greater than
// everything, the first NaN wins.  The order is total, so a reduction may combine pairs in any grouping.
#pragma once

// Does the pair (bv, bi) come before (av, ai) in that order?
__device__ __forceinline__ bool argmax_before(float bv, int bi, float av, int ai) {
  const bool an = av != av, bn = bv != bv;
  return an ? (bn && bi < ai) : (bn || bv > av || (bv == av && bi < ai));
}
// A thread meets its columns in ascending order: a strictly greater value (or the first NaN) replaces the pair.
__device__ __forceinline__ void argmax_take(float v, int i, float& bv, int& bi) {
  if (v > bv || (v != v && bv == bv)) { bv = v; bi = i; }
}
