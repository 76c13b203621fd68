// The keyed bijection on [0, n) the device-resident samplers shuffle with (episodes.hip, mixture.hip): permute_index of
// vla_adapter_amd/episodes.py, bit for bit.  Include after common.h (splitmix64_key).
#pragma once

namespace {

typedef unsigned long long u64;

// One pass of the 4-round balanced Feistel network over two halves of `half` bits (1 <= half <= 32): a bijection on [0, 4^half)
// whatever the round function is, since each round (L, R) -> (R, L ^ F(R)) is undone by (L, R) -> (R ^ F(L), L).
__device__ __forceinline__ u64 feistel4(u64 x, u64 key, int half) {
  const u64 mask = (1ull << half) - 1ull;
  u64 l = x >> half, r = x & mask;
#pragma unroll
  for (int round = 0; round < 4; ++round) {
    const u64 f = splitmix64_key(splitmix64_key(key, (u64)round), r) & mask;
    const u64 t = l ^ f;
    l = r;
    r = t;
  }
  return (l << half) | r;
}

// permute_index of episodes.py: i in [0, n) -> the keyed bijection's image in [0, n).  Results >= n are walked on along their cycle.
// Termination: i lies inside [0, n), the walk follows the cycle of a permutation of [0, 4^half) through i, so it comes back to i - an
// element of [0, n) - after at most 4^half steps and stops at the first element below n it meets; 4^half < 4 n.
__device__ __forceinline__ u64 permute_index(u64 i, u64 n, u64 key) {
  if (n <= 1ull) return 0ull;
  const int bits = 64 - __clzll((long long)(n - 1ull));
  const int half = (bits + 1) / 2;                 // >= 1 because n >= 2
  u64 y = i;
  do {
    y = feistel4(y, key, half);
  } while (y >= n);
  return y;
}

}  // namespace
