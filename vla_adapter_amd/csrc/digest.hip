// State digest: a position-weighted 64-bit digest of a contiguous view of 16-bit words (a flat parameter / moment buffer), left in
// device memory.  Declared in include/vla_digest.h, which states the rule; tests/digest_rule_np.py restates it in numpy and is what
// the kernel is tested against, bit for bit.
//   pass 1  every thread walks units of the view at the grid's stride - 16-byte groups (two chunks, one 16-byte load) where the view
//           starts on a 16-byte boundary, single chunks (four 2-byte loads, bounds-checked: the tail, or the whole of a view that
//           starts anywhere else) - and sums (q_c + 1) * w_c modulo 2^64; a workgroup's sum goes to scratch[blockIdx.x]
//   pass 2  one workgroup adds the partial sums and the length term into out
// A view one workgroup covers takes pass 1 alone, which then writes out.  Plain C++, no atomics; a wrapping sum does not depend on
// the order of its terms, so neither the grid nor the reduction tree shows in the result.  Both launch on the caller's stream,
// allocate nothing and read nothing back: a captured graph may hold them.
#include "common.h"
#include "../../include/vla_digest.h"

namespace {

typedef unsigned long long u64;
constexpr int DG_THREADS = 256;
constexpr int DG_MAX_BLOCKS = 1024;
constexpr u64 DG_GOLDEN = 0x9E3779B97F4A7C15ull, DG_LENGTH = 0xD1B54A32D192ED03ull;

// (q + 1) * (mix(c + key) | 1): the splitmix64 finaliser of the chunk index under the salt's key, made odd
__device__ __forceinline__ u64 term(u64 q, u64 c, u64 key) {
  u64 z = c + key;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (q + 1ull) * (z | 1ull);
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}

// The workgroup's wrapping sum, valid in thread 0 (every thread of the workgroup calls it).
__device__ __forceinline__ u64 block_sum(u64 v, u64* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 s = 0;
  if (threadIdx.x == 0)
#pragma unroll
    for (int w = 0; w < DG_THREADS / 64; ++w) s += sm[w];
  return s;
}

// groups: the 16-byte groups read with vector loads (0 when x is not 16-byte aligned); the chunks 2 * groups .. chunks - 1 are read
// word by word, every word index checked against n.  dst[blockIdx.x] = the workgroup's sum + add (add: the length term when this is
// the only pass, else 0).
__global__ void __launch_bounds__(DG_THREADS)
digest_partial_kernel(const unsigned short* __restrict__ x, long long n, long long groups, u64 key, u64 add, u64* __restrict__ dst) {
  __shared__ u64 sm[DG_THREADS / 64];
  const long long tid = (long long)blockIdx.x * DG_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * DG_THREADS;
  const long long chunks = (n + 3) >> 2;
  const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x);
  u64 s = 0;
  for (long long g = tid; g < groups; g += nthreads) {
    const uint4 u = xv[g];
    s += term((u64)u.x | ((u64)u.y << 32), (u64)(2 * g), key) + term((u64)u.z | ((u64)u.w << 32), (u64)(2 * g + 1), key);
  }
  for (long long c = 2 * groups + tid; c < chunks; c += nthreads) {
    u64 q = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long w = 4 * c + k;
      if (w < n) q |= (u64)x[w] << (16 * k);
    }
    s += term(q, (u64)c, key);
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) dst[blockIdx.x] = s + add;
}

__global__ void __launch_bounds__(DG_THREADS)
digest_final_kernel(const u64* __restrict__ partial, int count, u64 add, u64* __restrict__ out) {
  __shared__ u64 sm[DG_THREADS / 64];
  u64 s = 0;
  for (int i = threadIdx.x; i < count; i += DG_THREADS) s += partial[i];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) out[0] = s + add;
}

}  // namespace

extern "C" int vla_state_digest_slots(void) { return DG_MAX_BLOCKS; }

extern "C" int vla_state_digest(void* stream, const void* x, long long n, unsigned long long salt, unsigned long long* scratch,
                                long long scratch_slots, unsigned long long* out) {
  VLA_REQUIRE(x && out, "state_digest: null pointer");
  VLA_REQUIRE(n >= 1, "state_digest: n >= 1 (an empty view has no digest)");
  VLA_REQUIRE(n <= 0x3fffffffffffffffll, "state_digest: n overflows the byte count");
  VLA_REQUIRE(((uintptr_t)x & 1) == 0, "state_digest: x must be 2-byte aligned");
  VLA_REQUIRE(((uintptr_t)out & 7) == 0 && ((uintptr_t)scratch & 7) == 0, "state_digest: out and scratch must be 8-byte aligned");
  VLA_REQUIRE(scratch_slots >= 0 && (scratch || scratch_slots == 0), "state_digest: null scratch with scratch_slots > 0");
  const long long groups = ((uintptr_t)x & 15) == 0 ? n / 8 : 0;
  const long long chunks = (n + 3) / 4;
  const long long units = groups + (chunks - 2 * groups);
  long long nb = (units + DG_THREADS - 1) / DG_THREADS;
  if (nb > DG_MAX_BLOCKS) nb = DG_MAX_BLOCKS;
  if (nb > scratch_slots) nb = scratch_slots;
  if (nb < 1) nb = 1;
  const u64 key = DG_GOLDEN * ((u64)salt + 1ull), length = (u64)n * DG_LENGTH;
  if (nb == 1) {
    hipLaunchKernelGGL(digest_partial_kernel, dim3(1), dim3(DG_THREADS), 0, (hipStream_t)stream, (const unsigned short*)x, n, groups, key,
                       length, (u64*)out);
    VLA_CHECK_LAUNCH("state_digest");
    return VLA_OK;
  }
  hipLaunchKernelGGL(digest_partial_kernel, dim3((unsigned)nb), dim3(DG_THREADS), 0, (hipStream_t)stream, (const unsigned short*)x, n, groups,
                     key, (u64)0, (u64*)scratch);
  VLA_CHECK_LAUNCH("state_digest (partial sums)");
  hipLaunchKernelGGL(digest_final_kernel, dim3(1), dim3(DG_THREADS), 0, (hipStream_t)stream, (const u64*)scratch, (int)nb, length, (u64*)out);
  VLA_CHECK_LAUNCH("state_digest (final sum)");
  return VLA_OK;
}
