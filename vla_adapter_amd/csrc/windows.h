// What the three window pickers of the episode data path share (episode_sample_kernel of episodes.hip, mixture_sample_kernel of
// mixture.hip, heldout_sweep_kernel of heldout.hip): each decides in its own way which (episode, step) sample b of the batch is, and
// all end in emit_windows, which turns that into the row, the clamped prompt length and the batch's prompt offsets.  Include after
// common.h.
#pragma once

namespace {

// Keys the window shuffle of a dataset's epochs (EPISODE_STREAM of vla_adapter_amd/episodes.py): apart from the augmentation's and
// the collator's draws under equal seed words; a mix keys its datasets' own epochs as a single store's are.
constexpr unsigned long long EPISODE_STREAM = 0xE9150DE5A391Eull;

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The largest i in [lo, hi] with tab[i] <= v (lo when there is none): ends inside [lo, hi] on any table.
template <class T>
__device__ __forceinline__ int last_not_above(const T* __restrict__ tab, int lo, int hi, long long v) {
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if ((long long)tab[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The pickers' common tail, called by EVERY thread of the one workgroup (the scan needs all of them).  Thread b < B holds window
// (episode e, step t inside it); e and t are ignored for b >= B.  It writes ep[b] = e, row[b] = the window's first row clamped into
// the episode, and - after a Hillis-Steele scan in `scan` (one int per thread of the workgroup) of the prompt lengths clamped to
// [0, Pmax] - out_off[b + 1]; thread 0 writes out_off[0] = 0.
__device__ __forceinline__ void emit_windows(int b, int B, int e, long long t, const long long* __restrict__ episode_off,
                                             const int* __restrict__ prompt_off, int Pmax, int* __restrict__ scan,
                                             int* __restrict__ ep, long long* __restrict__ row, int* __restrict__ out_off) {
  int len = 0;
  if (b < B) {
    const long long e0 = episode_off[e], e1 = episode_off[e + 1];
    ep[b] = e;
    row[b] = clampll(e0 + t, e0, e1 > e0 ? e1 - 1 : e0);
    len = (int)clampll((long long)prompt_off[e + 1] - (long long)prompt_off[e], 0ll, (long long)Pmax);
  }
  scan[b] = len;
  __syncthreads();
  for (int d = 1; d < (int)blockDim.x; d <<= 1) {
    const int v = b >= d ? scan[b - d] : 0;
    __syncthreads();
    scan[b] += v;
    __syncthreads();
  }
  if (b < B) out_off[b + 1] = scan[b];
  if (b == 0) out_off[0] = 0;
}

}  // namespace
