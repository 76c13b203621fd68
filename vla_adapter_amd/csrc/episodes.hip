// Training from device-resident episodes: which transitions form the batch of a step, and the raw batch itself - the part of the
// reference's RLDS stage that cuts every episode into windows of one observation plus NUM_ACTIONS_CHUNK - 1 future actions
// (prismatic/vla/datasets/rlds/traj_transforms.py:14-57, configured in prismatic/vla/datasets/datasets.py:183-189) and shuffles the
// windows.  Declared in include/vla_episodes.h.
//   vla_episode_sample   (seed, rank, world, step) -> the B windows of this rank's batch: episode, first row, prompt offsets
//   vla_episode_gather   those windows -> frames_u8 / actions_raw / proprio_raw / prompt_flat, the dict GPUInputStage.collate consumes
// Both launch on the caller's stream, allocate nothing and read nothing back: a captured graph may hold them.  Every output element is
// written by exactly one thread (plain stores, no atomics).  The sampling rule is restated in Python (vla_adapter_amd/episodes.py:
// sample_position, permute_index, locate), which is what the kernel is tested against, bit for bit.
#include "common.h"
#include "permute.h"                            // feistel4 / permute_index: shared with mixture.hip
#include "windows.h"                            // EPISODE_STREAM, clampll, last_not_above, emit_windows: shared with mixture.hip, heldout.hip
#include "episode_row.h"                        // episode_row: the row a sample reads, shared with jpeg.hip
#include "../../include/vla_episodes.h"

namespace {

constexpr int SAMPLE_MAX_B = 1024;
constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;                   // independent loads a thread has in flight
constexpr int GATHER_MAX_BLOCKS = 2048;            // memory-bound grid: 256 CUs x 8 workgroups, the rest is strided

// One workgroup; thread b < B draws sample b, then all threads scan the prompt lengths (Hillis-Steele in LDS).
__global__ void __launch_bounds__(SAMPLE_MAX_B)
episode_sample_kernel(const long long* __restrict__ valid_off, const long long* __restrict__ episode_off,
                      const int* __restrict__ prompt_off, int E, u64 seed, u64 rank, u64 world, u64 step, int B, int Pmax,
                      int* __restrict__ ep, long long* __restrict__ row, int* __restrict__ out_off) {
  __shared__ int scan[SAMPLE_MAX_B];
  const int b = threadIdx.x;
  int e = 0;
  long long t = 0;
  if (b < B) {
    const long long n_tab = valid_off[E];
    if (n_tab >= 1) {
      const u64 n = (u64)n_tab;
      const u64 pos = (step * world + rank) * (u64)B + (u64)b;
      const u64 epoch = pos / n, i = pos % n;
      const long long j = (long long)permute_index(i, n, splitmix64_key(seed ^ EPISODE_STREAM, epoch));
      e = last_not_above(valid_off, 0, E - 1, j);
      t = j - valid_off[e];
    }
  }
  emit_windows(b, B, e, t, episode_off, prompt_off, Pmax, scan, ep, row, out_off);
}

// grid (nbx + 1, B): workgroups x < nbx of sample b move its frame row in units of V (uint4: 16 B, unsigned char: 1 B), workgroup
// x == nbx writes the sample's actions, proprio and prompt (and, for the last sample, the zero tail of the prompt buffer).
template <class V>
__global__ void __launch_bounds__(GATHER_THREADS)
episode_gather_kernel(const V* __restrict__ frames, const float* __restrict__ actions, const float* __restrict__ proprio,
                      const long long* __restrict__ episode_off, const long long* __restrict__ prompt_flat,
                      const int* __restrict__ prompt_off, const int* __restrict__ ep, const long long* __restrict__ row,
                      const int* __restrict__ out_off, V* __restrict__ out_frames, float* __restrict__ out_actions,
                      float* __restrict__ out_proprio, long long* __restrict__ out_prompt, int B, int E, long long T, long long units,
                      int chunk, int A, int Pd, long long n_flat, int Pmax, int nbx) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const EpisodeRow w = episode_row(episode_off, ep, row, b, E, T);
  const int e = w.e;
  const long long e1 = w.e1, r = w.r;
  if ((int)blockIdx.x < nbx) {
    const V* __restrict__ src = frames + r * units;
    V* __restrict__ dst = out_frames + (long long)b * units;
    const long long stride = (long long)nbx * GATHER_THREADS;
    long long i = (long long)blockIdx.x * GATHER_THREADS + tid;
    for (; i + (GATHER_UNROLL - 1) * stride < units; i += GATHER_UNROLL * stride) {
      V v[GATHER_UNROLL];
#pragma unroll
      for (int u = 0; u < GATHER_UNROLL; ++u) v[u] = src[i + u * stride];
#pragma unroll
      for (int u = 0; u < GATHER_UNROLL; ++u) dst[i + u * stride] = v[u];
    }
    for (; i < units; i += stride) dst[i] = src[i];
    return;
  }
  const int n_act = chunk * A;
  for (int idx = tid; idx < n_act; idx += GATHER_THREADS) {
    const int k = idx / A, a = idx - k * A;
    const long long rk = min(r + k, e1 - 1);         // traj_transforms.py:41-43: minimum(index, goal_timestep)
    out_actions[(long long)b * n_act + idx] = actions[rk * A + a];
  }
  for (int d = tid; d < Pd; d += GATHER_THREADS) out_proprio[(long long)b * Pd + d] = proprio[r * Pd + d];
  const long long cap = (long long)B * Pmax;
  const long long o0 = clampll((long long)prompt_off[e], 0ll, n_flat), o1 = clampll((long long)prompt_off[e + 1], o0, n_flat);
  const long long d0 = clampll((long long)out_off[b], 0ll, cap), d1 = clampll((long long)out_off[b + 1], d0, cap);
  const long long len = o1 - o0;
  for (long long j = tid; j < d1 - d0; j += GATHER_THREADS) out_prompt[d0 + j] = j < len ? prompt_flat[o0 + j] : 0ll;
  if (b == B - 1)
    for (long long j = d1 + tid; j < cap; j += GATHER_THREADS) out_prompt[j] = 0ll;
}

}  // namespace

extern "C" int vla_episode_sample(void* stream, const long long* valid_off, const long long* episode_off, const int* prompt_off, int E,
                                  unsigned long long seed, long long rank, long long world, long long step, int B, int Pmax, int* ep,
                                  long long* row, int* out_off) {
  VLA_REQUIRE(valid_off && episode_off && prompt_off && ep && row && out_off, "episode_sample: null pointer");
  VLA_REQUIRE(E >= 1 && B >= 1 && B <= SAMPLE_MAX_B && Pmax >= 0, "episode_sample: E >= 1, 1 <= B <= 1024 (one workgroup), Pmax >= 0");
  VLA_REQUIRE(world >= 1 && rank >= 0 && rank < world && step >= 0, "episode_sample: 0 <= rank < world, step >= 0");
  // (step * world + rank) * B + (B - 1), the position of the batch's last sample, stays below 2^63: the kernel forms it in u64
  const long long most = (0x7fffffffffffffffll - (B - 1)) / B;
  VLA_REQUIRE(rank <= most && step <= (most - rank) / world, "episode_sample: the stream position overflows 63 bits");
  VLA_REQUIRE((long long)B * Pmax <= 0x7fffffffll, "episode_sample: B * Pmax must fit int32 offsets");
  const int threads = (B + 63) / 64 * 64;
  hipLaunchKernelGGL(episode_sample_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, valid_off, episode_off, prompt_off, E, (u64)seed,
                     (u64)rank, (u64)world, (u64)step, B, Pmax, ep, row, out_off);
  VLA_CHECK_LAUNCH("episode_sample");
  return VLA_OK;
}

extern "C" int vla_episode_gather(void* stream, const unsigned char* frames, const float* actions, const float* proprio,
                                  const long long* episode_off, const long long* prompt_flat, const int* prompt_off, const int* ep,
                                  const long long* row, const int* out_off, unsigned char* out_frames, float* out_actions,
                                  float* out_proprio, long long* out_prompt, int B, int E, long long T, long long row_bytes, int chunk,
                                  int A, int Pd, long long n_flat, int Pmax) {
  VLA_REQUIRE(actions && proprio && episode_off && prompt_off && ep && row && out_off, "episode_gather: null input pointer");
  VLA_REQUIRE(out_actions && out_proprio, "episode_gather: null output pointer");
  VLA_REQUIRE(B >= 1 && B <= 65535 && E >= 1 && T >= 1 && row_bytes >= 0, "episode_gather: 1 <= B <= 65535, E, T >= 1, row_bytes >= 0");
  // row_bytes == 0: a store whose frames are not raw pixels (JPEG: vla_jpeg_decode_rows fills the frames) - no frame workgroup runs
  VLA_REQUIRE((frames && out_frames) || row_bytes == 0, "episode_gather: null frames / out_frames with row_bytes > 0");
  VLA_REQUIRE(chunk >= 1 && A >= 1 && Pd >= 1 && n_flat >= 0 && Pmax >= 0, "episode_gather: chunk, A, Pd >= 1, n_flat, Pmax >= 0");
  VLA_REQUIRE((long long)chunk * A <= 0x7fffffffll && (long long)B * Pmax <= 0x7fffffffll, "episode_gather: chunk * A and B * Pmax must fit int32");
  VLA_REQUIRE(out_prompt || Pmax == 0, "episode_gather: null out_prompt with Pmax > 0");
  VLA_REQUIRE(prompt_flat || n_flat == 0, "episode_gather: null prompt_flat with n_flat > 0");
  const bool wide = row_bytes % 16 == 0 && ((uintptr_t)frames | (uintptr_t)out_frames) % 16 == 0;
  const long long units = wide ? row_bytes / 16 : row_bytes;
  const long long want = (units + (long long)GATHER_THREADS * GATHER_UNROLL - 1) / ((long long)GATHER_THREADS * GATHER_UNROLL);
  const long long most = GATHER_MAX_BLOCKS / B > 1 ? GATHER_MAX_BLOCKS / B : 1;
  const int nbx = (int)(want < most ? want : most);
  const dim3 grid((unsigned)(nbx + 1), (unsigned)B);
  if (wide)
    hipLaunchKernelGGL(episode_gather_kernel<uint4>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, (const uint4*)frames, actions, proprio,
                       episode_off, prompt_flat, prompt_off, ep, row, out_off, (uint4*)out_frames, out_actions, out_proprio, out_prompt, B, E, T,
                       units, chunk, A, Pd, n_flat, Pmax, nbx);
  else
    hipLaunchKernelGGL(episode_gather_kernel<unsigned char>, grid, dim3(GATHER_THREADS), 0, (hipStream_t)stream, frames, actions, proprio,
                       episode_off, prompt_flat, prompt_off, ep, row, out_off, out_frames, out_actions, out_proprio, out_prompt, B, E, T, units,
                       chunk, A, Pd, n_flat, Pmax, nbx);
  VLA_CHECK_LAUNCH("episode_gather");
  return VLA_OK;
}
