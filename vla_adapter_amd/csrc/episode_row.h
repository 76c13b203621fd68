// Which row of the store a sample (ep[b], row[b]) of a batch reads: stated once for the two kernels that turn a picker's windows into
// frames - episode_gather_kernel (episodes.hip: raw frames) and the JPEG decode (jpeg.hip).  A bad index stays inside its episode.
#pragma once

namespace {

struct EpisodeRow {
  int e;                  // ep[b] clamped into [0, E)
  long long e0, e1;       // episode e's rows clamped into [0, T), e0 < e1
  long long r;            // row[b] clamped into [e0, e1)
};

__device__ __forceinline__ EpisodeRow episode_row(const long long* __restrict__ episode_off, const int* __restrict__ ep,
                                                  const long long* __restrict__ row, int b, int E, long long T) {
  EpisodeRow w;
  w.e = min(max(ep[b], 0), E - 1);
  w.e0 = min(max(episode_off[w.e], 0ll), T - 1);
  w.e1 = min(max(episode_off[w.e + 1], w.e0 + 1), T);
  w.r = min(max(row[b], w.e0), w.e1 - 1);
  return w;
}

}  // namespace
