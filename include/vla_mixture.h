/* C ABI of the dataset mixture of libvla_native.so (several device-resident datasets -> one raw batch per step, every sample
 * normalised with its own dataset's statistics): a fourth header beside vla_native.h, vla_serve.h and vla_episodes.h.
 *
 * As with vla_episodes.h: the three earlier headers, their signature tables in the Python binding and VLA_ABI_VERSION are pinned by
 * tests; these calls were added later, change no descriptor and no existing signature, and are looked up by name.  They live in the
 * same library and follow the same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a
 * hipStream_t; every pointer is a device pointer; nothing is allocated, read back or synchronised, so a captured graph may hold every
 * call - and are compiled from csrc/mixture.hip.  No atomics: every output element is written exactly once by one thread.
 *
 * The store (vla_adapter_amd/mixture.py): D datasets whose episodes lie back to back in ONE set of the tables of vla_episodes.h
 * (episode_off, valid_off, prompt_off over all E episodes), plus
 *   dataset_off int32 [D + 1]  episode index range of each dataset (0 ... E);  N_d = valid_off[dataset_off[d + 1]] - valid_off[dataset_off[d]]
 *   quota_off   int64 [D + 1]  prefix sum of the datasets' quotas q_d of one period of Q = quota_off[D] draws
 */
#ifndef VLA_MIXTURE_H
#define VLA_MIXTURE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Which windows of which datasets form the batch of (rank, step): one workgroup, 1 <= B <= 1024.  Sample b, in 64-bit arithmetic:
 *   position = (step * world + rank) * B + b,  k = position / Q,  s = position % Q,
 *   s2 = permute_index(s, Q, key(seed ^ MIX_STREAM, k))      the slot's place in period k's shuffled order
 *   d  = the largest d in [0, D) with quota_off[d] <= s2     (binary search)
 *   c  = k * q_d + (s2 - quota_off[d])                       the ordinal of this draw in dataset d's own endless stream
 *   ep_d = c / N_d,  i = c % N_d,
 *   j  = valid_off[dataset_off[d]] + permute_index(i, N_d, key(epoch_key(seed, ep_d), d + 1))
 *   e  = the episode of dataset d with valid_off[e] <= j < valid_off[e + 1] (binary search),  t = j - valid_off[e]
 * with permute_index / epoch_key of vla_adapter_amd/episodes.py and key = splitmix64_key, bit for bit (mixture.sample_windows).
 *   ds      int32 [B]      = d
 *   ep      int32 [B]      = e, a global episode index
 *   row     int64 [B]      = episode_off[e] + t, kept inside episode e
 *   out_off int32 [B + 1]  = exclusive scan of the chosen episodes' prompt lengths, each clamped into [0, Pmax]
 * ep / row / out_off are what vla_episode_gather takes.  Every period gives dataset d exactly q_d draws, with ordinals
 * [k q_d, (k + 1) q_d): each dataset runs through its own endless epochs, every window once per N_d ordinals, whatever B and world
 * are.  Q and N_d are read from the tables on the device.  A bad table does not make the kernel read outside: both searches end
 * inside their table (dataset_off is clamped into [0, E]); N_d < 1 yields window 0 of the dataset's first episode; Q < 1 yields
 * dataset 0 with c = position.  0 <= rank < world, step >= 0, and the position of the batch's last sample,
 * (step world + rank) B + B - 1, below 2^63 (refused otherwise: the kernel forms it in 64 bits). */
int vla_mixture_sample(void* stream, const long long* valid_off, const long long* episode_off, const int* prompt_off,
                       const int* dataset_off, const long long* quota_off, int E, int D, unsigned long long seed, long long rank,
                       long long world, long long step, int B, int Pmax, int* ds, int* ep, long long* row, int* out_off);

/* vla_normalize_bounds with one statistics set per row: x f32 [R, row_len] -> y, row_len % Dim == 0; element (r, i) uses column
 * i % Dim of set min(max(sel[r], 0), n_sets - 1) of low / high f32 [n_sets, Dim], mask / zero u8 [n_sets, Dim] (NULL: all ones / all
 * zeros).  The arithmetic is normalize_bounds_kernel's, operation for operation (no contraction): a row is bit-identical to
 * vla_normalize_bounds on that row with that set. */
int vla_normalize_bounds_rows(void* stream, const float* x, float* y, long long R, int row_len, int Dim, const int* sel, int n_sets,
                              const float* low, const float* high, const unsigned char* mask, const unsigned char* zero_mask);

#ifdef __cplusplus
}
#endif
#endif
