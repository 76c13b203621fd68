/* C ABI of the held-out validation sweep of libvla_native.so (device-resident episodes -> validation batches in order, and the sweep's
 * L1 sums per dataset): a fifth header beside vla_native.h, vla_serve.h, vla_episodes.h and vla_mixture.h.
 *
 * As with vla_mixture.h: the four earlier headers, their signature tables in the Python binding and VLA_ABI_VERSION are pinned by
 * tests; these calls were added later, change no descriptor and no existing signature, and are looked up by name.  They live in the
 * same library and follow the same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a
 * hipStream_t; every pointer is a device pointer; nothing is allocated, read back or synchronised, so a captured graph may hold every
 * call - and are compiled from csrc/heldout.hip.  No atomics: every output element is written exactly once by one thread.
 *
 * The split (vla_adapter_amd/episodes.py, mixture.py: holdout=f): every dataset holds out its last H_d episodes.  Nothing is copied or
 * reordered; beside the tables of vla_episodes.h / vla_mixture.h the store keeps
 *   val_off     int64 [E + 1]  prefix sum of the windows the HELD-OUT episodes yield (a training episode contributes 0);  Nv = val_off[E]
 * and its training valid_off is the complementary prefix sum, so the training samplers never draw a held-out episode.
 */
#ifndef VLA_HELDOUT_H
#define VLA_HELDOUT_H

#ifdef __cplusplus
extern "C" {
#endif

/* Which held-out windows form validation batch batch_j of this rank: one workgroup, 1 <= B <= 1024.  Sample b, in 64-bit arithmetic:
 *   w = ((batch_j * world + rank) * B + b) * stride,   valid = w < Nv   (Nv is read from val_off[E] on the device)
 *   a valid sample:    e = the episode with val_off[e] <= w < val_off[e + 1] (binary search, episodes without a held-out window are
 *                      stepped over),  t = w - val_off[e]
 *   an invalid sample: window 0 of the held-out set (w = 0), so everything downstream runs on in-range data
 *   ds      int32 [B]      = the largest d in [0, D) with dataset_off[d] <= e (dataset_off int32 [D + 1]); 0 when dataset_off is NULL
 *   ep      int32 [B]      = e, a global episode index
 *   row     int64 [B]      = episode_off[e] + t, kept inside episode e
 *   out_off int32 [B + 1]  = exclusive scan of the chosen episodes' prompt lengths, each clamped into [0, Pmax]
 *   valid   u8    [B]      = 1 or 0
 * ep / row / out_off are what vla_episode_gather takes.  No shuffle: the windows w = 0, stride, 2 stride, ... below Nv are visited in
 * order, each exactly once over all ranks and batches.  A bad table does not make the kernel read outside: both searches end inside
 * their table; Nv < 1 makes every sample invalid.  0 <= rank < world, batch_j >= 0, stride >= 1; dataset_off may be NULL when D == 1. */
int vla_heldout_sweep(void* stream, const long long* val_off, const long long* episode_off, const int* prompt_off,
                      const int* dataset_off, int E, int D, long long rank, long long world, long long batch_j, long long stride,
                      int B, int Pmax, int* ds, int* ep, long long* row, int* out_off, unsigned char* valid);

/* The L1 errors of one validation batch, added to the sweep's sums.  pred / target bf16 [B, C, A]; ds int32 [B] or NULL (all rows
 * dataset 0); valid u8 [B]; acc f64 [D, C, A]; cnt int64 [D].  For every dataset d and cell (c, a):
 *   S = 0.0;  for b = 0 .. B - 1 in ascending order, where valid[b] != 0 and min(max(ds[b], 0), D - 1) == d:
 *       S += (double) fabsf((float) pred[b, c, a] - (float) target[b, c, a])        the difference in f32, the sum in f64
 *   acc[d, c, a] += S;   cnt[d] += the number of such rows
 * One partial sum per batch, then one add.  A row with valid == 0 is never read: a NaN there does not reach acc.  One thread per
 * cell (64 per workgroup, the grid runs over the cells) keeps the partial sum in a register; one further workgroup counts the rows. */
int vla_heldout_l1_accumulate(void* stream, const void* pred, const void* target, const int* ds, const unsigned char* valid, int B,
                              int C, int A, int D, double* acc, long long* cnt);

#ifdef __cplusplus
}
#endif
#endif
