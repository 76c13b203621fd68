/* C ABI of the episode sampler of libvla_native.so (device-resident demonstrations -> one raw batch per step): a third header beside
 * vla_native.h and vla_serve.h.
 *
 * As with vla_serve.h: vla_native.h, its signature table in the Python binding and VLA_ABI_VERSION are pinned by the tests that guard
 * the training ABI; these calls were added later, change no descriptor and no existing signature, and are looked up by name.  They live
 * in the same library and follow the same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error();
 * `stream` is a hipStream_t; every pointer is a device pointer; nothing is allocated, read back or synchronised, so a captured graph
 * may hold every call - and are compiled from csrc/episodes.hip.  No atomics: every output element is written exactly once by one
 * thread.
 *
 * The store (vla_adapter_amd/episodes.py): T transitions of E episodes back to back;
 *   episode_off int64 [E + 1]  row offsets of the episodes (0 ... T)
 *   valid_off   int64 [E + 1]  prefix sum of max(len_e - (chunk - 1), 0): the windows an episode yields (chunk_act_obs drops its
 *                              last future_action_window_size steps as window starts); N = valid_off[E] windows in all
 *   prompt_off  int32 [E + 1]  offsets of the episodes' prompts in the store's prompt_flat
 */
#ifndef VLA_EPISODES_H
#define VLA_EPISODES_H

#ifdef __cplusplus
extern "C" {
#endif

/* Which windows form the batch of (rank, step): one workgroup, 1 <= B <= 1024.  Sample b, in 64-bit arithmetic:
 *   position = (step * world + rank) * B + b,  epoch = position / N,  i = position % N,
 *   j = permute_index(i, N, key(seed, epoch))   the keyed bijection on [0, N) of vla_adapter_amd/episodes.py (4-round balanced
 *                                               Feistel network over splitmix64_key, cycle-walked), bit for bit
 *   e = the episode with valid_off[e] <= j < valid_off[e + 1] (binary search),  t = j - valid_off[e]
 *   ep      int32 [B]      = e
 *   row     int64 [B]      = episode_off[e] + t, the global row of the window's first step, kept inside episode e
 *   out_off int32 [B + 1]  = exclusive scan of the chosen episodes' prompt lengths, each clamped into [0, Pmax]  (out_off[B] <= B * Pmax)
 * One epoch therefore visits every window exactly once across all ranks and steps; every rank passes the same seed.  N is read from
 * valid_off[E] on the device; with N < 1 (a bad table) every sample is window 0 of episode 0.  0 <= rank < world, step >= 0, and the position
 * of the batch's last sample, (step world + rank) B + B - 1, below 2^63 (refused otherwise: the kernel forms it in 64 bits). */
int vla_episode_sample(void* stream, const long long* valid_off, const long long* episode_off, const int* prompt_off, int E,
                       unsigned long long seed, long long rank, long long world, long long step, int B, int Pmax, int* ep,
                       long long* row, int* out_off);

/* The raw batch of the chosen windows, one launch.  Store: frames u8 [T, row_bytes] (row_bytes = n_img * H * W * 3), actions f32 [T, A],
 * proprio f32 [T, Pd], prompt_flat int64 [n_flat]; ep / row / out_off from vla_episode_sample.  With e = ep[b] clamped into [0, E),
 * [e0, e1) = episode e's rows clamped into [0, T) and r = row[b] clamped into [e0, e1):
 *   out_frames  u8    [B, row_bytes]   = frames[r]      16-byte chunks when row_bytes % 16 == 0 and frames / out_frames are 16-B aligned,
 *                                                       else byte by byte (decided on the host); a row is spread over several workgroups
 *   out_actions f32   [B, chunk, A]    = actions[min(r + k, e1 - 1)]     (chunk_act_obs' clamp to the goal step: it cannot bind for a
 *                                                       window start the sampler chose, and keeps a bad index inside its episode)
 *   out_proprio f32   [B, Pd]          = proprio[r]
 *   out_prompt  int64 [B * Pmax]       = the chosen prompts back to back at out_off[b], 0 behind out_off[B]
 * Prompt offsets of the store are clamped into [0, n_flat], those of the batch into [0, B * Pmax]; a destination range longer than its
 * prompt is zero-filled: no table makes the kernel read or write outside.  out_prompt may be NULL when Pmax == 0.  row_bytes == 0 (a
 * store that keeps its frames in another form, vla_jpeg.h): no frame is copied, frames and out_frames may be NULL. */
int vla_episode_gather(void* stream, const unsigned char* frames, const float* actions, const float* proprio,
                       const long long* episode_off, const long long* prompt_flat, const int* prompt_off, const int* ep,
                       const long long* row, const int* out_off, unsigned char* out_frames, float* out_actions, float* out_proprio,
                       long long* out_prompt, int B, int E, long long T, long long row_bytes, int chunk, int A, int Pd,
                       long long n_flat, int Pmax);

#ifdef __cplusplus
}
#endif
#endif
