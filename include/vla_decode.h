/* C ABI of greedy action-token decoding with a key/value cache (VLAEngine.generate): a header of its own beside vla_native.h.
 *
 * The token-CE objective trains the VLM to emit the action ids behind the prompt; the reference serves such a model with
 * OpenVLA.predict_action (prismatic/models/vlas/openvla.py:36-106): greedy `generate`, one token at a time.  These entry points are what
 * one cached single-token step needs beside the existing norms and GEMMs (run at M = B).  Conventions of every family: the caller
 * owns all memory, everything runs on `stream` (a hipStream_t), nothing is allocated, read back or synchronised - a captured graph may
 * hold every call - and the result is VLA_OK (0) or a negative code with the text in vla_last_error().  No atomics: every output
 * element is written once, every reduction runs in a fixed order.
 *
 * Positions live in device memory, `int pos[B]`: one captured step graph is replayed once per token and every row of a ragged batch
 * advances from its own length.  A position outside [0, S_cap) cannot make a kernel touch memory outside the cache: the append skips
 * such a row and the attention clamps the key count.
 *
 * The cache of one layer is k_cache / v_cache bf16 [B, S_cap, Hkv * dh] with sample stride cache_sb and row stride cache_ss
 * (elements; both multiples of 8, the pointers 16-B aligned).
 */
#ifndef VLA_DECODE_H
#define VLA_DECODE_H

#ifdef __cplusplus
extern "C" {
#endif

/* The prompt-only batch of a generation, right-padded to L, one launch: no placeholders and no stop id stand behind the prompt.
 *   prompt_flat int64 [n_flat], prompt_off int32 [B + 1]: as the serving family takes them (offsets clamped into [0, n_flat]).
 * Row b with P = its prompt length:
 *   ids            int64 [B, L] = prompt | pad_id up to L
 *   attention_mask u8    [B, L] = j < P
 *   pos            int32 [B]    = Np + P - 1: the row of the multimodal sequence [id 0 | Np patches | ids 1..] that holds the last
 *                                 prompt id - the row whose logits give the first token
 *   last_row       int32 [B]    = b * (Np + L) + pos[b]: the same row in the flattened [B * (Np + L), D] hidden states
 *   row_ok         u8    [B]    = (1 <= P <= L)
 * A row that is not ok is written as the row of the one-id prompt [pad_id].  Every element of the five outputs is written. */
int vla_decode_prompt(void* stream, const long long* prompt_flat, const int* prompt_off, long long n_flat, long long* ids,
                      unsigned char* attention_mask, int* pos, int* last_row, unsigned char* row_ok, int B, int L, int Np,
                      long long pad_id);

/* Rotary embedding of one new token per sample and its append to the cache.
 *   qkv bf16 [B, (Hq + 2 Hkv) dh], row stride ld_qkv: the q|k|v projection of the step (with bias), M = B.
 * q is rotated in place at position pos[b] (HF rotate_half, tables f32 [S_cap, dh / 2] of bf16-rounded values, every product rounded:
 * the bits the full-sequence rotation writes for that position); the rotated k and the v go to row pos[b] of sample b of k_cache /
 * v_cache (the k and v columns of qkv stay as they were).  A row with pos[b] outside [0, S_cap) is skipped whole.  dh even. */
int vla_decode_rope_append(void* stream, void* qkv, const float* cos_t, const float* sin_t, const int* pos, void* k_cache,
                           void* v_cache, int B, int Hq, int Hkv, int dh, int ld_qkv, int S_cap, long long cache_sb, int cache_ss);

/* Single-query attention over the cache: for every (b, query head) the one query row against keys / values 0 .. pos[b] of sample b
 * (no key mask: rows are right-padded and the new token overwrote the first pad slot, so every key up to pos[b] is valid; nothing
 * behind pos[b] is read).  q bf16 [B, Hq dh] (row stride ld_q, rotated), out bf16 [B, Hq dh] (row stride ld_out).  GQA: Hq % Hkv == 0
 * with at most 8 query heads per kv head; dh 64 or 128.  Scores, softmax and the weighted sum in fp32, rounded once to bf16.
 * pos[b] is clamped into [0, S_cap). */
int vla_decode_attn(void* stream, const void* q, const void* k_cache, const void* v_cache, const int* pos, void* out, int B, int Hq,
                    int Hkv, int dh, int ld_q, int ld_out, int S_cap, long long cache_sb, int cache_ss, float scale);

/* Number of vocabulary slabs the lm_head pass cuts V rows into: the workspace of vla_decode_lm_head_argmax holds B * slabs pairs. */
int vla_decode_argmax_slabs(int V);

/* lm_head and greedy choice in one stream of W, and the hand-over to the next step.
 *   x bf16 [B, D] (row stride ld_x): the final-norm output of the rows to decode; W bf16 [V, D] (row stride ld_w).
 *   logit[b, v] = bf16(sum_d x[b, d] W[v, d]) - accumulated in fp32, rounded once, as a bf16 lm_head emits it.
 *   id int64 [B] = the argmax of logit[b, :] in torch.argmax's order: the lowest index among equal values, a NaN above everything,
 *                  the first NaN wins (the order the token-accuracy metric uses).
 * Two passes: one (value, index) pair per slab of rows and sample into part_val f32 / part_idx int32 [B, slabs], then a finish that
 * walks the slabs in a fixed order.  logits_out bf16 [B, V] (row stride ld_logits) or NULL: the very values that were compared.
 * out_ids int64 [B, T] or NULL.  Not NULL - the advance, with t = *step (int32, device):
 *   out_ids[b, t] = id[b] (when t < T);  x_next[b, :] = embed[id[b], :] (embed bf16 [vocab_e, D], row strides ld_embed / ld_next; the id
 *   is clamped into the table);  pos[b] += 1;  *step = t + 1.
 * pos_from int32 [B] or NULL.  Not NULL - the first advance of a generation, behind the prefill: t = 0 whatever *step holds,
 * pos[b] = pos_from[b] + 1 and *step = 1, so that a replayed prefill graph resets the counters it does not own.
 * D % 8 == 0, D <= 4096, B <= 64; x, W, embed, x_next 16-B aligned with row strides that are multiples of 8. */
int vla_decode_lm_head_argmax(void* stream, const void* x, int ld_x, const void* W, int ld_w, int B, int D, int V, float* part_val,
                              int* part_idx, long long* id, void* logits_out, long long ld_logits, long long* out_ids, int T, int* step,
                              int* pos, const int* pos_from, const void* embed, int vocab_e, int ld_embed, void* x_next,
                              int ld_next);

#ifdef __cplusplus
}
#endif
#endif
