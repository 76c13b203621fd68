/* C ABI of action-token sampling (VLAEngine.generate with sample= / return_logprobs): a header of its own beside vla_decode.h.
 *
 * One decoding step for B rows on the bf16 logits the lm_head pass of vla_decode_lm_head_argmax stores (logits_out): temperature,
 * top-k, top-p, a Gumbel-max draw and the log-probability of the drawn token - or the greedy token with its log-probability - and the
 * advance of include/vla_decode.h.  The rule is restated in float64 by tests/sample_rule_np.py and written out in DESIGN section 23.
 * Conventions of every family: the caller owns all memory, everything runs on `stream` (a hipStream_t), nothing is allocated, read
 * back or synchronised - a captured graph may hold the call - and the result is VLA_OK (0) or a negative code with the text in
 * vla_last_error().  Every output element is written once; every floating-point sum runs in a fixed order (the histograms are integer
 * sums in LDS, which commute): the same inputs give the same bits.  No workspace is needed.
 *
 * The parameter block lives in device memory, as pos[] and *step do: one captured step graph serves every setting and every seed.
 * `params` points to 24 bytes, 8-B aligned:
 *     offset  0  float              temperature   > 0
 *     offset  4  float              top_p         in (0, 1]; 1 switches the filter off
 *     offset  8  int                top_k         0 switches the filter off; >= V keeps everything
 *     offset 12  int                greedy        not 0: the greedy rule, the three settings above are not read
 *     offset 16  unsigned long long seed
 * A temperature that is not above 0, a top_p outside (0, 1] or a negative top_k is the caller's error (the host wrappers refuse
 * them); on the device such a row is treated as a non-finite row (below), nothing faults.
 */
#ifndef VLA_SAMPLE_H
#define VLA_SAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* logits bf16 [B, V] (row stride ld_logits >= V, elements; 2-B aligned), B <= 64, V >= 1.  Row b, with l = its logits and t the step
 * index (*step, int32 on the device - or 0 when pos_from is given, whatever *step holds):
 *   z = l / temperature (fp32, correctly rounded);
 *   top-k: keep z >= the k-th largest z (ties kept);  top-p: over the softmax of what top-k kept, walk the classes of equal z in
 *   ascending order and drop a class while the cumulative probability through it is <= 1 - top_p (the largest class stays);
 *   draw: id = argmax over the kept v of z[v] + g[v], g = -logf(-logf(u)), u = ((r >> 41) + 0.5) / 2^23 (exact in fp32, inside (0, 1)),
 *         r = splitmix64_key(splitmix64_key(splitmix64_key(seed ^ SAMPLE_STREAM, s), t), v), s = streams[b] (int64 [B]) or b when
 *         streams is NULL; equal sums go to the lowest id;
 *   logprob = z[id] - logsumexp(z over the kept v).
 *   greedy: id = the argmax of l in the order of vla_decode_lm_head_argmax (lowest index among equals, a NaN above everything),
 *           logprob = log_softmax(l)[id]: no temperature, no filter.
 *   A row with a NaN or +inf logit, or whose largest logit is -inf, takes the greedy id; its logprob and its probs_out row are NaN.
 * Outputs: id int64 [B];  logprob_out f32 [B, T] or NULL: element [b, t] is written when 0 <= t < T;  probs_out f32 [B, V] (row stride
 * ld_probs >= V) or NULL: the filtered, renormalised probabilities, exactly 0 for a removed token.
 * out_ids int64 [B, T] or NULL.  Not NULL - the advance of include/vla_decode.h with the same meaning of T, step, pos, pos_from, embed
 * (bf16 [vocab_e, D]), x_next (bf16 [B, D]) and their strides: out_ids[b, t] = id[b], x_next[b, :] = embed[id[b], :], pos[b] += 1 (or
 * pos_from[b] + 1), *step = t + 1.  NULL: *step and pos are only read.  step is never NULL.  With the advance D % 8 == 0, embed and
 * x_next 16-B aligned with row strides that are multiples of 8 and at least D. */
int vla_sample_tokens(void* stream, const void* logits, long long ld_logits, int B, int V, const void* params, const long long* streams,
                      long long* id, float* logprob_out, float* probs_out, long long ld_probs, long long* out_ids, int T, int* step,
                      int* pos, const int* pos_from, const void* embed, int vocab_e, int ld_embed, void* x_next, int ld_next, int D);

#ifdef __cplusplus
}
#endif
#endif
