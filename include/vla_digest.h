/* C ABI of the state digest of libvla_native.so (a position-weighted 64-bit digest of a flat buffer of 16-bit words, computed on the
 * device): a sixth header beside vla_native.h, vla_serve.h, vla_episodes.h, vla_mixture.h and vla_heldout.h.
 *
 * As with vla_heldout.h: the five earlier headers, their signature tables in the Python binding and VLA_ABI_VERSION are pinned by
 * tests; these calls were added later, change no descriptor and no existing signature, and are looked up by name.  They live in the
 * same library and follow the same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a
 * hipStream_t; every pointer is a device pointer; nothing is allocated, read back or synchronised, so a captured graph may hold the
 * call - and are compiled from csrc/digest.hip.  No atomics: every workgroup writes one partial sum, one workgroup adds them.  The
 * header's last entry serves the same end - two runs of the same step must be comparable bit for bit - for the one logged number that
 * was not: the token-CE loss sum.
 *
 * The rule (restated in numpy in tests/digest_rule_np.py).  The operand is a contiguous view of n 16-bit words.
 * Its 2 n bytes are zero-padded to a multiple of 8 and read as little-endian 64-bit chunks q_c, c = 0 .. ceil(n / 4) - 1; c counts from
 * the view's first word, so the digest of a buffer does not depend on where it lives.  With all arithmetic modulo 2^64:
 *   z = c + 0x9E3779B97F4A7C15 * (salt + 1)
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB
 *   z = z ^ z >> 31
 *   digest = sum over c of (q_c + 1) * (z | 1)  +  n * 0xD1B54A32D192ED03
 * A wrapping sum is associative and commutative: every reduction tree gives the same bits, and the launch geometry does not show in
 * the result.
 */
#ifndef VLA_DIGEST_H
#define VLA_DIGEST_H

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: the number of 64-bit scratch slots vla_state_digest can use (one per workgroup of its first pass). */
int vla_state_digest_slots(void);

/* out[0] (u64, 8-byte aligned) = the digest of the n >= 1 words at x (2-byte aligned) under `salt`.
 * Where x lies on a 16-byte boundary the whole 16-byte groups are read with 16-byte loads (two chunks each) and only the last n % 8
 * words one by one; any other start is read word by word.  No byte outside [x, x + 2 n) is read.
 * First pass: W workgroups each leave one partial sum in scratch[0 .. W), W <= min(scratch_slots, vla_state_digest_slots()); a second
 * one-workgroup pass adds them and the length term into out.  A view small enough for one workgroup (at most 256 units, a unit being a
 * 16-byte group or a single chunk), or scratch_slots <= 1, takes the first pass alone, which then writes out itself and touches no
 * scratch (scratch may be NULL).  Nothing but out[0] and scratch[0 .. W) is written. */
int vla_state_digest(void* stream, const void* x, long long n, unsigned long long salt, unsigned long long* scratch,
                     long long scratch_slots, unsigned long long* out);

/* vla_token_ce_metrics (vla_native.h) with the loss sum taken in a fixed order, so that the logged token-CE loss has the same bits in
 * every run of the same step (the f32 atomicAdd per row of vla_token_ce_metrics leaves the last bit to the order in which the workgroups
 * finish; the gradient never read that sum, only the exact count).  Same operands, same counters and pred_ids, plus
 *   terms  f32 [rows]  scratch, written whole: a valid row's logsumexp(logits) - logits[label], 0 for any other row
 * loss_sum_and_count[0] += the sum of the valid rows' terms, added by one workgroup of 256 threads: thread t the valid rows t, t + 256,
 * ... in ascending order, the lanes of a wave by the xor butterfly 32, 16, .. 1, the four waves in index order; [1] += their number.
 * Compiled from csrc/elementwise.hip, beside the kernel it shares with vla_token_ce_metrics. */
int vla_token_ce_metrics_ordered(void* stream, const void* logits, long long ld_logits, const long long* shifted_labels,
                                 const unsigned char* row_class, int rows, int V, float* loss_sum_and_count, unsigned long long* counters,
                                 int* pred_ids, long long tokenizer_len, int n_bins, float* terms);

#ifdef __cplusplus
}
#endif
#endif
