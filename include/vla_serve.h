/* C ABI of the serving entry points of libvla_native.so (batched predict_actions): a second header beside vla_native.h.
 *
 * Why a second header: vla_native.h, its signature table in the Python binding and VLA_ABI_VERSION are pinned by the tests that
 * guard the training ABI; the serving calls were added later, change no descriptor and no existing signature, and are looked up by
 * name (vla_native.h, "Added since without a version change").  They live in the same library, follow the same conventions - return
 * VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a hipStream_t; every pointer is a device pointer unless
 * marked host; nothing is allocated, read back or synchronised, so a captured graph may hold every call - and are compiled from
 * csrc/serve.hip.  No atomics: every output element is written exactly once by one thread.
 */
#ifndef VLA_SERVE_H
#define VLA_SERVE_H

#ifdef __cplusplus
extern "C" {
#endif

/* The batch of OpenVLAForActionPrediction._prepare_input_for_action_prediction + _prepare_labels_for_action_prediction
 * (prismatic/extern/hf/modeling_prismatic.py:747-782) plus right padding to L, one launch.
 *   prompt_flat int64 [n_flat]: the samples' prompt ids back to back, exactly as the processor returned them (nothing is trimmed);
 *   prompt_off  int32 [B + 1]: offsets into prompt_flat, clamped into [0, n_flat] (a bad table cannot make the kernel read outside).
 * Row b, with P = its prompt length and n = P + num_tokens + 1:
 *   ids            int64 [B, L] = prompt | num_tokens x fill_id | stop_id | pad_id up to L
 *   labels         int64 [B, L] = ignore_index over the prompt | num_tokens x action_label | stop_id | ignore_index
 *   attention_mask u8    [B, L] = j < n   (NOT ids != pad_id: the reference attends every id the processor returned)
 *   hid_row        int32 [B]    = P - 1: text-relative first row of the hidden states predict_action returns (:855, :927)
 *   row_ok         u8    [B]    = (P >= 1 && n <= L)
 * A row that is not ok (empty prompt, or one that does not fit L) is written as the well-formed row of the one-id prompt [pad_id]
 * (hid_row 0), so that the forward stays finite; vla_unnormalize_actions turns its actions into NaN.  Every element of the five
 * outputs is written.  L >= num_tokens + 2, num_tokens >= 1. */
int vla_serve_tokens(void* stream, const long long* prompt_flat, const int* prompt_off, long long n_flat, long long* ids,
                     long long* labels, unsigned char* attention_mask, int* hid_row, unsigned char* row_ok, int B, int L,
                     int num_tokens, long long fill_id, long long stop_id, long long action_label, long long pad_id,
                     long long ignore_index);

/* The evaluator's normalize_proprio (experiments/robot/openvla_utils.py:671-701) - not the training normalisation: the unmasked
 * dimensions are clipped too and there is no zero-mask.  x [n / D, D] f32 (x_is_f64 == 0) or f64; low / high f64 [D] (min / max for
 * "bounds", q01 / q99 for "bounds_q99": the caller resolves them); mask u8 [D] or NULL (all ones).
 *   y f32 = (float) clip(mask[d] ? 2 * (x - low[d]) / (high[d] - low[d] + 1e-8) - 1 : x, -1, 1)
 * evaluated in f64 in numpy's association, every operation rounded on its own (no fused multiply-add), rounded once to f32; a NaN
 * stays a NaN (np.clip). */
int vla_normalize_proprio_serve(void* stream, const void* x, int x_is_f64, float* y, long long n, int D, const double* low,
                                const double* high, const unsigned char* mask);

/* The back end of predict_action, _unnormalize_actions (modeling_prismatic.py:784-805) on the head's bf16 output.
 * pred bf16 [B, row] (row stride ld_pred elements), row = chunk * Da; low / high f64 [Da]; mask u8 [Da] or NULL (all ones);
 * row_ok u8 [B] or NULL (all ok).  out f64 [B, row] (row stride ld_out):
 *   a = (float) pred;  out = mask[d] ? 0.5f * (a + 1.0f) * (high[d] - low[d] + 1e-8) + low[d] : a        (d = column % Da)
 * with a + 1 and the product by 0.5 in f32 and the rest in f64 - numpy's promotion on the reference's float32 array - and no fused
 * multiply-add: bit-identical to the host function.  Rows with row_ok == 0 are NaN throughout. */
int vla_unnormalize_actions(void* stream, const void* pred, double* out, int B, int row, int Da, int ld_pred, int ld_out,
                            const double* low, const double* high, const unsigned char* mask, const unsigned char* row_ok);

/* The hidden states predict_action returns, for a batch: out bf16 [B, T, D] (compact) = rows [r, r + T) of sample b of
 * hs bf16 [B, S, D] (batch stride s_batch, row stride ld, in elements), r = Np + hid_row[b] clamped into [0, S - T] (hid_row from
 * vla_serve_tokens is always inside).  D, ld, s_batch % 8 == 0, hs / out 16-B aligned (rows move in 16-B chunks); S >= T. */
int vla_serve_gather_hidden(void* stream, const void* hs, const int* hid_row, void* out, int B, int S, int Np, int T, int D,
                            long long s_batch, int ld);

#ifdef __cplusplus
}
#endif
#endif
