/* C ABI of the evaluator's frame pipeline of libvla_native.so (the reference's resize_image_for_policy: a JPEG round trip, then TF's
 * lanczos3 resize with antialiasing): a ninth header beside vla_native.h, in the manner of vla_jpeg_index.h.
 *
 * vla_native.h and VLA_ABI_VERSION are pinned by the tests that guard them; these calls were added later, change no descriptor and no
 * existing signature, and are looked up by name.  They live in the same library and follow the same conventions - return VLA_OK (0)
 * or a negative code with the text in vla_last_error(); `stream` is a hipStream_t; every pointer is a device pointer; nothing is
 * allocated, read back or synchronised, so a captured graph may hold the calls - and are compiled from csrc/policy_image.hip around
 * csrc/jpeg_forward.h, csrc/jpeg_core.h and stage B of csrc/jpeg.hip.  No atomics: every output element is written by one thread.
 *
 * What is pinned: the round trip is, bit for bit, what Pillow / libjpeg-turbo gives for saving a frame as a
 * 4:2:0 baseline file of the given quality and opening it again; the resize is, bit for bit, the float32 numpy rule of
 * tests/policy_image_rule_np.py.  What is not: TensorFlow's own last bits, the order of the two resize passes, numpy's sin against
 * glibc's sinf in the weights, and that tf.image.encode_jpeg / tf.io.decode_image run libjpeg at quality 95, 4:2:0, islow and fancy
 * upsampling.
 */
#ifndef VLA_POLICY_IMAGE_H
#define VLA_POLICY_IMAGE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for N images of H x W: round_trip != 0 - what vla_policy_jpeg_round_trip needs (H and W multiples of 16 inside
 * [16, 4096]); round_trip == 0 - what vla_policy_lanczos3_resize needs for H x W -> out_h x out_w (the float32 intermediate of the
 * vertical pass, N * out_h * W * 3 floats; 0 when one of the two passes has nothing to do).  -> -1 for a shape the call refuses.
 * Host arithmetic only. */
long long vla_policy_image_workspace_bytes(long long N, int H, int W, int out_h, int out_w, int round_trip);

/* frames u8 [N, H, W, 3], image n at frames + n * in_stride (in_stride >= H * W * 3) -> out_frames, image n at out_frames + n *
 * out_stride, the pixels a 4:2:0 baseline JPEG file of the frame decodes to.  qtab: u16 [2, 64], the luminance and the chrominance
 * quantisation table in natural (row-major) order, entries 1 .. 255 (input_stage.jpeg_quant_tables; a zero is taken as 1).  Three
 * launches: one wave per 16 x 16 MCU - colour conversion, chroma downsampling, forward DCT, quantisation, dequantisation into the
 * coefficient layout of the decode - then stage B of vla_jpeg_decode_rows, unchanged.  H and W: multiples of 16 inside [16, 4096]
 * (an edge MCU would need libjpeg's edge replication: refused).  workspace: 16-byte aligned, vla_policy_image_workspace_bytes(N, H, W,
 * 0, 0, 1) bytes.  frames and out_frames may not overlap. */
int vla_policy_jpeg_round_trip(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W,
                               const unsigned short* qtab, void* workspace, long long workspace_bytes, unsigned char* out_frames,
                               long long out_stride);

/* frames u8 [N, H, W, 3] (image n at frames + n * in_stride) -> out u8 [N, out_h, out_w, 3], contiguous: tf.image.resize(method =
 * "lanczos3", antialias = True), rounded half to even and clamped to 0 .. 255.  starts_* int32 [out_len], weights_* f32 [out_len,
 * span_*]: the spans of input_stage.tf_lanczos3_spans(H, out_h) (v) and (W, out_w) (h); tap k of output p reads source
 * min(clamp(starts[p], 0, in_len - 1) + k, in_len - 1), so no table makes a kernel read outside.  The vertical pass runs first, into a
 * float32 intermediate in `workspace` (4-byte aligned, vla_policy_image_workspace_bytes(N, H, W, out_h, out_w, 0) bytes), then the
 * horizontal pass; a pass whose length does not change is not run (its tables may be null), and the other one then goes from u8 to u8.
 * With H == out_h and W == out_w the call is refused: there is nothing to do.  Every sum is acc = 0; acc += w * v over the span in source
 * order, in float32 without contraction. */
int vla_policy_lanczos3_resize(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W, int out_h,
                               int out_w, const int* starts_v, const float* weights_v, int span_v, const int* starts_h,
                               const float* weights_h, int span_h, void* workspace, long long workspace_bytes, unsigned char* out);

#ifdef __cplusplus
}
#endif
#endif
