/* C ABI of the JPEG encoder of libvla_native.so (raw frames on the device -> complete baseline files, byte for byte what Pillow
 * saves): a tenth header beside vla_native.h, in the manner of vla_policy_image.h.
 *
 * vla_native.h and VLA_ABI_VERSION are pinned by the tests that guard them; these calls were added later, change no descriptor and no
 * existing signature, and are looked up by name.  They live in the same library and follow the same conventions - return VLA_OK (0)
 * or a negative code with the text in vla_last_error(); `stream` is a hipStream_t; every pointer is a device pointer; nothing is
 * allocated, read back or synchronised - and are compiled from csrc/jpeg_encode.hip around csrc/jpeg_encode_core.h, with the MCU stage
 * of csrc/policy_image.hip (csrc/jpeg_forward.h) in front.  No global atomics: every output byte is written by one thread.
 *
 * What is pinned: for H and W multiples of 16 the file of frame n is, in every byte, what
 * Image.save(buf, "JPEG", quality = q, subsampling = 2, restart_marker_rows = restart_rows) of Pillow / libjpeg-turbo writes, where
 * qtab = input_stage.jpeg_quant_tables(q): SOI, JFIF APP0, DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1 (the standard tables), DRI, SOS,
 * the restart intervals with RSTn between them, EOI.  Optimised Huffman tables, other samplings and a file without restart markers are
 * not built.
 *
 * The size of the files is not known before they are coded, so the encode is two calls around one read of the caller's:
 *   vla_jpeg_encode_plan   frames -> the quantised coefficients and the length of every restart interval in `workspace`, and frame_off
 *   (the caller reads frame_off[N], the byte count, and provides `out`)
 *   vla_jpeg_encode_write  workspace, frame_off -> out
 */
#ifndef VLA_JPEG_ENCODE_H
#define VLA_JPEG_ENCODE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for N frames of H x W with a restart interval of restart_rows rows of MCUs: the int16 coefficients (N * H * W * 3
 * bytes), and an int64 offset and an int32 length per interval.  -> -1 for what the calls refuse: H or W no multiple of 16 inside
 * [16, 4096], N outside [1, 2^20], restart_rows < 1 (the serial form, one segment per file, is left to the host) or an interval of
 * more than 65535 MCUs.  Host arithmetic only. */
long long vla_jpeg_encode_workspace_bytes(long long N, int H, int W, int restart_rows);

/* frames u8 [N, H, W, 3], image n at frames + n * in_stride (in_stride >= H * W * 3); qtab: u16 [2, 64], the luminance and the
 * chrominance quantisation table in natural order, entries 1 .. 255 -> frame_off int64 [N + 1]: the byte offsets of the N files laid
 * back to back, frame_off[0] = 0 and frame_off[N] the byte count; and in `workspace` (16-byte aligned,
 * vla_jpeg_encode_workspace_bytes) what vla_jpeg_encode_write reads.  Three launches: the MCU stage (one wave per MCU), the length of
 * every interval (one wave per interval, coded as it will be written, stuffed bytes counted), the prefix sums (one workgroup). */
int vla_jpeg_encode_plan(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W,
                         const unsigned short* qtab, int restart_rows, void* workspace, long long workspace_bytes, long long* frame_off);

/* workspace and frame_off as vla_jpeg_encode_plan left them for the same N, H, W, qtab, restart_rows -> out u8 [out_bytes]: file n at
 * out + frame_off[n].  out_bytes >= frame_off[N]; no byte at or behind out + out_bytes is written whatever the tables hold.  Two
 * launches: headers, RSTn markers and EOI (one workgroup per frame), the intervals (one wave per interval).  The workspace is only
 * read. */
int vla_jpeg_encode_write(void* stream, long long N, int H, int W, const unsigned short* qtab, int restart_rows, const void* workspace,
                          long long workspace_bytes, const long long* frame_off, unsigned char* out, long long out_bytes);

#ifdef __cplusplus
}
#endif
#endif
