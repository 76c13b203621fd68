/* C ABI of the JPEG frame store of libvla_native.so (episodes whose frames are baseline JPEG files in device memory -> the frames of
 * one raw batch): a seventh header beside vla_native.h, in the manner of vla_episodes.h.
 *
 * vla_native.h, its signature table in the Python binding and VLA_ABI_VERSION are pinned by the tests that guard the training ABI;
 * these calls were added later, change no descriptor and no existing signature, and are looked up by name.  They live in the same
 * library and follow the same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a
 * hipStream_t; every pointer is a device pointer; nothing is allocated, read back or synchronised, so a captured graph may hold the
 * call - and are compiled from csrc/jpeg.hip around the decode core of csrc/jpeg_core.h.  No atomics: every element of out_frames
 * and of status is written exactly once by one thread.
 *
 * The store (vla_adapter_amd/jpeg_store.py parses it once at load): N = T * n_img images, image (t, cam) at index t * n_img + cam;
 *   bytes    u8     [n_bytes]      the JPEG files back to back (only their entropy-coded bytes are read)
 *   img_seg  int64  [N + 1]        the segments of image i are rows img_seg[i] .. img_seg[i + 1] of seg_tab (one without restart
 *                                  markers, else one per restart interval)
 *   seg_tab  int64  [S, 4]         per segment: the bytes [lo, hi) between two markers, and the MCUs [mcu0, mcu1) they code
 *   img_tab  int32  [N, 12]        per image: quantisation table, DC table, AC table of Y, Cb, Cr (3 + 3 + 3 pool ids), the restart
 *                                  interval, the sampling, 0
 *   qt_pool  uint16 [nQ, 64]       the distinct quantisation tables, zigzag order
 *   ht_pool  int32  [nH, 548]      the distinct Huffman tables in derived form: maxcode[18], valptr - mincode [18], an 8-bit
 *                                  lookahead [256] of (length << 8 | symbol), huffval[256]
 */
#ifndef VLA_JPEG_H
#define VLA_JPEG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `workspace` for `slots` = B * n_img images of H x W: the dequantised int16 coefficients and, behind them, the u8 planes
 * (Y, Cb, Cr) the inverse DCT writes.  Host arithmetic only; -1 for arguments vla_jpeg_decode_rows refuses. */
long long vla_jpeg_workspace_bytes(long long slots, int H, int W, int h2v2);

/* The frames of a batch: out_frames[b, cam] = image r * n_img + cam decoded to RGB, for every b < B and cam < n_img, where r is row[b]
 * clamped into episode ep[b] exactly as vla_episode_gather clamps it (one definition: csrc/episode_row.h) - a bad index still gives
 * an in-range frame of that episode.  H and W are multiples of 16 (whole MCUs); h2v2 = 1: 4:2:0, 0: 4:4:4, one sampling per store.
 * The arithmetic is libjpeg's defaults (islow IDCT, fancy upsampling, 16-bit colour tables), bit for bit.
 *   stage A  one work item per (image, segment k < max_seg): Huffman decode of the segment, DC predictors reset, dequantised
 *            coefficients into workspace; mapping = 0: one lane per item, 1: one wave per item (its first lane decodes)
 *   stage B  inverse DCT of every block into the planes of workspace, then upsampling and colour conversion into out_frames
 *   out_frames u8 [B, n_img, H, W, 3], image (b, cam) at out_frames + (b * n_img + cam) * out_stride, out_stride >= H * W * 3
 *   status     u8 [B, n_img, max_seg]: 0 = the segment decoded (or the image has no such segment), 1 = it ran out of bytes, 2 = a
 *              code that is in no table, 3 = a run past the block's end; after a non-zero status the segment's remaining
 *              coefficients are zero.  Every slot is written.
 * No stream and no table makes a kernel read or write outside: byte ranges are clamped into [0, n_bytes], segment rows into [0, S],
 * MCU ranges into the image, table ids into the pools.  workspace: 16-byte aligned, workspace_bytes >= vla_jpeg_workspace_bytes. */
int vla_jpeg_decode_rows(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg, const long long* seg_tab,
                         long long S, const int* img_tab, const unsigned short* qt_pool, int nQ, const int* ht_pool, int nH,
                         const long long* episode_off, int E, long long T, const int* ep, const long long* row, int B, int n_img, int H,
                         int W, int h2v2, int max_seg, int mapping, void* workspace, long long workspace_bytes,
                         unsigned char* out_frames, long long out_stride, unsigned char* status);

#ifdef __cplusplus
}
#endif
#endif
