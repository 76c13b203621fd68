/* C ABI of the scan index of the JPEG frame store of libvla_native.so (segments without restart markers cut into pieces that decode in
 * parallel): an eighth header beside vla_native.h, in the manner of vla_jpeg.h.
 *
 * vla_native.h, VLA_ABI_VERSION and vla_jpeg.h with its two symbols are pinned by the tests that guard them; these calls were added
 * later, change no descriptor and no existing signature, and are looked up by name.  They live in the same library and follow the
 * same conventions - return VLA_OK (0) or a negative code with the text in vla_last_error(); `stream` is a hipStream_t; every pointer
 * is a device pointer; nothing is allocated, read back or synchronised - and are compiled from csrc/jpeg_index.hip and csrc/jpeg.hip
 * around the decode core of csrc/jpeg_core.h.  No atomics: for a monotone piece_off every word is written by one thread (under a
 * non-monotone one two segments own the same rows and both write them - either one's words, all of them in range).
 *
 * The entropy decode of vla_jpeg_decode_rows is serial per segment, and a file without restart markers is one segment.  A restart
 * marker says two things: where a decoder may begin, and that the DC predictors are zero there.  One serial walk of a segment, done
 * once at load, records the same for any MCU inside it - the byte and the bit at which the MCU begins, and the three predictors
 * there - and every later decode begins each piece from its record.  The files are not touched and the pixels do not change.
 *
 * The store of vla_jpeg.h (bytes, img_seg, seg_tab, img_tab, qt_pool, ht_pool) gains one table, row for row beside seg_tab:
 *   seg_ent  int32  [S, 4]         per segment: bit (0 .. 7: bits of the byte at lo that are already consumed), then the DC predictors
 *                                  of Y, Cb, Cr at its first MCU.  lo names the byte that holds the next unread bit, never the stuffed
 *                                  0x00 of a 0xFF 0x00 pair.
 * Segment [m0, m1) of S becomes max(1, ceil((m1 - m0) / piece_mcus)) pieces of piece_mcus MCUs (the last one shorter), which are
 * segments of the new store of S' rows in every respect.  A piece's hi is the next piece's lo; one more when that piece begins
 * inside a byte, which the two share; two more when the shared byte is 0xFF, so that its stuffed 0x00 lies inside the range.  The last
 * piece keeps the segment's hi.  A walk that stops with a non-zero status inside piece j leaves pieces 0 .. j valid, piece j with the
 * segment's hi, and every later piece with lo = hi = the segment's hi and a zero entry: decoded, they report that they ran out of
 * bytes and hold zero coefficients, and the image's pixels are those of the decode without an index.
 */
#ifndef VLA_JPEG_INDEX_H
#define VLA_JPEG_INDEX_H

#ifdef __cplusplus
extern "C" {
#endif

/* The pieces of the segments [s_begin, s_end) of the store (0 <= s_begin <= s_end <= S): one work item per segment s walks it once and
 * writes every word of rows piece_off[s] .. piece_off[s + 1] of out_seg_tab (int64 [S', 4]: lo, hi, mcu0, mcu1) and of out_seg_ent
 * (int32 [S', 4]), and out_status[s] (u8 [S]: 0 = the walk reached the segment's last MCU, else the status vla_jpeg_decode_rows
 * reports for it).  Nothing else is written.  piece_off int64 [S + 1] comes from the host, which knows every segment's MCU count;
 * img_seg is the store's own (it finds a segment's image, and so its tables).  mapping = 0: one lane per segment, 1: one wave per
 * segment (its first lane walks, from a copy of the segment in LDS when it fits).  1 <= piece_mcus <= 2^20.  S_out: the rows of
 * out_seg_tab / out_seg_ent, S' of the plan.
 * A walk is serial and may take tens of milliseconds for a large scan, so a caller with a large store bounds every launch by walking
 * it in slices of segments.
 * No stream and no table makes a kernel read or write outside: byte ranges are clamped into [0, n_bytes], MCU ranges into the image,
 * table ids into the pools, piece_off into [0, S'] and made monotone, and a walk writes no more rows than piece_off gives it. */
int vla_jpeg_index_build(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg, const long long* seg_tab,
                         long long S, const int* img_tab, const unsigned short* qt_pool, int nQ, const int* ht_pool, int nH, long long N,
                         int H, int W, int h2v2, int piece_mcus, const long long* piece_off, long long s_begin, long long s_end, int mapping,
                         long long* out_seg_tab, int* out_seg_ent, long long S_out, unsigned char* out_status);

/* vla_jpeg_decode_rows with an entry state per segment: the same three launches and the same kernels, stage A beginning segment s at
 * bit seg_ent[s][0] of its first byte with the predictors seg_ent[s][1 .. 3].  Every other argument, the outputs and the memory
 * contract are vla_jpeg_decode_rows's.  The bit is masked to 0 .. 7; the predictors feed arithmetic only (a wrapping add, then a
 * product that saturates to int16), so any value is safe and none is clamped. */
int vla_jpeg_decode_rows_at(void* stream, const unsigned char* bytes, long long n_bytes, const long long* img_seg, const long long* seg_tab,
                            const int* seg_ent, long long S, const int* img_tab, const unsigned short* qt_pool, int nQ, const int* ht_pool,
                            int nH, const long long* episode_off, int E, long long T, const int* ep, const long long* row, int B, int n_img,
                            int H, int W, int h2v2, int max_seg, int mapping, void* workspace, long long workspace_bytes,
                            unsigned char* out_frames, long long out_stride, unsigned char* status);

#ifdef __cplusplus
}
#endif
#endif
