// Stage B of the JPEG decode - dequantised coefficient blocks -> the planes Y, Cb, Cr -> RGB pixels - as the one function both of its
// callers launch it through: vla_jpeg_decode_rows (csrc/jpeg.hip, behind the entropy decode of a file) and vla_policy_jpeg_round_trip
// (csrc/policy_image.hip, behind the forward half of csrc/jpeg_forward.h).  The kernels live in csrc/jpeg.hip and nowhere else.
#pragma once

#include <hip/hip_runtime.h>

namespace vlajpeg {

// coef: short [slots, blocks_per_image, 64] laid out by block_index (jpeg_core.h), 16-byte aligned; planes: u8 [slots, blocks_per_image
// * 64] of workspace; out_frames: u8, image `slot` at slot * out_stride, out_stride >= H * W * 3.  Two launches on `st`, nothing
// allocated or read back.  The caller has checked that H and W are multiples of 16 inside [16, 4096], that slots >= 1 and that
// stage_b_fits().  -> VLA_OK or VLA_ERR_LAUNCH.
int stage_b(hipStream_t st, const short* coef, unsigned char* planes, long long slots, int H, int W, int h2v2, unsigned char* out_frames,
            long long out_stride);

// whether the two grids of stage_b fit one launch each
bool stage_b_fits(long long slots, int H, int W);

}  // namespace vlajpeg
