// The MCU stage of the forward half (csrc/jpeg_forward.h) as the encoder launches it: the kernel of vla_policy_jpeg_round_trip
// (csrc/policy_image.hip, and nowhere else), keeping the quantised values in place of the dequantised ones.
#pragma once

#include <hip/hip_runtime.h>

namespace vlajpeg {

// frames: u8 [N, H, W, 3], image n at frames + n * in_stride; qtab: u16 [2, 64] in natural order -> quant: short [N * mcus_per_image, 6,
// 64], 16-byte aligned: the six blocks of every MCU in coding order (Y Y Y Y Cb Cr), each in zigzag order.  One launch on `st`, nothing
// allocated or read back.  The caller has checked that H and W are multiples of 16 inside [16, 4096] and that N >= 1.
// -> VLA_OK, VLA_ERR_LAUNCH, or VLA_ERR_ARG when the grid does not fit one launch.
int stage_a_quantised(hipStream_t st, const unsigned char* frames, long long in_stride, long long N, int H, int W, const unsigned short* qtab,
                      short* quant);

}  // namespace vlajpeg
