// Glue kernels of the backbone-training steps (LoRA and full fine-tune through DINOv2 + SigLIP, two images): LayerScale as a
// parameter, strided 3-level row copies (feature-buffer <-> per-backbone layouts, prefix-token placement).  HBM-bound, 16 B per
// lane wherever the addresses allow it.
#include "common.h"
#include "../../include/vla_native.h"

namespace {

// dst[g][r][0:cols] = src[g][r][0:cols]  (bf16; 16-B lanes when VEC)
template <bool VEC>
__global__ void copy_rows3d_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int groups, int rows, int cols, long long s_sg,
                                   long long s_sr, long long d_sg, long long d_sr) {
  const int per = VEC ? cols >> 3 : cols;
  const long long total = (long long)groups * rows * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long gr = i / per;
    const int c = (int)(i - gr * per);
    const int g = (int)(gr / rows), r = (int)(gr - (long long)g * rows);
    const bf16_t* s = src + g * s_sg + r * s_sr;
    bf16_t* d = dst + g * d_sg + r * d_sr;
    if (VEC) reinterpret_cast<uint4*>(d)[c] = reinterpret_cast<const uint4*>(s)[c];
    else d[c] = s[c];
  }
}

// out = bf16(x + bf16(a * ls)): LayerScale (modeling_prismatic.py:58-66, `x * self.scale_factor`) + the block's residual add
__global__ void layerscale_fwd_kernel(const bf16_t* __restrict__ a, const bf16_t* __restrict__ ls, const bf16_t* __restrict__ x,
                                      bf16_t* __restrict__ out, long long rows, int cols8) {
  const long long total = rows * cols8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cols8);
    float fa[8], fl[8], fx[8], o[8];
    unpack8(reinterpret_cast<const uint4*>(a)[i], fa);
    unpack8(reinterpret_cast<const uint4*>(ls)[c], fl);
    unpack8(reinterpret_cast<const uint4*>(x)[i], fx);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = fx[k] + rbf(fa[k] * fl[k]);
    reinterpret_cast<uint4*>(out)[i] = pack8(o);
  }
}

// da = bf16(dy * ls) (no dls: each lane owns 8 columns, the 4 waves of a block split the rows of its chunk)
__global__ __launch_bounds__(256) void layerscale_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ ls,
                                                             bf16_t* __restrict__ da, int rows, int cols, int rows_per) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 512 + lane * 8;
  const int r0 = blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
  if (c >= cols) return;
  float fl[8];
  unpack8(*reinterpret_cast<const uint4*>(ls + c), fl);
  for (int r = r0 + w; r < r1; r += 4) {
    float fd[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(dy + (long long)r * cols + c), fd);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = fd[k] * fl[k];
    *reinterpret_cast<uint4*>(da + (long long)r * cols + c) = pack8(o);
  }
}

// the same with dls in a fixed summation order (common.h, CR): one workgroup per column slice over all rows
template <int LPR>
__global__ __launch_bounds__(CR_THREADS) void layerscale_bwd_dls_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ a,
                                                                        const bf16_t* __restrict__ ls, bf16_t* __restrict__ da,
                                                                        float* __restrict__ dls, int rows, int cols) {
  __shared__ float sm[CR_THREADS / 64][64];
  const int c = CR<LPR>::col();
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < cols) {
    float fl[8];
    unpack8(*reinterpret_cast<const uint4*>(ls + c), fl);
    for (int r = CR<LPR>::row0(); r < rows; r += CR<LPR>::GROUPS) {
      float fd[8], fa[8], o[8];
      unpack8(*reinterpret_cast<const uint4*>(dy + (long long)r * cols + c), fd);
      unpack8(*reinterpret_cast<const uint4*>(a + (long long)r * cols + c), fa);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        o[k] = fd[k] * fl[k];
        acc[k] += fd[k] * fa[k];
      }
      *reinterpret_cast<uint4*>(da + (long long)r * cols + c) = pack8(o);
    }
  }
  CR<LPR>::add(acc, dls, cols, sm);
}

inline dim3 grid1d(long long n, int per) {
  long long b = (n + per - 1) / per;
  return dim3((unsigned)(b < 1 ? 1 : (b > 65535 * 8 ? 65535 * 8 : b)));
}

}  // namespace

extern "C" int vla_copy_rows3d(void* stream, const void* src, void* dst, int groups, int rows, int cols, long long src_group_stride,
                               long long src_row_stride, long long dst_group_stride, long long dst_row_stride) {
  VLA_REQUIRE(src && dst && groups > 0 && rows > 0 && cols > 0, "copy_rows3d: bad args");
  const bool vec = cols % 8 == 0 && src_group_stride % 8 == 0 && src_row_stride % 8 == 0 && dst_group_stride % 8 == 0 && dst_row_stride % 8 == 0 &&
                   ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)groups * rows * (vec ? cols / 8 : cols);
  if (vec)
    hipLaunchKernelGGL(copy_rows3d_kernel<true>, grid1d(total, 256), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, groups, rows, cols,
                       src_group_stride, src_row_stride, dst_group_stride, dst_row_stride);
  else
    hipLaunchKernelGGL(copy_rows3d_kernel<false>, grid1d(total, 256), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, groups, rows, cols,
                       src_group_stride, src_row_stride, dst_group_stride, dst_row_stride);
  VLA_CHECK_LAUNCH("copy_rows3d");
  return VLA_OK;
}

extern "C" int vla_layerscale_fwd(void* stream, const void* a, const void* ls, const void* x, void* out, long long rows, int cols) {
  VLA_REQUIRE(a && ls && x && out && rows > 0 && cols > 0 && cols % 8 == 0, "layerscale_fwd: cols must be a multiple of 8");
  VLA_REQUIRE(((((uintptr_t)a) | ((uintptr_t)ls) | ((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0, "layerscale_fwd: 16-B aligned contiguous tensors");
  hipLaunchKernelGGL(layerscale_fwd_kernel, grid1d(rows * (cols / 8), 256), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a, (const bf16_t*)ls,
                     (const bf16_t*)x, (bf16_t*)out, rows, cols / 8);
  VLA_CHECK_LAUNCH("layerscale_fwd");
  return VLA_OK;
}

extern "C" int vla_layerscale_bwd(void* stream, const void* dy, const void* a, const void* ls, void* da, float* dls, int rows, int cols) {
  VLA_REQUIRE(dy && ls && da && rows > 0 && cols > 0 && cols % 8 == 0 && (dls == nullptr || a != nullptr), "layerscale_bwd: bad args (cols % 8 == 0)");
  VLA_REQUIRE(((((uintptr_t)dy) | ((uintptr_t)ls) | ((uintptr_t)da) | ((uintptr_t)a)) & 15) == 0, "layerscale_bwd: 16-B aligned contiguous tensors");
  if (dls) {
    CR_LAUNCH(layerscale_bwd_dls_kernel, rows, cols, 1, stream, (const bf16_t*)dy, (const bf16_t*)a, (const bf16_t*)ls, (bf16_t*)da, dls,
              rows, cols);
    VLA_CHECK_LAUNCH("layerscale_bwd");
    return VLA_OK;
  }
  const int gx = (cols + 511) / 512;
  int gy = (rows + 63) / 64;
  if (gy > 1024) gy = 1024;
  const int rows_per = (rows + gy - 1) / gy;
  gy = (rows + rows_per - 1) / rows_per;
  hipLaunchKernelGGL(layerscale_bwd_kernel, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)ls,
                     (bf16_t*)da, rows, cols, rows_per);
  VLA_CHECK_LAUNCH("layerscale_bwd");
  return VLA_OK;
}
