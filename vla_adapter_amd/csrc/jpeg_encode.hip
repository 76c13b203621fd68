// The JPEG encoder where the frames are: raw frames -> complete baseline files, byte for byte Pillow's.  Declared in
// include/vla_jpeg_encode.h; DESIGN.md section 21.
//   stage 1   policy_forward_kernel<.., QUANT> (csrc/policy_image.hip through jpeg_stage_a.h): one wave per MCU -> the quantised values,
//             int16 in zigzag order, the MCUs in coding order
//   stage 2   encode_interval_kernel: one wave per restart interval.  The DC predictor of a block is coefficient 0 of the previous block
//             of its component, so a block's bits depend on no bitstream state: a lane codes one block (csrc/jpeg_encode_core.h:
//             code_block), the wave's prefix sum of the bit lengths gives every block its bit offset, and the lanes OR their codes into
//             a bit buffer in LDS (LDS atomics: two blocks may share a word).  Then the buffer's whole bytes leave 64 at a time, a lane
//             each; a ballot of the 0xFF bytes gives every lane the count of stuffed zeros in front of it.  An interval longer than 64
//             blocks takes several such rounds, the unfinished byte carried over.  The kernel runs twice: once without stores for the
//             interval's length (vla_jpeg_encode_plan), once with them (vla_jpeg_encode_write).
//   stage 3   encode_offsets_kernel: frame_off and every interval's offset, an exclusive prefix sum in one workgroup;
//             encode_markers_kernel: header, RSTn and EOI of every frame.
// Global memory: every byte of `out` is written by one thread, no atomics; nothing is allocated, read back or synchronised.
#include "common.h"
#include "jpeg_encode_core.h"
#include "jpeg_stage_a.h"
#include "../../include/vla_jpeg_encode.h"

namespace {

using namespace vlajpeg;

constexpr int ENC_LANES = 64;                   // one wave per workgroup
constexpr int CHUNK_BLOCKS = 64;                // blocks coded per round: one per lane
// The bit buffer of one round.  THE BOUND (jpeg_encode_core.h: MAX_BLOCK_BITS): a coded value is at most a 16-bit code and 11 extra
// bits, a block at most 64 of them = 1728 bits = 216 bytes, so 64 blocks and the 7 bits carried over from the round before end inside
// word 64 * 216 / 4 = 3456; an emission spans two words, and one more word of room makes 3460.  Stuffing happens behind the buffer,
// on the way out.  (Observed: noise at quality 100 stays under 90 bytes a block.)
constexpr int CHUNK_WORDS = CHUNK_BLOCKS * MAX_BLOCK_BYTES / 4 + 4;
constexpr int COEF_STRIDE = 66;                 // shorts between two blocks in LDS: 33 words, so the lanes' blocks start in 32 different banks
constexpr int OFF_THREADS = 256;

struct CountEmit {
  __device__ __forceinline__ void operator()(unsigned, int) {}
};

// ORs `n` bits at bit position `p` of the buffer (bit 0 = the most significant bit of word 0): at most two words.
struct LdsEmit {
  unsigned* bits;
  int p;
  __device__ __forceinline__ void operator()(unsigned v, int n) {
    const int word = p >> 5, sh = p & 31;
    if (n > 0 && word + 1 < CHUNK_WORDS) {              // (n + sh <= 27 + 31 < 64; the word check cannot fail inside THE BOUND)
      const u64 x = (u64)v << (64 - n - sh);
      atomicOr(&bits[word], (unsigned)(x >> 32));
      if ((unsigned)x) atomicOr(&bits[word + 1], (unsigned)x);
    }
    p += n;
  }
};

__device__ __forceinline__ unsigned buffer_byte(const unsigned* bits, int j) { return (bits[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu; }

// One wave per restart interval.  quant: stage 1's values; interval s = image s / I, interval s % I of it, `per` MCUs long (the last of
// an image may be shorter).  WRITE: the stuffed bytes go to out + seg_off[s] (bytes at or past out_bytes are dropped); else their
// count goes to seg_len[s].
template <bool WRITE>
__global__ void __launch_bounds__(ENC_LANES)
encode_interval_kernel(const short* __restrict__ quant, int I, int per, int n_mcu, int* __restrict__ seg_len, const i64* __restrict__ seg_off,
                       u8* __restrict__ out, i64 out_bytes) {
  __shared__ unsigned s_tab[ENC_TABLES][ENC_WORDS];
  __shared__ unsigned s_bits[CHUNK_WORDS];
  __shared__ alignas(16) short s_coef[CHUNK_BLOCKS * COEF_STRIDE];
  const int lane = threadIdx.x;
  if (lane < ENC_TABLES) derive_codes(lane, s_tab[lane]);
  const i64 s = blockIdx.x;
  const i64 img = s / I;
  const int m0 = (int)(s - img * I) * per, m1 = m0 + per < n_mcu ? m0 + per : n_mcu;
  const int n_blocks = (m1 - m0) * 6;
  const short* __restrict__ base = quant + (img * n_mcu + m0) * 384;
  i64 pos = WRITE ? seg_off[s] : 0;
  const i64 pos0 = pos;
  int carry_bits = 0;
  unsigned carry_byte = 0;
  __syncthreads();

  for (int b0 = 0; b0 < n_blocks; b0 += CHUNK_BLOCKS) {
    const int nb = n_blocks - b0 < CHUNK_BLOCKS ? n_blocks - b0 : CHUNK_BLOCKS;
    const bool last = b0 + CHUNK_BLOCKS >= n_blocks;
    for (int w = lane; w < CHUNK_WORDS; w += ENC_LANES) s_bits[w] = w == 0 ? carry_byte << 24 : 0u;
    for (int idx = lane; idx < nb * 8; idx += ENC_LANES) {        // the round's blocks, 16 bytes a lane
      const int blk = idx >> 3, part = idx & 7;
      const uint4 v = *reinterpret_cast<const uint4*>(base + (i64)(b0 + blk) * 64 + part * 8);
      unsigned* d = reinterpret_cast<unsigned*>(s_coef + blk * COEF_STRIDE + part * 8);
      d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    __syncthreads();

    // the bit length of every block, their prefix sum, the codes at their offsets
    const int b = b0 + lane;
    const bool live = lane < nb;
    const short* zz = s_coef + lane * COEF_STRIDE;
    const int chroma = live && b % 6 >= 4;
    const unsigned* dc = s_tab[chroma ? 2 : 0];
    const unsigned* ac = s_tab[chroma ? 3 : 1];
    int pred = 0, len = 0;
    if (live) {
      const int pb = predictor_block(b);
      pred = pb < 0 ? 0 : (int)base[(i64)pb * 64];
      CountEmit count;
      len = code_block(zz, pred, dc, ac, count);
    }
    int incl = len;
#pragma unroll
    for (int d = 1; d < ENC_LANES; d <<= 1) {
      const int t = __shfl_up(incl, d, ENC_LANES);
      if (lane >= d) incl += t;
    }
    const int total = carry_bits + __shfl(incl, ENC_LANES - 1, ENC_LANES);
    if (live) {
      LdsEmit emit{s_bits, carry_bits + incl - len};
      code_block(zz, pred, dc, ac, emit);
    }
    __syncthreads();

    // the whole bytes leave, the last round's unfinished byte padded with ones; a stuffed zero behind every 0xFF
    const int rem = total & 7;
    const int n_bytes = (total >> 3) + (last && rem ? 1 : 0);
    for (int j0 = 0; j0 < n_bytes; j0 += ENC_LANES) {
      const int j = j0 + lane;
      const bool has = j < n_bytes;
      unsigned byte = has ? buffer_byte(s_bits, j) : 0u;
      if (has && last && rem && j == n_bytes - 1) byte = pad_ones(byte, rem);
      const bool ff = has && byte == 0xFF;
      const u64 m = __ballot(ff);
      if (WRITE && has) {
        const i64 at = pos + lane + __popcll(m & ((1ull << lane) - 1ull));
        if (at >= 0 && at < out_bytes) out[at] = (u8)byte;
        if (ff && at + 1 >= 0 && at + 1 < out_bytes) out[at + 1] = 0;
      }
      pos += (n_bytes - j0 < ENC_LANES ? n_bytes - j0 : ENC_LANES) + __popcll(m);
    }
    carry_bits = last ? 0 : rem;
    carry_byte = carry_bits ? buffer_byte(s_bits, total >> 3) : 0u;
    __syncthreads();
  }
  if (!WRITE && lane == 0) seg_len[s] = (int)(pos - pos0);
}

// frame_off [N + 1] and seg_off [N * I] from seg_len [N * I]: a frame is its header, its intervals with two bytes of RSTn between
// them, and two bytes of EOI.  One workgroup walks the frames OFF_THREADS at a time.
__global__ void __launch_bounds__(OFF_THREADS)
encode_offsets_kernel(const int* __restrict__ seg_len, i64 N, int I, i64* __restrict__ seg_off, i64* __restrict__ frame_off) {
  __shared__ i64 s_scan[OFF_THREADS];
  const int tid = threadIdx.x;
  i64 carry = 0;
  for (i64 n0 = 0; n0 < N; n0 += OFF_THREADS) {
    const i64 n = n0 + tid;
    i64 size = 0;
    if (n < N) {
      size = HEADER_BYTES + 2 * (I - 1) + 2;
      for (int i = 0; i < I; ++i) size += seg_len[n * I + i];
    }
    s_scan[tid] = size;
    __syncthreads();
    for (int d = 1; d < OFF_THREADS; d <<= 1) {
      const i64 t = tid >= d ? s_scan[tid - d] : 0;
      __syncthreads();
      s_scan[tid] += t;
      __syncthreads();
    }
    if (n < N) {
      i64 run = carry + s_scan[tid] - size;
      frame_off[n] = run;
      run += HEADER_BYTES;
      for (int i = 0; i < I; ++i) {
        if (i) run += 2;
        seg_off[n * I + i] = run;
        run += seg_len[n * I + i];
      }
    }
    carry += s_scan[OFF_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) frame_off[N] = carry;
}

// Header, RSTn markers and EOI of frame blockIdx.x; a byte at or past out_bytes is dropped.
__global__ void __launch_bounds__(ENC_LANES)
encode_markers_kernel(int H, int W, const unsigned short* __restrict__ qtab, int restart_rows, int I, const i64* __restrict__ seg_off,
                      const i64* __restrict__ frame_off, u8* __restrict__ out, i64 out_bytes) {
  __shared__ u8 s_hdr[HEADER_BYTES + 3];
  const int lane = threadIdx.x;
  if (lane == 0) write_header(s_hdr, H, W, qtab, restart_rows);
  __syncthreads();
  const i64 n = blockIdx.x, off = frame_off[n], end = frame_off[n + 1];
  auto store = [&](i64 at, unsigned b) {
    if (at >= 0 && at < out_bytes) out[at] = (u8)b;
  };
  for (int j = lane; j < HEADER_BYTES; j += ENC_LANES) store(off + j, s_hdr[j]);
  for (int i = 1 + lane; i < I; i += ENC_LANES) {
    const i64 p = seg_off[n * I + i];
    store(p - 2, 0xFF);
    store(p - 1, restart_marker(i));
  }
  if (lane == 0) {
    store(end - 2, 0xFF);
    store(end - 1, 0xD9);
  }
}

bool shape_ok(long long N, int H, int W, int restart_rows) { return N >= 1 && N <= (1 << 20) && encode_shape_ok(H, W, restart_rows); }

struct Layout {
  long long coef_bytes, intervals, total;
};
Layout layout_of(long long N, int H, int W, int restart_rows) {
  Layout l;
  l.coef_bytes = N * (long long)H * W * 3;              // 1.5 int16 values a pixel; a multiple of 16, since H * W is one of 256
  l.intervals = N * intervals_per_image(H, restart_rows);
  l.total = l.coef_bytes + l.intervals * 12;
  return l;
}

}  // namespace

extern "C" long long vla_jpeg_encode_workspace_bytes(long long N, int H, int W, int restart_rows) {
  if (!shape_ok(N, H, W, restart_rows)) return -1;
  return layout_of(N, H, W, restart_rows).total;
}

extern "C" int vla_jpeg_encode_plan(void* stream, const unsigned char* frames, long long in_stride, long long N, int H, int W,
                                    const unsigned short* qtab, int restart_rows, void* workspace, long long workspace_bytes,
                                    long long* frame_off) {
  VLA_REQUIRE(frames && qtab && workspace && frame_off, "jpeg_encode_plan: null pointer");
  VLA_REQUIRE(shape_ok(N, H, W, restart_rows),
              "jpeg_encode_plan: H and W must be multiples of 16 inside [16, 4096], 1 <= N <= 2^20, restart_rows >= 1 with at most 65535 MCUs "
              "an interval (a file without restart markers is coded serially: left to the host)");
  VLA_REQUIRE(in_stride >= (long long)H * W * 3, "jpeg_encode_plan: in_stride must be at least H * W * 3");
  const Layout l = layout_of(N, H, W, restart_rows);
  VLA_REQUIRE((uintptr_t)workspace % 16 == 0 && workspace_bytes >= l.total,
              "jpeg_encode_plan: workspace must be 16-byte aligned and hold vla_jpeg_encode_workspace_bytes");
  VLA_REQUIRE((uintptr_t)frame_off % 8 == 0, "jpeg_encode_plan: frame_off must be 8-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  short* quant = (short*)workspace;
  i64* seg_off = (i64*)((unsigned char*)workspace + l.coef_bytes);
  int* seg_len = (int*)(seg_off + l.intervals);
  const int rc = stage_a_quantised(st, frames, in_stride, N, H, W, qtab, quant);
  if (rc != VLA_OK) return rc;
  const int I = intervals_per_image(H, restart_rows);
  hipLaunchKernelGGL(encode_interval_kernel<false>, dim3((unsigned)l.intervals), dim3(ENC_LANES), 0, st, quant, I, restart_rows * (W >> 4),
                     mcus_per_image(H, W, 1), seg_len, (const i64*)nullptr, (u8*)nullptr, (i64)0);
  VLA_CHECK_LAUNCH("jpeg_encode_plan (lengths)");
  hipLaunchKernelGGL(encode_offsets_kernel, dim3(1), dim3(OFF_THREADS), 0, st, seg_len, (i64)N, I, seg_off, (i64*)frame_off);
  VLA_CHECK_LAUNCH("jpeg_encode_plan (offsets)");
  return VLA_OK;
}

extern "C" int vla_jpeg_encode_write(void* stream, long long N, int H, int W, const unsigned short* qtab, int restart_rows,
                                     const void* workspace, long long workspace_bytes, const long long* frame_off, unsigned char* out,
                                     long long out_bytes) {
  VLA_REQUIRE(qtab && workspace && frame_off && out, "jpeg_encode_write: null pointer");
  VLA_REQUIRE(shape_ok(N, H, W, restart_rows), "jpeg_encode_write: the shape vla_jpeg_encode_plan refuses");
  const Layout l = layout_of(N, H, W, restart_rows);
  VLA_REQUIRE((uintptr_t)workspace % 16 == 0 && workspace_bytes >= l.total,
              "jpeg_encode_write: workspace must be 16-byte aligned and hold vla_jpeg_encode_workspace_bytes");
  VLA_REQUIRE((uintptr_t)frame_off % 8 == 0 && out_bytes >= 1, "jpeg_encode_write: frame_off must be 8-byte aligned, out_bytes >= 1");
  const hipStream_t st = (hipStream_t)stream;
  const short* quant = (const short*)workspace;
  const i64* seg_off = (const i64*)((const unsigned char*)workspace + l.coef_bytes);
  const int I = intervals_per_image(H, restart_rows);
  hipLaunchKernelGGL(encode_markers_kernel, dim3((unsigned)N), dim3(ENC_LANES), 0, st, H, W, qtab, restart_rows, I, seg_off,
                     (const i64*)frame_off, out, (i64)out_bytes);
  VLA_CHECK_LAUNCH("jpeg_encode_write (markers)");
  hipLaunchKernelGGL(encode_interval_kernel<true>, dim3((unsigned)l.intervals), dim3(ENC_LANES), 0, st, quant, I, restart_rows * (W >> 4),
                     mcus_per_image(H, W, 1), (int*)nullptr, seg_off, out, (i64)out_bytes);
  VLA_CHECK_LAUNCH("jpeg_encode_write (intervals)");
  return VLA_OK;
}
