// bf16 NT GEMM for gfx950:  C[M,N] = epilogue(A[M,K] . B[N,K]^T)   (both operands K-contiguous, the
// nn.Linear layout; fp32 accumulation on v_mfma_f32_16x16x32_bf16).
//
// Replaces every cuBLAS call the reference reaches through nn.Linear: timm ViT qkv/proj/fc1/fc2,
// PrismaticProjector (modeling_prismatic.py:261-273), Qwen2 q/k/v/o/gate/up/down, the action head's Linears
// (action_heads.py:337-410), and - with pre-transposed operands - their dX / dW products.
//
// Structure (cdna_hip_programming.md section 5):
//   * block tile BM x BN x 64 with (BM/64) x 2 waves, each wave a 64 x (BN/2) sub-tile of 16x16 MFMA tiles;
//   * A/B tiles stream HBM->LDS with global_load_lds_dwordx4 (1 KiB per wave-instruction) into a ring of STAGES
//     buffers; the LDS image is linear with the 16-B-chunk XOR swizzle applied on the SOURCE address and on the
//     fragment read (rule 21);
//   * ONE raw s_barrier per K-tile; with STAGES=3 the loads run TWO K-tiles ahead and the loop waits with a COUNTED
//     s_waitcnt vmcnt(pieces-per-stage) - never vmcnt(0) inside the loop ("Pipelining across barriers"): a tile's
//     pieces are retired by every wave's own counted wait, the barrier then publishes them to the other waves and
//     proves every wave has finished reading the buffer that the next stage overwrites;
//   * operands are swapped at the MFMA (A-operand := B rows) so each lane owns 4 consecutive n of one row m: the
//     epilogue stages the wave's tile through LDS and stores whole row segments with 16-B lanes;
//   * XCD-aware bijective tile order (T1).
// Tiles: 128x128 (8 waves, 2 stages, 2 blocks/CU), 128x64 (4 waves, 2 stages, 48 KiB, 3 blocks/CU) and, under the latency hint,
// 128x128 on a four-stage and 64x128 on a six-stage ring; large products go to gemm256.hip, small outputs to gemm_skinny.hip.
// plan_nt below picks one per call.
//
// Epilogue rounding points follow the reference under bf16 autocast: bf16(acc+bias) -> act -> bf16 -> (+residual) -> bf16.
#include <algorithm>
#include "gemm_epilogue.h"
#include "gemm_params.h"

namespace {

constexpr int BK = 64;
constexpr int EPI_PAD = 16;  // bytes of padding per staged epilogue row (keeps 16-B alignment, spreads banks)

// Per-element activation of the split-K finalize pass, on the ROUNDED linear value: the Act* functors of gemm_epilogue.h with the
// roundings written out (open-coded: dispatched through epi_with_act, splitk_finalize_kernel's SGPR count moves)
__device__ __forceinline__ float apply_act(float v, int act) {
  switch (act) {
    case VLA_ACT_GELU: return rbf(gelu_erf(v));
    case VLA_ACT_RELU: return fmaxf(v, 0.f);
    case VLA_ACT_GELU_TANH: return rbf(gelu_tanh(v));
    default: return v;
  }
}

template <int BM, int BN, int STAGES, int WN = 2>
struct Cfg {
  static constexpr int NW = (BM / 64) * WN;              // waves: (BM/64) along M x WN along N
  static constexpr int NTHREADS = NW * 64;
  static constexpr int WTN = BN / WN;                    // wave tile: 64 x WTN
  static constexpr int NT = WTN / 16;                    // 16-wide n tiles per wave (4 or 2)
  static constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  static constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  static constexpr int PIECES = STAGE_BYTES / 1024;      // 1 KiB LDS-DMA pieces per stage
  static constexpr int PPW = PIECES / NW;                // pieces per wave per stage
  static constexpr int EPI_STRIDE = WTN * 2 + EPI_PAD;   // bytes per staged output row
  static constexpr int LDS_BYTES = STAGES * STAGE_BYTES;
  static constexpr int NHALF = NW * 64 * EPI_STRIDE <= LDS_BYTES ? 1 : 2;   // output staged in 1 or 2 row-halves per wave
  static constexpr int EPI_ROWS = 64 / NHALF;
  static constexpr int EPI_BYTES = NW * EPI_ROWS * EPI_STRIDE;
  static_assert(EPI_BYTES <= LDS_BYTES, "epilogue staging must fit the operand ring");
  static_assert(PIECES % NW == 0, "pieces must divide evenly over the waves");
};

// ROPE is a compile-time switch (0 none / 1 rotate_half / 2 interleaved): the epilogue's extra registers and table
// loads must not leak into the plain kernel that every other GEMM of the step runs.
// F8: operands are OCP e4m3 bytes with per-row fp32 scales (p.scaleA[m], p.scaleB[n]); a K-tile is still 128 B per row = 128
// elements = ONE v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16 tile (unit block scales): the same bytes moved, the same LDS
// reads and the same MFMA cycles per K-tile as the bf16 form, at twice the FLOPs (lane l holds row l % 16, k = 32 (l / 16) +
// byte: tools/probe_f8.py).  The scales are applied to the fp32 accumulator before anything else of the epilogue.
// EXT: K extension - the contraction continues over a second operand pair, C = epilogue(A . B^T + A2 . B2^T) with A2 [M, K2]
// (lda2) and B2 [N, K2] (ldb2): K-tiles [0, K / 64) stream from (A, B), the rest from (A2, B2), one accumulator, one rounding.
// This is how a LoRA-wrapped Linear runs (vla-scripts/finetune.py:832-844): y = x W^T + (2 x A^T) B^T with the low-rank
// branch inside the base GEMM's fp32 accumulator - the base product keeps its bias / RoPE / SwiGLU epilogue and no
// read-modify-write pass over y exists (backward alike: dx = dy W + dt A).
template <int BM, int BN, int STAGES, int ROPE, int WN = 2, bool F8 = false, bool EXT = false>
__global__ __launch_bounds__((BM / 64) * 64 * WN) __attribute__((amdgpu_waves_per_eu((F8 && EXT) ? 4 : 1)))   // (fp8 + extension: two
void gemm_nt_kernel(GemmP p) {                                   //  workgroups per CU like every other form: 128 registers, no spill)
  using C = Cfg<BM, BN, STAGES, WN>;
  constexpr int EB = F8 ? 1 : 2;                           // bytes per operand element
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid / WN, wc = wid - wr * WN;

  const int swz = xcd_order(blockIdx.x, p.ntiles);         // every XCD a contiguous run of tiles
  // group-M order inside the XCD's run: GM row-panels x all column tiles, row index fastest, so the ~32-64 tiles an
  // XCD has in flight form a GM x (32/GM) patch whose A panels stay in that XCD's 4 MiB L2 while B tiles stream once
  // (row-major order re-streamed every B tile from beyond L2 for every row panel: 44 x 17 MB for the gate/up GEMM).
  // 6 for the 128-row tiles: in the two/three-stream step the XCD's L2 is shared with the other streams' kernels and the
  // smaller patch wins (same-box sweep: 8 -> 31.55 ms/step, 6 -> 30.85, 5 -> 30.8, 4 -> 31.0, 3 -> 30.85, 12 -> 32.3;
  // isolated launches are indifferent between 4 and 8).
  constexpr int GM = 6;                                    // A panels kept L2-resident per XCD
  const int tiles_m = p.ntiles / p.tiles_n, per_group = GM * p.tiles_n;
  const int grp = swz / per_group, rem = swz - grp * per_group;
  const int gm = min(GM, tiles_m - grp * GM);
  const int bm = grp * GM + rem % gm, bn = rem / gm;
  const int m0 = bm * BM, n0 = bn * BN;
  const int z = blockIdx.z;
  const char* Ab = reinterpret_cast<const char*>(p.A) + (long long)z * p.sA * EB;
  const char* Bb = reinterpret_cast<const char*>(p.B) + (long long)z * p.sB * EB;

  // ---- staging: piece pc (1 KiB = 8 LDS rows) of a stage; pieces [0, BM/8) are A rows, the rest B rows.
  //      lane -> row 8pc + (lane>>3); LDS chunk lane&7 holds global chunk (lane&7) ^ (row&7)
  const int kc = ((lane & 7) ^ ((lane >> 3) & 7)) * 16;      // bytes
  const char* pp[C::PPW];
#pragma unroll
  for (int i = 0; i < C::PPW; ++i) {
    const int pc = wid * C::PPW + i;                      // wave-uniform
    if (pc < BM / 8) {
      const int ra = min(m0 + pc * 8 + (lane >> 3), p.M - 1);
      pp[i] = Ab + grouped_row(ra, p.gA, p.sgA, p.lda) * EB + kc;
    } else {
      const int rb = min(n0 + (pc - BM / 8) * 8 + (lane >> 3), p.N - 1);
      pp[i] = Bb + (long long)rb * p.ldb * EB + kc;
    }
  }
  const char* pp2[EXT ? C::PPW : 1];
  if constexpr (EXT) {
#pragma unroll
    for (int i = 0; i < C::PPW; ++i) {
      const int pc = wid * C::PPW + i;
      if (pc < BM / 8) pp2[i] = reinterpret_cast<const char*>(p.A2) + (long long)min(m0 + pc * 8 + (lane >> 3), p.M - 1) * p.lda2 * 2 + kc;
      else pp2[i] = reinterpret_cast<const char*>(p.B2) + (long long)min(n0 + (pc - BM / 8) * 8 + (lane >> 3), p.N - 1) * p.ldb2 * 2 + kc;
    }
  }
  // (split-K: slice z owns p.K of the contraction - the last slice what is left of p.Ktot when the slices are uneven)
  const int nt1 = (p.Ktot > 0 ? min(p.K, p.Ktot - z * p.K) : p.K) / (F8 ? 2 * BK : BK);        // K-tiles of 128 B per row from (A, B)
  auto stage = [&](int buf, int t) {               // K-tile t: 128 B further along every row per tile
    char* base = smem + buf * C::STAGE_BYTES + wid * C::PPW * 1024;
    if (EXT && t >= nt1) {
#pragma unroll
      for (int i = 0; i < C::PPW; ++i) glds16(pp2[i] + (t - nt1) * 128, base + i * 1024);
    } else {
#pragma unroll
      for (int i = 0; i < C::PPW; ++i) glds16(pp[i] + t * 128, base + i * 1024);
    }
  };

  f32x4 acc[C::NT][4];  // [ni][mi]
#pragma unroll
  for (int a = 0; a < C::NT; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (bytes) inside an operand tile, per k-step s: row*128 + ((4s + (lane>>4)) ^ (lane&7))*16
  const int frow = lane & 15;
  int foff[2], foff2[2];                      // foff2: the bf16 K-extension tiles of an fp8 product (F8 && EXT)
#pragma unroll
  for (int s = 0; s < 2; ++s) {               // (fp8: the lane's 32 contiguous bytes = chunks 2q and 2q + 1, q = lane >> 4)
    foff[s] = frow * 128 + (((F8 ? 2 * (lane >> 4) + s : 4 * s + (lane >> 4)) ^ (lane & 7)) << 4);
    foff2[s] = frow * 128 + (((4 * s + (lane >> 4)) ^ (lane & 7)) << 4);
  }

  // epilogue coordinates: lane owns, for tile (ni, mi): m = 16mi + (lane&15), n = 16ni + 4(lane>>4) + {0..3}.
  // The bias slice is fetched HERE (one 8-B load per n-tile) so its latency hides under the main loop; fetched in the
  // epilogue it cost a dependent global load per element right on every tile's tail.
  const int wm0 = m0 + wr * 64, wn0 = n0 + wc * C::WTN;
  const int lq = lane >> 4, lr = lane & 15;
  // Tile-local first column of this wave's 16-wide n tile ni.  Plain: WTN consecutive columns.  Fused rotate_half on the
  // 8-wave geometry (32 columns per wave, head dim 64): the wave owns 16 columns of EACH half of one head, so that the
  // rotation partners d <-> d + 32 are n tiles 0 and 1 of the same lane (no exchange between waves).
  // Head dim 128 (Qwen2.5-1.5B, round 4): the tile's 128 columns are ONE head, the halves are columns [0, 64) and [64, 128): wave wc owns
  // 16 columns of each (n tile 0: 16 wc .., n tile 1: 64 + 16 wc ..) - the same lane-local rotation, another column map.
  constexpr bool PERM = ROPE == 1 && C::NT == 2;
  const bool wide = PERM && p.rope_dh == 128;          // (wave-uniform)
  auto cbase = [&](int ni) { return PERM ? (wide ? ni * 64 + wc * 16 : (wc >> 1) * 64 + ni * 32 + (wc & 1) * 16) : wc * C::WTN + ni * 16; };
  const bf16_t* bias = p.bias ? p.bias + (long long)z * p.sBias : nullptr;
  float bv[C::NT][4];
  {
    const bool bvec = bias && (((size_t)bias & 7) == 0);
#pragma unroll
    for (int ni = 0; ni < C::NT; ++ni) {
      const int n = n0 + cbase(ni) + lq * 4;
      if (bvec && n + 3 < p.N) {
        const uint2 b2 = *reinterpret_cast<const uint2*>(bias + n);
        bv[ni][0] = bf_lo(b2.x); bv[ni][1] = bf_hi(b2.x);
        bv[ni][2] = bf_lo(b2.y); bv[ni][3] = bf_hi(b2.y);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[ni][j] = (bias && n + j < p.N) ? bf2f(bias[n + j]) : 0.f;
      }
    }
  }

  // (fp8 base product with a bf16 K extension - a LoRA-wrapped Linear on e4m3 base operands: the dequantisation scales are applied
  //  to the accumulator BETWEEN the two contractions, so the low-rank branch adds to the dequantised base product)
  const int nt = nt1 + (EXT ? p.K2 / BK : 0);
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nt) stage(s, s);
  int buf = 0;
  static_assert(C::NT <= 4, "wave tiles are 64 x 32 or 64 x 64");
  static_assert(STAGES >= 2 && STAGES <= 6 && 4 * C::PPW < 64, "the counted waits below cover rings of 2 to 6 stages (vmcnt is a 6-bit counter)");
  // One K-tile (written as a macro so that the fp8 product with a bf16 extension can run it as TWO loops - e4m3 tiles, then bf16
  // tiles - each with one MFMA form and one set of fragment offsets: as one loop with a per-tile branch the kernel needed 200
  // registers and lost its second resident workgroup).  All fragment reads of the K-tile (both 32-deep k-steps) are issued up
  // front: the second k-step's LDS latency hides under the first k-step's MFMAs instead of stalling between them.
#define VLA_KTILE(F8T, FO)                                                                                                           \
  do {                                                                                                                               \
    /* retire this wave's pieces of tile t; up to STAGES-2 younger tiles stay in flight (in-order return: a counted wait) */       \
    if (STAGES >= 6 && t + 4 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * C::PPW) : "memory");                                  \
    else if (STAGES >= 5 && t + 3 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * C::PPW) : "memory");                             \
    else if (STAGES >= 4 && t + 2 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * C::PPW) : "memory");                             \
    else if (STAGES >= 3 && t + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::PPW) : "memory");                                 \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                            \
    __builtin_amdgcn_s_barrier(); /* tile t visible to every wave; every wave is done reading tile t-1's buffer */                    \
    asm volatile("" ::: "memory");                                                                                                   \
    if (t + STAGES - 1 < nt) {                                                                                                       \
      int nb = buf + STAGES - 1;                                                                                                     \
      if (nb >= STAGES) nb -= STAGES;                                                                                                \
      stage(nb, t + STAGES - 1);                                                                                                     \
    }                                                                                                                                \
    const char* sa = smem + buf * C::STAGE_BYTES + wr * 64 * 128;                                                                    \
    const char* sb = smem + buf * C::STAGE_BYTES + C::A_BYTES; /* B tile; n tile i of this wave starts at row cbase(i) */             \
    bf16x8 fm[2][4], fn[2][C::NT];                                                                                                   \
    _Pragma("unroll") for (int s = 0; s < 2; ++s) {                                                                                  \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) fm[s][i] = *reinterpret_cast<const bf16x8*>(sa + i * 16 * 128 + FO[s]);          \
      _Pragma("unroll") for (int i = 0; i < C::NT; ++i) fn[s][i] = *reinterpret_cast<const bf16x8*>(sb + cbase(i) * 128 + FO[s]);    \
    }                                                                                                                                \
    if constexpr (F8T) {                                                                                                             \
      _Pragma("unroll") for (int ni = 0; ni < C::NT; ++ni)                                                                           \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                                             \
          acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(cat8(fn[0][ni], fn[1][ni]), cat8(fm[0][mi], fm[1][mi]),     \
                                                                         acc[ni][mi], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);            \
    } else {                                                                                                                         \
      _Pragma("unroll") for (int s = 0; s < 2; ++s)                                                                                  \
        _Pragma("unroll") for (int ni = 0; ni < C::NT; ++ni)                                                                         \
          _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                                           \
            acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fn[s][ni], fm[s][mi], acc[ni][mi], 0, 0, 0);                       \
    }                                                                                                                                \
    if (++buf == STAGES) buf = 0;                                                                                                    \
  } while (0)
  if constexpr (F8 && EXT) {
    for (int t = 0; t < nt1; ++t) VLA_KTILE(true, foff);
    // dequantisation of the base product, then the bf16 extension adds to it
    {
      float fsa[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) fsa[mi] = p.scaleA[min(wm0 + mi * 16 + lr, p.M - 1)];
#pragma unroll
      for (int ni = 0; ni < C::NT; ++ni)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float sbv = p.scaleB[min(n0 + cbase(ni) + lq * 4 + j, p.N - 1)];
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) acc[ni][mi][j] *= fsa[mi] * sbv;
        }
    }
    for (int t = nt1; t < nt; ++t) VLA_KTILE(false, foff2);
  } else {
    for (int t = 0; t < nt; ++t) VLA_KTILE(F8, foff);
  }
#undef VLA_KTILE
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // all waves done with the operand tiles before the staging regions are overwritten
  asm volatile("" ::: "memory");

  // ---------------- epilogue ----------------
  if constexpr (F8 && !EXT) {
    // dequantisation: acc[m][n] *= scaleA[m] * scaleB[n] (fp32, before alpha / bias / activation)
    float sa[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) sa[mi] = p.scaleA[min(wm0 + mi * 16 + lr, p.M - 1)];
#pragma unroll
    for (int ni = 0; ni < C::NT; ++ni) {
      const int n = n0 + cbase(ni) + lq * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float sbv = p.scaleB[min(n + j, p.N - 1)];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi][j] *= sa[mi] * sbv;
      }
    }
  }
  if (ROPE == 0 && p.ws != nullptr) {
    // split-K slice z: park the raw accumulators in its own fp32 plane ws[z][M][N] (plain 16-B stores; fp32 atomics into one
    // plane were throughput-bound: 4 M atomics per GEMM); the planes are summed and bias / activation / residual / bf16
    // rounding applied once, in splitk_finalize_kernel.  (Few-tile long-K problems are otherwise one serial K loop.)
    float* plane = p.ws + (long long)z * p.M * p.N;
#pragma unroll
    for (int ni = 0; ni < C::NT; ++ni)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int m = wm0 + mi * 16 + lr, n = wn0 + ni * 16 + lq * 4;
        if (m < p.M && n + 3 < p.N)
          *reinterpret_cast<f32x4*>(plane + (long long)m * p.N + n) = acc[ni][mi];
      }
    return;
  }
  char* reg = smem + wid * (C::EPI_ROWS * C::EPI_STRIDE);

  if (ROPE == 3) {
    // ---- SwiGLU backward fused into the dH = dY.W_down GEMM (VLA_ACT_SWIGLU_BWD): the accumulator holds dH for this
    // wave's 64 x 64 patch; read the matching interleaved pre-activations GU[m, 2I], emit dGU in the same layout.
    // dH is never written (saves a 110 MB write + read per layer) and the stand-alone pass (548 MB of traffic) is gone.
    const bf16_t* GU = p.R + (long long)z * p.sR;          // aux input rides in the residual slot, row stride ldr
    bf16_t* Cb = p.C + (long long)z * p.sC;
    constexpr int ROWB = 2 * C::WTN * 2 + 16;              // staged row: 2*WTN bf16 (+16 B pad)
    constexpr int CH2 = 2 * C::WTN / 8, RPP2 = 64 / CH2;   // 16-B chunks per staged row, rows per pass
    constexpr int NIT = 32 / RPP2;                         // passes per 32-row half
    char* reg2 = smem + wid * (32 * ROWB);
    if (wn0 >= p.N || wm0 >= p.M) return;                  // (N % 64 == 0: a wave's WTN h-columns are all inside or all outside)
    // The pre-activations of the wave's patch arrive the way its results leave: whole 16-B row segments, ALL requested before
    // the first is used (row clamped, no per-element condition), staged in the wave's LDS region and overwritten IN PLACE by dGU
    // (same interleaved layout).  The former per-lane 8-B gathers (16 rows x 32 B per load instruction, each behind its own
    // bounds branch and wait) made this epilogue as long as the K loop of the live-row backward's M = 2048 GEMM.
    u32x4 gin[2][NIT];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int row = it * RPP2 + lane / CH2, ch = lane % CH2;
        const int m = min(wm0 + half * 32 + row, p.M - 1);
        gin[half][it] = *reinterpret_cast<const u32x4*>(GU + grouped_row(m, p.gR, p.sgR, p.ldr) + 2 * wn0 + ch * 8);
      }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int row = it * RPP2 + lane / CH2, ch = lane % CH2;
        *reinterpret_cast<u32x4*>(reg2 + row * ROWB + ch * 16) = gin[half][it];
      }
#pragma unroll
      for (int mh = 0; mh < 2; ++mh) {
        const int mi = 2 * half + mh;
#pragma unroll
        for (int ni = 0; ni < C::NT; ++ni) {
          char* rowp = reg2 + (mh * 16 + lr) * ROWB + (ni * 32 + lq * 4) * 2;
          float gg[4], uu[4], dg[4], du[4];
          unpack4(*reinterpret_cast<const uint2*>(rowp), gg);
          unpack4(*reinterpret_cast<const uint2*>(rowp + 32), uu);
#pragma unroll
          for (int j = 0; j < 4; ++j) swiglu_bwd(rbf(acc[ni][mi][j] * p.alpha), gg[j], uu[j], dg[j], du[j]);
          *reinterpret_cast<uint2*>(rowp) = pack4(dg);
          *reinterpret_cast<uint2*>(rowp + 32) = pack4(du);
        }
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int row = it * RPP2 + lane / CH2, ch = lane % CH2;
        const int m = wm0 + half * 32 + row, n2 = 2 * wn0 + ch * 8;
        if (m < p.M)
          *reinterpret_cast<uint4*>(Cb + (long long)m * p.ldc + n2) = *reinterpret_cast<const uint4*>(reg2 + row * ROWB + ch * 16);
      }
    }
    return;
  }
  if (p.act == VLA_ACT_SWIGLU) {
    // columns interleaved in 16s: even tiles are gate, odd tiles the matching up columns
    bf16_t* C2 = p.C2 + (long long)z * p.sC2;
#pragma unroll
    for (int pr = 0; pr < C::NT / 2; ++pr)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int m = wm0 + mi * 16 + lr;
        float h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float g = rbf(epi_linear(acc[2 * pr][mi][j], p.alpha, bv[2 * pr][j]));
          const float u = rbf(epi_linear(acc[2 * pr + 1][mi][j], p.alpha, bv[2 * pr + 1][j]));
          acc[2 * pr][mi][j] = g;
          acc[2 * pr + 1][mi][j] = u;
          h[j] = swiglu_h(g, u);
        }
        const int hc = (wn0 >> 1) + pr * 16 + lq * 4;
        if (m < p.M && hc + 3 < (p.N >> 1)) *reinterpret_cast<uint2*>(C2 + (long long)m * p.ldc2 + hc) = pack4(h);
      }
    if (p.C == nullptr) return;
  } else {
    // alpha, bias, activation (gemm_epilogue.h; the activation's own bf16 rounding is the pack into the staging tile below)
    float alpha = p.alpha;
    if (p.bias_post) {                        // epi_linear<true>, its rounding taken in a pass of its own
#pragma unroll
      for (int ni = 0; ni < C::NT; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ni][mi][j] = rbf(acc[ni][mi][j] * alpha);
      alpha = 1.f;
    }
    auto finish = [&](auto fn) {
#pragma unroll
      for (int ni = 0; ni < C::NT; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ni][mi][j] = fn(epi_linear(acc[ni][mi][j], alpha, bv[ni][j]));
    };
    epi_with_act(p.act, finish);
    // ---- fused rotary embedding on the projected q/k columns (saves a full read+write pass per projection)
    if (ROPE != 0 && n0 + cbase(0) < p.rope_cols) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int pos = min(wm0 + mi * 16 + lr, p.M - 1) % p.rope_T;
        if (ROPE == 2) {
          // interleaved: the partners are neighbours inside the lane's four columns
#pragma unroll
          for (int ni = 0; ni < C::NT; ++ni) {
            const int d = (wn0 + ni * 16 + lq * 4) % p.rope_dh;
            const float4 c = *reinterpret_cast<const float4*>(p.rope_cos + (long long)pos * p.rope_dh + d);
            const float4 sn = *reinterpret_cast<const float4*>(p.rope_sin + (long long)pos * p.rope_dh + d);
            const float x0 = rbf(acc[ni][mi][0]), x1 = rbf(acc[ni][mi][1]), x2 = rbf(acc[ni][mi][2]), x3 = rbf(acc[ni][mi][3]);
            acc[ni][mi][0] = rope_rot_a(x0, x1, c.x, sn.x);
            acc[ni][mi][1] = rope_rot_b(x0, x1, c.y, sn.y);
            acc[ni][mi][2] = rope_rot_a(x2, x3, c.z, sn.z);
            acc[ni][mi][3] = rope_rot_b(x2, x3, c.w, sn.w);
          }
        } else if (ROPE == 1 && C::NT == 4) {
          // HF rotate_half, head dim 64 == this wave's 64 columns: d <-> d+32 are tiles ni and ni+2 of the same lane
          const int half = p.rope_dh >> 1;
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const int d = ni * 16 + lq * 4;
            const f32x4 c = *reinterpret_cast<const f32x4*>(p.rope_cos + (long long)pos * half + d);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(p.rope_sin + (long long)pos * half + d);
            rope_half<4>(acc[ni][mi], acc[ni + 2][mi], c, sn);
          }
        } else if (ROPE == 1 && C::NT == 2) {
          // same rotation on the permuted 8-wave layout: n tile 0 holds head columns d = 16 (wc & 1) + 4 lq + j, tile 1 d + 32
          const int half = p.rope_dh >> 1, d = (wide ? wc * 16 : (wc & 1) * 16) + lq * 4;
          const f32x4 c = *reinterpret_cast<const f32x4*>(p.rope_cos + (long long)pos * half + d);
          const f32x4 sn = *reinterpret_cast<const f32x4*>(p.rope_sin + (long long)pos * half + d);
          rope_half<4>(acc[0][mi], acc[1][mi], c, sn);
        }
      }
    }
  }

  // stage the wave's 64 x WTN tile (bf16) through its private LDS region (NHALF passes), then store 16 B per lane
  bf16_t* Cb = p.C + (long long)z * p.sC;
  const bf16_t* Rb = p.R ? p.R + (long long)z * p.sR : nullptr;
  const bool vec_ok = ((p.ldc & 7) == 0) && (!Rb || (p.ldr & 7) == 0);
  constexpr int CH = C::WTN / 8;        // 16-B chunks per staged row
  constexpr int RPP = 64 / CH;          // rows per pass
  constexpr int MIH = 4 / C::NHALF;     // 16-row m tiles per half
#pragma unroll
  for (int half = 0; half < C::NHALF; ++half) {
#pragma unroll
    for (int ni = 0; ni < C::NT; ++ni)
#pragma unroll
      for (int mh = 0; mh < MIH; ++mh) {
        const int mi = half * MIH + mh;
        *reinterpret_cast<uint2*>(reg + (mh * 16 + lr) * C::EPI_STRIDE + (ni * 16 + lq * 4) * 2) = pack4(acc[ni][mi]);
      }
    // The common case - the wave's rows and columns all inside C, 16-B aligned rows, plain row addressing - without a branch
    // per row segment, the residual segments all requested before the first is added (as in gemm256.hip: in the general loop
    // below every conditional residual load is followed by its own vmcnt(0)).
    {
      constexpr int NIT = C::EPI_ROWS / RPP;
      const int wmh = wm0 + half * C::EPI_ROWS;
      const bool plain_rows = (p.res_mod | p.gR | p.gC | p.c_live_mod) == 0;
      if (plain_rows && vec_ok && wmh + C::EPI_ROWS <= p.M && n0 + cbase(C::NT - 1) + 16 <= p.N) {
        const int row0 = lane / CH, ch = lane % CH;
        const int n = n0 + cbase(ch >> 1) + (ch & 1) * 8;
        if (Rb) {
          u32x4 rv[NIT];
#pragma unroll
          for (int it = 0; it < NIT; ++it) rv[it] = *reinterpret_cast<const u32x4*>(Rb + (long long)(wmh + it * RPP + row0) * p.ldr + n);
#pragma unroll
          for (int it = 0; it < NIT; ++it) {
            const int row = it * RPP + row0;
            const uint4 v = *reinterpret_cast<const uint4*>(reg + row * C::EPI_STRIDE + ch * 16);
            *reinterpret_cast<uint4*>(Cb + (long long)(wmh + row) * p.ldc + n) = add_packed8(v, rv[it]);
          }
        } else {
#pragma unroll
          for (int it = 0; it < NIT; ++it) {
            const int row = it * RPP + row0;
            *reinterpret_cast<uint4*>(Cb + (long long)(wmh + row) * p.ldc + n) = *reinterpret_cast<const uint4*>(reg + row * C::EPI_STRIDE + ch * 16);
          }
        }
        continue;
      }
    }
#pragma unroll
    for (int it = 0; it < C::EPI_ROWS / RPP; ++it) {
      const int row = it * RPP + lane / CH, ch = lane % CH;
      const int m = wm0 + half * C::EPI_ROWS + row, n = n0 + cbase(ch >> 1) + (ch & 1) * 8;
      uint4 v = *reinterpret_cast<const uint4*>(reg + row * C::EPI_STRIDE + ch * 16);
      if (m >= p.M || n >= p.N) continue;
      if (!row_live(m, p.c_live_mod, p.c_live_from)) continue;              // row never read again (live-row backward)
      const long long roff = residual_row(m, p.res_mod, p.gR, p.sgR, p.ldr);
      const long long crow = grouped_row(m, p.gC, p.sgC, p.ldc);
      if (vec_ok && n + 8 <= p.N) {
        if (Rb) v = add_packed8(v, *reinterpret_cast<const uint4*>(Rb + roff + n));
        *reinterpret_cast<uint4*>(Cb + crow + n) = v;
      } else {
        const unsigned wv[4] = {v.x, v.y, v.z, v.w};          // (store_tail8 of gemm_epilogue.h, open-coded: the call changes the SGPR count
#pragma unroll                                                 //  of the interleaved-RoPE instantiations)
        for (int k = 0; k < 8; ++k) {
          if (n + k < p.N) {
            float f = (k & 1) ? bf_hi(wv[k >> 1]) : bf_lo(wv[k >> 1]);
            if (Rb) f += bf2f(Rb[roff + n + k]);
            Cb[crow + n + k] = f2bf(f);
          }
        }
      }
    }
  }
}

// split-K second pass: C = bf16(bf16(act(bf16(sum_z ws[z] * alpha + bias))) + R); 4 columns per thread
__global__ void splitk_finalize_kernel(const float* __restrict__ ws, const bf16_t* __restrict__ bias, const bf16_t* __restrict__ R,
                                       bf16_t* __restrict__ C, int M, int N, int ldc, int ldr, int act, float alpha, int split, int vec) {
  const long long total = (long long)M * N / 4, plane = (long long)M * N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int m = (int)(i * 4 / N), n = (int)(i * 4 - (long long)m * N);
    // every plane's segment (and the bias / residual segments) is requested before the first one is used: summed in a rolled
    // loop, each plane paid its own dependent round trip (13 us in situ for 29 MB on the live-row backward's chain)
    f32x4 pv[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) pv[z] = z < split ? *reinterpret_cast<const f32x4*>(ws + z * plane + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    // (vec: bias / R / C rows are 8-B aligned - host-checked; otherwise element accesses)
    uint2 braw = {0, 0}, rraw = {0, 0};
    if (vec) {
      if (bias) braw = *reinterpret_cast<const uint2*>(bias + n);
      if (R) rraw = *reinterpret_cast<const uint2*>(R + (long long)m * ldr + n);
    } else {
      if (bias) braw = uint2{(unsigned)bias[n] | ((unsigned)bias[n + 1] << 16), (unsigned)bias[n + 2] | ((unsigned)bias[n + 3] << 16)};
      if (R) {
        const bf16_t* rp = R + (long long)m * ldr + n;
        rraw = uint2{(unsigned)rp[0] | ((unsigned)rp[1] << 16), (unsigned)rp[2] | ((unsigned)rp[3] << 16)};
      }
    }
    f32x4 a = pv[0];
#pragma unroll
    for (int z = 1; z < 8; ++z) a += pv[z];                   // (same order as the rolled sum; absent planes add +0)
    for (int z = 8; z < split; ++z) a += *reinterpret_cast<const f32x4*>(ws + z * plane + i * 4);
    const float bb[4] = {bf_lo(braw.x), bf_hi(braw.x), bf_lo(braw.y), bf_hi(braw.y)};
    const float rr[4] = {bf_lo(rraw.x), bf_hi(rraw.x), bf_lo(rraw.y), bf_hi(rraw.y)};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = epi_linear(a[j], alpha, bias ? bb[j] : 0.f);
      if (act != VLA_ACT_NONE) v = apply_act(rbf(v), act);
      if (R) v = rbf(v) + rr[j];
      o[j] = v;
    }
    if (vec) {
      *reinterpret_cast<uint2*>(C + (long long)m * ldc + n) = pack4(o);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) C[(long long)m * ldc + n + j] = f2bf(o[j]);
    }
  }
}

template <int BM, int BN, int STAGES, int ROPE, int WN = 2, bool F8 = false, bool EXT = false>
int launch(const GemmP& p0, int nb, hipStream_t st) {
  using C = Cfg<BM, BN, STAGES, WN>;
  if (int rc = vla_lds_limit<gemm_nt_kernel<BM, BN, STAGES, ROPE, WN, F8, EXT>>(C::LDS_BYTES, "gemm_nt_kernel")) return rc;
  GemmP p = p0;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.ntiles = ((p.M + BM - 1) / BM) * p.tiles_n;
  hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, STAGES, ROPE, WN, F8, EXT>), dim3(p.ntiles, 1, nb), dim3(C::NTHREADS), C::LDS_BYTES, st, p);
  return VLA_OK;
}

// The gemm.hip launch of a plan.  ROPE 3 is the SwiGLU-backward epilogue; the deep rings and the 128 x 64 tile exist only for the
// plain bf16 forms (128 x 64: not with rotate_half), so only the instantiations a plan can select are compiled.
template <int ROPE, bool F8 = false, bool EXT = false>
int launch_nt(int kernel, const GemmP& p, int nb, hipStream_t st) {
  if constexpr (!F8 && !EXT && ROPE != 3) {
    if (kernel == VLA_KERNEL_NT_64x128_S6) return launch<64, 128, 6, ROPE, 4>(p, nb, st);
    if (kernel == VLA_KERNEL_NT_128x128_S4) return launch<128, 128, 4, ROPE, 4>(p, nb, st);
    if constexpr (ROPE != 1)
      if (kernel == VLA_KERNEL_NT_128x64) return launch<128, 64, 2, ROPE>(p, nb, st);
  }
  return launch<128, 128, 2, ROPE, 4, F8, EXT>(p, nb, st);     // 8 waves (2x4) of 64x32
}

// ---------------------------------------------------------------- routing: one plan per call
// Test / benchmarking overrides, read once per call (tests flip them in the middle of a process):
//   VLA_GEMM_TILE=2|3|6   force 128x128 (8 waves) | 128x64 | 256x256; any non-zero value also keeps the product off gemm_skinny.hip
//   VLA_NO_SKINNY, VLA_NO_SMALL_ROWS   keep every / the <= 512-row products off gemm_skinny.hip
//   VLA_NO_SPLITK         no automatic split-K
//   VLA_GEMM256_GRID=n    workgroups of the persistent 256x256 kernel (default one per CU, 0 = one per tile)
struct NtOverrides {
  int tile;
  bool no_skinny, no_small_rows, no_splitk, grid_set;
  long long grid;
};
NtOverrides nt_overrides() {
  const char* tile = getenv("VLA_GEMM_TILE");
  const char* nsk = getenv("VLA_NO_SPLITK");
  const char* grid = getenv("VLA_GEMM256_GRID");
  return {tile ? atoi(tile) : 0, getenv("VLA_NO_SKINNY") != nullptr, getenv("VLA_NO_SMALL_ROWS") != nullptr, nsk && *nsk,
          grid != nullptr, grid ? atoll(grid) : 0};
}

// Caller's hint (per thread, read at launch = at graph capture): the following products run on an otherwise idle chip and are bound
// by latency, not throughput (batch-1 predict_action).  It selects the deep operand rings (bit-identical), gemm_skinny.hip's short-M
// tiles, the uneven split-K and the key-split attention (these three change the fp32 association).
thread_local int g_latency_hint = 0;

// When the 256 x 256 8-phase kernel (one workgroup per CU) is chosen automatically: problems with at least a chip-full of
// its tiles' worth of work in both dimensions.
bool use_256(int M, int N, int K, int batch, int act, int ncu) {
  const long long tiles = (long long)((M + 255) / 256) * ((N + 255) / 256) * batch;
  // the SwiGLU-backward epilogue streams GU in and dGU out (4 N bytes per row against 2 K of operands: as long as a short K
  // loop, HBM-bound on the full sequence): the 128-row kernel's second resident workgroup overlaps it with the other one's
  // K loop (live rows, M = 2048: 38 vs 44 us; full sequence, M = 11264: 166 vs 191 us)
  if (act == VLA_ACT_SWIGLU_BWD) return false;
  // a GELU epilogue (10 us of VALU per round of tiles) with a thin tail round (ViT fc1: 544 tiles = two rounds + 32) is the one
  // large shape the 128-row kernel still wins isolated (96 vs 106-114 us: its second resident workgroup computes under the
  // first one's epilogue); on the step the two routings tie (25.25-25.34 vs 25.29-25.32 ms)
  if ((act == VLA_ACT_GELU || act == VLA_ACT_GELU_TANH) && tiles > ncu && (tiles % ncu) != 0 && (tiles % ncu) * 4 < ncu) return false;
  // Rounds model (round 3, tools/bench_tiles_b16.py): a 256 x 256 tile is four 128 x 128 tiles of work on one CU; the 128-row kernel
  // keeps two workgroups per CU and reaches ~0.87 of the 256-row kernel's per-CU rate.  Cost in units of "one 128 x 128 tile at
  // the 256-row kernel's rate":  rounds256 x 4  against  rounds128 x 2 / 0.87.  Reproduces every measured winner of the batch-32
  // step (gate/up, down, o, q|k|v, ViT qkv / proj / fc2, task K/V -> 256) and of the batch-16 shapes of the LoRA / full steps, where
  // the round-2 threshold (>= 96 tiles) sent two shapes the wrong way: LLM q|k|v 5632 x 1152 (110 tiles = 0.43 round: 25.2 vs
  // 17.3 us) and ViT fc1 / dX fc2 4096 x 4352 (272 tiles = 1.06 rounds: 58.3 vs 47.8 us).
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128) * batch;
  const double est256 = (double)((tiles + ncu - 1) / ncu) * 4.0, est128 = (double)((t128 + 2 * ncu - 1) / (2 * ncu)) * (2.0 / 0.87);
  return M >= 1024 && N >= 768 && K >= 256 && est256 < est128;
}

// gemm_skinny.hip's tile for a small-output product, -1 when it is not one: (a) tall-skinny, N = 64 / 128 / 192 and M >= 1024 (the LoRA
// t / dt products), or (b) under the latency hint M <= 512 (the batch-1 pass); K < 2048, bias / activation / residual / RoPE epilogue.
// Contractions of 2048 and more stay on the 128-row tiles with split-K (measured, tools/diag/bench_skinny.py: with K cut into slices here
// as well, 64-row tiles pull twice the operand rows per output and lose - dt of gate/up, K = 9728: 57.7 vs 32.1 us; t of down 22.8 vs 20.0).
int skinny_tile(const vla_gemm_desc* d, bool latency, int ncu, bool no_small_rows) {
  const bool tall = (d->N == 64 || d->N == 128 || d->N == 192) && d->M >= 1024;                         // (a)
  // (b) only under the caller's latency hint (the batch-1 pass): in a training step the head's products are off the critical path (measured:
  // no change of the step), and a product's bits would depend on its row count - the live-row backward equals the full one bit for bit
  // because every row is computed by the same instruction sequence whatever M is (tests/test_engine_gpu.py)
  const bool shortm = latency && d->M <= 512 && d->N % 16 == 0 && d->K >= 512 && !no_small_rows;
  if (!(tall || shortm) || d->K % 128 != 0 || d->K >= 2048 || d->ldc % 8 != 0 || ((uintptr_t)d->C & 15) != 0) return -1;
  if (!(d->act == VLA_ACT_NONE || d->act == VLA_ACT_GELU || d->act == VLA_ACT_RELU || d->act == VLA_ACT_GELU_TANH)) return -1;
  if (d->bias && ((uintptr_t)d->bias & 15) != 0) return -1;
  if (d->R && (d->ldr % 8 != 0 || ((uintptr_t)d->R & 15) != 0)) return -1;
  if ((d->rope_mode == 1 && (d->rope_dh != 64 || d->rope_cols % 64 != 0 || tall)) ||
      (d->rope_mode == 2 && (d->rope_dh % 8 != 0 || d->rope_cols % 8 != 0 || (((uintptr_t)d->rope_cos | (uintptr_t)d->rope_sin) & 15) != 0)))
    return -1;
  // Tile: what a CU has to pull through its L1 is (tile rows + tile columns) x K operand rows per workgroup, times the workgroups it gets -
  // minimised over the instantiated tiles (every CU busy, as few rows each as possible; ties: the larger tile)
  int best = -1;
  long long best_cost = 0;
  for (int t = 0; t < SKINNY_TILES; ++t) {
    const int tm = 16 * SKINNY_TILE[t][0], tn = 16 * SKINNY_TILE[t][1];
    if (tall && d->N % tn != 0) continue;
    if (d->rope_mode == 1 && tn != 64) continue;              // rotate_half: both halves of a head inside one tile row
    const long long wgs = (long long)((d->M + tm - 1) / tm) * ((d->N + tn - 1) / tn), cost = (long long)(tm + tn) * ((wgs + ncu - 1) / ncu);
    if (best < 0 || cost < best_cost || (cost == best_cost && t > best)) best = t, best_cost = cost;
  }
  // (b) only for tiles up to 32 x 64 (96 operand rows per workgroup): measured in the batch-1 pass (profiles/r04_prof_predict_summary.txt, us under
  // the profiler, this kernel vs gemm.hip's 64 x 128 six-stage ring): 16 x 16 tiles 5.1 vs 10.6 (the head's 8-row products), 32 x 32 6.6 vs 12,
  // 32 x 64 8.9-10.4 vs 12.7-12.9 (LLM o, ViT proj) - but 64 x 64 13.3 vs 12.3 (ViT q|k|v) and 64 x 96 17.3 vs 13.4 (ViT fc1): with 128+ operand
  // rows per workgroup the LDS-DMA ring keeps more bytes in flight than register fragments at one or two waves per SIMD do
  if (!tall && best_cost > 96) return -1;
  return best;
}

// K extension on the 256 x 256 kernel (round 4; bf16 operands): the routing of the plain product over K + K2, provided the extension's rows
// are addressable like the main operands' (32-bit per-lane byte offsets, no row groups on A) and the epilogue is one the kernel has
// (plain / activation / residual / rotate_half at head dim 64 / SwiGLU forward).
bool ext_on_256(const vla_gemm_desc* d, int force, int ncu) {
  if (d->fp8 || d->batch != 1 || d->split_k > 1 || d->act == VLA_ACT_SWIGLU_BWD || d->rope_mode == 2 || d->a_group != 0 ||
      (d->rope_mode == 1 && d->rope_dh != 64) || !vla_gemm256_extent_ok(d))
    return false;
  const unsigned long long ra = (unsigned long long)((d->M + 255) / 256) * 256, rb = (unsigned long long)((d->N + 255) / 256) * 256;
  if ((ra * d->lda2 + d->K2) * 2 >= (1ull << 32) || (rb * d->ldb2 + d->K2) * 2 >= (1ull << 32)) return false;
  if (force != 0) return force == 6;
  const long long t256 = (long long)((d->M + 255) / 256) * ((d->N + 255) / 256);
  if (d->rope_mode == 1 && t256 < 192) return false;
  return use_256(d->M, d->N, d->K + d->K2, 1, d->act, ncu);
}

struct NtPlan { int kernel, split; };

// The kernel and the K-slice count of a validated descriptor.  Calibrated on MI355X (tools/bench_kernels.py, tools/bench_tiles_b16.py):
//  * 256x256 (gemm256.hip, one workgroup per CU) for chip-filling products by the rounds model of use_256;
//  * 128x128 with EIGHT waves (2x4 waves of 64x32, 2 blocks/CU = 16 waves/CU) otherwise: the K-loop is latency/barrier bound
//    (rocprofv3 PMC: SQ_WAIT_ANY 30-40 %, MFMA busy ~41 % with 4 waves), so more resident waves win over operand reuse per wave;
//  * 128x64 (4 waves, 3 blocks/CU) only for long-K problems that fill less than half the chip with square tiles;
//  * under the latency hint, launches of at most one workgroup per CU on deeper operand rings; small outputs on gemm_skinny.hip.
NtPlan plan_nt(const vla_gemm_desc* d, bool latency, int ncu, const NtOverrides& ov) {
  const int force = ov.tile, kt = d->K / BK;
  // split-K: slices of ceil(K-tiles / split_k) K-tiles; when that does not divide, the last slice is shorter and fewer slices may be needed
  const int asked = d->split_k > 1 ? d->split_k : 1, per = (kt + asked - 1) / asked, split = (kt + per - 1) / per;
  // small-output products (the LoRA t / dt products; the action head's Linears on 8 x B rows; the batch-1 pass)
  if (force == 0 && !ov.no_skinny && d->batch == 1 && split == 1 && d->a_group == 0 && d->c_group == 0 && d->r_group == 0 &&
      d->res_mod == 0 && d->c_live_mod == 0 && !d->fp8 && d->K2 == 0 && d->C) {
    const int t = skinny_tile(d, latency, ncu, ov.no_small_rows);
    if (t >= 0) return {VLA_KERNEL_NT_SKINNY + t, 1};
  }
  const bool fits256 = vla_gemm256_extent_ok(d) != 0;     // operands of 4 GiB and more: the 64-bit-pointer 128-row kernel
  if (d->K2 > 0) return {!d->fp8 && ext_on_256(d, force, ncu) ? VLA_KERNEL_NT_256 : VLA_KERNEL_NT_128x128, 1};
  if (d->fp8) {
    // e4m3 operands.  With the K loop halved, the 256 x 256 kernel's per-tile costs weigh twice as much: on the step's shapes the
    // 128-row kernel (two workgroups per CU, one's epilogue under the other's K loop) is as fast or faster (gate/up 162 vs 162 us,
    // down 62 vs 70, ViT fc1 63 vs 87), on big squares the 256-row kernel wins (8192^3: 2503 vs 2108 TF/s) - it takes those.
    const bool big = force == 6 || (force == 0 && d->M >= 4096 && d->N >= 4096 && d->K >= 4096);
    return {big && d->c_group == 0 && d->r_group == 0 && fits256 && !(d->rope_mode == 1 && d->rope_dh != 64) ? VLA_KERNEL_NT_256
                                                                                                              : VLA_KERNEL_NT_128x128, 1};
  }
  const int nb = asked > 1 ? asked : d->batch;       // (the tile rules see the requested slice count)
  bool square = false;
  if (asked == 1) {
    // rotate_half RoPE: the LLM's q|k|v projection goes to the 256-row kernel when it fills most of the chip with its tiles (whole-batch
    // launch, M = 11264: 220 tiles, 26.64-26.69 vs 26.84-26.85 ms on the step, same box); the half-batch launches of the two-pipeline
    // forward (110 tiles) measured 26.10-26.20 vs 26.07-26.10 and stay on the 128-row kernel.
    const long long t256 = (long long)((d->M + 255) / 256) * ((d->N + 255) / 256) * nb;
    if (force == 6 || (force == 0 && (d->rope_mode == 0 || t256 >= 192) && use_256(d->M, d->N, d->K, nb, d->act, ncu))) {
      // interleaved RoPE on the 256-row kernel: the plain epilogue without residual (the head's K|V projections); rotate_half at head
      // dim 128: the 128-row kernel's column map (one head per 128-column tile), the 256-row kernel's is built on 64-wide heads
      if (fits256 && !(d->rope_mode == 2 && (d->R || d->act != VLA_ACT_NONE)) && !(d->rope_mode == 1 && d->rope_dh != 64))
        return {VLA_KERNEL_NT_256, 1};
      square = true;          // (refused: the 128-row square tile)
    }
  }
  if (d->act == VLA_ACT_SWIGLU_BWD) return {VLA_KERNEL_NT_128x128, split};
  // In situ (whole training step, same-box A/B) the 8-wave 128x128 geometry beats the narrow tile on every shape of the step,
  // including the M=256 head GEMMs that overlap the LLM on the side stream (48.5 vs 49.5 vs 52.0 ms/step for always-square / mixed /
  // always-narrow).  Exception: long-K problems that fill less than half the chip with square tiles (the live-row gate/up dX GEMM:
  // M 2048, N 896, K 9728 -> 112 tiles): the narrow tile doubles the number of K loops in flight.
  const long long tiles = (long long)((d->M + 127) / 128) * ((d->N + 127) / 128) * nb;
  const bool narrow = !square && d->rope_mode != 1 && force != 2 && (force == 3 || (tiles <= 128 && d->K / asked >= 4096 && d->N % 64 == 0));
  if (narrow) return {VLA_KERNEL_NT_128x64, split};
  // Launches of at most one workgroup per CU (batch-1 inference: every product; the training step: the action head's x-chain) are
  // bound by the LATENCY of a K-tile, not by bandwidth: with the two-stage ring one K-tile is in flight per workgroup and every tile
  // costs a full trip to HBM (~1.2 us against 0.2 us of MFMAs: 17-22 us for ANY product of the batch-1 pass, K = 896-1152, whatever its
  // size).  They run on a four-stage ring (128 KiB of LDS: the CU is theirs anyway), three K-tiles in flight - or, when even 64-row tiles
  // leave CUs idle, on 64 x 128 tiles with a six-stage ring (144 KiB, five in flight, twice the workgroups: what such a launch can keep
  // in flight is workgroups x ring bytes) -, the same K order and MFMA sequence: bit-identical (test_gemm_deep_ring_bit_identical).
  // Only under the latency hint: in the training step the same launches share the chip with two other streams' kernels, and a 128-KiB
  // workgroup waits for a whole CU's LDS where the 64-KiB one slips in beside another (step 24.13 -> 24.44 ms same box with the deep
  // ring on every sub-round launch).
  if (latency && per >= 4) {
    const int runs = split > 1 ? split : d->batch;
    const long long wgs = (long long)((d->M + 127) / 128) * ((d->N + 127) / 128) * runs, wgs64 = (long long)((d->M + 63) / 64) * ((d->N + 127) / 128) * runs;
    if (wgs64 <= ncu) return {VLA_KERNEL_NT_64x128_S6, split};     // 64-row tiles, six stages: twice the workgroups, five K-tiles in flight
    if (wgs <= ncu) return {VLA_KERNEL_NT_128x128_S4, split};      // 128-row tiles, four stages
  }
  return {VLA_KERNEL_NT_128x128, split};
}

// The automatic split-K of a product the caller lets the library split (few-tile long-K problems: batch-1 inference, the live-row
// backward's M = B*64 GEMM over K = 2I).  The K loop of a tile is serial, so a problem with fewer tiles than the chip has workgroup slots
// (two per CU) runs at the latency of ONE long loop on part of the CUs; K slices meet in an fp32 workspace and are summed by
// splitk_finalize_kernel.  1 = do not split.
int auto_split_k(const vla_gemm_desc* d, bool latency, int ncu, const NtOverrides& ov) {
  const bool plain = !d->fp8 && d->K2 == 0 && d->batch == 1 && !d->bias_post_round && d->C && d->a_group == 0 && d->c_group == 0 &&
                     d->r_group == 0 && d->rope_mode == 0 && d->c_live_mod == 0 && d->res_mod == 0 && d->N % 4 == 0 &&
                     (d->act == VLA_ACT_NONE || d->act == VLA_ACT_GELU || d->act == VLA_ACT_RELU || d->act == VLA_ACT_GELU_TANH);
  if (!plain || d->K < 2048 || ov.no_splitk) return 1;
  const long long tiles = (long long)((d->M + 127) / 128) * ((d->N + 127) / 128), t64 = (long long)((d->M + 63) / 64) * ((d->N + 127) / 128);
  // the batch-1 pass (latency hint): as many K slices as give every CU one 64 x 128 workgroup, >= 4 K-tiles each (the slices need not
  // divide K: the last one is shorter) - ViT fc2 256 x 1152 x 4352: 7 slices of 10 K-tiles on 252 workgroups instead of 4 on 144
  if (latency && t64 * 2 <= ncu) return (int)std::max(2LL, std::min({ncu / t64, (long long)(d->K / BK) / 4, 16LL}));
  if (tiles > ncu) return 1;
  for (int sk = 8; sk >= 2; sk /= 2)          // even slices of >= 512, at most two workgroups per CU
    if (tiles * sk <= 2 * ncu && d->K % (BK * sk) == 0 && d->K / sk >= 512) return sk;
  return 1;
}

// second pass of a split-K product: the `split` fp32 planes of d->ws summed in order, then alpha / bias / activation / residual / rounding
int splitk_finalize(const vla_gemm_desc* d, int split, hipStream_t st) {
  const long long total = (long long)d->M * d->N / 4;
  const unsigned nblk = (unsigned)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(splitk_finalize_kernel, dim3(nblk), dim3(256), 0, st, (const float*)d->ws, (const bf16_t*)d->bias,
                     (const bf16_t*)d->R, (bf16_t*)d->C, d->M, d->N, d->ldc, d->ldr, d->act, d->alpha == 0.f ? 1.f : d->alpha, split,
                     (d->ldc % 4 == 0 && ((uintptr_t)d->C & 7) == 0 && (!d->R || (d->ldr % 4 == 0 && ((uintptr_t)d->R & 7) == 0)) &&
                      (!d->bias || ((uintptr_t)d->bias & 7) == 0)) ? 1 : 0);
  VLA_CHECK_LAUNCH("gemm_splitk_finalize");
  return VLA_OK;
}

}  // namespace

// gemm256_kernel keeps its per-lane operand addresses as 32-bit BYTE offsets from a wave-uniform base (the 128-row kernel uses
// 64-bit pointers): every operand row a 256-row tile can touch - tiles round M and N up to 256, row groups included - must
// start below 4 GiB minus one row.  Pure host arithmetic (no device query): exported so that the routing is unit-testable.
extern "C" int vla_gemm256_extent_ok(const vla_gemm_desc* d) {
  if (!d || d->M <= 0 || d->N <= 0 || d->K <= 0) return 0;
  const unsigned long long EB = d->fp8 ? 1 : 2, lim = 1ull << 32;
  const unsigned long long ra = (unsigned long long)((d->M + 255) / 256) * 256 - 1, rb = (unsigned long long)((d->N + 255) / 256) * 256 - 1;
  const unsigned long long offA = d->a_group > 0 ? (ra / d->a_group) * (unsigned long long)d->a_group_stride + (ra % d->a_group) * (unsigned long long)d->lda
                                                 : ra * (unsigned long long)d->lda;
  const unsigned long long offB = rb * (unsigned long long)d->ldb;
  return (offA + d->K) * EB < lim && (offB + d->K) * EB < lim;
}

extern "C" int vla_gemm_latency_hint(int on) {
  const int prev = g_latency_hint;
  if (on >= 0) g_latency_hint = on ? 1 : 0;
  return prev;
}

extern "C" int vla_gemm_nt_plan(const vla_gemm_desc* d, int latency, int num_cus, int* split) {
  if (!d || d->M <= 0 || d->N <= 0 || d->K < BK || d->batch <= 0) return VLA_ERR_ARG;
  const bool lat = latency < 0 ? g_latency_hint > 0 : latency > 0;
  const int ncu = num_cus > 0 ? num_cus : vla_num_cus();
  const NtOverrides ov = nt_overrides();
  const NtPlan pl = plan_nt(d, lat, ncu, ov);
  if (split) *split = d->split_k > 1 ? pl.split : auto_split_k(d, lat, ncu, ov);
  return pl.kernel;
}

extern "C" int vla_gemm_bf16_nt(void* stream, const vla_gemm_desc* d) {
  VLA_REQUIRE(d && d->A && d->B, "gemm: null operand");
  VLA_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->batch > 0, "gemm: empty problem");
  VLA_REQUIRE(d->K % BK == 0, "gemm: K must be a multiple of 64 (pad the operands)");
  VLA_REQUIRE(d->lda % 8 == 0 && d->ldb % 8 == 0, "gemm: lda/ldb must be multiples of 8 elements (16-B rows)");
  if (d->fp8)
    VLA_REQUIRE(d->fp8 == 1 && d->a_scale && d->b_scale && d->K % 128 == 0 && d->lda % 16 == 0 && d->ldb % 16 == 0 && d->batch == 1 &&
                    d->split_k <= 1 && d->rope_mode != 2 && d->a_group == 0 && (d->act != VLA_ACT_SWIGLU_BWD || d->K2 > 0),
                "gemm: fp8 needs scales, K % 128 == 0, 16-B rows, batch 1, no split-K / interleaved RoPE / row groups on A (SwiGLU backward: with a K extension only)");
  VLA_REQUIRE(((uintptr_t)d->A & 15) == 0 && ((uintptr_t)d->B & 15) == 0, "gemm: A/B must be 16-B aligned");
  VLA_REQUIRE(d->sA % 8 == 0 && d->sB % 8 == 0, "gemm: batch strides of A/B must keep 16-B alignment");
  if (d->act == VLA_ACT_SWIGLU_BWD) {
    VLA_REQUIRE(d->C && d->R && !d->bias && d->rope_mode == 0 && d->N % 64 == 0 && d->ldc % 8 == 0 && d->ldr % 4 == 0 &&
                    ((uintptr_t)d->R & 7) == 0 && d->c_group == 0 && d->res_mod == 0,
                "gemm: swiglu_bwd needs C = dGU [M, 2N] (ldc%8), R = GU [M, 2N] (interleaved), N%64 == 0");
  } else if (d->act == VLA_ACT_SWIGLU) {
    VLA_REQUIRE(d->C2 && d->N % 32 == 0 && d->ldc2 % 4 == 0 && ((uintptr_t)d->C2 & 7) == 0 && d->sC2 % 4 == 0,
                "gemm: swiglu needs C2, N%32==0, ldc2%4==0");
    VLA_REQUIRE(!d->R, "gemm: swiglu epilogue takes no residual");
  } else {
    VLA_REQUIRE(d->C, "gemm: null C");
  }
  if (d->C) VLA_REQUIRE(((uintptr_t)d->C & 15) == 0 || (d->ldc % 8) != 0, "gemm: C must be 16-B aligned");
  if (d->C && d->ldc % 8 == 0) VLA_REQUIRE(d->sC % 8 == 0, "gemm: sC must keep 16-B alignment");
  if (d->R && d->ldc % 8 == 0 && d->ldr % 8 == 0 && d->act != VLA_ACT_SWIGLU_BWD)
    VLA_REQUIRE(((uintptr_t)d->R & 15) == 0 && d->sR % 8 == 0, "gemm: R must be 16-B aligned");
  VLA_REQUIRE(d->a_group >= 0 && d->c_group >= 0 && d->a_group_stride % 8 == 0 &&
                  (d->c_group == 0 || d->ldc % 8 != 0 || d->c_group_stride % 8 == 0),
              "gemm: row-group strides must keep 16-B alignment");
  const bool split_k = d->split_k > 1;
  VLA_REQUIRE(d->bias_post_round == 0 || (d->bias_post_round == 1 && d->bias && d->rope_mode != 1 && !split_k && d->act == VLA_ACT_NONE),
              "gemm: bias_post_round needs a bias and a plain epilogue (no rotate_half rope / split-K / activation)");
  if (split_k) {
    VLA_REQUIRE(d->ws && d->batch == 1 && d->rope_mode == 0 && d->c_group == 0 && d->r_group == 0 &&
                    d->res_mod == 0 && d->c_live_mod == 0 && d->C &&
                    (d->act == VLA_ACT_NONE || d->act == VLA_ACT_GELU || d->act == VLA_ACT_RELU || d->act == VLA_ACT_GELU_TANH),
                "gemm: split_k needs an fp32 workspace [split_k, M, N], batch 1 and a plain epilogue");
    VLA_REQUIRE(d->N % 4 == 0 && ((uintptr_t)d->ws & 15) == 0, "gemm: split_k needs N % 4 == 0 and a 16-B aligned workspace");
  }
  VLA_REQUIRE(d->c_live_mod >= 0 && d->c_live_from >= 0 && (d->c_live_mod == 0 || d->c_live_from < d->c_live_mod),
              "gemm: c_live_from must lie inside c_live_mod");
  VLA_REQUIRE(d->r_group >= 0 && d->r_group_stride % 8 == 0 && (d->r_group == 0 || d->res_mod == 0),
              "gemm: r_group stride must keep 16-B alignment; r_group and res_mod are exclusive");
  if (d->K2 != 0)
    VLA_REQUIRE(d->K2 > 0 && d->K2 % BK == 0 && d->A2 && d->B2 && d->lda2 % 8 == 0 && d->ldb2 % 8 == 0 && (((uintptr_t)d->A2 | (uintptr_t)d->B2) & 15) == 0 &&
                    d->batch == 1 && !split_k && d->rope_mode != 2,
                "gemm: the K extension needs A2 / B2 (bf16, 16-B aligned rows, K2 % 64 == 0), batch 1, no split-K / interleaved RoPE");
  if (d->rope_mode != 0) {
    VLA_REQUIRE(d->rope_mode == 1 || d->rope_mode == 2, "gemm: rope_mode 0/1/2");
    VLA_REQUIRE(d->rope_cos && d->rope_sin && d->rope_T > 0 && d->rope_dh > 0 && d->rope_dh % 4 == 0 && d->rope_cols % 64 == 0 &&
                    (((uintptr_t)d->rope_cos | (uintptr_t)d->rope_sin) & 15) == 0 && d->act != VLA_ACT_SWIGLU,
                "gemm: bad rope arguments");
    if (d->rope_mode == 1) VLA_REQUIRE(d->rope_dh == 64 || (d->rope_dh == 128 && d->N % 128 == 0 && d->rope_cols % 128 == 0),
                                       "gemm: fused rotate_half RoPE needs head dim 64, or 128 with N and rope_cols multiples of 128");
  }

  const NtOverrides ov = nt_overrides();
  const int ncu = vla_num_cus();
  const NtPlan pl = plan_nt(d, g_latency_hint > 0, ncu, ov);

  GemmP p;
  p.A = (const bf16_t*)d->A; p.B = (const bf16_t*)d->B; p.C = (bf16_t*)d->C;
  p.bias = (const bf16_t*)d->bias; p.R = (const bf16_t*)d->R; p.C2 = (bf16_t*)d->C2;
  p.M = d->M; p.N = d->N; p.K = d->K; p.lda = d->lda; p.ldb = d->ldb; p.ldc = d->ldc; p.ldr = d->ldr;
  p.ldc2 = d->ldc2; p.res_mod = d->res_mod; p.act = d->act;
  p.sA = d->sA; p.sB = d->sB; p.sC = d->sC; p.sR = d->sR; p.sC2 = d->sC2; p.sBias = d->sBias;
  p.tiles_n = p.ntiles = 0; p.batch = 1; p.stagger = 0;
  p.alpha = d->alpha == 0.f ? 1.f : d->alpha;
  p.gA = d->a_group; p.sgA = d->a_group_stride; p.gC = d->c_group; p.sgC = d->c_group_stride;
  p.gR = d->r_group; p.sgR = d->r_group_stride;
  p.c_live_mod = d->c_live_mod; p.c_live_from = d->c_live_from;
  p.bias_post = d->bias_post_round;
  p.ws = nullptr; p.Ktot = 0;
  if (split_k) {
    const int kt = d->K / BK;
    p.ws = d->ws;
    p.K = (kt + pl.split - 1) / pl.split * BK;   // every z slice owns that many K-tiles of the contraction (the last one what is left of Ktot)
    p.Ktot = d->K;
    p.sA = p.sB = p.K;             // ... starting that many elements further along the rows of A and B
    p.bias = nullptr; p.R = nullptr;
  }
  p.rope_mode = d->rope_mode; p.rope_T = d->rope_T; p.rope_dh = d->rope_dh; p.rope_cols = d->rope_cols;
  p.rope_cos = d->rope_cos; p.rope_sin = d->rope_sin;
  p.scaleA = d->fp8 ? d->a_scale : nullptr; p.scaleB = d->fp8 ? d->b_scale : nullptr;
  p.A2 = (const bf16_t*)d->A2; p.B2 = (const bf16_t*)d->B2; p.K2 = d->K2; p.lda2 = d->lda2; p.ldb2 = d->ldb2;

  hipStream_t st = (hipStream_t)stream;
  const int nb = pl.split > 1 ? pl.split : d->batch;
  const int rope = d->act == VLA_ACT_SWIGLU_BWD ? 3 : d->rope_mode;
  int rc;
  if (pl.kernel < VLA_KERNEL_NT_SKINNY + SKINNY_TILES) rc = vla_gemm_skinny_launch(p, pl.kernel - VLA_KERNEL_NT_SKINNY, st);
  else if (pl.kernel == VLA_KERNEL_NT_256)
    // (a column peel of the tail round - the last column tiles on the 128-row kernel behind this launch - turned ViT fc1's 105 us into
    //  ~80 isolated and cost 0.1 ms on the step: the other streams already fill the tail round.  tools/diag/gemm256_pruned_paths.patch)
    rc = vla_gemm256_launch(p, d->act == VLA_ACT_SWIGLU ? 1 : d->act == VLA_ACT_SWIGLU_BWD ? 2 : 0, d->batch, ov.grid_set ? ov.grid : ncu, st);
  else if (d->K2 > 0 && d->fp8)    // e4m3 base operands, bf16 extension: the scales meet the accumulator between the two contractions
    rc = rope == 3 ? launch_nt<3, true, true>(pl.kernel, p, nb, st) : rope == 1 ? launch_nt<1, true, true>(pl.kernel, p, nb, st)
                                                                                : launch_nt<0, true, true>(pl.kernel, p, nb, st);
  else if (d->K2 > 0)
    rc = rope == 3 ? launch_nt<3, false, true>(pl.kernel, p, nb, st) : rope == 1 ? launch_nt<1, false, true>(pl.kernel, p, nb, st)
                                                                                 : launch_nt<0, false, true>(pl.kernel, p, nb, st);
  else if (d->fp8) rc = rope == 1 ? launch_nt<1, true>(pl.kernel, p, nb, st) : launch_nt<0, true>(pl.kernel, p, nb, st);
  else if (rope == 3) rc = launch_nt<3>(pl.kernel, p, nb, st);
  else if (rope == 2) rc = launch_nt<2>(pl.kernel, p, nb, st);
  else if (rope == 1) rc = launch_nt<1>(pl.kernel, p, nb, st);
  else rc = launch_nt<0>(pl.kernel, p, nb, st);
  if (rc) return rc;
  VLA_CHECK_LAUNCH("gemm_bf16_nt");
  if (pl.split > 1) return splitk_finalize(d, pl.split, st);
  return VLA_OK;
}
