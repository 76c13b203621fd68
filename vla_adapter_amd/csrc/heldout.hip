// Validation on held-out episodes of a device-resident store: the part of the reference's run_validation (vla-scripts/finetune.py:
// 605-685) over its RLDS val split (rlds/dataset.py:234-236) that decides which held-out windows form a validation batch and reduces
// the batch's L1 errors.  Declared in include/vla_heldout.h.
//   vla_heldout_sweep           (rank, world, batch j, stride) -> the B windows of this rank's j-th validation batch, in order, and which
//                               of them exist: dataset, episode, first row, prompt offsets, valid
//   vla_heldout_l1_accumulate   |pred - target| of the valid rows, summed per dataset and cell into f64, and the rows counted
// Both launch on the caller's stream, allocate nothing and read nothing back: a captured graph may hold them.  Every output element is
// written by exactly one thread (plain stores, no atomics).  Both rules are restated in Python (vla_adapter_amd/heldout.py:
// sweep_windows, l1_accumulate_reference), which is what the kernels are tested against, bit for bit.
#include "common.h"
#include "windows.h"
#include "../../include/vla_heldout.h"

// The accumulation's additions round one by one, in the order the header states.
#pragma clang fp contract(off)

namespace {

constexpr int SWEEP_MAX_B = 1024;
constexpr int ACC_THREADS = 64;                    // one wave per workgroup: C * A cells are a few hundred at most (ALOHA: 25 x 14)

// One workgroup; thread b < B locates window w_b, then all threads scan the prompt lengths (emit_windows).
__global__ void __launch_bounds__(SWEEP_MAX_B)
heldout_sweep_kernel(const long long* __restrict__ val_off, const long long* __restrict__ episode_off, const int* __restrict__ prompt_off,
                     const int* __restrict__ dataset_off, int E, int D, long long first, long long stride, int B, int Pmax,
                     int* __restrict__ ds, int* __restrict__ ep, long long* __restrict__ row, int* __restrict__ out_off,
                     unsigned char* __restrict__ valid) {
  __shared__ int scan[SWEEP_MAX_B];
  const int b = threadIdx.x;
  int e = 0;
  long long t = 0;
  if (b < B) {
    const long long nv = val_off[E];
    const long long w = (first + (long long)b) * stride;
    const bool ok = w < nv;                          // (nv < 1, a bad table: no sample is valid)
    const long long j = ok ? w : 0ll;                // a sample past the end takes window 0: everything downstream runs on in-range data
    e = last_not_above(val_off, 0, E - 1, j);
    t = j - val_off[e];
    ds[b] = dataset_off ? last_not_above(dataset_off, 0, D - 1, (long long)e) : 0;
    valid[b] = ok ? 1 : 0;
  }
  emit_windows(b, B, e, t, episode_off, prompt_off, Pmax, scan, ep, row, out_off);
}

// Workgroups x < nbx: thread (x, tid) owns cell i = x * ACC_THREADS + tid of the C * A cells and walks the datasets and, per dataset,
// the rows in ascending order with the partial sum in a register; workgroup x == nbx counts the rows, thread tid the datasets
// tid, tid + ACC_THREADS, ...  A row with valid == 0 is never loaded.
__global__ void __launch_bounds__(ACC_THREADS)
heldout_l1_accumulate_kernel(const bf16_t* __restrict__ pred, const bf16_t* __restrict__ target, const int* __restrict__ ds,
                             const unsigned char* __restrict__ valid, int B, int cells, int D, double* __restrict__ acc,
                             long long* __restrict__ cnt, int nbx) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x == nbx) {
    for (int d = tid; d < D; d += ACC_THREADS) {
      long long n = 0;
      for (int b = 0; b < B; ++b) {
        const int db = ds ? min(max(ds[b], 0), D - 1) : 0;
        n += (valid[b] != 0 && db == d) ? 1 : 0;
      }
      cnt[d] += n;
    }
    return;
  }
  const int i = (int)blockIdx.x * ACC_THREADS + tid;
  if (i >= cells) return;
  for (int d = 0; d < D; ++d) {
    double s = 0.0;
    for (int b = 0; b < B; ++b) {
      const int db = ds ? min(max(ds[b], 0), D - 1) : 0;
      if (valid[b] != 0 && db == d) {
        const long long k = (long long)b * cells + i;
        s += (double)fabsf(bf2f(pred[k]) - bf2f(target[k]));
      }
    }
    acc[(long long)d * cells + i] += s;
  }
}

}  // namespace

extern "C" int vla_heldout_sweep(void* stream, const long long* val_off, const long long* episode_off, const int* prompt_off,
                                 const int* dataset_off, int E, int D, long long rank, long long world, long long batch_j,
                                 long long stride, int B, int Pmax, int* ds, int* ep, long long* row, int* out_off,
                                 unsigned char* valid) {
  VLA_REQUIRE(val_off && episode_off && prompt_off && ds && ep && row && out_off && valid, "heldout_sweep: null pointer");
  VLA_REQUIRE(E >= 1 && D >= 1 && D <= E, "heldout_sweep: E >= 1, 1 <= D <= E (every dataset holds an episode)");
  VLA_REQUIRE(dataset_off || D == 1, "heldout_sweep: null dataset_off with D > 1");
  VLA_REQUIRE(B >= 1 && B <= SWEEP_MAX_B && Pmax >= 0, "heldout_sweep: 1 <= B <= 1024 (one workgroup), Pmax >= 0");
  VLA_REQUIRE((long long)B * Pmax <= 0x7fffffffll, "heldout_sweep: B * Pmax must fit int32 offsets");
  VLA_REQUIRE(world >= 1 && rank >= 0 && rank < world && batch_j >= 0, "heldout_sweep: 0 <= rank < world, batch_j >= 0");
  VLA_REQUIRE(stride >= 1, "heldout_sweep: stride >= 1");
  // ((batch_j * world + rank) * B + b) * stride stays below 2^62 for every b < B
  const long long lim = 0x3fffffffffffffffll;
  VLA_REQUIRE(world <= lim / B / stride && batch_j < lim / B / stride / world, "heldout_sweep: the window index overflows 64 bits");
  const long long first = (batch_j * world + rank) * (long long)B;
  const int threads = (B + 63) / 64 * 64;
  hipLaunchKernelGGL(heldout_sweep_kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, val_off, episode_off, prompt_off, dataset_off, E, D,
                     first, stride, B, Pmax, ds, ep, row, out_off, valid);
  VLA_CHECK_LAUNCH("heldout_sweep");
  return VLA_OK;
}

extern "C" int vla_heldout_l1_accumulate(void* stream, const void* pred, const void* target, const int* ds, const unsigned char* valid,
                                         int B, int C, int A, int D, double* acc, long long* cnt) {
  VLA_REQUIRE(pred && target && valid && acc && cnt, "heldout_l1_accumulate: null pointer");
  VLA_REQUIRE(B >= 1 && C >= 1 && A >= 1 && D >= 1, "heldout_l1_accumulate: B, C, A, D >= 1");
  VLA_REQUIRE((long long)C * A <= 0x7fffffffll - ACC_THREADS && (long long)D * C * A <= 0x7fffffffffffll, "heldout_l1_accumulate: extents overflow");
  const int cells = C * A;
  const int nbx = (cells + ACC_THREADS - 1) / ACC_THREADS;
  hipLaunchKernelGGL(heldout_l1_accumulate_kernel, dim3((unsigned)(nbx + 1)), dim3(ACC_THREADS), 0, (hipStream_t)stream, (const bf16_t*)pred,
                     (const bf16_t*)target, ds, valid, B, cells, D, acc, cnt, nbx);
  VLA_CHECK_LAUNCH("heldout_l1_accumulate");
  return VLA_OK;
}
