// Kernels the three trace generators share (and msm.hip, prover.hip, capi.hip use through trace.h): Montgomery batch inversion
// over Fq, the round-flag table (generate_round_flags, src/starks/common/round_flags.rs:21-44), the range-check columns
// (generate_range_checks, :71-87) and the fq_inv self-test.
#include "trace_common.h"
#include "trace.h"

#ifndef BN254S_BATCH_INV_CH
#define BN254S_BATCH_INV_CH 4
#endif
// ---- batched field inversion ------------------------------------------------------------------------------
// out[e] = in[e]^-1 (0 -> 0); each thread owns CH elements strided by the grid size.
// (The backward pass is unrolled by template recursion: the unroller refuses a body of two inlined products "as too large" even
// under a pragma, and a rolled loop would index v[] / pre[] dynamically, i.e. keep them in scratch memory.)
template <int J, int CH>
__device__ __forceinline__ void batch_inv_back(const fq (&v)[CH], const fq (&pre)[CH], fq& inv, u64* __restrict__ out, size_t count,
                                               size_t tid, size_t T) {
  if constexpr (J >= 0) {
    const size_t e = tid + J * T;
    if (e < count) {
      if (fq_is_zero(v[J])) {
        st_fq(out, count, e, fq_zero());
      } else {
        st_fq(out, count, e, fq_mul(inv, pre[J]));
        if constexpr (J > 0) inv = fq_mul(inv, v[J]);
      }
    }
    batch_inv_back<J - 1, CH>(v, pre, inv, out, count, tid, T);
  }
}
template <int CH>
__global__ __launch_bounds__(64) void k_fq_batch_inv(const u64* __restrict__ in, u64* __restrict__ out, size_t count) {
  LATENCY_KERNEL_PRIO();
  size_t T = (size_t)gridDim.x * blockDim.x, tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  fq v[CH], pre[CH];
  fq acc = fq_one();
#pragma unroll
  for (int j = 0; j < CH; j++) {
    size_t e = tid + j * T;
    v[j] = e < count ? ld_fq(in, count, e) : fq_zero();
    pre[j] = acc;
    if (!fq_is_zero(v[j])) acc = fq_mul(acc, v[j]);
  }
  fq inv = fq_inv(acc);
  batch_inv_back<CH - 1, CH>(v, pre, inv, out, count, tid, T);
}

// Goldilocks inverses of counter and counter-511 for counter in [0,512): computed once per context.
__global__ void k_round_flag_table(u64* tbl /* [2][512] */) {
  LATENCY_KERNEL_PRIO();
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= 512) return;
  tbl[c] = c == 0 ? 0 : gl_inv((u64)c);
  u64 cp = gl_sub((u64)c, 511);
  tbl[512 + c] = cp == 0 ? 0 : gl_inv(cp);
}

// ---- range-check columns (generate_range_checks, scalar_mul_stark.rs:71-87) ----------------------------
// LDS-privatised histogram.  blockIdx.y selects the half of the 2^16 bins kept in LDS (32768 u32 = 128 KB);
// every block sweeps its slice of the range-checked columns once per half.  The witness columns are far from
// uniform (aux_hi limbs sit at 2^13 +- 1, many flags are 0/1), so before touching LDS each wave peels off up to
// two "leader" values with ballots and adds their multiplicity with one atomic.
__global__ __launch_bounds__(1024) void k_histogram(const u64* __restrict__ trace, size_t N, int col_begin, int col_end,
                                                    u32* __restrict__ hist, int* __restrict__ err) {
  __shared__ u32 h[32768];
  const u32 half = blockIdx.y;
  for (int b = threadIdx.x; b < 32768; b += blockDim.x) h[b] = 0;
  __syncthreads();
  const size_t total = (size_t)(col_end - col_begin) * N;
  const size_t per = (total + gridDim.x - 1) / gridDim.x;
  const size_t lo = (size_t)blockIdx.x * per, hi = min(total, lo + per);
  const u64* src = trace + (size_t)col_begin * N;
  const int lane = threadIdx.x & 63;
  for (size_t base = lo; base < hi; base += blockDim.x) {
    size_t i = base + threadIdx.x;
    u64 v = i < hi ? src[i] : ~0ULL;
    if (i < hi && v >= 65536) atomicCAS(err, 0, BN254S_E_INTERNAL);
    bool active = i < hi && (v >> 15) == half;
    u32 bin = (u32)v & 32767;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      unsigned long long m = __ballot(active);
      if (m == 0) break;
      int leader = __ffsll((long long)m) - 1;
      u32 lv = __shfl(bin, leader);
      bool same = active && bin == lv;
      unsigned long long ms = __ballot(same);
      if (lane == leader) atomicAdd(&h[lv], (u32)__popcll(ms));
      active = active && !same;
    }
    if (active) atomicAdd(&h[bin], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 32768; b += blockDim.x) {
    u32 cnt = h[b];
    if (cnt) atomicAdd(&hist[half * 32768 + b], cnt);
  }
}
__global__ __launch_bounds__(256) void k_range_columns(u64* __restrict__ trace, size_t N, int freq_col, int range_col,
                                                       const u32* __restrict__ hist) {
  LATENCY_KERNEL_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  trace[(size_t)range_col * N + i] = i < 65536 ? i : 65535;
  trace[(size_t)freq_col * N + i] = i < 65536 ? (u64)hist[i] : 0;
}

// Debug / parity: out[i] = in[i]^-1 mod p on canonical words (0 -> 0), one lane per element, by divsteps (fq_inv) and by Fermat
// (fq_inv_fermat): out[n][8] = the two results.
__global__ __launch_bounds__(64) void k_fq_inv_selftest(const u64* __restrict__ in, u64* __restrict__ out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const fq a = fq_from_canonical(in + 4 * i);
  const bool z = fq_is_zero(a);
  const fqw r0 = fq_to_canonical(z ? a : fq_inv(a)), r1 = fq_to_canonical(z ? a : fq_inv_fermat(a));
  for (int k = 0; k < 4; k++) {
    out[8 * i + k] = r0.l[k];
    out[8 * i + 4 + k] = r1.l[k];
  }
}
void launch_fq_inv_selftest(const u64* in, u64* out, size_t n, hipStream_t st) {
  k_fq_inv_selftest<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(in, out, n);
}

void launch_fq_batch_inv(const u64* in, u64* out, size_t count, hipStream_t st) {
  // one divstep inversion (~12 k instructions) per CH elements plus three products (~1 k) per element: CH = 4 keeps the arrays in
  // registers (no scratch) and puts 4x as many waves on the GPU as the CH = 8 of the Fermat days
  const int CH = BN254S_BATCH_INV_CH;
  size_t threads = (count + CH - 1) / CH;
  k_fq_batch_inv<CH><<<(unsigned)((threads + 63) / 64), 64, 0, st>>>(in, out, count);
}
void launch_round_flag_table(u64* tbl, hipStream_t st) { k_round_flag_table<<<2, 256, 0, st>>>(tbl); }
void launch_range_columns(u64* trace, size_t N, int rc_begin, int rc_end, int freq_col, int range_col, u32* hist, int* err,
                          hipStream_t st) {
  hipMemsetAsync(hist, 0, 65536 * 4, st);
  k_histogram<<<dim3(128, 2), 1024, 0, st>>>(trace, N, rc_begin, rc_end, hist, err);
  k_range_columns<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(trace, N, freq_col, range_col, hist);
}

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void trace_shared_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_range_columns));
}
