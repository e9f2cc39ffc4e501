// Auxiliary polynomial columns: LogUp range-check helpers + running sum, and cross-table-lookup Z columns.
//
// Replaces (un-vendored starky 0.4.0, driven from reference src/starks/common/prover.rs:46-65):
//   lookup_helper_columns  for Stark::lookups() (scalar_mul_stark.rs:493-500):
//       h_k = 1/(beta+f_2k) + 1/(beta+f_2k+1),  Z_0 = 0,  Z_{i+1} = Z_i + sum_k h_k(i) - freq(i)/(beta+table(i))
//   get_ctl_data / partial_sums for looked tables with no looking tables (scalar_mul_ctl.rs:20-55):
//       Z_i = sum_{j>=i} filter_j / (sum_m col_m(j) beta^m + gamma)
// Output column order (starky prove_with_commitment): per challenge [h_0..h_{m-1}, Z], then the CTL Z's
// in (ctl, challenge) order.
#include <algorithm>
#include "aux.h"

static constexpr int LOGUP_SPAN = 16;  // helper columns (pairs of range-checked columns) per thread of k_logup_helpers
static constexpr int LOGUP_INV_BATCH = 4;  // table entries per thread of k_logup_inv_table

// Every range-checked value and every table value lies in 0..65535 (k_histogram rejects anything else), so per challenge there
// are only 65536 denominators beta + v.  inv[2 v + ch] = (beta_ch + v)^-1 for v = 0..65535: both challenges of a value sit in
// one 16-byte entry, one gather serves both.  A thread inverts LOGUP_INV_BATCH consecutive words with one field inversion
// (Montgomery's trick); a zero denominator (beta_ch + v = 0 mod p, probability ~2^-47 per proof) gives a zero entry and leaves
// its neighbours alone.  The batched inversion this replaces zeroed all 30 helpers of its chunk then; neither form, nor the
// reference, can prove such a trace, so the difference is not reproduced.
__global__ __launch_bounds__(256) void k_logup_inv_table(u64 beta0, u64 beta1, u64* __restrict__ inv) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;  // words 4t .. 4t+3 = values 2t, 2t+1
  if (t >= 2 * 65536 / LOGUP_INV_BATCH) return;
  u64 d[LOGUP_INV_BATCH], pre[LOGUP_INV_BATCH];
  u64 acc = 1;
#pragma unroll
  for (int j = 0; j < LOGUP_INV_BATCH; j++) {
    const u64 x = gl_add((j & 1) ? beta1 : beta0, (u64)(2 * t + (j >> 1)));
    d[j] = x ? x : 1;  // (restored to 0 below)
    pre[j] = acc;
    acc = gl_mul(acc, d[j]);
  }
  u64 r = gl_inv(acc);
  u64 o[LOGUP_INV_BATCH];
#pragma unroll
  for (int j = LOGUP_INV_BATCH - 1; j >= 0; j--) {
    const u64 x = gl_add((j & 1) ? beta1 : beta0, (u64)(2 * t + (j >> 1)));
    o[j] = x ? gl_mul(r, pre[j]) : 0;
    r = gl_mul(r, d[j]);
  }
  ulonglong2* out = reinterpret_cast<ulonglong2*>(inv) + 2 * (size_t)t;
  out[0] = make_ulonglong2(o[0], o[1]);
  out[1] = make_ulonglong2(o[2], o[3]);
}

// the table entry of a trace value: the index is masked, so whatever the value the load stays inside the table; `bad` collects
// the values so that one test per thread finds a value above 65535
__device__ __forceinline__ ulonglong2 logup_inv_at(const ulonglong2* __restrict__ inv, u64 v, u64& bad) {
  bad |= v;
  return inv[(u32)v & 0xFFFFu];
}

// h_k = 1/(a + beta) + 1/(b + beta) for both challenges: two table reads and two additions.  A thread owns LOGUP_SPAN helpers
// of one row; the last helper of an odd column count is 1/(a + beta), one read.  psum[(ch*nchunks + chunk)*N + i] = the sum of
// the thread's helpers, for k_logup_terms.  A value above 65535 (trace generation never produces one) sets *err.
__global__ __launch_bounds__(256) void k_logup_helpers(const u64* __restrict__ trace, size_t N, int rc_begin, int n_rc,
                                                       const u64* __restrict__ inv_tab, u64* __restrict__ aux, int helpers_per_ch,
                                                       u64* __restrict__ psum, int nchunks, int* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const ulonglong2* inv = reinterpret_cast<const ulonglong2*>(inv_tab);
  const int chunk = blockIdx.y;
  const int k0 = chunk * LOGUP_SPAN;  // first helper of this thread
  const int k1 = min(k0 + LOGUP_SPAN, helpers_per_ch);
  const int kp = min(k1, n_rc / 2);   // helpers below kp have two columns
  const u64* col = trace + (size_t)(rc_begin + 2 * k0) * N + i;
  u64* out0 = aux + (size_t)k0 * N + i;
  u64* out1 = out0 + (size_t)(helpers_per_ch + 1) * N;
  u64 s0 = 0, s1 = 0, bad = 0;
#pragma unroll 4
  for (int k = k0; k < kp; k++) {
    const ulonglong2 ia = logup_inv_at(inv, col[0], bad), ib = logup_inv_at(inv, col[N], bad);
    const u64 h0 = gl_add(ia.x, ib.x), h1 = gl_add(ia.y, ib.y);
    *out0 = h0;
    *out1 = h1;
    s0 = gl_add(s0, h0);
    s1 = gl_add(s1, h1);
    col += 2 * N;
    out0 += N;
    out1 += N;
  }
  if (kp < k1) {  // the single column of an odd count
    const ulonglong2 ia = logup_inv_at(inv, col[0], bad);
    *out0 = ia.x;
    *out1 = ia.y;
    s0 = gl_add(s0, ia.x);
    s1 = gl_add(s1, ia.y);
  }
  psum[(size_t)chunk * N + i] = s0;
  psum[(size_t)(nchunks + chunk) * N + i] = s1;
  if (bad >> 16) atomicCAS(err, 0, BN254S_E_INTERNAL);
}

// term[i] = sum_chunks psum[i] - freq[i] / (beta + table[i])
__global__ __launch_bounds__(256) void k_logup_terms(const u64* __restrict__ trace, size_t N, int table_col, int freq_col,
                                                     const u64* __restrict__ inv_tab, const u64* __restrict__ psum, int nchunks,
                                                     u64* __restrict__ terms, int* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  u64 bad = 0;
  const ulonglong2 t = logup_inv_at(reinterpret_cast<const ulonglong2*>(inv_tab), trace[(size_t)table_col * N + i], bad);
  const u64 f = trace[(size_t)freq_col * N + i];
  u64 s0 = 0, s1 = 0;
  for (int c = 0; c < nchunks; c++) {
    s0 = gl_add(s0, psum[(size_t)c * N + i]);
    s1 = gl_add(s1, psum[(size_t)(nchunks + c) * N + i]);
  }
  terms[i] = gl_sub(s0, gl_mul(f, t.x));
  terms[N + i] = gl_sub(s1, gl_mul(f, t.y));
  if (bad >> 16) atomicCAS(err, 0, BN254S_E_INTERNAL);
}

// One block per column: 1024 threads, fewer for a column of fewer than 1024 rows (N is a multiple of the block).  mode 0: out[0] = 0, out[i+1] = out[i] + in[i] (exclusive prefix);
// mode 1: out[i] = sum_{j >= i} in[j] (inclusive suffix).
__global__ __launch_bounds__(1024) void k_scan(const u64* __restrict__ in, size_t in_stride, u64* __restrict__ out,
                                               size_t out_stride, size_t N, int mode) {
  LATENCY_KERNEL_PRIO();
  __shared__ u64 part[1024];
  const int t = threadIdx.x;
  const u64* src = in + (size_t)blockIdx.x * in_stride;
  u64* dst = out + (size_t)blockIdx.x * out_stride;
  const int T = blockDim.x;
  const size_t per = N / T;
  auto idx = [&](size_t q) { return mode ? N - 1 - q : q; };  // scan order position -> memory index
  size_t q0 = (size_t)t * per;
  u64 s = 0;
  for (size_t q = 0; q < per; q++) s = gl_add(s, src[idx(q0 + q)]);
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    u64 v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] = gl_add(part[t], v);
    __syncthreads();
  }
  u64 run = t ? part[t - 1] : 0;  // sum of everything before this thread's chunk
  for (size_t q = 0; q < per; q++) {
    u64 x = src[idx(q0 + q)];
    if (mode == 0) {
      dst[idx(q0 + q)] = run;
      run = gl_add(run, x);
    } else {
      run = gl_add(run, x);
      dst[idx(q0 + q)] = run;
    }
  }
}

// CTL terms: filter/combine for every (ctl, challenge); terms[(ctl*2+ch)*N + i].
__global__ __launch_bounds__(256) void k_ctl_terms(const u64* __restrict__ trace, size_t N, CtlSpecDev spec, u64 beta0,
                                                   u64 gamma0, u64 beta1, u64 gamma1, u64* __restrict__ terms,
                                                   int* __restrict__ err) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int ctl = blockIdx.y;
  u64 f = trace[(size_t)spec.filter_col[ctl] * N + i];
  u64 t0 = 0, t1 = 0;
  if (f == 1) {
    u64 a0 = 0, a1 = 0;
    for (int m = spec.ncols[ctl] - 1; m >= 0; m--) {
      int start = spec.col_start[ctl][m], nb = spec.col_bits[ctl][m];
      u64 v = 0;
      for (int b = nb - 1; b >= 0; b--) v = gl_add(gl_dbl(v), trace[(size_t)(start + b) * N + i]);
      a0 = gl_add(gl_mul(a0, beta0), v);
      a1 = gl_add(gl_mul(a1, beta1), v);
    }
    t0 = gl_inv(gl_add(a0, gamma0));
    t1 = gl_inv(gl_add(a1, gamma1));
  } else if (f != 0) {
    atomicCAS(err, 0, BN254S_E_INTERNAL);  // starky: "Non-binary filter?"
  }
  terms[(size_t)(ctl * 2 + 0) * N + i] = t0;
  terms[(size_t)(ctl * 2 + 1) * N + i] = t1;
}

// [inverse table | psum | terms | CTL terms]
static constexpr size_t LOGUP_INV_WORDS = 2 * 65536;
size_t aux_scratch_words(const StarkShape& sh, size_t N) {
  int nchunks = (sh.n_helpers() + LOGUP_SPAN - 1) / LOGUP_SPAN;
  return LOGUP_INV_WORDS + (size_t)(2 * nchunks + 2 + 2 * sh.n_ctl) * N;
}

void aux_build(const StarkShape& sh, const u64* d_trace, size_t N, const u64 betas[2], const u64 gammas[2], u64* d_aux,
               u64* d_scratch, int* d_err, hipStream_t st) {
  const int n_rc = sh.n_rc(), m = sh.n_helpers();
  const int nchunks = (m + LOGUP_SPAN - 1) / LOGUP_SPAN;
  u64* inv = d_scratch;
  u64* psum = inv + LOGUP_INV_WORDS;
  u64* terms = psum + (size_t)2 * nchunks * N;
  u64* cterms = terms + 2 * N;
  const unsigned scan_threads = (unsigned)std::min<size_t>(1024, N);
  k_logup_inv_table<<<(unsigned)(LOGUP_INV_WORDS / LOGUP_INV_BATCH / 256), 256, 0, st>>>(betas[0], betas[1], inv);
  dim3 g1((unsigned)((N + 255) / 256), nchunks);
  k_logup_helpers<<<g1, 256, 0, st>>>(d_trace, N, sh.rc_begin, n_rc, inv, d_aux, m, psum, nchunks, d_err);
  k_logup_terms<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(d_trace, N, sh.table_col, sh.freq_col, inv, psum, nchunks, terms, d_err);
  // Z columns sit after the helpers of each challenge: column ch*(m+1) + m
  k_scan<<<2, scan_threads, 0, st>>>(terms, N, d_aux + (size_t)m * N, (size_t)(m + 1) * N, N, 0);
  if (sh.n_ctl == 0) return;  // (bn254s_selftest_logup: the lookup columns alone)
  dim3 g3((unsigned)((N + 255) / 256), sh.n_ctl);
  k_ctl_terms<<<g3, 256, 0, st>>>(d_trace, N, sh.ctl, betas[0], gammas[0], betas[1], gammas[1], cterms, d_err);
  k_scan<<<2 * sh.n_ctl, scan_threads, 0, st>>>(cterms, N, d_aux + (size_t)2 * (m + 1) * N, N, N, 1);
}

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void aux_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_logup_terms));
}
