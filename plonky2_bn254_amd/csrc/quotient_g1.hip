// Quotient-polynomial evaluation for the G1 scalar-mul STARK (K-quotient of DESIGN.md).
//
// Replaces starky `compute_quotient_polys` / `eval_vanishing_poly` calling the reference's AIR
//   G1ScalarMulStark::eval_packed_generic   src/starks/curves/g1/scalar_mul_stark.rs:226-339
//   eval_g1_add                             src/starks/curves/g1/add.rs:125-185
//   eval_is_modulus_zero / eval_modulus_zero  src/starks/modular/is_modulus_zero.rs:69-84, modulus_zero.rs:163-198
//   eval_round_flags / EvalEq               src/starks/common/round_flags.rs:46-81, common/eq.rs:25-51
// on every point of the 2N-point coset, one lane per point, columns read coalesced from the
// bit-reversed LDE.  Constraint numbering e follows the reference's emission order exactly (see
// quotient_common.h for why).  Within a `eval_modulus_zero` block the 32 limb constraints are linear in the
// witness, so their alpha-weighted sum is re-associated:
//   sum_i w_i*constr_i = qsign * sum_j quot_j * M_j  +  sum_d (lo_d*u_d + hi_d*B*u_d) - off*sum u_d  -  sum_i w_i*input_i
// with M_j = sum_t w_{j+t} m_t and u_d = w_{d+1} - B*w_d depending on alpha only (host-precomputed).
#include "quotient_sched.h"
#include "quotient.h"

static constexpr int G1_K_AIR = 1111;
// first constraint index of the five eval_modulus_zero blocks inside eval_g1_add
static constexpr int G1_MZ_E0[5] = {0, 50, 83, 132, 165};

// Parts 0..4: the five eval_modulus_zero blocks of eval_g1_add (each with the small groups emitted next to it);
// part 5: the schedule.  One lane per LDE point and part; the parts write independent partial sums, so one launch covers
// them all: blockIdx.y selects the part (k_quotient_g1_parts below).
template <int part>
__device__ __forceinline__ void g1_add_part(const QArgs& A, size_t j) {
  const size_t M2 = A.stride;
  const u64* __restrict__ tl = A.tl;
  const qc64 W0 = QCONST(u64, A.W);
  const qc64 W1 = QCONST(u64, A.W + A.K);
  const qc32 W3 = QCONST(u32, A.W + 2 * (size_t)A.K);  // cut weights (accw_mad)
  u64 tot0 = 0, tot1 = 0;
  int e = 0;
  const int AUX = G1L::AUX;
  const u64 filter = TL(G1L::FILTER);
  const u64 is_x_eq_filter = TL(AUX + G1_AUX_IS_X_EQ_FILTER);
  u64 ax[16], lam[16], t16[16], u16[16];
  ld16(tl, M2, j, G1L::A, ax);
  if constexpr (part == 0) {
    // block 0: delta_x * inv - 1 + is_x_eq (eval_is_modulus_zero), then filter*is_x_eq*delta_x[i], then e = 49
    const u64 is_x_eq = TL(AUX + G1_AUX_IS_X_EQ);
    ld16(tl, M2, j, G1L::B, u16);
#pragma unroll
    for (int i = 0; i < 16; i++) u16[i] = gl_sub(u16[i], ax[i]);  // delta_x
    ld16(tl, M2, j, AUX + G1_AUX_IS_X_EQ_AUX, t16);               // inv limbs
    const u64 c0 = gl_sub(is_x_eq, 1);
    mz_block<true>(tl, M2, j, AUX + G1_AUX_IS_X_EQ_AUX + 16, A, G1_MZ_E0[0], 0,
             filter, [&](int i) __attribute__((always_inline)) { u64 v = conv16<true>(u16, t16, i); return i == 0 ? gl_add(v, c0) : v; }, tot0, tot1);
    e = 33;
    AccW g;
    accw_init(g);
#pragma unroll
    for (int i = 0; i < 16; i++) accw_mad(g, u16[i], W3 + 8 * (e + i));
    e += 16;
    u64 f = gl_mul(filter, is_x_eq);
    tot0 = gl_add(tot0, gl_mul(f, acc3_red(g.a0)));
    tot1 = gl_add(tot1, gl_mul(f, acc3_red(g.a1)));
    EMIT(gl_sub(gl_mul(filter, is_x_eq), is_x_eq_filter));  // e = 49
  } else if constexpr (part == 1) {
    // block 1: lambda*delta_x - (b.y - a.y) under filter - is_x_eq_filter
    ld16(tl, M2, j, AUX + G1_AUX_LAMBDA, lam);
    ld16(tl, M2, j, G1L::B, u16);
#pragma unroll
    for (int i = 0; i < 16; i++) u16[i] = gl_sub(u16[i], ax[i]);  // delta_x
    ld16(tl, M2, j, G1L::B + 16, t16);                          // b.y
    ld16(tl, M2, j, G1L::A + 16, ax);                           // a.y (a.x no longer needed)
#pragma unroll
    for (int i = 0; i < 16; i++) t16[i] = gl_sub(t16[i], ax[i]);  // b.y - a.y, formed here: three arrays live in the block, not four
    mz_block<true>(tl, M2, j, AUX + G1_AUX_LAMBDA_AUX, A, G1_MZ_E0[1], 1,
             gl_sub(filter, is_x_eq_filter),
             [&](int i) __attribute__((always_inline)) {
               u64 v = conv16<true>(lam, u16, i);
               return i < 16 ? gl_sub(v, t16[i < 16 ? i : 0]) : v;
             },
             tot0, tot1);
  } else if constexpr (part == 2) {
    // block 2: 2*lambda*a.y - 3*a.x^2 under is_x_eq_filter, then a.y == b.y (e = 116..131)
    ld16(tl, M2, j, AUX + G1_AUX_LAMBDA, lam);
    ld16(tl, M2, j, G1L::A + 16, u16);  // a.y
    mz_block<true>(tl, M2, j, AUX + G1_AUX_LAMBDA_AUX, A, G1_MZ_E0[2], 2,
             is_x_eq_filter,
             [&](int i) __attribute__((always_inline)) {
               u64 ly = conv16<true>(lam, u16, i), xx = conv16<true>(ax, ax, i);
               return gl_sub(gl_dbl(ly), gl_add(gl_dbl(xx), xx));
             },
             tot0, tot1);
    e = 116;
    ld16(tl, M2, j, G1L::B + 16, t16);
    AccW g;
    accw_init(g);
#pragma unroll
    for (int i = 0; i < 16; i++) accw_mad(g, gl_sub(u16[i], t16[i]), W3 + 8 * (e + i));
    tot0 = gl_add(tot0, gl_mul(is_x_eq_filter, acc3_red(g.a0)));
    tot1 = gl_add(tot1, gl_mul(is_x_eq_filter, acc3_red(g.a1)));
  } else if constexpr (part == 3) {
    // block 3: lambda^2 - (a.x + b.x + c.x)
    ld16(tl, M2, j, AUX + G1_AUX_LAMBDA, lam);
    ld16(tl, M2, j, G1L::B, t16);
    ld16(tl, M2, j, G1L::C, u16);
#pragma unroll
    for (int i = 0; i < 16; i++) ax[i] = gl_add(gl_add(ax[i], t16[i]), u16[i]);  // a.x + b.x + c.x: two arrays live in the block
    mz_block<true>(tl, M2, j, AUX + G1_AUX_X_AUX, A, G1_MZ_E0[3], 3, filter,
             [&](int i) __attribute__((always_inline)) {
               u64 v = conv16<true>(lam, lam, i);
               return i < 16 ? gl_sub(v, ax[i < 16 ? i : 0]) : v;
             },
             tot0, tot1);
  } else {
    // block 4: lambda*(c.x - a.x) + c.y + a.y
    ld16(tl, M2, j, AUX + G1_AUX_LAMBDA, lam);
    ld16(tl, M2, j, G1L::C, u16);
#pragma unroll
    for (int i = 0; i < 16; i++) u16[i] = gl_sub(u16[i], ax[i]);  // c.x - a.x
    ld16(tl, M2, j, G1L::C + 16, t16);                          // c.y
    ld16(tl, M2, j, G1L::A + 16, ax);                           // a.y
#pragma unroll
    for (int i = 0; i < 16; i++) t16[i] = gl_add(t16[i], ax[i]);  // c.y + a.y
    mz_block<true>(tl, M2, j, AUX + G1_AUX_Y_AUX, A, G1_MZ_E0[4], 4, filter,
             [&](int i) __attribute__((always_inline)) {
               u64 v = conv16<true>(lam, u16, i);
               return i < 16 ? gl_add(v, t16[i < 16 ? i : 0]) : v;
             },
             tot0, tot1);
  }
  store_part(A, part, j, tot0, tot1);
}

// All six parts of a proof in one grid: 6 x 2N lanes of independent work per launch instead of 2N lanes six times over, so
// a SIMD always has a next wave to start when one retires (no drain between parts).  The schedule (the longest part) takes
// blockIdx.y = 0: workgroups are dispatched x first, then y, so it starts first and does not form the tail.
__global__ __launch_bounds__(256, 2) void k_quotient_g1_parts(QArgs A) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.count) return;
  switch (blockIdx.y) {
    case 0: schedule_part<G1L, false>(A, j, q_next(A, j), 198, 5); break;
    case 1: g1_add_part<0>(A, j); break;
    case 2: g1_add_part<1>(A, j); break;
    case 3: g1_add_part<2>(A, j); break;
    case 4: g1_add_part<3>(A, j); break;
    default: g1_add_part<4>(A, j); break;
  }
}

__global__ __launch_bounds__(256) void k_quotient_finish(QArgs A, StarkShape sh) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.count) return;
  finish_point(A, sh, j);
}
void quotient_finish_launch(const QArgs& A, const StarkShape& sh, hipStream_t st) {
  k_quotient_finish<<<(unsigned)((A.count + 255) / 256), 256, 0, st>>>(A, sh);
}

// ---- per-context point tables ---------------------------------------------------------------------------------
__global__ void k_point_tables(u64* x, u64* lfirst, u64* llast, unsigned log_n, u64 w_n, u64 w_2n) {
  const size_t N = (size_t)1 << log_n;
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= 2 * N) return;
  size_t h = j >> log_n;
  u32 k = bitrev32((u32)(j & (N - 1)), log_n);
  u64 shift = h ? gl_mul(GL_GEN, w_2n) : GL_GEN;
  u64 xv = gl_mul(shift, gl_pow(w_n, k));
  u64 gn = gl_pow(GL_GEN, N);            // x^N = g^N * (-1)^h
  u64 zh = gl_sub(h ? gl_neg(gn) : gn, 1);
  u64 ninv = gl_inv((u64)N % GL_P);
  u64 winv = gl_inv(w_n);
  x[j] = xv;
  lfirst[j] = gl_mul(gl_mul(zh, ninv), gl_inv(gl_sub(xv, 1)));
  llast[j] = gl_mul(gl_mul(gl_mul(zh, ninv), winv), gl_inv(gl_sub(xv, winv)));
}

// the same constants for `count` consecutive rows k0 .. of coset h in natural order (window mode of QArgs)
__global__ void k_point_tables_window(u64* x, u64* lfirst, u64* llast, unsigned log_n, u32 h, size_t k0, size_t count, u64 w_n,
                                      u64 w_2n) {
  const size_t N = (size_t)1 << log_n;
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const u64 k = (k0 + j) & (N - 1);
  u64 shift = h ? gl_mul(GL_GEN, w_2n) : GL_GEN;
  u64 xv = gl_mul(shift, gl_pow(w_n, k));
  u64 gn = gl_pow(GL_GEN, N);
  u64 zh = gl_sub(h ? gl_neg(gn) : gn, 1);
  u64 ninv = gl_inv((u64)N % GL_P);
  u64 winv = gl_inv(w_n);
  x[j] = xv;
  lfirst[j] = gl_mul(gl_mul(zh, ninv), gl_inv(gl_sub(xv, 1)));
  llast[j] = gl_mul(gl_mul(gl_mul(zh, ninv), winv), gl_inv(gl_sub(xv, winv)));
}
void quotient_point_tables_window(u64* d_x, u64* d_lfirst, u64* d_llast, unsigned log_n, int h, size_t k0, size_t count, hipStream_t st) {
  k_point_tables_window<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(d_x, d_lfirst, d_llast, log_n, (u32)h, k0, count,
                                                                       gl_root_of_unity(log_n), gl_root_of_unity(log_n + 1));
}
void quotient_window_args(QArgs& A, const u64* d_tw, const u64* d_aw, const QPointTables& pt, u64* d_part, size_t stride, size_t count,
                          size_t k0, int h) {
  A.tl = d_tw;
  A.al = d_aw;
  A.pt = pt;
  A.part = d_part;
  A.stride = stride;
  A.count = count;
  A.k0 = k0;
  A.natural = 1;
  A.hsel = (u32)h;
}

void quotient_point_tables(u64* d_x, u64* d_lfirst, u64* d_llast, unsigned log_n, hipStream_t st) {
  size_t M2 = (size_t)2 << log_n;
  k_point_tables<<<(unsigned)((M2 + 255) / 256), 256, 0, st>>>(d_x, d_lfirst, d_llast, log_n, gl_root_of_unity(log_n),
                                                             gl_root_of_unity(log_n + 1));
}

// ---- host: alpha-dependent tables ---------------------------------------------------------------------------
void quotient_host_tables(int K, const u64 alphas[2], const int* mz_e0, int n_blocks, std::vector<u64>& W, std::vector<u64>& mzt) {
  W.assign(QUOTIENT_W_WORDS(K), 0);
  for (int a = 0; a < 2; a++) {
    u64 v = 1;
    for (int e = K - 1; e >= 0; e--) {
      W[(size_t)a * K + e] = v;
      v = gl_mul(v, alphas[a]);
    }
  }
  static const u64 MOD[16] = {64839, 55420, 35862, 15392, 51853, 26737, 27281, 38785,
                              22621, 33153, 17846, 47184, 41001, 57649, 20082, 12388};
  const u64 B = 1ULL << 16, OFF = 1ULL << 29;
  mzt.assign(QUOTIENT_MZT_WORDS, 0);
  for (int blk = 0; blk < n_blocks; blk++)
    for (int a = 0; a < 2; a++) {
      const u64* w = &W[(size_t)a * K + mz_e0[blk] + 1];  // w[i], i = 0..31: weight of constr_i
      u64* T = &mzt[(size_t)(blk * 2 + a) * 80];
      for (int jj = 0; jj < 17; jj++) {
        u64 s = 0;
        for (int t = 0; t < 16; t++)
          if (jj + t < 32) s = gl_add(s, gl_mul(w[jj + t], MOD[t]));
        T[jj] = s;
      }
      u64 usum = 0;
      for (int d = 0; d < 31; d++) {
        u64 u = gl_sub(w[d + 1], gl_mul(B, w[d]));
        T[17 + d] = u;
        T[48 + d] = gl_mul(B, u);
        usum = gl_add(usum, u);
      }
      T[79] = gl_mul(OFF, usum);
    }
  // the same weights cut in 22-bit limbs for accw_mad (quotient_common.h): 8 u32 per term, both alphas side by side
  for (int e = 0; e < K; e++) w3_store(&W[2 * (size_t)K + 4 * (size_t)e], W[e], W[(size_t)K + e]);
  for (int blk = 0; blk < n_blocks; blk++)
    for (int t = 0; t < 80; t++)
      w3_store(&mzt[QUOTIENT_MZT3_OFF + (size_t)(blk * 80 + t) * 4], mzt[(size_t)(blk * 2) * 80 + t], mzt[(size_t)(blk * 2 + 1) * 80 + t]);
}

void quotient_fill_args(QArgs& A, const StarkShape& sh, const u64* d_tl, const u64* d_al, const u64* d_W, const u64* d_mzt,
                        const QPointTables& pt, const u64 betas[2], const u64 gammas[2], unsigned log_n, u64* d_out,
                        u64* d_part) {
  A.tl = d_tl;
  A.al = d_al;
  A.W = d_W;
  A.mzt = d_mzt;
  A.pt = pt;
  for (int i = 0; i < 2; i++) {
    A.betas[i] = betas[i];
    A.gammas[i] = gammas[i];
  }
  const size_t N = (size_t)1 << log_n;
  u64 gn = gl_pow(GL_GEN, N);
  A.zh_inv[0] = gl_inv(gl_sub(gn, 1));
  A.zh_inv[1] = gl_inv(gl_sub(gl_neg(gn), 1));
  A.w_inv = gl_inv(gl_root_of_unity(log_n));
  A.out = d_out;
  A.part = d_part;
  A.n_parts = 0;
  A.log_n = log_n;
  A.K = sh.n_total_constraints();
  A.stride = A.count = 2 * N;  // the whole LDE domain in leaf order; quotient_window_args() narrows it
  A.k0 = 0;
  A.natural = 0;
  A.hsel = 0;
}

int g1_quotient_mz_blocks(const int** e0) {
  *e0 = G1_MZ_E0;
  return 5;
}
void g1_quotient_launch(const QArgs& A0, const StarkShape& sh, hipStream_t st) {
  QArgs A = A0;
  A.n_parts = 6;
  const unsigned g = (unsigned)((A.count + 255) / 256);
  k_quotient_g1_parts<<<dim3(g, 6), 256, 0, st>>>(A);
  quotient_finish_launch(A, sh, st);
}

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void quotient_g1_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_point_tables));
}
