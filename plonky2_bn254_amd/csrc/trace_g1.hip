// G1 scalar-multiplication STARK: trace generation on the GPU (K-trace-A / K-trace-B of DESIGN.md).
//
// Replaces the single-threaded CPU loops of the reference:
//   G1ScalarMulStark::generate_trace / generate_one_set / generate_first_row / generate_transition
//     (src/starks/curves/g1/scalar_mul_stark.rs:55-213),
//   generate_g1_add (src/starks/curves/g1/add.rs:52-122),
//   generate_is_modulus_zero (src/starks/modular/is_modulus_zero.rs:36-66),
//   generate_modulus_zero (src/starks/modular/modulus_zero.rs:77-123, incl. pol_remove_root_2exp),
//   generate_round_flags (src/starks/common/round_flags.rs:21-44), generate_range_checks (:71-87).
// Column layout: src/starks/curves/g1/scalar_mul_view.rs:34-49 (G1L, layout.h).
//
// Phase A (no inversions, Jacobian coordinates): the 256 doublings D_k = 2^k x are the only sequential part (one lane per
// instance); the running sums S_k and C_k = S_k + D_k come from a 256-lane prefix scan per instance (chain_scan.h).
// Every intermediate point (offset, C_k, D_k) is stored.  Phase A': all Z are inverted with Montgomery's batch trick
// (trace_shared.hip).  Phase B (one thread per trace row): affine a, b, c, lambda and the limb / quotient / carry witnesses;
// the exact division by p is a multiplication by p^-1 mod 2^288.
// The trace is written column-major (trace[c*N + row]), so consecutive lanes write consecutive words.
#include "trace_common.h"
#include "chain_coop.h"
#include "trace.h"

// ---- phase A: doubling chain (sequential); the running sums are k_sum_scan<CurveG1> (trace_common.h) ----------------
// Cooperative form of the chain: four lanes per instance, lane p computes the p-th product of a level, the sums between the
// products are integer combinations with one reduction each (chain_coop.h), values travel through LDS:
//   level 1   a = X^2            b = Y^2              Z' = (2Y) Z
//   level 2   c = b^2            s = (X + b)^2        f = (3a)^2
//   combine   X' = f + 4a + 4c - 4s                   w = 6s - 6a - 6c - f          (= d - X' with d = 2 (s - a - c))
//   level 3   m = (3a) w
//   combine   Y' = m - 8c
// Same formulas as g1_double, every stored value canonical: the points are bit for bit those of k_dbl_chain_one_lane, in 3 products
// + 2 reductions of latency per doubling instead of 7 products + 13 additions.
namespace g1coop {
using namespace chain_coop;
enum { SX, SY, SZ, SA, SB, SC, SS, SF, SWW, SM, NSLOT };
constexpr int INST_W = NSLOT * SLOT_W;
// (product: chain_coop.h)
}  // namespace g1coop

__global__ __launch_bounds__(64) void k_g1_dbl_chain_coop(const u64* __restrict__ xs, int n, u64* __restrict__ px,
                                                          u64* __restrict__ py, u64* __restrict__ pz) {
  using namespace g1coop;
  LATENCY_KERNEL_PRIO();
  __shared__ __attribute__((aligned(16))) u32 lds[16 * INST_W];
  const int lane = threadIdx.x, grp = lane >> 2, p = lane & 3;
  const int inst_raw = blockIdx.x * 16 + grp;
  const bool live = inst_raw < n;
  const int inst = live ? inst_raw : n - 1;  // idle groups shadow the last instance and store nothing
  u32* g = lds + grp * INST_W;
  const size_t cnt = (size_t)NPTS * n;
  if (p < 2) {
    lds_st(g, p == 0 ? SX : SY, fq_from_canonical(xs + 8 * inst + 4 * p));
  } else if (p == 2) {
    lds_st(g, SZ, fq_one());
  }
  u64* const out = p == 0 ? px : p == 1 ? py : pz;
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k <= 256; k++) {
    const size_t e = (size_t)(257 + k) * n + inst;
    if (live && p < 3) st_fq(out, cnt, e, lds_ld(g, p));  // slots SX, SY, SZ = 0, 1, 2
    if (k == 256) break;
    {  // level 1 (lane 3 repeats lane 0)
      const int sa = p == 1 || p == 2 ? SY : SX, sb = p == 1 ? SY : p == 2 ? SZ : SX;
      const fq r = product(g, sa, sa, p == 2 ? 2u : 1u, 0u, sb, sb, 1u, 0u);
      __syncthreads();
      if (p < 3) lds_st(g, p == 0 ? SA : p == 1 ? SB : SZ, r);
    }
    __syncthreads();
    {  // level 2: b b, (X + b)(X + b), (3a)(3a)
      const int s1 = p == 1 ? SX : p == 2 ? SA : SB;
      const u32 f = p == 2 ? 3u : 1u, gg = p == 1 ? 1u : 0u;
      const fq r = product(g, s1, SB, f, gg, s1, SB, f, gg);
      if (p < 3) lds_st(g, p == 0 ? SC : p == 1 ? SS : SF, r);  // the slots written are not read at this level
    }
    __syncthreads();
    {  // X' = f + 4a + 4c - 4s (+ 4p) on lane 0, w = 6s - 6a - 6c - f (+ 13p) on lane 1
      const bool w = p == 1;
      const fq r = combine(g, SF, w ? -1 : 1, SA, w ? -6 : 4, SC, w ? -6 : 4, SS, w ? 6 : -4, w ? 13 : 4);
      if (p < 2) lds_st(g, w ? SWW : SX, r);  // X is not read again in this doubling
    }
    __syncthreads();
    {  // level 3: m = (3a) w
      const fq r = product(g, SA, SA, 3u, 0u, SWW, SWW, 1u, 0u);
      if (p == 0) lds_st(g, SM, r);
    }
    __syncthreads();
    {  // Y' = m - 8c (+ 8p)
      const fq r = combine(g, SM, 1, SC, -8, SC, 0, SC, 0, 8);
      if (p == 0) lds_st(g, SY, r);
    }
    __syncthreads();
  }
}

// ---- phase B ------------------------------------------------------------------------------------------------
// denominators: add row: b.x - a.x (or 2 a.y when the x coincide); doubling row: 2 a.y
__global__ __launch_bounds__(64) void k_g1_row_den(const u64* __restrict__ scalars, int n, const u64* __restrict__ pts,
                                                   const u64* __restrict__ zi, u64* __restrict__ den) {
  LATENCY_KERNEL_PRIO();
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t nrows = (size_t)n * 512;
  if (r >= nrows) return;
  const RowPos pos = row_pos(r, scalars);
  const int inst = pos.inst, k = pos.k;
  size_t cnt = (size_t)NPTS * n;
  fq d;
  if (pos.adding()) {
    AffPt<g1j> a = affine_pt<g1j>(pts, zi, cnt, (size_t)sum_point(pos.s, k) * n + inst);
    AffPt<g1j> b = affine_pt<g1j>(pts, zi, cnt, (size_t)(257 + k) * n + inst);
    d = fq_sub(b.x, a.x);
    if (fq_is_zero(d)) d = fq_dbl(a.y);
  } else {
    AffPt<g1j> a = affine_pt<g1j>(pts, zi, cnt, (size_t)(257 + k) * n + inst);
    d = fq_dbl(a.y);
  }
  st_fq(den, nrows, r, d);
}

// one thread per trace row
__global__ __launch_bounds__(64) void k_g1_rows(const u64* __restrict__ scalars, int n, const u64* __restrict__ pts,
                                                const u64* __restrict__ zi, const u64* __restrict__ deninv,
                                                const u64* __restrict__ rf_tbl, u64* __restrict__ trace, size_t N,
                                                int* __restrict__ err) {
  LATENCY_KERNEL_PRIO();
  typedef G1L L;
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t nrows = (size_t)n * 512;
  if (r >= nrows) return;
  const RowPos pos = row_pos(r, scalars);
  const int inst = pos.inst, k = pos.k;
  const bool adding = pos.adding(), bitk = pos.bitk();
  const size_t cnt = (size_t)NPTS * n;

  // Three affine points per row, one after the other (packed into limbs at once, trace_common.h):  P1 = the running sum S (S_(k-1) on
  // an adding row, S_k on a doubling row), P2 = D_k, P3 = C_k (adding) or D_(k+1) (doubling).   adding: a = P1, b = P2, c = P3,
  // double = P2, sum = bit ? P3 : P1;   doubling: a = b = P2, c = P3, double = P3, sum = P1.
  auto put = [&](int col, u64 v) { trace[(size_t)col * N + r] = v; };
  auto put_p = [&](int col, const P16& p) { p16_put(trace, N, r, col, p); };
  P16 ax, ay, bx, by, lam, invl, s1x, s1y;
  bool x_eq;
  {
    const AffPt<g1j> p1 = affine_pt<g1j>(pts, zi, cnt, (size_t)sum_point(pos.s, adding ? k : k + 1) * n + inst);
    const AffPt<g1j> p2 = affine_pt<g1j>(pts, zi, cnt, (size_t)(257 + k) * n + inst);
    AffPt<g1j> a = p2;
    if (adding) a = p1;
    const AffPt<g1j>& b = p2;
    const fq di = ld_fq(deninv, nrows, r);
    x_eq = fq_eq(a.x, b.x);
    fq lambda, inv;
    if (!x_eq) {
      lambda = fq_mul(fq_sub(b.y, a.y), di);  // add.rs:66
      inv = di;
    } else {
      fq xx = fq_sqr(a.x);
      lambda = fq_mul(fq_add(fq_dbl(xx), xx), di);  // 3x^2 / 2y, add.rs:80
      inv = fq_zero();
    }
    ax = p16_pack(a.x); ay = p16_pack(a.y); bx = p16_pack(b.x); by = p16_pack(b.y);
    lam = p16_pack(lambda); invl = p16_pack(inv);
    s1x = p16_pack(p1.x); s1y = p16_pack(p1.y);
  }
  put_p(L::A, ax); put_p(L::A + 16, ay);
  put_p(L::B, bx); put_p(L::B + 16, by);
  put_p(L::AUX + G1_AUX_LAMBDA, lam);
  put_p(L::AUX + G1_AUX_IS_X_EQ_AUX, invl);
  P16 cx, cy;
  {
    const AffPt<g1j> p3 = affine_pt<g1j>(pts, zi, cnt, (size_t)(adding ? 1 + k : 258 + k) * n + inst);
    cx = p16_pack(p3.x);
    cy = p16_pack(p3.y);
  }
  put_p(L::C, cx); put_p(L::C + 16, cy);
  put_p(L::DOUBLE, p16_sel(adding, bx, cx)); put_p(L::DOUBLE + 16, p16_sel(adding, by, cy));
  const bool sum_is_c = adding && bitk;
  put_p(L::SUM, p16_sel(sum_is_c, cx, s1x)); put_p(L::SUM + 16, p16_sel(sum_is_c, cy, s1y));
  const u64 is_x_eq = x_eq ? 1 : 0;
  put(L::AUX + G1_AUX_IS_X_EQ, is_x_eq);
  put(L::AUX + G1_AUX_IS_X_EQ_FILTER, is_x_eq);

  __shared__ long long mz_buf[31][MZ_LANES];  // the polynomial of the current witness block (trace_common.h)
  mz_lds_t* const slots = (mz_lds_t*)&mz_buf[0][threadIdx.x];
  auto mac = [&](int coef, const P16& x, const P16* xs, const P16& y, const P16* ys) {
    mac_lds(slots, coef * 4 + (xs ? 1 : ys ? 2 : 0), x, y, xs ? *xs : ys ? *ys : x);
  };
  auto emit = [&](int col) { gen_modulus_zero_lds(slots, trace, N, r, col, err); };
  // is_modulus_zero witness: delta_x * inv - 1 + is_zero   (is_modulus_zero.rs:57-59)
  zero_lds(slots);
  mac(1, bx, &ax, invl, nullptr);
  slots[0] += (long long)is_x_eq - 1;
  emit(L::AUX + G1_AUX_IS_X_EQ_AUX + 16);
  // lambda witness
  zero_lds(slots);
  if (!x_eq) {  // lambda*(b.x-a.x) - (b.y-a.y)
    mac(1, lam, nullptr, bx, &ax);
    lin_lds(slots, -1, by);
    lin_lds(slots, 1, ay);
  } else {  // 2*a.y*lambda - 3*a.x^2
    mac(2, lam, nullptr, ay, nullptr);
    mac(-3, ax, nullptr, ax, nullptr);
  }
  emit(L::AUX + G1_AUX_LAMBDA_AUX);
  // x witness: lambda^2 - (a.x + b.x + c.x)
  zero_lds(slots);
  mac(1, lam, nullptr, lam, nullptr);
  lin_lds(slots, -1, ax);
  lin_lds(slots, -1, bx);
  lin_lds(slots, -1, cx);
  emit(L::AUX + G1_AUX_X_AUX);
  // y witness: lambda*(c.x - a.x) + c.y + a.y
  zero_lds(slots);
  mac(1, lam, nullptr, cx, &ax);
  lin_lds(slots, 1, cy);
  lin_lds(slots, 1, ay);
  emit(L::AUX + G1_AUX_Y_AUX);

  put_schedule<L>(trace, N, r, pos, rf_tbl);
}

// ---- host driver ------------------------------------------------------------------------------------------------
// word offsets of the arrays in the scratch buffer: the points (X, Y, Z: pa_load), the inverses of Z, the row denominators
// and their inverses, then the tail all kinds have
struct G1Scratch : ScratchCarve {
  size_t pts, zi, den, deninv, rf, hist;
  explicit G1Scratch(size_t n) {
    const size_t cnt = (size_t)NPTS * n, nrows = n * 512;
    pts = take(3 * 4 * cnt), zi = take(4 * cnt), den = take(4 * nrows), deninv = take(4 * nrows);
    rf = take(RF_WORDS), hist = take(HIST_WORDS);
  }
};
size_t g1_trace_scratch_words(size_t n) { return G1Scratch(n).words; }

int g1_generate_trace_device(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N,
                             u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range) {
  typedef G1L L;
  const size_t cnt = (size_t)NPTS * n, nrows = n * 512;
  const G1Scratch sc(n);
  u64 *pts = d_scratch + sc.pts, *zi = d_scratch + sc.zi, *den = d_scratch + sc.den, *deninv = d_scratch + sc.deninv;
  u64* rf = d_scratch + sc.rf;
  u32* hist = (u32*)(d_scratch + sc.hist);
  if (nrows < N) hipMemsetAsync(d_trace, 0, (size_t)L::W * N * 8, st);
  launch_round_flag_table(rf, st);
  static const bool one_lane_chain = getenv("BN254S_G1_CHAIN_ONE_LANE") != nullptr;  // A/B measurements
  if (one_lane_chain)
    k_dbl_chain_one_lane<CurveG1><<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_x, (int)n, pts, nullptr);
  else
    launch_g1_dbl_chain(d_x, (int)n, pts, pts + 4 * cnt, pts + 8 * cnt, st);
  k_sum_scan<CurveG1><<<(unsigned)n, 256, 0, st>>>(d_scalars, d_off, (int)n, pts, nullptr, d_err);
  launch_fq_batch_inv(pts + 8 * cnt, zi, cnt, st);
  k_g1_row_den<<<(unsigned)((nrows + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zi, den);
  launch_fq_batch_inv(den, deninv, nrows, st);
  k_g1_rows<<<(unsigned)((nrows + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zi, deninv, rf, d_trace, N, d_err);
  if (with_range) launch_range_columns(d_trace, N, L::RC_BEGIN, L::RC_END, L::FREQ, L::RANGE, hist, d_err, st);
  if (d_outputs) k_outputs<CurveG1><<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zi, d_outputs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

void launch_g1_dbl_chain(const u64* d_x, int n, u64* px, u64* py, u64* pz, hipStream_t st) {
  k_g1_dbl_chain_coop<<<(unsigned)((n + 15) / 16), 64, 0, st>>>(d_x, n, px, py, pz);
}

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void trace_g1_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_g1_rows));
}
