// G2 scalar-multiplication and Fq-exponentiation STARKs: trace generation on the GPU.
//
// Replaces, for G2: G2ScalarMulStark::generate_trace / generate_one_set (src/starks/curves/g2/scalar_mul_stark.rs:55-213,
// the textual twin of the G1 file), generate_g2_add (src/starks/curves/g2/add.rs:59-130),
// generate_is_ext_modulus_zero / generate_ext_modulus_zero (g2/ext/is_modulus_zero.rs:30-46, ext/modulus_zero.rs:38-46)
// and the Fq2 limb-polynomial helpers (g2/ext/{mul,add,sub,convert}.rs);
// for Fq exp: FqExpStark::generate_trace / generate_one_set (src/starks/fields/exp_stark.rs:53-206) and
// generate_fq_mul (src/starks/fields/mul.rs:22-40).
// Same structure as trace_g1.hip: a sequential inversion-free chain per instance, Montgomery batch inversion,
// then one lane per trace row.  The points are six SoA Fq vectors one after the other, X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1
// (pa_load, trace_common.h); the batched inversion works on Fq, so the norm of every Z is kept beside them (znorm).
#include "trace_common.h"
#include "chain_coop.h"
#include "trace.h"

// ======================================== G2 ==================================================================
// phase A as in trace_g1.hip: sequential doubling chain, then the running sums by a parallel scan (k_sum_scan<CurveG2>)
// ---- cooperative doubling chain: eight lanes per instance ----------------------------------------------------------
// The chain is 256 dependent doublings; one lane per instance leaves 2 waves running 6.7 k instructions per doubling.  Here
// lane (p, c) of an instance's group of eight computes component c of the p-th Fq2 product of a level (a component is ONE
// two-product Montgomery reduction), values travel through LDS, and the sums between the products are evaluated as small
// integer combinations with one reduction each:
//   level 1   a = X^2            b = Y^2              Z' = (2Y) Z          n = |Z|^2 (lane (3, 0): the norm the inversion needs)
//   level 2   c = b^2            s = (X + b)^2        f = (3a)^2
//   combine   X' = f + 4a + 4c - 4s                   w = 6s - 6a - 6c - f          (= d - X' with d = 2 (s - a - c))
//   level 3   m = (3a) w
//   combine   Y' = m - 8c
// Same formulas as g2_double, every stored value canonical: the chain's points are bit for bit those of k_dbl_chain_one_lane.
namespace g2coop {
using namespace chain_coop;
enum { SX, SY, SZ, SA, SB, SC, SS, SF, SWW, SM, NSLOT };
constexpr int INST_W = NSLOT * 2 * SLOT_W;  // dwords per instance
// (product: chain_coop.h)
}  // namespace g2coop

// The c0 and c1 vectors of a coordinate reach the chain as a pair passed by value, as they always have.  (Measured at 128
// instances: with six pointer arguments, or one base pointer and the vector chosen by arithmetic, the same loop takes 1.16 ms
// instead of 1.10 ms, profiles/trace_refactor_times.txt.)
struct VecPair {
  u64 *c0, *c1;
};
__global__ __launch_bounds__(64) void k_g2_dbl_chain_coop(const u64* __restrict__ xs, int n, VecPair px, VecPair py, VecPair pz,
                                                          u64* __restrict__ znorm) {
  using namespace g2coop;
  LATENCY_KERNEL_PRIO();
  __shared__ __attribute__((aligned(16))) u32 lds[8 * INST_W];
  const int lane = threadIdx.x, grp = lane >> 3, p = (lane >> 1) & 3, c = lane & 1;
  const int inst_raw = blockIdx.x * 8 + grp;
  const bool live = inst_raw < n;
  const int inst = live ? inst_raw : n - 1;  // idle groups shadow the last instance and store nothing
  u32* g = lds + grp * INST_W;
  const size_t cnt = (size_t)NPTS * n;
  if (p < 2) {
    lds_st(g, 2 * (p == 0 ? SX : SY) + c, fq_from_canonical(xs + 16 * inst + 8 * p + 4 * c));
  } else if (p == 2) {
    lds_st(g, 2 * SZ + c, c ? fq_zero() : fq_one());
  }
  u64* const out = p == 0 ? (c ? px.c1 : px.c0) : p == 1 ? (c ? py.c1 : py.c0) : (c ? pz.c1 : pz.c0);
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k <= 256; k++) {
    const size_t e = (size_t)(257 + k) * n + inst;
    if (live && p < 3) st_fq(out, cnt, e, lds_ld(g, 2 * p + c));  // slots SX, SY, SZ = 0, 1, 2
    {  // level 1
      const int sa = p == 0 ? SX : p == 3 ? SZ : SY, sb = p == 0 ? SX : p == 1 ? SY : SZ;
      const fq r = product(g, c, p == 3, sa, sa, p == 2 ? 2u : 1u, 0u, sb, sb, 1u, 0u);
      __syncthreads();
      if (p == 3) {
        if (live && c == 0) st_fq(znorm, cnt, e, r);
      } else {
        lds_st(g, 2 * (p == 0 ? SA : p == 1 ? SB : SZ) + c, r);
      }
    }
    if (k == 256) break;
    __syncthreads();
    {  // level 2: b b, (X + b)(X + b), (3a)(3a); the fourth pair repeats the first
      const int s1 = p == 1 ? SX : p == 2 ? SA : SB, s2 = SB;
      const u32 f = p == 2 ? 3u : 1u, gg = p == 1 ? 1u : 0u;
      const fq r = product(g, c, false, s1, s2, f, gg, s1, s2, f, gg);
      if (p < 3) lds_st(g, 2 * (p == 0 ? SC : p == 1 ? SS : SF) + c, r);  // written slots are not read at this level
    }
    __syncthreads();
    {  // X' = f + 4a + 4c - 4s (pair 0, + 4p), w = 6s - 6a - 6c - f (pair 1, + 13p); the other pairs repeat pair 0
      const bool w = p == 1;
      const fq r = combine(g, 2 * SF + c, w ? -1 : 1, 2 * SA + c, w ? -6 : 4, 2 * SC + c, w ? -6 : 4, 2 * SS + c, w ? 6 : -4, w ? 13 : 4);
      if (p < 2) lds_st(g, 2 * (w ? SWW : SX) + c, r);  // X is not read again in this doubling
    }
    __syncthreads();
    {  // level 3: m = (3a) w
      const fq r = product(g, c, false, SA, SA, 3u, 0u, SWW, SWW, 1u, 0u);
      if (p == 0) lds_st(g, 2 * SM + c, r);
    }
    __syncthreads();
    {  // Y' = m - 8c (+ 8p)
      const fq r = combine(g, 2 * SM + c, 1, 2 * SC + c, -8, 2 * SC + c, 0, 2 * SC + c, 0, 8);
      if (p == 0) lds_st(g, 2 * SY + c, r);
    }
    __syncthreads();
  }
}

// per row: inv-input slots [0] = norm(den), [1] = dx.c0, [2] = dx.c1  (each an Fq SoA vector of nrows)
__global__ __launch_bounds__(64) void k_g2_row_den(const u64* __restrict__ scalars, int n, const u64* __restrict__ pts,
                                                   const u64* __restrict__ zni, u64* __restrict__ inv_in) {
  LATENCY_KERNEL_PRIO();
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t nrows = (size_t)n * 512;
  if (r >= nrows) return;
  const RowPos pos = row_pos(r, scalars);
  const int inst = pos.inst, k = pos.k;
  size_t cnt = (size_t)NPTS * n;
  fq2 den, dx = fq2_zero();
  if (pos.adding()) {
    AffPt<g2j> a = affine_pt<g2j>(pts, zni, cnt, (size_t)sum_point(pos.s, k) * n + inst);
    AffPt<g2j> b = affine_pt<g2j>(pts, zni, cnt, (size_t)(257 + k) * n + inst);
    dx = fq2_sub(b.x, a.x);
    den = fq2_is_zero(dx) ? fq2_dbl(a.y) : dx;
  } else {
    AffPt<g2j> a = affine_pt<g2j>(pts, zni, cnt, (size_t)(257 + k) * n + inst);
    den = fq2_dbl(a.y);
  }
  st_fq(inv_in, 3 * nrows, r, fq2_norm(den));
  st_fq(inv_in, 3 * nrows, nrows + r, dx.c0);
  st_fq(inv_in, 3 * nrows, 2 * nrows + r, dx.c1);
}

__global__ __launch_bounds__(64) void k_g2_rows(const u64* __restrict__ scalars, int n, const u64* __restrict__ pts,
                                                const u64* __restrict__ zni, const u64* __restrict__ inv_out,
                                                const u64* __restrict__ rf_tbl, u64* __restrict__ trace, size_t N,
                                                int* __restrict__ err) {
  LATENCY_KERNEL_PRIO();
  typedef G2L L;
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t nrows = (size_t)n * 512;
  if (r >= nrows) return;
  const RowPos pos = row_pos(r, scalars);
  const int inst = pos.inst, k = pos.k;
  const bool adding = pos.adding(), bitk = pos.bitk();
  const size_t cnt = (size_t)NPTS * n;
  // Three affine points per row, one after the other (the field elements of a point are packed into limbs and dropped before the
  // next conversion starts):  P1 = the running sum S (S_(k-1) on an adding row, S_k on a doubling row), P2 = D_k, P3 = C_k (adding)
  // or D_(k+1) (doubling).   adding: a = P1, b = P2, c = P3, double = P2, sum = bit ? P3 : P1;   doubling: a = b = P2, c = P3,
  // double = P3, sum = P1.
  auto put = [&](int col, u64 v) { trace[(size_t)col * N + r] = v; };
  auto put_p = [&](int col, const P16& p) { p16_put(trace, N, r, col, p); };
  P16 ax0, ax1, ay0, ay1, bx0, bx1, by0, by1, l0, l1, s1x0, s1x1, s1y0, s1y1;
  bool z0, z1, x_eq;
  {
    const AffPt<g2j> p1 = affine_pt<g2j>(pts, zni, cnt, (size_t)sum_point(pos.s, adding ? k : k + 1) * n + inst);
    const AffPt<g2j> p2 = affine_pt<g2j>(pts, zni, cnt, (size_t)(257 + k) * n + inst);
    AffPt<g2j> a = p2;
    if (adding) a = p1;
    const AffPt<g2j>& b = p2;
    const fq2 dxm = fq2_sub(b.x, a.x);
    z0 = fq_is_zero(dxm.c0);
    z1 = fq_is_zero(dxm.c1);
    x_eq = z0 && z1;
    const fq2 den = x_eq ? fq2_dbl(a.y) : dxm;
    const fq2 di = fq2_inv_from_norm_inv(den, ld_fq(inv_out, 3 * nrows, r));
    fq2 lambda;
    if (!x_eq) {
      lambda = fq2_mul(fq2_sub(b.y, a.y), di);  // g2/add.rs:73
    } else {
      fq2 xx = fq2_sqr(a.x);
      lambda = fq2_mul(fq2_add(fq2_dbl(xx), xx), di);  // g2/add.rs:86
    }
    ax0 = p16_pack(a.x.c0); ax1 = p16_pack(a.x.c1); ay0 = p16_pack(a.y.c0); ay1 = p16_pack(a.y.c1);
    bx0 = p16_pack(b.x.c0); bx1 = p16_pack(b.x.c1); by0 = p16_pack(b.y.c0); by1 = p16_pack(b.y.c1);
    l0 = p16_pack(lambda.c0); l1 = p16_pack(lambda.c1);
    s1x0 = p16_pack(p1.x.c0); s1x1 = p16_pack(p1.x.c1); s1y0 = p16_pack(p1.y.c0); s1y1 = p16_pack(p1.y.c1);
  }
  put_p(L::A, ax0); put_p(L::A + 16, ax1); put_p(L::A + 32, ay0); put_p(L::A + 48, ay1);
  put_p(L::B, bx0); put_p(L::B + 16, bx1); put_p(L::B + 32, by0); put_p(L::B + 48, by1);
  put_p(L::AUX + G2_AUX_LAMBDA, l0); put_p(L::AUX + G2_AUX_LAMBDA + 16, l1);
  P16 cx0, cx1, cy0, cy1;
  {
    const AffPt<g2j> p3 = affine_pt<g2j>(pts, zni, cnt, (size_t)(adding ? 1 + k : 258 + k) * n + inst);
    cx0 = p16_pack(p3.x.c0); cx1 = p16_pack(p3.x.c1); cy0 = p16_pack(p3.y.c0); cy1 = p16_pack(p3.y.c1);
  }
  put_p(L::C, cx0); put_p(L::C + 16, cx1); put_p(L::C + 32, cy0); put_p(L::C + 48, cy1);
  // double = adding ? b : c;  sum = adding ? (bit ? c : a (= P1)) : P1
  put_p(L::DOUBLE, p16_sel(adding, bx0, cx0)); put_p(L::DOUBLE + 16, p16_sel(adding, bx1, cx1));
  put_p(L::DOUBLE + 32, p16_sel(adding, by0, cy0)); put_p(L::DOUBLE + 48, p16_sel(adding, by1, cy1));
  const bool sum_is_c = adding && bitk;
  put_p(L::SUM, p16_sel(sum_is_c, cx0, s1x0)); put_p(L::SUM + 16, p16_sel(sum_is_c, cx1, s1x1));
  put_p(L::SUM + 32, p16_sel(sum_is_c, cy0, s1y0)); put_p(L::SUM + 48, p16_sel(sum_is_c, cy1, s1y1));
  put(L::AUX + G2_AUX_IS_X_EQ, x_eq);
  put(L::AUX + G2_AUX_IS_C0_ZERO, z0);
  put(L::AUX + G2_AUX_IS_C1_ZERO, z1);
  put(L::AUX + G2_AUX_IS_X_EQ_FILTER, x_eq);
  const fq inv0 = ld_fq(inv_out, 3 * nrows, nrows + r), inv1 = ld_fq(inv_out, 3 * nrows, 2 * nrows + r);
  __shared__ long long mz_buf[31][MZ_LANES];  // the polynomial of the current witness block (trace_common.h)
  mz_lds_t* const slots = (mz_lds_t*)&mz_buf[0][threadIdx.x];
  auto mac = [&](int coef, const P16& x, const P16* xs, const P16& y, const P16* ys) {
    mac_lds(slots, coef * 4 + (xs ? 1 : ys ? 2 : 0), x, y, xs ? *xs : ys ? *ys : x);
  };
  auto emit = [&](int col) { gen_modulus_zero_lds(slots, trace, N, r, col, err); };
  // is_modulus_zero witnesses of delta_x.c0 and delta_x.c1 (ext/is_modulus_zero.rs:35-36): (b.x - a.x).ck * inv_k - 1 + is_zero_k
  {
    const P16 t = p16_pack(inv0);
    put_p(L::AUX + G2_AUX_C0_AUX, t);
    zero_lds(slots);
    mac(1, bx0, &ax0, t, nullptr);
    slots[0] += (long long)z0 - 1;
    emit(L::AUX + G2_AUX_C0_AUX + 16);
  }
  {
    const P16 t = p16_pack(inv1);
    put_p(L::AUX + G2_AUX_C1_AUX, t);
    zero_lds(slots);
    mac(1, bx1, &ax1, t, nullptr);
    slots[0] += (long long)z1 - 1;
    emit(L::AUX + G2_AUX_C1_AUX + 16);
  }
  // lambda witness
  if (!x_eq) {  // lambda * (b.x - a.x) - (b.y - a.y)
    zero_lds(slots);
    mac(1, l0, nullptr, bx0, &ax0);
    mac(-1, l1, nullptr, bx1, &ax1);
    lin_lds(slots, -1, by0);
    lin_lds(slots, 1, ay0);
    emit(L::AUX + G2_AUX_LAMBDA_AUX);
    zero_lds(slots);
    mac(1, l0, nullptr, bx1, &ax1);
    mac(1, l1, nullptr, bx0, &ax0);
    lin_lds(slots, -1, by1);
    lin_lds(slots, 1, ay1);
    emit(L::AUX + G2_AUX_LAMBDA_AUX + 80);
  } else {  // 2 * lambda * a.y - 3 * a.x^2
    zero_lds(slots);
    mac(2, l0, nullptr, ay0, nullptr);
    mac(-2, l1, nullptr, ay1, nullptr);
    mac(-3, ax0, nullptr, ax0, nullptr);
    mac(3, ax1, nullptr, ax1, nullptr);
    emit(L::AUX + G2_AUX_LAMBDA_AUX);
    zero_lds(slots);
    mac(2, l0, nullptr, ay1, nullptr);
    mac(2, l1, nullptr, ay0, nullptr);
    mac(-6, ax0, nullptr, ax1, nullptr);
    emit(L::AUX + G2_AUX_LAMBDA_AUX + 80);
  }
  // x witness: lambda^2 - (a.x + b.x + c.x)
  zero_lds(slots);
  mac(1, l0, nullptr, l0, nullptr);
  mac(-1, l1, nullptr, l1, nullptr);
  lin_lds(slots, -1, ax0);
  lin_lds(slots, -1, bx0);
  lin_lds(slots, -1, cx0);
  emit(L::AUX + G2_AUX_X_AUX);
  zero_lds(slots);
  mac(2, l0, nullptr, l1, nullptr);
  lin_lds(slots, -1, ax1);
  lin_lds(slots, -1, bx1);
  lin_lds(slots, -1, cx1);
  emit(L::AUX + G2_AUX_X_AUX + 80);
  // y witness: lambda*(c.x - a.x) + c.y + a.y
  zero_lds(slots);
  mac(1, l0, nullptr, cx0, &ax0);
  mac(-1, l1, nullptr, cx1, &ax1);
  lin_lds(slots, 1, cy0);
  lin_lds(slots, 1, ay0);
  emit(L::AUX + G2_AUX_Y_AUX);
  zero_lds(slots);
  mac(1, l0, nullptr, cx1, &ax1);
  mac(1, l1, nullptr, cx0, &ax0);
  lin_lds(slots, 1, cy1);
  lin_lds(slots, 1, ay1);
  emit(L::AUX + G2_AUX_Y_AUX + 80);

  put_schedule<L>(trace, N, r, pos, rf_tbl);
}

// word offsets of the arrays in the scratch buffer: the points, the norms of Z and their inverses, the three inversion inputs
// per row (k_g2_row_den) and their inverses, then the tail all kinds have
struct G2Scratch : ScratchCarve {
  size_t pts, znorm, zni, inv_in, inv_out, rf, hist;
  explicit G2Scratch(size_t n) {
    const size_t cnt = (size_t)NPTS * n, nrows = n * 512;
    pts = take(3 * 8 * cnt), znorm = take(4 * cnt), zni = take(4 * cnt), inv_in = take(4 * 3 * nrows), inv_out = take(4 * 3 * nrows);
    rf = take(RF_WORDS), hist = take(HIST_WORDS);
  }
};
size_t g2_trace_scratch_words(size_t n) { return G2Scratch(n).words; }

int g2_generate_trace_device(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N,
                             u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range) {
  typedef G2L L;
  const size_t cnt = (size_t)NPTS * n, nrows = n * 512;
  const G2Scratch sc(n);
  u64 *pts = d_scratch + sc.pts, *znorm = d_scratch + sc.znorm, *zni = d_scratch + sc.zni;
  u64 *inv_in = d_scratch + sc.inv_in, *inv_out = d_scratch + sc.inv_out, *rf = d_scratch + sc.rf;
  u32* hist = (u32*)(d_scratch + sc.hist);
  if (nrows < N) hipMemsetAsync(d_trace, 0, (size_t)L::W * N * 8, st);
  launch_round_flag_table(rf, st);
  static const bool one_lane_chain = getenv("BN254S_G2_CHAIN_ONE_LANE") != nullptr;  // A/B measurements
  if (one_lane_chain)
    k_dbl_chain_one_lane<CurveG2><<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_x, (int)n, pts, znorm);
  else
    launch_g2_dbl_chain(d_x, (int)n, pts, znorm, st);
  k_sum_scan<CurveG2><<<(unsigned)n, 256, 0, st>>>(d_scalars, d_off, (int)n, pts, znorm, d_err);
  launch_fq_batch_inv(znorm, zni, cnt, st);
  k_g2_row_den<<<(unsigned)((nrows + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zni, inv_in);
  launch_fq_batch_inv(inv_in, inv_out, 3 * nrows, st);
  k_g2_rows<<<(unsigned)((nrows + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zni, inv_out, rf, d_trace, N, d_err);
  if (with_range) launch_range_columns(d_trace, N, L::RC_BEGIN, L::RC_END, L::FREQ, L::RANGE, hist, d_err, st);
  if (d_outputs) k_outputs<CurveG2><<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, pts, zni, d_outputs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

void launch_g2_dbl_chain(const u64* d_x, int n, u64* pts, u64* znorm, hipStream_t st) {
  const size_t v = 4 * (size_t)NPTS * n;
  VecPair px{pts, pts + v}, py{pts + 2 * v, pts + 3 * v}, pz{pts + 4 * v, pts + 5 * v};
  k_g2_dbl_chain_coop<<<(unsigned)((n + 7) / 8), 64, 0, st>>>(d_x, n, px, py, pz, znorm);
}

// ======================================== Fq exp ==============================================================
// table per instance: 0 = one, 1+k = C_k = P_{k-1} * x^(2^k), 257+k = x^(2^k)
__global__ __launch_bounds__(64) void k_fq_chain(const u64* __restrict__ scalars, const u64* __restrict__ xs, int n,
                                                 u64* __restrict__ tab) {
  LATENCY_KERNEL_PRIO();
  int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= n) return;
  size_t cnt = (size_t)NPTS * n;
  u64 s[4];
  for (int i = 0; i < 4; i++) s[i] = scalars[4 * inst + i];
  fq sq = fq_from_canonical(xs + 4 * inst), prod = fq_one();
  st_fq(tab, cnt, inst, prod);
  for (int k = 0; k < 256; k++) {
    fq c = fq_mul(prod, sq);
    st_fq(tab, cnt, (size_t)(1 + k) * n + inst, c);
    st_fq(tab, cnt, (size_t)(257 + k) * n + inst, sq);
    if ((s[k >> 6] >> (k & 63)) & 1) prod = c;
    sq = fq_sqr(sq);
  }
  st_fq(tab, cnt, (size_t)513 * n + inst, sq);
}

__global__ __launch_bounds__(64) void k_fq_rows(const u64* __restrict__ scalars, int n, const u64* __restrict__ tab,
                                                const u64* __restrict__ rf_tbl, u64* __restrict__ trace, size_t N,
                                                int* __restrict__ err) {
  LATENCY_KERNEL_PRIO();
  typedef FQL L;
  size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t nrows = (size_t)n * 512;
  if (r >= nrows) return;
  const RowPos pos = row_pos(r, scalars);
  const int inst = pos.inst, k = pos.k;
  const bool mul_step = pos.adding(), bitk = pos.bitk();
  const size_t cnt = (size_t)NPTS * n;
  fq a, b, c, square, product;
  if (mul_step) {
    a = ld_fq(tab, cnt, (size_t)sum_point(pos.s, k) * n + inst);
    b = ld_fq(tab, cnt, (size_t)(257 + k) * n + inst);
    c = ld_fq(tab, cnt, (size_t)(1 + k) * n + inst);
    square = b;
    product = bitk ? c : a;
  } else {
    a = ld_fq(tab, cnt, (size_t)(257 + k) * n + inst);
    b = a;
    c = ld_fq(tab, cnt, (size_t)(258 + k) * n + inst);
    square = c;
    product = ld_fq(tab, cnt, (size_t)sum_point(pos.s, k + 1) * n + inst);
  }
  auto put = [&](int col, u64 v) { trace[(size_t)col * N + r] = v; };
  int al[16], bl[16], cl[16], t[16];
  fq_to_limbs(a, al);
  fq_to_limbs(b, bl);
  fq_to_limbs(c, cl);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    put(L::A + i, al[i]);
    put(L::B + i, bl[i]);
    put(L::C + i, cl[i]);
  }
  fq_to_limbs(square, t);
#pragma unroll
  for (int i = 0; i < 16; i++) put(L::DOUBLE + i, t[i]);
  fq_to_limbs(product, t);
#pragma unroll
  for (int i = 0; i < 16; i++) put(L::SUM + i, t[i]);
  __shared__ long long mz_buf[31][MZ_LANES];  // the arguments of gen_modulus_zero (trace_common.h)
  long long* const mz_slots = &mz_buf[0][threadIdx.x];
  long long diff[31];
  pol_mul16(al, bl, diff);  // a*b - c  (fields/mul.rs:34-38)
#pragma unroll
  for (int i = 0; i < 16; i++) diff[i] -= (long long)cl[i];
  gen_modulus_zero(diff, mz_slots, trace, N, r, L::AUX, err);
  put_schedule<L>(trace, N, r, pos, rf_tbl);
}

__global__ void k_fq_outputs(const u64* __restrict__ scalars, int n, const u64* __restrict__ tab, u64* __restrict__ out4) {
  LATENCY_KERNEL_PRIO();
  int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= n) return;
  u64 s[4];
  for (int i = 0; i < 4; i++) s[i] = scalars[4 * inst + i];
  const fqw v = fq_to_canonical(ld_fq(tab, (size_t)NPTS * n, (size_t)sum_point(s, 256) * n + inst));
  for (int i = 0; i < 4; i++) out4[4 * inst + i] = v.l[i];
}

// word offsets of the arrays in the scratch buffer: the table of k_fq_chain, then the tail all kinds have
struct FqScratch : ScratchCarve {
  size_t tab, rf, hist;
  explicit FqScratch(size_t n) { tab = take(4 * (size_t)NPTS * n), rf = take(RF_WORDS), hist = take(HIST_WORDS); }
};
size_t fq_trace_scratch_words(size_t n) { return FqScratch(n).words; }

int fq_generate_trace_device(const u64* d_scalars, const u64* d_x, size_t n, u64* d_trace, size_t N, u64* d_scratch,
                             u64* d_outputs, int* d_err, hipStream_t st, bool with_range) {
  const size_t nrows = n * 512;
  const FqScratch sc(n);
  u64 *tab = d_scratch + sc.tab, *rf = d_scratch + sc.rf;
  u32* hist = (u32*)(d_scratch + sc.hist);
  if (nrows < N) hipMemsetAsync(d_trace, 0, (size_t)FQL::W * N * 8, st);
  launch_round_flag_table(rf, st);
  k_fq_chain<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_scalars, d_x, (int)n, tab);
  k_fq_rows<<<(unsigned)((nrows + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, tab, rf, d_trace, N, d_err);
  if (with_range)
    launch_range_columns(d_trace, N, FQL::RC_BEGIN, FQL::RC_END, FQL::FREQ, FQL::RANGE, hist, d_err, st);
  if (d_outputs) k_fq_outputs<<<(unsigned)((n + 63) / 64), 64, 0, st>>>(d_scalars, (int)n, tab, d_outputs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// loads this translation unit's code object (the HIP runtime defers that to the first launch otherwise)
void trace_g2fq_module_warm() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_fq_chain));
}
