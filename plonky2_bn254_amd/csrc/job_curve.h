// What the front-ends of curve jobs share (job_outputs.hip, job_check.hip, scalar_mul.hip, msm.hip): the traits G1 / G2 that name a
// curve for window_ladder.h and for the kernels written once for both curves, with the load of an affine point from canonical
// words and its on-curve test; the affine subtraction a - b (k_smul_sub, k_msm_finish); and the predicate on the pointers and the
// count of a batch of jobs.
#pragma once
#include <climits>
#include "g2_endo.h"
#include "window_ladder.h"

namespace {

__device__ __forceinline__ bool on_curve(const fq& x, const fq& y) {  // y^2 == x^3 + 3
  const fq one = fq_one();
  return fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), fq_add(one, fq_dbl(one))));
}
__device__ __forceinline__ bool on_curve(const fq2& x, const fq2& y) { return g2_on_twist(x, y); }
__device__ __forceinline__ void jo_clear_if(fq& a, bool flag) {
  const u32 keep = flag ? 0u : ~0u;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) a.l[j] &= keep;
}
__device__ __forceinline__ void jo_clear_if(fq2& a, bool flag) {
  jo_clear_if(a.c0, flag);
  jo_clear_if(a.c1, flag);
}

// P_: the Jacobian point (E: the same, as an element of window_ladder.h), F_: its coordinate field, W_: the window, KIND_: the job
// kind of bn254s_prove_batch
template <class P_, class F_, int W_, int KIND_>
struct Curve {
  using P = P_;
  using E = P_;
  using F = F_;
  static constexpr bool IS_CURVE = true;
  static constexpr int W = W_, NL = sizeof(P) / sizeof(u32), KIND = KIND_;
  static constexpr int FW = sizeof(F) / sizeof(fq) * 4, PW = 2 * FW;  // words of a coordinate and of an affine point
  static __device__ __forceinline__ E dbl(const E& a) { return pt_double(a); }
  static __device__ __forceinline__ E add(const E& a, const E& b) { return pt_add_lean(a, b); }
  static __device__ __forceinline__ void identity_if(E& q, bool flag) { jo_clear_if(q.z, flag); }
  // PW canonical words below p -> (x, y, 1); false for a point off the curve
  static __device__ __forceinline__ bool load(const u64* w, E& p) {
    fe_from_canonical(w, p.x);
    fe_from_canonical(w + FW, p.y);
    fe_one(p.z);
    return on_curve(p.x, p.y);
  }
};
struct G1 : Curve<g1j, fq, 3, 0> {};
struct G2 : Curve<g2j, fq2, 2, 1> {};

// (x3, y3) = (x1, y1) - (x2, y2) for affine points a, b of one curve in two steps: pt_sub_slope says which case it is and gives the
// slope lambda = num / den of the two that have a difference, pt_sub_point inverts den and finishes.
//   SUB_GENERAL   lambda = (-y2 - y1) / (x2 - x1)
//   SUB_DOUBLED   a == -b, the subtraction doubles a: lambda = 3 x1^2 / 2 y1  (y1 != 0: both group orders are odd)
//   SUB_EQUAL     a == b, the difference is O
//   SUB_SAME_X    x1 == x2 with y1 neither y2 nor -y2, which no two points of a curve are
// The case is known before the inversion, so that a caller leaves for the last two without it: one function that answered after
// the inversion took k_smul_sub<G2> from 175 to 256 registers.
enum { SUB_GENERAL, SUB_DOUBLED, SUB_EQUAL, SUB_SAME_X };
template <class F>
__device__ __forceinline__ void pt_tangent(const F& x1, const F& y1, F& num, F& den) {  // the slope of the doubling
  const F xx = fe_sqr(x1);
  num = fe_add(fe_add(xx, xx), xx);
  den = fe_add(y1, y1);
}
template <class F>
__device__ __forceinline__ int pt_sub_slope(const F& x1, const F& y1, const F& x2, const F& y2, F& num, F& den) {
  num = fe_sub(fe_neg(y2), y1);
  den = fe_sub(x2, x1);
  if (!fe_is_zero(den)) return SUB_GENERAL;
  if (fe_is_zero(fe_sub(y1, y2))) return SUB_EQUAL;
  if (!fe_is_zero(fe_add(y1, y2))) return SUB_SAME_X;
  pt_tangent(x1, y1, num, den);
  return SUB_DOUBLED;
}
template <class F>
__device__ __forceinline__ void pt_sub_point(const F& x1, const F& y1, const F& x2, const F& num, const F& den, F& x3, F& y3) {
  const F lam = fe_mul(num, fe_inv(den));
  x3 = fe_sub(fe_sub(fe_sqr(lam), x1), x2);
  y3 = fe_sub(fe_mul(lam, fe_sub(x1, x3)), y1);
}

// out: the call's first output buffer
inline bool batch_args_ok(int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n, const void* out) {
  return kind >= 0 && kind <= 2 && scalars && x && (kind == 2 || offset) && out && n > 0 &&
         n < (size_t)UINT_MAX;  // the first bad index travels as a 32-bit word
}
constexpr size_t point_words(int kind) { return kind == 0 ? 8 : kind == 1 ? 16 : 4; }
inline const char* curve_name(int kind) { return kind == 0 ? "the curve y^2 = x^3 + 3" : "the twist curve y^2 = x^3 + b'"; }

}  // namespace
