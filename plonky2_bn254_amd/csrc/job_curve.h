// What the one-lane-per-job front-ends of curve jobs share (job_outputs.hip, job_check.hip, scalar_mul.hip): the trait that names a curve for
// window_ladder.h, with the load of an affine point from canonical words and its on-curve test, and the predicate on the
// pointers and the count of a batch of jobs.
#pragma once
#include <climits>
#include "g2_endo.h"
#include "window_ladder.h"

namespace {

__device__ __forceinline__ bool jo_on_curve(const fq& x, const fq& y) {  // y^2 == x^3 + 3
  const fq one = fq_one();
  return fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), fq_add(one, fq_dbl(one))));
}
__device__ __forceinline__ bool jo_on_curve(const fq2& x, const fq2& y) { return g2_on_twist(x, y); }
__device__ __forceinline__ void jo_clear_if(fq& a, bool flag) {
  const u32 keep = flag ? 0u : ~0u;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) a.l[j] &= keep;
}
__device__ __forceinline__ void jo_clear_if(fq2& a, bool flag) {
  jo_clear_if(a.c0, flag);
  jo_clear_if(a.c1, flag);
}

// P: the Jacobian point, F: its coordinate field, W_: the window, KIND_: the job kind of bn254s_prove_batch
template <class P, class F, int W_, int KIND_>
struct Curve {
  using E = P;
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
    return jo_on_curve(p.x, p.y);
  }
};
struct G1 : Curve<g1j, fq, 3, 0> {};
struct G2 : Curve<g2j, fq2, 2, 1> {};

// out: the call's first output buffer
inline bool batch_args_ok(int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n, const void* out) {
  return kind >= 0 && kind <= 2 && scalars && x && (kind == 2 || offset) && out && n > 0 &&
         n < (size_t)UINT_MAX;  // the first bad index travels as a 32-bit word
}
constexpr size_t point_words(int kind) { return kind == 0 ? 8 : kind == 1 ? 16 : 4; }

}  // namespace
