// The square root in Fq2 = Fq[u]/(u^2 + 1) that the kernels share (root_front.hip, map_to_g2.hip), in two Fq
// exponentiations with the exponent (p+1)/4 of sqrt_ladder.h (p = 3 mod 4); why the formulas hold: the head of root_front.hip.
// One lane per element, blocks of G1R_LANES lanes, `tab` the ladder's table in LDS.  Also the sign of an Fq2 element on
// canonical words (sgn_words), which the kernels that make a root and the one that checks it (root_links.hip) share.
#pragma once
#include "sqrt_ladder.h"
#include "g2_recover_constants.inc"

namespace {

__device__ __forceinline__ fq fq_from_limbs(const u32 (&l)[FQ_NL]) {
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = l[j];
  return r;
}
// c ? a : b limb by limb (a select of whole structs goes through their addresses, and with them through scratch memory)
__device__ __forceinline__ fq fq_select(bool c, const fq& a, const fq& b) {
  const u32 m = 0u - (u32)c;
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = (a.l[j] & m) | (b.l[j] & ~m);
  return r;
}

// src/fields/sgn.rs:20-27 on canonical words: the parity of c0, or of c1 when c0 is zero
__device__ __forceinline__ bool sgn_words(const fqw& c0, const fqw& c1) {
  const bool zero0 = (c0.l[0] | c0.l[1] | c0.l[2] | c0.l[3]) == 0;
  return (c0.l[0] & 1) || (zero0 && (c1.l[0] & 1));
}

// Step 1 is fq_root (sqrt_ladder.h) of the norm nrm of g: alpha = nrm^((p+1)/4), and nrm and with it g is a square iff alpha^2 == nrm.
// Step 2: a root y of g from alpha and square of step 1; bad is raised where a check fails.
// Every lane runs the ladder, so that a wave stays together: where g is no square it works on delta = 1 (t = 1, an inverse of 2)
// and the caller masks its y.
__device__ __forceinline__ fq2 fq2_root_from_alpha(u32 (*tab)[FQ_NL][G1R_LANES], const fq2& g, const fq& alpha, bool square, bool& bad) {
  fq delta = fq_select(fq_is_zero(g.c1), g.c0, fq_mul(fq_add(alpha, g.c0), fq_from_limbs(G2R_HALF)));
  delta = fq_select(square, delta, fq_one());
  const fq t = sqrt_ladder(tab, delta);  // overwrites the lane's own table entries: no barrier
  const fq t2 = fq_sqr(t);
  const bool plus = fq_eq(t2, delta);
  bad |= !plus && !fq_eq(t2, fq_neg(delta));
  const fq o = fq_mul(g.c1, fq_inv(fq_dbl(t)));
  fq2 y;
  y.c0 = fq_select(plus, t, o);
  y.c1 = fq_select(plus, o, t);
  bad |= square && !fq2_eq(fq2_sqr(y), g);
  return y;
}
__device__ __forceinline__ fq2 fq2_root(u32 (*tab)[FQ_NL][G1R_LANES], const fq2& g, const fq& nrm, bool& square, bool& bad) {
  const fq alpha = fq_root(tab, nrm, square, bad);
  return fq2_root_from_alpha(tab, g, alpha, square, bad);
}

}  // namespace
