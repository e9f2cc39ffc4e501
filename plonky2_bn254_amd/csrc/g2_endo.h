// What the kernels on points of the twist curve E'(Fq2) share (g2_subgroup.hip, g2_cofactor.hip): the endomorphism
// psi = twist^-1 o Frobenius_p o twist, psi(x, y) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2)), and the complete additions
// on Jacobian coordinates.  Device code only.
#pragma once
#include "chain_scan.h"
#include "g2_recover_constants.inc"
#include "g2_subgroup_constants.inc"

namespace {

__device__ __forceinline__ fq g2s_limbs(const u32 (&l)[FQ_NL]) {
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = l[j];
  return r;
}
__device__ __forceinline__ fq2 fq2_conj(const fq2& a) {
  fq2 r;
  r.c0 = a.c0;
  r.c1 = fq_neg(a.c1);
  return r;
}
// psi on Jacobian coordinates: x = X/Z^2 and y = Y/Z^3 are conjugated by conjugating X, Y and Z.  O (Z = 0) stays O.
__device__ __forceinline__ g2j g2_psi(const g2j& p) {
  fq2 gx, gy;
  gx.c0 = g2s_limbs(G2S_PSI_X_C0);
  gx.c1 = g2s_limbs(G2S_PSI_X_C1);
  gy.c0 = g2s_limbs(G2S_PSI_Y_C0);
  gy.c1 = g2s_limbs(G2S_PSI_Y_C1);
  g2j r;
  r.x = fq2_mul(fq2_conj(p.x), gx);
  r.y = fq2_mul(fq2_conj(p.y), gy);
  r.z = fq2_conj(p.z);
  return r;
}
// p + (x2, y2) for an affine, finite second operand (Z2 = 1: 8 products and 3 squarings against the 11 and 5 of g2_add),
// complete: an infinite p gives the affine point, equal points double, opposite points give O.
__device__ __forceinline__ g2j g2_madd(const g2j& p, const fq2& x2, const fq2& y2) {
  g2j r;
  if (pt_inf(p)) {
    r.x = x2;
    r.y = y2;
    r.z = fq2_one();
    return r;
  }
  const fq2 z1z1 = fq2_sqr(p.z);
  const fq2 h = fq2_sub(fq2_mul(x2, z1z1), p.x), rr = fq2_sub(fq2_mul(fq2_mul(y2, p.z), z1z1), p.y);
  if (fq2_is_zero(h)) return fq2_is_zero(rr) ? g2_double(p) : pt_infinity((const g2j*)nullptr);
  const fq2 hh = fq2_sqr(h), hhh = fq2_mul(h, hh), v = fq2_mul(p.x, hh);
  r.x = fq2_sub(fq2_sub(fq2_sqr(rr), hhh), fq2_dbl(v));
  r.y = fq2_sub(fq2_mul(rr, fq2_sub(v, r.x)), fq2_mul(p.y, hhh));
  r.z = fq2_mul(p.z, h);
  return r;
}
// p + q, complete like pt_add_complete (chain_scan.h): either operand may be O, equal points double, opposite points give O.
// It is pt_add_lean (chain_scan.h) on the twist: with pt_add_complete in its place the compiler puts 340 bytes per lane into
// scratch memory, with this form none.
__device__ __forceinline__ g2j g2_add_lean(const g2j& p, const g2j& q) { return pt_add_lean(p, q); }
// t == -(x, y) for a Jacobian t and an affine, finite (x, y), by cross-multiplication: X == x Z^2 and Y == -y Z^3.  O is not
// the negative of a finite point.
__device__ __forceinline__ bool g2_is_neg_of_affine(const g2j& t, const fq2& x, const fq2& y) {
  if (pt_inf(t)) return false;
  const fq2 zz = fq2_sqr(t.z);
  return fq2_eq(t.x, fq2_mul(x, zz)) && fq2_eq(t.y, fq2_neg(fq2_mul(fq2_mul(y, t.z), zz)));
}
// y^2 == x^3 + b' for canonical-range coordinates
__device__ __forceinline__ bool g2_on_twist(const fq2& x, const fq2& y) {
  fq2 b;
  b.c0 = g2s_limbs(G2R_B_C0);
  b.c1 = g2s_limbs(G2R_B_C1);
  return fq2_eq(fq2_sqr(y), fq2_add(fq2_mul(fq2_sqr(x), x), b));
}

}  // namespace
