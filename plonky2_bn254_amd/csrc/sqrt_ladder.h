// a^((p+1)/4) in Fq for the root kernels (root_front.hip, map_to_g1.hip, map_to_g2.hip): p = 3 (mod 4), so the result squares to
// a where a is a square and to -a where it is none.  One lane per element, blocks of G1R_LANES lanes.
#pragma once
#include "fq_dev.h"
#include "g1_recover_constants.inc"

constexpr int G1R_LANES = 64, G1R_ENTRIES = (1 << G1R_WINDOW) - 1;  // g^1 .. g^15 (a zero digit multiplies by nothing)

// g^((p+1)/4) by a fixed-window ladder over the compile-time digits of the exponent: 4 x 62 squarings and one product per non-zero
// digit, against 256 squarings and 109 products of a bit-at-a-time ladder.  The lane's powers g^1 .. g^15 (150 words: too many to
// keep in registers beside a product's working set) live in LDS as tab[entry][limb][lane]: a wave's 64 lanes read 64 consecutive
// words, one per bank, whatever the entry.  A lane only ever reads what it wrote itself: no barrier, also not between two
// ladders that use the same table one after the other.
__device__ __forceinline__ void tab_store(u32 (*tab)[FQ_NL][G1R_LANES], int e, const fq& a) {
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) tab[e][j][threadIdx.x] = a.l[j];
}
__device__ __forceinline__ fq tab_load(const u32 (*tab)[FQ_NL][G1R_LANES], int e) {
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = tab[e][j][threadIdx.x];
  return r;
}
__device__ __forceinline__ fq sqrt_ladder(u32 (*tab)[FQ_NL][G1R_LANES], const fq& g) {
  fq t = g;
#pragma unroll 1
  for (int e = 0; e < G1R_ENTRIES; e++) {
    tab_store(tab, e, t);
    if (e + 1 < G1R_ENTRIES) t = fq_mul(t, g);
  }
  fq c = tab_load(tab, G1R_SQRT_DIGITS[0] - 1);
#pragma unroll 1
  for (int i = 1; i < G1R_NDIGITS; i++) {
#pragma unroll 1
    for (int s = 0; s < G1R_WINDOW; s++) c = fq_sqr(c);
    const int d = G1R_SQRT_DIGITS[i];  // the same in every lane; 32-bit entries, so that it is a scalar load
    if (d) c = fq_mul(c, tab_load(tab, d - 1));
  }
  return c;
}
// c = a^((p+1)/4) and what it squares to.  square: c^2 == a, a is a square and c its root (also for a = 0, like the comparison with
// -a); bad: c^2 is neither a nor -a, the ladder is wrong.
__device__ __forceinline__ fq fq_root(u32 (*tab)[FQ_NL][G1R_LANES], const fq& a, bool& square, bool& bad) {
  const fq c = sqrt_ladder(tab, a);
  const fq c2 = fq_sqr(c);
  square = fq_eq(c2, a);
  bad = !square && !fq_eq(c2, fq_neg(a));  // neither root nor non-residue
  return c;
}
