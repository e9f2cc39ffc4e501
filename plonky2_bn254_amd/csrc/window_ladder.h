// A fixed-window, left-to-right ladder over a 256-bit multiplier that differs from lane to lane (job_outputs.hip): one lane per
// job, blocks of WL_LANES lanes.  Written once over a trait C that names the group:
//   C::E                 an element (g1j, g2j: a Jacobian point; fq: a field element, the group written multiplicatively)
//   C::W, C::NL          the window in bits and the 32-bit limbs of an element (30, 60, 10)
//   C::dbl(a), C::add(a, b), C::identity_if(a, flag)
// The lane's table [1]x .. [2^W - 1]x lives in LDS as tab[entry][limb][lane], like the table of sqrt_ladder.h: whatever entry a
// lane asks for, the 64 lanes of a wave touch 64 consecutive words, one per bank.  A lane only ever reads what it wrote itself,
// so there is no barrier anywhere.  The digit selects data, never a branch: a zero digit loads entry 1 and turns it into the
// identity (Z = 0 for a point, 1 for a field element), and C::add has to cope with that operand.
#pragma once
#include "chain_scan.h"

constexpr int WL_LANES = 64;

template <int NL>
__device__ __forceinline__ void wl_put_fq(u32 (*tab)[NL][WL_LANES], int e, int j0, const fq& a) {
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) tab[e][j0 + j][threadIdx.x] = a.l[j];
}
template <int NL>
__device__ __forceinline__ fq wl_get_fq(u32 (*tab)[NL][WL_LANES], int e, int j0) {
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = tab[e][j0 + j][threadIdx.x];
  return r;
}
template <int NL>
__device__ __forceinline__ void wl_put(u32 (*tab)[NL][WL_LANES], int e, const fq& a) {
  wl_put_fq(tab, e, 0, a);
}
template <int NL>
__device__ __forceinline__ void wl_get(u32 (*tab)[NL][WL_LANES], int e, fq& a) {
  a = wl_get_fq(tab, e, 0);
}
template <int NL>
__device__ __forceinline__ void wl_put(u32 (*tab)[NL][WL_LANES], int e, const g1j& p) {
  wl_put_fq(tab, e, 0, p.x);
  wl_put_fq(tab, e, FQ_NL, p.y);
  wl_put_fq(tab, e, 2 * FQ_NL, p.z);
}
template <int NL>
__device__ __forceinline__ void wl_get(u32 (*tab)[NL][WL_LANES], int e, g1j& p) {
  p.x = wl_get_fq(tab, e, 0);
  p.y = wl_get_fq(tab, e, FQ_NL);
  p.z = wl_get_fq(tab, e, 2 * FQ_NL);
}
template <int NL>
__device__ __forceinline__ void wl_put(u32 (*tab)[NL][WL_LANES], int e, const g2j& p) {
  wl_put_fq(tab, e, 0, p.x.c0);
  wl_put_fq(tab, e, FQ_NL, p.x.c1);
  wl_put_fq(tab, e, 2 * FQ_NL, p.y.c0);
  wl_put_fq(tab, e, 3 * FQ_NL, p.y.c1);
  wl_put_fq(tab, e, 4 * FQ_NL, p.z.c0);
  wl_put_fq(tab, e, 5 * FQ_NL, p.z.c1);
}
template <int NL>
__device__ __forceinline__ void wl_get(u32 (*tab)[NL][WL_LANES], int e, g2j& p) {
  p.x.c0 = wl_get_fq(tab, e, 0);
  p.x.c1 = wl_get_fq(tab, e, FQ_NL);
  p.y.c0 = wl_get_fq(tab, e, 2 * FQ_NL);
  p.y.c1 = wl_get_fq(tab, e, 3 * FQ_NL);
  p.z.c0 = wl_get_fq(tab, e, 4 * FQ_NL);
  p.z.c1 = wl_get_fq(tab, e, 5 * FQ_NL);
}

// The top `bits` bits of the 256-bit value s (s[3] the highest word), which is shifted left by as many: 0 < bits < 64.
__device__ __forceinline__ int wl_take(u64 (&s)[4], int bits) {
  const int d = (int)(s[3] >> (64 - bits));
  s[3] = (s[3] << bits) | (s[2] >> (64 - bits));
  s[2] = (s[2] << bits) | (s[1] >> (64 - bits));
  s[1] = (s[1] << bits) | (s[0] >> (64 - bits));
  s[0] <<= bits;
  return d;
}

// Entry d of the lane's table, the identity for d = 0.
template <class C>
__device__ __forceinline__ typename C::E wl_pick(u32 (*tab)[C::NL][WL_LANES], int d) {
  typename C::E q;
  wl_get(tab, d ? d - 1 : 0, q);
  C::identity_if(q, d == 0);
  return q;
}

// [s]x (x^s for a field element): the table, then the windows from the top.  The first window holds the 256 mod W bits that the
// others leave over (W of them where W divides 256) and starts the accumulator; every later window is W doublings and one
// addition of a table entry.
template <class C>
__device__ __forceinline__ typename C::E wl_ladder(u32 (*tab)[C::NL][WL_LANES], const typename C::E& x, u64 (&s)[4]) {
  using E = typename C::E;
  constexpr int ENTRIES = (1 << C::W) - 1, NWIN = (256 + C::W - 1) / C::W, W0 = 256 - C::W * (NWIN - 1);
  wl_put(tab, 0, x);
  E t = C::dbl(x);
#pragma unroll 1
  for (int e = 1; e < ENTRIES; e++) {
    wl_put(tab, e, t);
    if (e + 1 < ENTRIES) {
      E b;
      wl_get(tab, 0, b);
      t = C::add(t, b);
    }
  }
  E acc = wl_pick<C>(tab, wl_take(s, W0));
#pragma unroll 1
  for (int i = 1; i < NWIN; i++) {
#pragma unroll 1
    for (int j = 0; j < C::W; j++) acc = C::dbl(acc);
    acc = C::add(acc, wl_pick<C>(tab, wl_take(s, C::W)));
  }
  return acc;
}
