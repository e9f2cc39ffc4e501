// Phase A of the scalar-multiplication trace generators as a parallel prefix sum.
//
// generate_one_set (reference src/starks/curves/g1/scalar_mul_stark.rs:92-213, g2 twin) walks 256 double-and-add steps:
// C_k = S_k + D_k, S_{k+1} = bit_k ? C_k : S_k, D_{k+1} = 2 D_k.  Only the doublings are inherently sequential; the running
// sums are S_k = offset + sum_{j<k, bit_j} D_j, an inclusive scan over F_0 = offset, F_{k+1} = bit_k ? D_k : infinity.
// One 256-lane workgroup per instance runs that scan in LDS (8 Hillis-Steele steps with a complete addition law) and then
// adds D_k once more for C_k.  The trace only ever sees canonical affine coordinates, so the result is the same as the
// sequential walk; S_k = -D_k (the case the reference cannot prove, add.rs:49-51) is reported exactly where the
// sequential walk would meet it, in the final S_k + D_k.
#pragma once
#include "fq_dev.h"

__device__ __forceinline__ bool pt_inf(const g1j& p) { return fq_is_zero(p.z); }
__device__ __forceinline__ bool pt_inf(const g2j& p) { return fq2_is_zero(p.z); }
__device__ __forceinline__ g1j pt_infinity(const g1j*) {
  g1j r;
  r.x = fq_one();
  r.y = fq_one();
  r.z = fq_zero();
  return r;
}
__device__ __forceinline__ g2j pt_infinity(const g2j*) {
  g2j r;
  r.x = fq2_one();
  r.y = fq2_one();
  r.z = fq2_zero();
  return r;
}
__device__ __forceinline__ int pt_add(const g1j& a, const g1j& b, g1j& r) { return g1_add(a, b, r); }
__device__ __forceinline__ int pt_add(const g2j& a, const g2j& b, g2j& r) { return g2_add(a, b, r); }

// complete addition: either operand may be the point at infinity, equal points are doubled, opposite points give infinity
template <class P>
__device__ __forceinline__ P pt_add_complete(const P& p, const P& q) {
  if (pt_inf(p)) return q;
  if (pt_inf(q)) return p;
  P r;
  if (pt_add(p, q, r) == 2) r = pt_infinity((const P*)nullptr);
  return r;
}
__device__ __forceinline__ g1j pt_double(const g1j& p) { return g1_double(p); }
__device__ __forceinline__ g2j pt_double(const g2j& p) { return g2_double(p); }
// The same complete law with the formulas of g1_add / g2_add in another order: u2 and s2 are consumed as they are made, so
// fewer field elements are alive at the widest point.  For code that has a table or a second point beside the sum: on the twist
// pt_add_complete puts 340 bytes per lane into scratch memory there (g2_cofactor.hip), this form none.
template <class P>
__device__ __forceinline__ P pt_add_lean(const P& p, const P& q) {
  if (pt_inf(q)) return p;
  if (pt_inf(p)) return q;
  const auto z1z1 = fe_sqr(p.z), z2z2 = fe_sqr(q.z);
  const auto u1 = fe_mul(p.x, z2z2), s1 = fe_mul(fe_mul(p.y, q.z), z2z2);
  const auto h = fe_sub(fe_mul(q.x, z1z1), u1), rr = fe_sub(fe_mul(fe_mul(q.y, p.z), z1z1), s1);
  if (fe_is_zero(h)) return fe_is_zero(rr) ? pt_double(p) : pt_infinity((const P*)nullptr);
  const auto hh = fe_sqr(h), hhh = fe_mul(h, hh), v = fe_mul(u1, hh);
  P r;
  r.x = fe_sub(fe_sub(fe_sqr(rr), hhh), fe_add(v, v));
  r.y = fe_sub(fe_mul(rr, fe_sub(v, r.x)), fe_mul(s1, hhh));
  r.z = fe_mul(fe_mul(p.z, q.z), h);
  return r;
}

// LDS image of a point: word w of lane k at sh[w * 256 + k] (conflict-free for consecutive lanes)
__device__ __forceinline__ void lds_put_fq(u64* sh, int w0, int k, const fq& v) {
  const fqw w = fq_pack(v);
#pragma unroll
  for (int l = 0; l < 4; l++) sh[(w0 + l) * 256 + k] = w.l[l];
}
__device__ __forceinline__ fq lds_get_fq(const u64* sh, int w0, int k) {
  u64 w[4];
#pragma unroll
  for (int l = 0; l < 4; l++) w[l] = sh[(w0 + l) * 256 + k];
  return fq_unpack(w);
}
__device__ __forceinline__ void lds_put(u64* sh, int k, const g1j& p) {
  lds_put_fq(sh, 0, k, p.x);
  lds_put_fq(sh, 4, k, p.y);
  lds_put_fq(sh, 8, k, p.z);
}
__device__ __forceinline__ void lds_get(const u64* sh, int k, g1j& p) {
  p.x = lds_get_fq(sh, 0, k);
  p.y = lds_get_fq(sh, 4, k);
  p.z = lds_get_fq(sh, 8, k);
}
__device__ __forceinline__ void lds_put(u64* sh, int k, const g2j& p) {
  lds_put_fq(sh, 0, k, p.x.c0);
  lds_put_fq(sh, 4, k, p.x.c1);
  lds_put_fq(sh, 8, k, p.y.c0);
  lds_put_fq(sh, 12, k, p.y.c1);
  lds_put_fq(sh, 16, k, p.z.c0);
  lds_put_fq(sh, 20, k, p.z.c1);
}
__device__ __forceinline__ void lds_get(const u64* sh, int k, g2j& p) {
  p.x.c0 = lds_get_fq(sh, 0, k);
  p.x.c1 = lds_get_fq(sh, 4, k);
  p.y.c0 = lds_get_fq(sh, 8, k);
  p.y.c1 = lds_get_fq(sh, 12, k);
  p.z.c0 = lds_get_fq(sh, 16, k);
  p.z.c1 = lds_get_fq(sh, 20, k);
}

// Inclusive scan of the 256 points held one per lane (lane k ends with F_0 + ... + F_k).  sh: sizeof(P)/8 * 256 words.
template <class P>
__device__ __forceinline__ void pt_scan256(P& f, u64* sh, int k) {
#pragma unroll 1
  for (int d = 1; d < 256; d <<= 1) {
    lds_put(sh, k, f);
    __syncthreads();
    if (k >= d) {
      P q;
      lds_get(sh, k - d, q);
      f = pt_add_complete(q, f);
    }
    __syncthreads();
  }
}

// The segmented twin: lane k also holds a head flag, and a head cuts the sum, (f1, p1) + (f2, p2) = (f1 | f2, f2 ? p2 : p1 + p2).
// Lane k ends with the sum from the last head at or before it (from lane 0 if there is none) up to itself, and with flag = "a head
// lies in lanes 0 .. k".  sh as above; shf: 256 flag words.
template <class P>
__device__ __forceinline__ void pt_seg_scan256(P& f, unsigned& flag, u64* sh, unsigned* shf, int k) {
#pragma unroll 1
  for (int d = 1; d < 256; d <<= 1) {
    lds_put(sh, k, f);
    shf[k] = flag;
    __syncthreads();
    if (k >= d) {
      if (!flag) {
        P q;
        lds_get(sh, k - d, q);
        f = pt_add_complete(q, f);
      }
      flag |= shf[k - d];
    }
    __syncthreads();
  }
}
