// Debug kernels of bn254s_selftest_fq: the field arithmetic of fq_dev.h and the cooperative pieces of chain_coop.h on raw
// residues (fq_unpack in, fq_pack out), one lane per row and one kernel per group.  The host has checked that every operand is
// below p, so every limb is canonical on entry.  Registers and scratch do not matter here; the point is that these are the very
// inline functions the prover's kernels use, compiled for the same target.
#include "chain_coop.h"
#include "fq_selftest.h"

namespace {

struct RowOut {  // consecutive four-word results of one row
  u64* o;
  __device__ __forceinline__ void put(const fq& v) {
    const fqw w = fq_pack(v);
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = w.l[k];
    o += 4;
  }
  __device__ __forceinline__ void put(const fq2& v) {
    put(v.c0);
    put(v.c1);
  }
};

// group 0: a b c d -> 17 results
__global__ __launch_bounds__(64) void k_fq_selftest_fq(const u64* __restrict__ in, u64* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* r = in + (size_t)FQ_SELFTEST_IN[0] * i;
  const fq a = fq_unpack(r), b = fq_unpack(r + 4), c = fq_unpack(r + 8), d = fq_unpack(r + 12);
  RowOut o{out + (size_t)FQ_SELFTEST_OUT[0] * i};
  o.put(fq_add(a, b));
  o.put(fq_sub(a, b));
  o.put(fq_neg(a));
  o.put(fq_dbl(a));
  o.put(fq_mul(a, b));
  o.put(fq_sqr(a));
  o.put(fq_mul2(a, b, c, d));
  o.put(fq_from_canonical(r));
  {
    const fqw w = fq_to_canonical(a);
#pragma unroll
    for (int k = 0; k < 4; k++) o.o[k] = w.l[k];
    o.o += 4;
  }
  const fq a3 = fq_tpl_lazy(a), b3 = fq_tpl_lazy(b), c3 = fq_tpl_lazy(c), d3 = fq_tpl_lazy(d);
  const fq ab = fq_add_lazy(a, b), cd = fq_add_lazy(c, d);
  o.put(fq_sqr(ab));
  o.put(fq_sqr(a3));
  o.put(fq_mul(a3, b));
  o.put(fq_mul(ab, fq_sub_lazy<2>(c, d)));
  o.put(fq_mul(fq_add_lazy(ab, cd), fq_sub_lazy<4>(ab, cd)));
  o.put(fq_mul(fq_add_lazy(a3, b3), fq_sub_lazy<6>(a3, b3)));
  o.put(fq_mul2(a3, b, c3, fq_sub_lazy<2>(fq_zero(), d)));
  o.put(fq_mul2(a3, b3, c3, fq_sub_lazy<6>(fq_zero(), d3)));
}

// group 1: x = (a, b), y = (c, d), x != 0 -> 15 results
__global__ __launch_bounds__(64) void k_fq_selftest_fq2(const u64* __restrict__ in, u64* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* r = in + (size_t)FQ_SELFTEST_IN[1] * i;
  fq2 x, y, x3, xy;
  x.c0 = fq_unpack(r);
  x.c1 = fq_unpack(r + 4);
  y.c0 = fq_unpack(r + 8);
  y.c1 = fq_unpack(r + 12);
  x3.c0 = fq_tpl_lazy(x.c0);
  x3.c1 = fq_tpl_lazy(x.c1);
  xy.c0 = fq_add_lazy(x.c0, y.c0);
  xy.c1 = fq_add_lazy(x.c1, y.c1);
  RowOut o{out + (size_t)FQ_SELFTEST_OUT[1] * i};
  o.put(fq2_mul(x, y));
  o.put(fq2_mul(x3, y));
  o.put(fq2_sqr<2>(x));
  o.put(fq2_sqr<4>(xy));
  o.put(fq2_sqr<6>(x3));
  o.put(fq2_norm(x));
  o.put(fq2_neg(x));
  o.put(fq2_inv(x));
}

// group 2: e0 .. e7 in a lane's own LDS slots 0 .. 7 (Fq slots e0 .. e3 for g1coop::product and combine; Fq2 slots
// (e0, e1) (e2, e3) (e4, e5) (e6, e7) for g2coop::product) -> 23 results.  The (fa, ga, fb, gb) are the tuples the two doubling
// chains pass (levels 1, 1, 2, 2, 3), the combine coefficients their three sets.
__global__ __launch_bounds__(64) void k_fq_selftest_coop(const u64* __restrict__ in, u64* __restrict__ out, size_t n) {
  using namespace chain_coop;
  __shared__ __attribute__((aligned(16))) u32 lds[64 * 8 * SLOT_W];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;  // (no barrier below: a lane reads only the slots it wrote)
  const u64* r = in + (size_t)FQ_SELFTEST_IN[2] * i;
  u32* g = lds + threadIdx.x * 8 * SLOT_W;
#pragma unroll
  for (int s = 0; s < 8; s++) lds_st(g, s, fq_unpack(r + 4 * s));
  RowOut o{out + (size_t)FQ_SELFTEST_OUT[2] * i};
  constexpr u32 T[5][4] = {{1, 0, 1, 0}, {2, 0, 1, 0}, {1, 1, 1, 1}, {3, 0, 3, 0}, {3, 0, 1, 0}};
#pragma unroll
  for (int t = 0; t < 5; t++) o.put(g1coop::product(g, 0, 1, T[t][0], T[t][1], 2, 3, T[t][2], T[t][3]));
#pragma unroll
  for (int t = 0; t < 5; t++) {
    o.put(g2coop::product(g, 0, false, 0, 1, T[t][0], T[t][1], 2, 3, T[t][2], T[t][3]));
    o.put(g2coop::product(g, 1, false, 0, 1, T[t][0], T[t][1], 2, 3, T[t][2], T[t][3]));
    o.put(g2coop::product(g, 0, true, 0, 1, T[t][0], T[t][1], 2, 3, T[t][2], T[t][3]));
  }
  o.put(combine(g, 0, 1, 1, 4, 2, 4, 3, -4, 4));
  o.put(combine(g, 0, -1, 1, -6, 2, -6, 3, 6, 13));
  o.put(combine(g, 0, 1, 1, -8, 1, 0, 1, 0, 8));
}

// group 3: Jacobian G1 P, Q and G2 P, Q (Z != 0) -> g1_double(P), g1_add(P, Q), g2_double(P), g2_add(P, Q) as raw X Y Z, then
// the two return codes of the additions
__global__ __launch_bounds__(64) void k_fq_selftest_curve(const u64* __restrict__ in, u64* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* r = in + (size_t)FQ_SELFTEST_IN[3] * i;
  RowOut o{out + (size_t)FQ_SELFTEST_OUT[3] * i};
  u64* codes = o.o + 72;
  {
    g1j p, q, s;
    p.x = fq_unpack(r);
    p.y = fq_unpack(r + 4);
    p.z = fq_unpack(r + 8);
    q.x = fq_unpack(r + 12);
    q.y = fq_unpack(r + 16);
    q.z = fq_unpack(r + 20);
    const g1j d = g1_double(p);
    o.put(d.x);
    o.put(d.y);
    o.put(d.z);
    codes[0] = (u64)g1_add(p, q, s);
    o.put(s.x);
    o.put(s.y);
    o.put(s.z);
  }
  {
    const u64* w = r + 24;
    g2j p, q, s;
    p.x.c0 = fq_unpack(w);
    p.x.c1 = fq_unpack(w + 4);
    p.y.c0 = fq_unpack(w + 8);
    p.y.c1 = fq_unpack(w + 12);
    p.z.c0 = fq_unpack(w + 16);
    p.z.c1 = fq_unpack(w + 20);
    q.x.c0 = fq_unpack(w + 24);
    q.x.c1 = fq_unpack(w + 28);
    q.y.c0 = fq_unpack(w + 32);
    q.y.c1 = fq_unpack(w + 36);
    q.z.c0 = fq_unpack(w + 40);
    q.z.c1 = fq_unpack(w + 44);
    const g2j d = g2_double(p);
    o.put(d.x);
    o.put(d.y);
    o.put(d.z);
    codes[1] = (u64)g2_add(p, q, s);
    o.put(s.x);
    o.put(s.y);
    o.put(s.z);
  }
}

}  // namespace

void launch_fq_selftest(int group, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + 63) / 64);
  if (group == 0) k_fq_selftest_fq<<<blocks, 64, 0, st>>>(in, out, n);
  else if (group == 1) k_fq_selftest_fq2<<<blocks, 64, 0, st>>>(in, out, n);
  else if (group == 2) k_fq_selftest_coop<<<blocks, 64, 0, st>>>(in, out, n);
  else k_fq_selftest_curve<<<blocks, 64, 0, st>>>(in, out, n);
}
