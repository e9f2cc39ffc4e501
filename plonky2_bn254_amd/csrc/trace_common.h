// Shared device helpers of the three trace generators (G1 / G2 / Fq exp) and of msm.hip: SoA vectors of field elements and
// points, the curve-generic kernels of phase A (doubling chain on one lane, running sums, outputs), limb conversion,
// generate_modulus_zero (reference src/starks/modular/modulus_zero.rs:77-123) and the frame of a row kernel (position of a
// row in the double-and-add schedule, packed limbs, the schedule columns).  The kernels all three share are in
// trace_shared.hip (trace.h).
#pragma once
#include "fq_dev.h"
#include "chain_scan.h"
#include "../../include/bn254_stark.h"

static constexpr int NPTS = 514;  // per instance: 0 = offset | one, 1+k = C_k (k<256), 257+k = D_k (k<=256)

// ---- SoA vectors of Fq elements: element e, limb l at base[l*count + e] ---------------------------------
// (the element is stored as the four 64-bit words of its Montgomery residue; registers hold ten 26-bit limbs, fq_dev.h)
__device__ __forceinline__ fq ld_fq(const u64* base, size_t count, size_t e) {
  u64 w[4];
#pragma unroll
  for (int l = 0; l < 4; l++) w[l] = base[l * count + e];
  return fq_unpack(w);
}
__device__ __forceinline__ void st_fq(u64* base, size_t count, size_t e, const fq& v) {
  const fqw w = fq_pack(v);
#pragma unroll
  for (int l = 0; l < 4; l++) base[l * count + e] = w.l[l];
}
// the same for a coordinate of either curve (fe_*, fq_dev.h): an Fq2 element is two Fq vectors in a row, c1 at base + 4 count
__device__ __forceinline__ void fe_ld(const u64* base, size_t count, size_t e, fq& r) { r = ld_fq(base, count, e); }
__device__ __forceinline__ void fe_ld(const u64* base, size_t count, size_t e, fq2& r) {
  r.c0 = ld_fq(base, count, e);
  r.c1 = ld_fq(base + 4 * count, count, e);
}
__device__ __forceinline__ void fe_st(u64* base, size_t count, size_t e, const fq& v) { st_fq(base, count, e, v); }
__device__ __forceinline__ void fe_st(u64* base, size_t count, size_t e, const fq2& v) {
  st_fq(base, count, e, v.c0);
  st_fq(base + 4 * count, count, e, v.c1);
}

// What differs between the curves: point, coordinate field, 64-bit words of a coordinate.
struct CurveG1 {
  using P = g1j;
  using F = fq;
  static constexpr int FW = 4;
};
struct CurveG2 {
  using P = g2j;
  using F = fq2;
  static constexpr int FW = 8;
};
// cnt points in SoA form, coordinate c (0 = X, 1 = Y, 2 = Z) at b + FW c cnt; inside it, word l of Fq component j (G2: c0, c1)
// of element e at [(4 j + l) cnt + e] (fe_ld / fe_st).  The trace scratch and the levels of the msm scan have this layout.
template <class P>
__device__ __forceinline__ P pa_load(const u64* b, size_t cnt, size_t e) {
  constexpr size_t FW = sizeof(P) / sizeof(fq) / 3 * 4;
  P p;
  fe_ld(b, cnt, e, p.x);
  fe_ld(b + FW * cnt, cnt, e, p.y);
  fe_ld(b + 2 * FW * cnt, cnt, e, p.z);
  return p;
}
template <class P>
__device__ __forceinline__ void pa_store(u64* b, size_t cnt, size_t e, const P& p) {
  constexpr size_t FW = sizeof(P) / sizeof(fq) / 3 * 4;
  fe_st(b, cnt, e, p.x);
  fe_st(b + FW * cnt, cnt, e, p.y);
  fe_st(b + 2 * FW * cnt, cnt, e, p.z);
}
// a^-1 from the batched inverse of norm(a); the norm of an Fq element is the element itself
__device__ __forceinline__ fq fe_inv_from_norm_inv(const fq&, const fq& ninv) { return ninv; }
__device__ __forceinline__ fq2 fe_inv_from_norm_inv(const fq2& a, const fq& ninv) { return fq2_inv_from_norm_inv(a, ninv); }
// G2 keeps norm(Z) of every point beside it, the input of the batched inversion; G1 inverts Z itself
__device__ __forceinline__ void st_znorm(u64*, size_t, size_t, const fq&) {}
__device__ __forceinline__ void st_znorm(u64* znorm, size_t cnt, size_t e, const fq2& z) { st_fq(znorm, cnt, e, fq2_norm(z)); }

// Affine coordinates (Montgomery) of point e of pts; zinv = the batched inverses of Z (G1) or of norm(Z) (G2).  (On G1 the
// inverse is zinv itself and Z is not loaded.)
template <class P>
struct AffPt {
  decltype(P::x) x, y;
};
template <class P>
__device__ __forceinline__ AffPt<P> affine_pt(const u64* pts, const u64* zinv, size_t cnt, size_t e) {
  using F = decltype(P::x);
  constexpr size_t FW = sizeof(F) / sizeof(fq) * 4;
  F x, y, z;
  fe_ld(pts + 2 * FW * cnt, cnt, e, z);
  const F zi = fe_inv_from_norm_inv(z, ld_fq(zinv, cnt, e)), z2 = fe_sqr(zi);
  fe_ld(pts, cnt, e, x);
  fe_ld(pts + FW * cnt, cnt, e, y);
  AffPt<P> r;
  r.x = fe_mul(x, z2);
  r.y = fe_mul(fe_mul(y, z2), zi);
  return r;
}

// index of the highest set bit of s below position k, or -1
__device__ __forceinline__ int last_set_below(const u64 s[4], int k) {
  for (int w = 3; w >= 0; w--) {
    int lo = w * 64;
    if (k <= lo) continue;
    u64 m = s[w];
    if (k < lo + 64) m &= (1ULL << (k - lo)) - 1;
    if (m) return lo + 63 - __clzll((long long)m);
  }
  return -1;
}
// point index of the running sum after step k-1 (S_{k-1}); k = 0 -> offset
__device__ __forceinline__ int sum_point(const u64 s[4], int k) {
  int j = last_set_below(s, k);
  return j < 0 ? 0 : 1 + j;
}

// ---- phase A and the outputs, for either curve (C = CurveG1 / CurveG2; znorm is used on G2 only) -------------------------------
// The doubling chain on one lane per instance: D_k = 2^k x at point 257 + k.  The drivers use the cooperative chains
// (chain_coop.h), which store the same values bit for bit; this one is kept for A/B measurements.
template <class C>
__global__ __launch_bounds__(64) void k_dbl_chain_one_lane(const u64* __restrict__ xs, int n, u64* __restrict__ pts,
                                                           u64* __restrict__ znorm) {
  LATENCY_KERNEL_PRIO();
  int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= n) return;
  size_t cnt = (size_t)NPTS * n;
  typename C::P D;
  fe_from_canonical(xs + 2 * C::FW * inst, D.x);
  fe_from_canonical(xs + 2 * C::FW * inst + C::FW, D.y);
  fe_one(D.z);
#pragma unroll 1
  for (int k = 0; k <= 256; k++) {
    size_t e = (size_t)(257 + k) * n + inst;
    pa_store(pts, cnt, e, D);
    st_znorm(znorm, cnt, e, D.z);
    if (k < 256) D = pt_double(D);
  }
}

// one workgroup per instance, lane k: S_k = offset + sum_{j<k, bit_j} D_j, then C_k = S_k + D_k
template <class C>
__global__ __launch_bounds__(256) void k_sum_scan(const u64* __restrict__ scalars, const u64* __restrict__ offs, int n,
                                                  u64* __restrict__ pts, u64* __restrict__ znorm, int* __restrict__ err) {
  using P = typename C::P;
  LATENCY_KERNEL_PRIO();
  __shared__ u64 sh[3 * C::FW * 256];
  const int inst = blockIdx.x, k = threadIdx.x;
  const size_t cnt = (size_t)NPTS * n;
  auto load = [&](int pt) { return pa_load<P>(pts, cnt, (size_t)pt * n + inst); };
  auto store = [&](int pt, const P& p) {
    size_t e = (size_t)pt * n + inst;
    pa_store(pts, cnt, e, p);
    st_znorm(znorm, cnt, e, p.z);
  };
  P f;
  if (k == 0) {
    fe_from_canonical(offs + 2 * C::FW * inst, f.x);
    fe_from_canonical(offs + 2 * C::FW * inst + C::FW, f.y);
    fe_one(f.z);
    store(0, f);
  } else {
    const int j = k - 1;
    const bool bit = (scalars[4 * inst + (j >> 6)] >> (j & 63)) & 1;
    f = bit ? load(257 + j) : pt_infinity((const P*)nullptr);
  }
  pt_scan256(f, sh, k);
  P d = load(257 + k), c;
  if (pt_inf(f)) {
    c = d;  // only after an S_j = -D_j further down, which is reported there
  } else if (pt_add(f, d, c) == 2) {
    atomicCAS(err, 0, BN254S_E_INVALID_POINT);
  }
  store(1 + k, c);
}

// final outputs: s*x + offset = S_255 in canonical affine form, 2 FW words per instance
template <class C>
__global__ void k_outputs(const u64* __restrict__ scalars, int n, const u64* __restrict__ pts, const u64* __restrict__ zinv,
                          u64* __restrict__ out) {
  LATENCY_KERNEL_PRIO();
  int inst = blockIdx.x * blockDim.x + threadIdx.x;
  if (inst >= n) return;
  u64 s[4];
  for (int i = 0; i < 4; i++) s[i] = scalars[4 * inst + i];
  const auto p = affine_pt<typename C::P>(pts, zinv, (size_t)NPTS * n, (size_t)sum_point(s, 256) * n + inst);
  fe_store_canonical(out + 2 * C::FW * inst, p.x);
  fe_store_canonical(out + 2 * C::FW * inst + C::FW, p.y);
}

__device__ __forceinline__ void fq_to_limbs(const fq& mont, int limbs[16]) {
  const fqw c = fq_to_canonical(mont);
#pragma unroll
  for (int i = 0; i < 16; i++) limbs[i] = (int)((c.l[i >> 2] >> (16 * (i & 3))) & 0xFFFF);
}

__device__ static constexpr int MOD_LIMBS[16] = {64839, 55420, 35862, 15392, 51853, 26737, 27281, 38785,
                                                  22621, 33153, 17846, 47184, 41001, 57649, 20082, 12388};
// p^-1 mod 2^288, 32-bit words
__device__ static constexpr u32 PINV288[9] = {0x1b799c77u, 0x782df87du, 0xe1359536u, 0x6121829au, 0xe7cc257fu,
                                               0x2750342fu, 0x6e777394u, 0x0a85dd48u, 0x5b52d390u};

// generate_modulus_zero (modulus_zero.rs:77-123): in = 31 signed limb coefficients of a multiple of p.
// Writes the 80 witness values to columns col0.. of `row` (trace column-major, N rows).
// The function is called four to ten times per row and is not inlined; its 31 inputs travel through LDS (coefficient i of the
// calling lane at in[i * MZ_LANES]: one wave per workgroup, a lane reads only what it wrote) - as a by-pointer argument they
// sat in scratch memory (256 B per lane in round 2).
static constexpr int MZ_LANES = 64;
typedef __attribute__((address_space(3))) long long mz_lds_t;
static __device__ __noinline__ void gen_modulus_zero_lds(const mz_lds_t* in_lds, u64* __restrict__ trace, size_t N, size_t row, int col0,
                                                         int* err) {
  // Everything is streamed from the LDS slots (in(i)) instead of being held in arrays: the function is called from kernels that keep
  // a dozen coordinates alive across the call, and its own registers add to theirs.
  auto in = [&](int i) -> long long { return in_lds[i * MZ_LANES]; };
  // low 288 bits of V = sum in[i] 2^(16 i), two's complement
  u32 v[9];
  long long carry = 0;
#pragma unroll
  for (int w = 0; w < 9; w++) {
    long long t = carry + in(2 * w) + (in(2 * w + 1) << 16);
    v[w] = (u32)t;
    carry = t >> 32;
  }
  // q = V * p^-1 mod 2^288 (exact quotient, two's complement)
  u32 q[9];
  u128 acc = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) {
#pragma unroll
    for (int i = 0; i <= k; i++) acc += (u64)v[i] * PINV288[k - i];
    q[k] = (u32)acc;
    acc >>= 32;
  }
  bool neg = (q[8] >> 31) != 0;
  bool nonzero = false;
  if (neg) {  // |q| = -q
    u64 c = 1;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      c += (u64)(~q[k]);
      q[k] = (u32)c;
      c >>= 32;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; k++) nonzero |= q[k] != 0;
  if ((q[8] >> 16) != 0) atomicCAS(err, 0, BN254S_E_INTERNAL);  // quotient wider than 17 limbs
  u64* out = trace + (size_t)col0 * N + row;
  out[0] = (!neg && nonzero) ? 1 : 0;
  int qs[17];  // signed limbs of the quotient
  const int sgn = neg ? -1 : 1;
#pragma unroll
  for (int i = 0; i < 17; i++) {
    const int qa = (int)((q[i >> 1] >> (16 * (i & 1))) & 0xFFFF);
    out[(size_t)(1 + i) * N] = (u64)qa;
    qs[i] = sgn * qa;
  }
  // constr = in - quot(x) * m(x), coefficient d formed when the division below needs it;
  // aux = constr / (x - 2^16) (pol_remove_root_2exp), shifted by 2^29, split in 16-bit halves
  long long a = 0;
  bool bad = false;
#pragma unroll
  for (int d = 0; d < 32; d++) {  // (unrolled: rolled it is 5 % slower for the row kernels and frees no registers they need)
    long long cd = d < 31 ? in(d) : 0;
#pragma unroll
    for (int i = 0; i < 17; i++) {
      const int jdx = d - i;
      if (jdx >= 0 && jdx < 16) cd -= (long long)qs[i] * MOD_LIMBS[jdx];
    }
    if (d == 31) {  // exactness: the last carry must vanish, otherwise `in` was not a multiple of p
      bad |= a != cd;
      break;
    }
    a = d == 0 ? -(cd >> 16) : (a - cd) >> 16;
    const long long sh = a + (1LL << 29);
    bad |= (sh < 0) | (sh > (1LL << 30));
    out[(size_t)(18 + d) * N] = (u64)(sh & 0xFFFF);
    out[(size_t)(49 + d) * N] = (u64)((sh >> 16) & 0xFFFF);
  }
  if (bad) atomicCAS(err, 0, BN254S_E_INTERNAL);
}

// stores the coefficients to the calling lane's LDS slots and calls the function above; `slots` = &buffer[0][lane] of a
// __shared__ long long buffer[31][MZ_LANES]
__device__ __forceinline__ void gen_modulus_zero(const long long* in, long long* slots, u64* __restrict__ trace, size_t N, size_t row,
                                                 int col0, int* err) {
  mz_lds_t* l = (mz_lds_t*)slots;
#pragma unroll
  for (int i = 0; i < 31; i++) l[i * MZ_LANES] = in[i];
  gen_modulus_zero_lds(l, trace, N, row, col0, err);
}

// ---- row-kernel helpers: packed limbs, limb products accumulated in LDS -------------------------------------------------------
// The sixteen 16-bit limbs of a coordinate are kept two to a register (P16).  The 31-coefficient polynomial of a witness block lives
// in the lane's LDS slots (the argument buffer of gen_modulus_zero_lds, trace_common.h); a limb product is a called function that
// unpacks its operands, forms the 31 coefficients in its own registers and adds them to the slots.  The row kernel itself then
// holds little more than its packed coordinates.  (Round 2, k_g2_rows: fourteen unpacked arrays and two or three polynomials:
// 256 + 256 registers and 784 B of scratch per lane.)
struct P16 {
  u32 w[8];
};
__device__ __forceinline__ P16 p16_pack(const fq& m) {
  const fqw cw = fq_to_canonical(m);
  P16 p;
#pragma unroll
  for (int i = 0; i < 8; i++) p.w[i] = (u32)(cw.l[i >> 1] >> (32 * (i & 1)));
  return p;
}
__device__ __forceinline__ void p16_unpack(const P16& p, int* l) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    l[2 * i] = (int)(p.w[i] & 0xFFFF);
    l[2 * i + 1] = (int)(p.w[i] >> 16);
  }
}
// slots += coef * (x - [mode 1] sub) * (y - [mode 2] sub) as limb polynomials; cm = coef * 4 + mode.  The packed operands travel as
// vector-typed arguments (registers; a struct argument of this size goes through the stack, i.e. scratch memory).
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
static __device__ __noinline__ void mac_lds_v(mz_lds_t* slots, int cm, u32x4 xa, u32x4 xb, u32x4 ya, u32x4 yb, u32x4 sa, u32x4 sb) {
  const int mode = cm & 3, coef = cm >> 2;
  int a[16], b[16], t[16];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    a[2 * i] = (int)(xa[i] & 0xFFFF);
    a[2 * i + 1] = (int)(xa[i] >> 16);
    a[8 + 2 * i] = (int)(xb[i] & 0xFFFF);
    a[8 + 2 * i + 1] = (int)(xb[i] >> 16);
    b[2 * i] = (int)(ya[i] & 0xFFFF);
    b[2 * i + 1] = (int)(ya[i] >> 16);
    b[8 + 2 * i] = (int)(yb[i] & 0xFFFF);
    b[8 + 2 * i + 1] = (int)(yb[i] >> 16);
    t[2 * i] = (int)(sa[i] & 0xFFFF);
    t[2 * i + 1] = (int)(sa[i] >> 16);
    t[8 + 2 * i] = (int)(sb[i] & 0xFFFF);
    t[8 + 2 * i + 1] = (int)(sb[i] >> 16);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    a[i] -= mode == 1 ? t[i] : 0;
    b[i] -= mode == 2 ? t[i] : 0;
    a[i] *= coef;
  }
  long long out[31];
#pragma unroll
  for (int i = 0; i < 31; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < 16; i++)
#pragma unroll
    for (int j = 0; j < 16; j++) out[i + j] += (long long)a[i] * b[j];
#pragma unroll
  for (int i = 0; i < 31; i++) slots[i * MZ_LANES] += out[i];
}
__device__ __forceinline__ void mac_lds(mz_lds_t* slots, int cm, const P16& x, const P16& y, const P16& sub) {
  mac_lds_v(slots, cm, u32x4{x.w[0], x.w[1], x.w[2], x.w[3]}, u32x4{x.w[4], x.w[5], x.w[6], x.w[7]}, u32x4{y.w[0], y.w[1], y.w[2], y.w[3]},
            u32x4{y.w[4], y.w[5], y.w[6], y.w[7]}, u32x4{sub.w[0], sub.w[1], sub.w[2], sub.w[3]},
            u32x4{sub.w[4], sub.w[5], sub.w[6], sub.w[7]});
}
__device__ __forceinline__ void lin_lds(mz_lds_t* slots, int coef, const P16& x) {
  int a[16];
  p16_unpack(x, a);
#pragma unroll
  for (int i = 0; i < 16; i++) slots[i * MZ_LANES] += (long long)(coef * a[i]);
}
__device__ __forceinline__ void zero_lds(mz_lds_t* slots) {
#pragma unroll
  for (int i = 0; i < 31; i++) slots[i * MZ_LANES] = 0;
}

__device__ __forceinline__ void pol_mul16(const int* a, const int* b, long long* out /*31*/) {
#pragma unroll
  for (int i = 0; i < 31; i++) out[i] = 0;
#pragma unroll
  for (int i = 0; i < 16; i++)
#pragma unroll
    for (int j = 0; j < 16; j++) out[i + j] += (long long)a[i] * b[j];
}

// ---- the frame of a row kernel ---------------------------------------------------------------------------------------------------
// Trace row r is row `row` of instance `inst`: step k of the double-and-add walk, an adding (Fq exp: multiplying) row when even,
// a doubling (squaring) row when odd.  s = the scalar.
// The row kernels sit at the register ceiling, and two things here decide whether they stay there.  The flags are functions,
// not members: a bool that goes through a member reaches the kernel as 8-bit arithmetic, which changes the allocation of
// k_g1_rows.  And s is indexed by constants only: one variable index into a member keeps the whole struct in scratch memory,
// so code that needs one indexes a local copy of the array.
struct RowPos {
  int inst, row, k;
  u64 s[4];
  __device__ __forceinline__ bool adding() const { return (row & 1) == 0; }
  __device__ __forceinline__ bool bitk() const {  // bit k of the scalar
    const u64 w[4] = {s[0], s[1], s[2], s[3]};
    return (w[k >> 6] >> (k & 63)) & 1;
  }
};
__device__ __forceinline__ RowPos row_pos(size_t r, const u64* scalars) {
  RowPos p;
  p.inst = (int)(r >> 9);
  p.row = (int)(r & 511);
  p.k = p.row >> 1;
  for (int i = 0; i < 4; i++) p.s[i] = scalars[4 * p.inst + i];
  return p;
}
// the sixteen limbs of a packed coordinate to columns col .. col + 15 of row r
__device__ __forceinline__ void p16_put(u64* trace, size_t N, size_t r, int col, const P16& p) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    trace[(size_t)(col + 2 * i) * N + r] = (u64)(p.w[i] & 0xFFFF);
    trace[(size_t)(col + 2 * i + 1) * N + r] = (u64)(p.w[i] >> 16);
  }
}
__device__ __forceinline__ P16 p16_sel(bool first, const P16& x, const P16& y) {
  P16 o;
#pragma unroll
  for (int i = 0; i < 8; i++) o.w[i] = first ? x.w[i] : y.w[i];
  return o;
}
// the schedule columns of layout L: bits rotated left by k (scalar_mul_stark.rs:163-167), round flags, bookkeeping
template <class L>
__device__ __forceinline__ void put_schedule(u64* trace, size_t N, size_t r, const RowPos& pos, const u64* rf_tbl) {
  auto put = [&](int col, u64 v) { trace[(size_t)col * N + r] = v; };
  const int row = pos.row;
  const u64 s[4] = {pos.s[0], pos.s[1], pos.s[2], pos.s[3]};
  for (int i = 0; i < 256; i++) {
    int src = (i + pos.k) & 255;
    put(L::BITS + i, (s[src >> 6] >> (src & 63)) & 1);
  }
  put(L::FLAGS + 0, row == 0);
  put(L::FLAGS + 1, row == 511);
  put(L::FLAGS + 2, (u64)row);
  put(L::FLAGS + 3, rf_tbl[row]);
  put(L::FLAGS + 4, rf_tbl[512 + row]);
  put(L::TIMESTAMP, (u64)pos.inst);
  put(L::IS_ADDING, pos.adding() ? 1 : 0);
  put(L::IDNL, pos.adding() ? 0 : (row == 511 ? 0 : 1));
  put(L::FILTER, 1);
}

// ---- scratch of a driver: word offsets taken one after the other; `words` is the size the driver asks its caller for ----------------
struct ScratchCarve {
  static constexpr size_t RF_WORDS = 1024 /* round-flag table */, HIST_WORDS = 65536 / 2 /* histogram, 65536 u32 */;
  size_t words = 0;
  size_t take(size_t w) {
    const size_t at = words;
    words += w;
    return at;
  }
};
