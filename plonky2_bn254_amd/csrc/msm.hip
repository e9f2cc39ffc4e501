// g1_msm and g2_msm on the device: the witness chain of a multi-scalar multiplication, written once for both curves.
//
// G1 is the reference's src/utils/g1_msm.rs:22-36.  The reference ships no g2_msm of its own, only its pieces: the G2 chain is
// the same circuit written with the G2 gadgets (G2Target::new_checked, set_random_g2, g2_scalar_mul, G2Target::neg and
// G2Target::add, curves/g2.rs:93-150).  The reference folds
//   offset_0 = R,  offset_{i+1} = s_i x_i + offset_i  (one G1SingleGenerator::run_once / g2_scalar_mul job per link, sequential),
//   msm = offset_n + (-R)                              (G1Target::add, curves/g1.rs:117-150: a doubling is allowed, infinity not)
// and proves the n triples (s_i, x_i, offset_i) in one STARK (hook.rs:63-71).  The chain is a prefix sum of points,
// offset_i = R + sum_{j<i} s_j x_j, so it is computed here in parallel:
//   1. products P_i = s_i x_i (Jacobian; s_i is any 256-bit value, P_i may be infinity), in chunks of at most CHUNK inputs: the
//      cooperative doubling chain of trace phase A (k_g1_dbl_chain_coop, trace_g1.hip; k_g2_dbl_chain_coop, trace_g2fq.hip)
//      stores D_k = 2^k x_i, then one 256-lane workgroup per input tree-reduces lane k = (bit_k ? D_k : infinity) with the
//      complete addition law (k_msm_products).  On G2, s_i is used as the full 256-bit value, never reduced mod r: a point on
//      the twist need not lie in the r-torsion subgroup (map_to_g2 proves such points before cofactor clearing), and the G2
//      trace computes s_i x_i bit by bit, so the chain must do the same;
//   2. an inclusive scan over F_0 = R, F_{i+1} = P_i (n + 1 points): blocks of 256 with pt_scan256, the block totals scanned one
//      level up (as many levels as needed: three for n up to 2^24), each block's prefix added back on the way down;
//   3. affine normalisation with one batched inversion over Fq: G1 inverts the n + 1 Z coordinates directly; G2 takes their
//      norms (k_g2_msm_norms), inverts the norms, and gets Z^-1 from the inverse norm (fq2_inv_from_norm_inv).  An infinite
//      offset_i (i >= 1) is reported with the first such index (the reference's G1Target / G2Target cannot be infinity either);
//   4. msm = offset_n - R (k_msm_finish, the twin of k_m2g_finish): offset_n == R is an error (the result would be infinity),
//      offset_n == -R doubles (the circuit's add allows it).
// The complete addition law is used throughout, so equal partial sums double and opposite ones give infinity exactly where the
// sequential fold meets them.  Everything runs on the context's own stream and pooled buffers, like bn254s_map_to_g2.
//
// The products could also come from a fused double-and-add with one workgroup per input that stores no D_k; the doubling chain
// of phase A is used instead because it is already tuned (four lanes per input on G1, 3 products of latency per doubling) and
// the 256-lane reduction after it is 8 additions deep, where a fused loop is 256 dependent doublings plus additions per input.
//
// What differs between the curves is in the traits G1 / G2 below (on top of CurveG1 / CurveG2, trace_common.h); the coordinate
// field is reached through the fe_* overloads (fq_dev.h, trace_common.h), the points through the pt_* / lds_* overloads
// (chain_scan.h) and their SoA arrays through pa_load / pa_store (trace_common.h).
#include <climits>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "proven_jobs.h"
#include "trace_common.h"
#include "trace.h"
#include "../../include/bn254_stark.h"

namespace {

struct G1 : CurveG1 {
  static constexpr int KIND = 0;  // job kind of bn254s_prove_batch
  static constexpr size_t CHUNK = 16384;  // inputs per product launch: 3 x 4 x NPTS words = 49 KB of D_k per input, 808 MB at most
  static constexpr const char *TAG = "g1_msm", *LARGEST = "G1 proof", *POOL = "msm", *POOL_PTS = "msm.pts";
  static constexpr size_t pts_words(size_t pcnt) { return 3 * 4 * pcnt; }
  // X, Y, Z one after the other at the count of this chunk, as k_msm_products reads them (a last chunk is shorter than a full
  // one, whose count is pcnt)
  static void dbl_chain(const u64* d_x, int m, u64* pts, size_t /* pcnt */, hipStream_t st) {
    const size_t cnt = (size_t)NPTS * m;
    launch_g1_dbl_chain(d_x, m, pts, pts + 4 * cnt, pts + 8 * cnt, st);
  }
};
struct G2 : CurveG2 {
  static constexpr int KIND = 1;
  // D_k (3 x 2 x 4 x NPTS words) and the chain's znorm (4 x NPTS words) are 28 x 514 x 8 B = 115 KB per input, 943 MB for a chunk
  static constexpr size_t CHUNK = 8192;
  static constexpr const char *TAG = "g2_msm", *LARGEST = "G2 proof", *POOL = "g2msm", *POOL_PTS = "g2msm.pts";
  static constexpr size_t pts_words(size_t pcnt) { return 6 * 4 * pcnt /* D_k */ + 4 * pcnt /* znorm */; }
  // the six arrays at the count of this chunk (launch_g2_dbl_chain), znorm behind the D_k of a full chunk
  static void dbl_chain(const u64* d_x, int m, u64* pts, size_t pcnt, hipStream_t st) {
    launch_g2_dbl_chain(d_x, m, pts, pts + 6 * 4 * pcnt, st);
  }
};

// A level of the scan is cnt points in the SoA form of pa_load / pa_store (trace_common.h), like the doubling chains' arrays.

// F_0 = R (canonical affine words -> Jacobian, Montgomery)
template <class C>
__global__ __launch_bounds__(64) void k_msm_init(const u64* __restrict__ R, u64* __restrict__ lv, size_t cnt) {
  if (threadIdx.x != 0) return;
  typename C::P p;
  fe_from_canonical(R, p.x);
  fe_from_canonical(R + C::FW, p.y);
  fe_one(p.z);
  pa_store(lv, cnt, 0, p);
}

// One workgroup per input i of the chunk: lane k holds bit_k(s_i) ? D_k : infinity, a tree reduction leaves s_i x_i in lane 0,
// stored as F_{first + i} of level 0.  D_k at element (257 + k) m + i of pts (count NPTS m, launch_g1_dbl_chain / _g2_).
template <class C>
__global__ __launch_bounds__(256) void k_msm_products(const u64* __restrict__ scalars, int m, const u64* __restrict__ pts,
                                                      u64* __restrict__ lv, size_t cnt, size_t first) {
  using P = typename C::P;
  __shared__ u64 sh[3 * C::FW * 256];
  const int inst = blockIdx.x, k = threadIdx.x;
  const size_t pcnt = (size_t)NPTS * m, e = (size_t)(257 + k) * m + inst;
  const bool bit = (scalars[4 * inst + (k >> 6)] >> (k & 63)) & 1;
  P f = bit ? pa_load<P>(pts, pcnt, e) : pt_infinity((const P*)nullptr);
#pragma unroll 1
  for (int h = 128; h > 0; h >>= 1) {
    if (k >= h && k < 2 * h) lds_put(sh, k, f);
    __syncthreads();
    if (k < h) {
      P q;
      lds_get(sh, k + h, q);
      f = pt_add_complete(f, q);
    }
    __syncthreads();
  }
  if (k == 0) pa_store(lv, cnt, first + inst, f);
}

// Inclusive scan of each block of 256 points of a level in place; lane 255's sum is the block total, element b of the next
// level (up == nullptr at the top level, which is a single block).
template <class C>
__global__ __launch_bounds__(256) void k_msm_scan_blocks(u64* __restrict__ lv, size_t cnt, u64* __restrict__ up, size_t up_cnt) {
  using P = typename C::P;
  __shared__ u64 sh[3 * C::FW * 256];
  const int k = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * 256 + k;
  P f = e < cnt ? pa_load<P>(lv, cnt, e) : pt_infinity((const P*)nullptr);
  pt_scan256(f, sh, k);
  if (e < cnt) pa_store(lv, cnt, e, f);
  if (up && k == 255) pa_store(up, up_cnt, blockIdx.x, f);
}

// After the level above is scanned, its element b is the sum of blocks 0..b of this level: block b + 1 adds it to its elements.
template <class C>
__global__ __launch_bounds__(256) void k_msm_scan_add(u64* __restrict__ lv, size_t cnt, const u64* __restrict__ up, size_t up_cnt) {
  using P = typename C::P;
  const size_t b = (size_t)blockIdx.x + 1, e = b * 256 + threadIdx.x;
  if (e >= cnt) return;
  const P pre = pa_load<P>(up, up_cnt, b - 1), f = pa_load<P>(lv, cnt, e);
  pa_store(lv, cnt, e, pt_add_complete(pre, f));
}

// G2 only: zn[e] = norm(Z_e) of level 0 (zero exactly when offset_e is infinity), the input of the batched inversion
__global__ __launch_bounds__(64) void k_g2_msm_norms(const u64* __restrict__ lv, size_t cnt, u64* __restrict__ zn) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  fq2 z;
  fe_ld(lv + 16 * cnt, cnt, e, z);
  st_fq(zn, cnt, e, fq2_norm(z));
}

// offsets_i in canonical affine words (out[2 FW i ..]); zni = the batched inverses of the Z words of level 0 (G1) or of their
// norms (G2).  An infinite offset writes nothing and lowers *inf_idx to its index.
template <class C>
__global__ __launch_bounds__(64) void k_msm_affine(const u64* __restrict__ lv, size_t cnt, const u64* __restrict__ zni,
                                                   u64* __restrict__ out, unsigned* __restrict__ inf_idx) {
  using F = typename C::F;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  F x, y, z;
  fe_ld(lv + 2 * C::FW * cnt, cnt, e, z);
  if (fe_is_zero(z)) {
    atomicMin(inf_idx, (unsigned)e);
    return;
  }
  const F zi = fe_inv_from_norm_inv(z, ld_fq(zni, cnt, e)), z2 = fe_sqr(zi);
  fe_ld(lv, cnt, e, x);
  fe_ld(lv + C::FW * cnt, cnt, e, y);
  fe_store_canonical(out + 2 * C::FW * e, fe_mul(x, z2));
  fe_store_canonical(out + 2 * C::FW * e + C::FW, fe_mul(fe_mul(y, z2), zi));
}

// result = offset_n - R (affine; offset_n == -R doubles, offset_n == R is reported).  Nothing to do after an infinite offset.
// The doubling needs y1 != 0, i.e. offset_n is not a point of order 2.  G1 has odd (prime) order.  On the twist,
// #E'(Fq2) = r (2p - r) is odd, so it has no point of order 2 either, whether or not offset_n lies in the r-torsion subgroup.
template <class C>
__global__ __launch_bounds__(64) void k_msm_finish(const u64* __restrict__ o, const u64* __restrict__ R, u64* __restrict__ res,
                                                   int* __restrict__ err, const unsigned* __restrict__ inf_idx) {
  using F = typename C::F;
  if (threadIdx.x != 0 || *inf_idx != UINT_MAX) return;
  bool same_x = true, same_y = true;
  for (int l = 0; l < C::FW; l++) {
    same_x &= o[l] == R[l];
    same_y &= o[C::FW + l] == R[C::FW + l];
  }
  if (same_x && same_y) {
    *err = BN254S_E_INVALID_POINT;
    return;
  }
  F x1, y1, x2, y2, num, den;
  fe_from_canonical(o, x1);
  fe_from_canonical(o + C::FW, y1);
  fe_from_canonical(R, x2);
  fe_from_canonical(R + C::FW, y2);
  y2 = fe_neg(y2);
  if (same_x) {  // o == -R: the tangent at o
    const F x1s = fe_sqr(x1);
    num = fe_add(fe_add(x1s, x1s), x1s);
    den = fe_add(y1, y1);
  } else {
    num = fe_sub(y2, y1);
    den = fe_sub(x2, x1);
  }
  const F lam = fe_mul(num, fe_inv(den));
  const F x3 = fe_sub(fe_sub(fe_sqr(lam), x1), x2);
  const F y3 = fe_sub(fe_mul(lam, fe_sub(x1, x3)), y1);
  fe_store_canonical(res, x3);
  fe_store_canonical(res + C::FW, y3);
}

// the arguments other than the context (n < 2^32: the first infinite index travels as a 32-bit word)
bool msm_args_ok(const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n) {
  return scalars && x && offset && n > 0 && n < (size_t)UINT_MAX;
}

// The chain into host memory: offs[(n + 1) x PW], res[PW].
template <class C>
int msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* R, size_t n, uint64_t* offs, uint64_t* res) {
  constexpr size_t PW = 2 * C::FW, JW = 3 * C::FW;  // words of an affine / a Jacobian point
  constexpr bool g2 = std::is_same<typename C::F, fq2>::value;
  const std::string tag = C::TAG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // levels of the scan: level 0 = the n + 1 points F, level l + 1 = the block totals of level l, until one block remains
  std::vector<size_t> cnt{n + 1}, at{0};
  size_t lv_words = JW * (n + 1);
  while (cnt.back() > 256) {
    cnt.push_back((cnt.back() + 255) / 256);
    at.push_back(lv_words);
    lv_words += JW * cnt.back();
  }
  const size_t m_max = n < C::CHUNK ? n : C::CHUNK, pcnt = (size_t)NPTS * m_max;
  u64* d = c->words(C::POOL, 4 * n /* s */ + PW * n /* x */ + PW /* R */ + lv_words + (g2 ? 2 : 1) * 4 * (n + 1) /* [zn,] zi */ +
                                 PW * (n + 1) /* out */ + PW /* result */ + 2 /* err, inf_idx */);
  u64* d_pts = c->words(C::POOL_PTS, C::pts_words(pcnt));
  if (!d || !d_pts) return BN254S_E_OOM;
  u64* d_s = d;
  u64* d_x = d_s + 4 * n;
  u64* d_R = d_x + PW * n;
  u64* d_lv = d_R + PW;
  u64* d_zn = d_lv + lv_words;  // (G2 only)
  u64* d_zi = d_zn + (g2 ? 4 * (n + 1) : 0);
  u64* d_out = d_zi + 4 * (n + 1);
  u64* d_res = d_out + PW * (n + 1);
  int* d_err = (int*)(d_res + PW);
  unsigned* d_inf = (unsigned*)(d_err + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, st));
  HIP_TRY(c, hipMemsetAsync(d_inf, 0xFF, 4, st));
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_R, R, PW * 8, hipMemcpyHostToDevice, st));
  k_msm_init<C><<<1, 64, 0, st>>>(d_R, d_lv, cnt[0]);
  for (size_t base = 0; base < n; base += C::CHUNK) {
    const int m = (int)(n - base < C::CHUNK ? n - base : C::CHUNK);
    C::dbl_chain(d_x + PW * base, m, d_pts, pcnt, st);
    k_msm_products<C><<<(unsigned)m, 256, 0, st>>>(d_s + 4 * base, m, d_pts, d_lv, cnt[0], base + 1);
  }
  const size_t top = cnt.size() - 1;
  for (size_t l = 0; l <= top; l++)
    k_msm_scan_blocks<C><<<(unsigned)((cnt[l] + 255) / 256), 256, 0, st>>>(d_lv + at[l], cnt[l], l < top ? d_lv + at[l + 1] : nullptr,
                                                                         l < top ? cnt[l + 1] : 0);
  for (size_t l = top; l-- > 0;)
    k_msm_scan_add<C><<<(unsigned)((cnt[l] + 255) / 256 - 1), 256, 0, st>>>(d_lv + at[l], cnt[l], d_lv + at[l + 1], cnt[l + 1]);
  const unsigned g0 = (unsigned)((cnt[0] + 63) / 64);
  if (g2) {  // the batched inversion works on Fq: invert the norms of Z
    k_g2_msm_norms<<<g0, 64, 0, st>>>(d_lv, cnt[0], d_zn);
    launch_fq_batch_inv(d_zn, d_zi, cnt[0], st);
  } else {  // the Z plane of level 0 is an Fq vector already
    launch_fq_batch_inv(d_lv + 8 * cnt[0], d_zi, cnt[0], st);
  }
  k_msm_affine<C><<<g0, 64, 0, st>>>(d_lv, cnt[0], d_zi, d_out, d_inf);
  k_msm_finish<C><<<1, 64, 0, st>>>(d_out + PW * n, d_R, d_res, d_err, d_inf);
  HIP_TRY(c, hipGetLastError());
  int h_err[2];
  HIP_TRY(c, hipMemcpyAsync(offs, d_out, (n + 1) * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(res, d_res, PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_err, d_err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const unsigned inf = (unsigned)h_err[1];
  if (inf != UINT_MAX) {
    c->set_err(tag + ": offset_" + std::to_string(inf) + " = R + s_0 x_0 + ... + s_" + std::to_string(inf - 1) + " x_" +
               std::to_string(inf - 1) + " is the point at infinity");
    return BN254S_E_INVALID_POINT;
  }
  if (h_err[0]) {
    c->set_err(tag + ": offset_n equals R, the result is the point at infinity");
    return h_err[0];
  }
  return BN254S_OK;
}

// The chain, its proofs (bn254s_prove_batch of the n links) and the check that the two agree.
template <class C>
int msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
        size_t per_proof, uint64_t* result, uint64_t* offsets_out, bn254s_proof** proofs) {
  constexpr size_t PW = 2 * C::FW;
  const std::string tag = C::TAG;
  int rc = proven_args(c, tag, C::LARGEST, msm_args_ok(scalars, x, offset, n) && result, params, proofs, n, per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> offs(PW * (n + 1)), outs;
  rc = msm_chain<C>(c, scalars, x, offset, n, offs.data(), result);
  if (rc != BN254S_OK) return rc;
  rc = prove_and_collect(c, tag, C::KIND, params, scalars, x, offs.data(), n, per_proof, proofs, outs);
  if (rc != BN254S_OK) return rc;
  // linkage: the trace generator computes s_i x_i + offset_i on its own; it must land on offset_{i+1}
  for (size_t j = 0; j < n; j++)
    if (memcmp(outs.data() + PW * j, offs.data() + PW * (j + 1), PW * 8) != 0) {
      c->set_err(tag + ": output " + std::to_string(j) + " of the proofs differs from offset_" + std::to_string(j + 1) + " of the chain");
      release_proofs(proofs, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  if (offsets_out) memcpy(offsets_out, offs.data(), offs.size() * 8);
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g1_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain<G1>(c, scalars, x, offset, n, offsets_out, result);
}
extern "C" int bn254s_g2_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain<G2>(c, scalars, x, offset, n, offsets_out, result);
}
extern "C" int bn254s_g1_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  return msm<G1>(c, params, scalars, x, offset, n, per_proof, result, offsets_out, proofs);
}
extern "C" int bn254s_g2_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  return msm<G2>(c, params, scalars, x, offset, n, per_proof, result, offsets_out, proofs);
}
