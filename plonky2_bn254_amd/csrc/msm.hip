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
//   2. an inclusive scan over F_0 = R, F_{i+1} = P_i (n + 1 points; launch_scan): blocks of 256 with pt_scan256
//      (k_msm_scan_blocks<C, false>), the block totals scanned one level up (as many levels as needed: three for n up to 2^24),
//      each block's prefix added back on the way down (k_msm_scan_add<C, false>);
//   3. affine normalisation with one batched inversion over Fq (launch_z_inverses, k_msm_affine): G1 inverts the n + 1 Z
//      coordinates directly; G2 takes their norms (k_g2_msm_norms), inverts the norms, and gets Z^-1 from the inverse norm
//      (fq2_inv_from_norm_inv).  An infinite offset_i (i >= 1) is reported with the first such index (the reference's G1Target /
//      G2Target cannot be infinity either);
//   4. msm = offset_n - R (k_msm_finish on pt_sub_slope / pt_sub_point, job_curve.h, like k_smul_sub): offset_n == R is an error
//      (the result would be infinity), offset_n == -R doubles (the circuit's add allows it).
// The complete addition law is used throughout, so equal partial sums double and opposite ones give infinity exactly where the
// sequential fold meets them.  Everything runs on the context's own stream and pooled buffers, like bn254s_map_to_g2.
//
// The products could also come from a fused double-and-add with one workgroup per input that stores no D_k; the doubling chain
// of phase A is used instead because it is already tuned (four lanes per input on G1, 3 products of latency per doubling) and
// the 256-lane reduction after it is 8 additions deep, where a fused loop is 256 dependent doublings plus additions per input.
//
// The lower half of the file is many MSMs at once as one segmented chain with R outside the scan (bn254s_msm_multi_chain,
// bn254s_msm_multi): the same products, the same scan kernels with head flags (SEG), and per attempt round (draw_rounds,
// offset_draw.h) the drawn R_j, the links, one batched inversion and the job check of every link; it has its own header comment.
//
// What differs between the curves is in the traits G1 / G2 (job_curve.h: the ones of job_outputs.hip, job_check.hip and
// scalar_mul.hip) and, for what only an MSM needs, in MsmG1 / MsmG2 below: the kernels are written over the first, the host
// functions over the second.  The coordinate field is reached through the fe_* overloads (fq_dev.h, trace_common.h), the points through the pt_* / lds_* overloads
// (chain_scan.h) and their SoA arrays through pa_load / pa_store (trace_common.h).
#include <climits>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "job_curve.h"
#include "job_device.h"
#include "offset_draw.h"
#include "proven_jobs.h"
#include "trace_common.h"
#include "trace.h"
#include "../../include/bn254_stark.h"

namespace {

// What only the MSMs need to know of a curve, beside the traits G1 / G2 that the kernels are written over (Curve)
struct MsmG1 {
  using Curve = G1;
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
struct MsmG2 {
  using Curve = G2;
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
  C::load(R, p);  // (its answer, whether R is on the curve, is not asked for)
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
// level (up == nullptr at the top level, which is a single block).  SEG: the segmented scan of (flag, point), flags[e] set where
// element e is the head of an MSM; a lane's flag becomes "a head at or before it in this block" and lane 255's pair is the block
// total with "this block contains a head".  The plain scan has no flags: both flag pointers are nullptr and never read.
template <class C, bool SEG>
__global__ __launch_bounds__(256) void k_msm_scan_blocks(u64* __restrict__ lv, unsigned* __restrict__ flags, size_t cnt, u64* __restrict__ up,
                                                         unsigned* __restrict__ up_flags, size_t up_cnt) {
  using P = typename C::P;
  __shared__ u64 sh[3 * C::FW * 256];
  const int k = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * 256 + k;
  P f = e < cnt ? pa_load<P>(lv, cnt, e) : pt_infinity((const P*)nullptr);
  unsigned flag = 0;
  if constexpr (SEG) {
    __shared__ unsigned shf[256];
    flag = e < cnt ? flags[e] : 0u;
    pt_seg_scan256(f, flag, sh, shf, k);
  } else {
    pt_scan256(f, sh, k);
  }
  if (e < cnt) {
    pa_store(lv, cnt, e, f);
    if constexpr (SEG) flags[e] = flag;
  }
  if (up && k == 255) {
    pa_store(up, up_cnt, blockIdx.x, f);
    if constexpr (SEG) up_flags[blockIdx.x] = flag;
  }
}

// After the level above is scanned, its element b is the sum of blocks 0..b of this level (SEG: from the last head in them on):
// block b + 1 adds it to its elements (SEG: to the lanes before its first head).
template <class C, bool SEG>
__global__ __launch_bounds__(256) void k_msm_scan_add(u64* __restrict__ lv, const unsigned* __restrict__ flags, size_t cnt,
                                                      const u64* __restrict__ up, size_t up_cnt) {
  using P = typename C::P;
  const size_t b = (size_t)blockIdx.x + 1, e = b * 256 + threadIdx.x;
  if (e >= cnt) return;
  if constexpr (SEG)
    if (flags[e]) return;
  const P pre = pa_load<P>(up, up_cnt, b - 1), f = pa_load<P>(lv, cnt, e);
  pa_store(lv, cnt, e, pt_add_complete(pre, f));
}

// The levels of a scan over n points: level 0 = the n points, level l + 1 = the block totals of level l, until one block remains
// (three levels for n up to 2^24).  at / fat: where a level starts among the point words / the flags of all levels.
struct ScanLevels {
  std::vector<size_t> cnt, at, fat;
  size_t words, flags;
  ScanLevels(size_t n, size_t jw) : cnt{n}, at{0}, fat{0}, words(jw * n), flags(n) {
    while (cnt.back() > 256) {
      cnt.push_back((cnt.back() + 255) / 256);
      at.push_back(words);
      fat.push_back(flags);
      words += jw * cnt.back();
      flags += cnt.back();
    }
  }
};

// the up-sweep and the down-sweep; d_flags: the flags of all levels, those of level 0 filled in (SEG), or nullptr
template <class C, bool SEG>
void launch_scan(const ScanLevels& lv, u64* d_lv, unsigned* d_flags, hipStream_t st) {
  const size_t top = lv.cnt.size() - 1;
  auto pts = [&](size_t l) { return l <= top ? d_lv + lv.at[l] : nullptr; };
  auto flg = [&](size_t l) { return SEG && l <= top ? d_flags + lv.fat[l] : nullptr; };
  for (size_t l = 0; l <= top; l++)
    k_msm_scan_blocks<C, SEG><<<(unsigned)((lv.cnt[l] + 255) / 256), 256, 0, st>>>(pts(l), flg(l), lv.cnt[l], pts(l + 1), flg(l + 1),
                                                                                 l < top ? lv.cnt[l + 1] : 0);
  for (size_t l = top; l-- > 0;)
    k_msm_scan_add<C, SEG><<<(unsigned)((lv.cnt[l] + 255) / 256 - 1), 256, 0, st>>>(pts(l), flg(l), lv.cnt[l], pts(l + 1), lv.cnt[l + 1]);
}

// G2 only: zn[e] = norm(Z_e) of level 0 (zero exactly when offset_e is infinity), the input of the batched inversion
__global__ __launch_bounds__(64) void k_g2_msm_norms(const u64* __restrict__ lv, size_t cnt, u64* __restrict__ zn) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  fq2 z;
  fe_ld(lv + 16 * cnt, cnt, e, z);
  st_fq(zn, cnt, e, fq2_norm(z));
}

// The batched inverses zi of the Z of cnt points (G1: the Z plane is an Fq vector already) or of their norms zn (G2: the batched
// inversion works on Fq)
template <class C>
void launch_z_inverses(const u64* pts, size_t cnt, u64* d_zn, u64* d_zi, hipStream_t st) {
  if constexpr (std::is_same<typename C::F, fq2>::value) {
    k_g2_msm_norms<<<(unsigned)((cnt + 63) / 64), 64, 0, st>>>(pts, cnt, d_zn);
    launch_fq_batch_inv(d_zn, d_zi, cnt, st);
  } else {
    launch_fq_batch_inv(pts + 2 * C::FW * cnt, d_zi, cnt, st);
  }
}

// Element e of the cnt points pts in canonical affine words w[PW]; zni: launch_z_inverses of pts.  false, and nothing written,
// for the point at infinity.
template <class C>
__device__ __forceinline__ bool affine_words(const u64* __restrict__ pts, const u64* __restrict__ zni, size_t cnt, size_t e, u64* w) {
  using F = typename C::F;
  F x, y, z;
  fe_ld(pts + 2 * C::FW * cnt, cnt, e, z);
  if (fe_is_zero(z)) return false;
  const F zi = fe_inv_from_norm_inv(z, ld_fq(zni, cnt, e)), z2 = fe_sqr(zi);
  fe_ld(pts, cnt, e, x);
  fe_ld(pts + C::FW * cnt, cnt, e, y);
  fe_store_canonical(w, fe_mul(x, z2));
  fe_store_canonical(w + C::FW, fe_mul(fe_mul(y, z2), zi));
  return true;
}

// offsets_i in canonical affine words (out[PW i ..]) from level 0 and its Z inverses.  An infinite offset writes nothing and
// lowers *inf_idx to its index.
template <class C>
__global__ __launch_bounds__(64) void k_msm_affine(const u64* __restrict__ lv, size_t cnt, const u64* __restrict__ zni,
                                                   u64* __restrict__ out, unsigned* __restrict__ inf_idx) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  if (!affine_words<C>(lv, zni, cnt, e, out + C::PW * e)) atomicMin(inf_idx, (unsigned)e);
}

// result = offset_n - R (pt_sub_slope, job_curve.h): offset_n == R is reported, offset_n == -R doubles, as does every other R that
// shares its x with offset_n (the chain does not ask for points of the curve).  Nothing to do after an infinite offset.
// The cases are told apart in the field, after fe_from_canonical: an R with a coordinate not below p, which the chain call does
// not refuse, counts as the residue it stands for (offset_n == R is then reported for it too).
// (The doubling needs y1 != 0: G1 has prime order and #E'(Fq2) = r (2p - r) is odd, so neither has a point of order 2.)
template <class C>
__global__ __launch_bounds__(64) void k_msm_finish(const u64* __restrict__ o, const u64* __restrict__ R, u64* __restrict__ res,
                                                   int* __restrict__ err, const unsigned* __restrict__ inf_idx) {
  using F = typename C::F;
  if (threadIdx.x != 0 || *inf_idx != UINT_MAX) return;
  F x1, y1, x2, y2, num, den, x3, y3;
  fe_from_canonical(o, x1);
  fe_from_canonical(o + C::FW, y1);
  fe_from_canonical(R, x2);
  fe_from_canonical(R + C::FW, y2);
  const int which = pt_sub_slope(x1, y1, x2, y2, num, den);
  if (which == SUB_EQUAL) {
    *err = BN254S_E_INVALID_POINT;
    return;
  }
  if (which == SUB_SAME_X) pt_tangent(x1, y1, num, den);  // (an R off the curve) the tangent at offset_n all the same
  pt_sub_point(x1, y1, x2, num, den, x3, y3);
  fe_store_canonical(res, x3);
  fe_store_canonical(res + C::FW, y3);
}

// the arguments other than the context (n < 2^32: the first infinite index travels as a 32-bit word)
bool msm_args_ok(const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n) {
  return scalars && x && offset && n > 0 && n < (size_t)UINT_MAX;
}

// The products of the n inputs, chunk by chunk through the D_k in d_pts (M::pts_words(products_pcnt<M>(n)) words), as elements
// first .. first + n - 1 of a level 0 of cnt points
template <class M>
size_t products_pcnt(size_t n) {
  return (size_t)NPTS * (n < M::CHUNK ? n : M::CHUNK);
}
template <class M>
void launch_products(const u64* d_s, const u64* d_x, size_t n, u64* d_pts, u64* d_lv, size_t cnt, size_t first, hipStream_t st) {
  using C = typename M::Curve;
  for (size_t base = 0; base < n; base += M::CHUNK) {
    const int m = (int)(n - base < M::CHUNK ? n - base : M::CHUNK);
    M::dbl_chain(d_x + C::PW * base, m, d_pts, products_pcnt<M>(n), st);
    k_msm_products<C><<<(unsigned)m, 256, 0, st>>>(d_s + 4 * base, m, d_pts, d_lv, cnt, first + base);
  }
}

// The chain into host memory: offs[(n + 1) x PW], res[PW].
template <class M>
int msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* R, size_t n, uint64_t* offs, uint64_t* res) {
  using C = typename M::Curve;
  constexpr size_t PW = C::PW, JW = 3 * C::FW;  // words of an affine / a Jacobian point
  constexpr bool g2 = std::is_same<typename C::F, fq2>::value;
  const std::string tag = M::TAG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t cnt0 = n + 1;  // level 0 = the n + 1 points F
  const ScanLevels levels(cnt0, JW);
  u64* d = c->words(M::POOL, 4 * n /* s */ + PW * n /* x */ + PW /* R */ + levels.words + (g2 ? 2 : 1) * 4 * cnt0 /* [zn,] zi */ +
                                 PW * cnt0 /* out */ + PW /* result */ + 2 /* err, inf_idx */);
  u64* d_pts = c->words(M::POOL_PTS, M::pts_words(products_pcnt<M>(n)));
  if (!d || !d_pts) return BN254S_E_OOM;
  u64 *d_s = d, *d_x = d_s + 4 * n, *d_R = d_x + PW * n, *d_lv = d_R + PW, *d_zn = d_lv + levels.words /* (G2 only) */;
  u64 *d_zi = d_zn + (g2 ? 4 * cnt0 : 0), *d_out = d_zi + 4 * cnt0, *d_res = d_out + PW * cnt0;
  int* d_err = (int*)(d_res + PW);
  unsigned* d_inf = (unsigned*)(d_err + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, st));
  HIP_TRY(c, hipMemsetAsync(d_inf, 0xFF, 4, st));
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_R, R, PW * 8, hipMemcpyHostToDevice, st));
  k_msm_init<C><<<1, 64, 0, st>>>(d_R, d_lv, cnt0);
  launch_products<M>(d_s, d_x, n, d_pts, d_lv, cnt0, 1, st);
  launch_scan<C, false>(levels, d_lv, nullptr, st);
  launch_z_inverses<C>(d_lv, cnt0, d_zn, d_zi, st);
  k_msm_affine<C><<<(unsigned)((cnt0 + 63) / 64), 64, 0, st>>>(d_lv, cnt0, d_zi, d_out, d_inf);
  k_msm_finish<C><<<1, 64, 0, st>>>(d_out + PW * n, d_R, d_res, d_err, d_inf);
  HIP_TRY(c, hipGetLastError());
  int h_err[2];
  HIP_TRY(c, hipMemcpyAsync(offs, d_out, cnt0 * PW * 8, hipMemcpyDeviceToHost, st));
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
template <class M>
int msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
        size_t per_proof, uint64_t* result, uint64_t* offsets_out, bn254s_proof** proofs) {
  constexpr size_t PW = M::Curve::PW;
  const std::string tag = M::TAG;
  int rc = proven_args(c, tag, M::LARGEST, msm_args_ok(scalars, x, offset, n) && result, params, proofs, n, per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> offs(PW * (n + 1)), outs;
  rc = msm_chain<M>(c, scalars, x, offset, n, offs.data(), result);
  if (rc != BN254S_OK) return rc;
  rc = prove_and_collect(c, tag, M::Curve::KIND, params, scalars, x, offs.data(), n, per_proof, proofs, outs);
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

// ---- many MSMs as one segmented chain (bn254s_msm_multi_chain, bn254s_msm_multi; DESIGN.md "Many MSMs in one chain") -------------
// m MSMs, MSM j the inputs first[j] .. first[j + 1] - 1 of n.  R is not in the scan:
//   1. k_mm_check      x_i and (where they are supplied) R_j on their curve
//   2. k_msm_products  P_i = s_i x_i, element i of level 0 (n points, no F_0)
//   3. k_mm_heads, k_msm_scan_blocks<C, true> / k_msm_scan_add<C, true>: the segmented inclusive scan of (head flag, P_i), I_i = the
//      sum from the head of i's MSM to i
//   4. per attempt round (draw_rounds, offset_draw.h; one round and nothing drawn for supplied R):
//        k_draw_inputs, hash_to_g1 | hash_to_g2, k_mm_take   R_j of the listed MSMs (round 0: all; later: the ones just rejected)
//        k_mm_link     element i = R_seg(i) + I_i (the output of link i); elements n .. n + m - 1 = the last I of each MSM (its result)
//        launch_z_inverses over the n + m Z
//        k_mm_affine   outputs, offsets (R_j at a head, else the output before), results and finite flags in canonical words
//        k_job_check of the n links, k_mm_min: the smallest (t << 16 | step) that hits per MSM
//        k_mm_accept   a listed MSM without a hit is accepted; the others are marked and counted -> the control words go to the host
//        k_draw_compact  the list of the marked MSMs, their attempt raised by one
//   5. k_mm_final      bad_link / bad_step / attempts per MSM; the rows of an unprovable MSM are cleared
// Every round links and checks all n jobs, also those of MSMs accepted before: their R_j has not moved, so their rows come out the
// same, and a round after the first happens only for inputs crafted against a hashed point.
// Where an output is infinite its link hits (at the top set bit of s_i), so the MSM is bad from that link or an earlier one on; the
// next link gets R_j as the offset it is checked with, which keeps the job check on point words and cannot lower the minimum.

constexpr u64 MM_DOMAIN = 0x626D6D00;  // "bmm\0" + kind: the last hash input
constexpr unsigned long long MM_MIN_NONE = ~0ULL;

// bad[0] (bad[1]): the smallest i (j) whose x_i (R_j) is off the curve; R == nullptr: drawn points, checked by their own kernels
template <class C>
__global__ __launch_bounds__(64) void k_mm_check(const u64* __restrict__ x, size_t n, const u64* __restrict__ R, size_t m,
                                                 unsigned* __restrict__ bad) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n + (R ? m : 0)) return;
  typename C::P p;
  if (!C::load(e < n ? x + C::PW * e : R + C::PW * (e - n), p)) atomicMin(bad + (e < n ? 0 : 1), (unsigned)(e < n ? e : e - n));
}

// the head flags of level 0
__global__ __launch_bounds__(256) void k_mm_heads(const unsigned* __restrict__ seg_of, size_t n, unsigned* __restrict__ flags) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) flags[e] = e == 0 || seg_of[e] != seg_of[e - 1];
}

// R_j of the listed MSMs from the drawn points.  A drawn point that is infinity (G2: the cleared image) fails the attempt: R_j
// becomes the first x of the MSM, a point every kernel below can work with, and fail[j] is set.
__global__ __launch_bounds__(256) void k_mm_take(const unsigned* __restrict__ list, size_t cnt, int pw, HashedPoints at,
                                                 const u64* __restrict__ x, const unsigned* __restrict__ first, u64* __restrict__ R,
                                                 unsigned char* __restrict__ fail, unsigned* __restrict__ ctl) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  if (k == 0) draw_self_check(at, ctl);
  const size_t j = list ? list[k] : k;
  const bool inf = at.finite && !at.finite[k];
  const u64* src = inf ? x + (size_t)pw * first[j] : at.points + (size_t)pw * k;
  for (int w = 0; w < pw; w++) R[(size_t)pw * j + w] = src[w];
  fail[j] = inf;
}

// ob: n + m points.  Element i < n: R_seg(i) + I_i, the output of link i; element n + j: the last I of MSM j, its result.
template <class C>
__global__ __launch_bounds__(64) void k_mm_link(const u64* __restrict__ lv, size_t n, size_t m, const unsigned* __restrict__ seg_of,
                                                const unsigned* __restrict__ first, const u64* __restrict__ R, u64* __restrict__ ob) {
  using P = typename C::P;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n + m) return;
  if (e >= n) {
    pa_store(ob, n + m, e, pa_load<P>(lv, n, (size_t)first[e - n + 1] - 1));
    return;
  }
  P p;
  C::load(R + C::PW * (size_t)seg_of[e], p);  // (on the curve: k_mm_check, or the hash-to-curve kernels' own checks)
  pa_store(ob, n + m, e, pt_add_complete(p, pa_load<P>(lv, n, e)));
}

// zni: launch_z_inverses of ob.  Lane i < n writes outputs[i] and the offset of the
// next link of its MSM (R_j in its place where the output is infinite, see above), and offsets[i] = R_j where i is a head; lane
// n + j writes results[j] and finite[j].  Every row is written by exactly one lane.
template <class C>
__global__ __launch_bounds__(64) void k_mm_affine(const u64* __restrict__ ob, const u64* __restrict__ zni, size_t n, size_t m,
                                                  const unsigned* __restrict__ seg_of, const unsigned* __restrict__ first,
                                                  const u64* __restrict__ R, u64* __restrict__ outputs, u64* __restrict__ offsets,
                                                  u64* __restrict__ results, unsigned char* __restrict__ finite) {
  constexpr int PW = C::PW;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, cnt = n + m;
  if (e >= cnt) return;
  u64 w[PW];
  const bool inf = !affine_words<C>(ob, zni, cnt, e, w);
  if (inf) {
#pragma unroll
    for (int l = 0; l < PW; l++) w[l] = 0;
  }
  if (e >= n) {
#pragma unroll
    for (int l = 0; l < PW; l++) results[PW * (e - n) + l] = w[l];
    finite[e - n] = !inf;
    return;
  }
  const size_t j = seg_of[e];
  const u64* r = R + PW * j;
#pragma unroll
  for (int l = 0; l < PW; l++) outputs[PW * e + l] = w[l];
  if (e == first[j]) {
#pragma unroll
    for (int l = 0; l < PW; l++) offsets[PW * e + l] = r[l];
  }
  if (e + 1 < first[j + 1]) {
#pragma unroll
    for (int l = 0; l < PW; l++) offsets[PW * (e + 1) + l] = inf ? r[l] : w[l];
  }
}

// minw[j] = the smallest (t << 16 | step) over the links of MSM j that hit, t the link's place in its MSM
__global__ __launch_bounds__(256) void k_mm_min(const unsigned short* __restrict__ step, size_t n, const unsigned* __restrict__ seg_of,
                                                const unsigned* __restrict__ first, unsigned long long* __restrict__ minw) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || step[i] == BN254S_JOB_STEP_NONE) return;
  const unsigned j = seg_of[i];
  atomicMin(minw + j, ((unsigned long long)(i - first[j]) << 16) | step[i]);
}

// A listed MSM without a hit (and with a finite drawn point) is accepted; every other one is marked in rejected[j] and counted.
__global__ __launch_bounds__(256) void k_mm_accept(const unsigned* __restrict__ list, size_t cnt, unsigned long long* __restrict__ minw,
                                                   const unsigned char* __restrict__ fail, unsigned char* __restrict__ rejected,
                                                   unsigned* __restrict__ ctl, int round) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const size_t j = list ? list[k] : k;
  if (fail[j]) minw[j] = BN254S_JOB_STEP_NONE;  // link 0, no step
  rejected[j] = minw[j] != MM_MIN_NONE;
  if (rejected[j]) atomicAdd(ctl + CTL_COUNT + round, 1u);
}

// Lane i < n clears the rows of link i where its MSM is unprovable; lane n + j writes bad_link[j], bad_step[j] and, for drawn
// points, raises the attempts of an MSM that ran out of them to max_attempts.
__global__ __launch_bounds__(256) void k_mm_final(size_t n, size_t m, int pw, const unsigned* __restrict__ seg_of,
                                                  const unsigned char* __restrict__ rejected, const unsigned long long* __restrict__ minw,
                                                  u64* __restrict__ outputs, u64* __restrict__ offsets, unsigned* __restrict__ bad_link,
                                                  unsigned short* __restrict__ bad_step, unsigned char* __restrict__ attempts, bool drawn) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n + m) return;
  if (e < n) {
    if (rejected[seg_of[e]])
      for (int w = 0; w < pw; w++) outputs[(size_t)pw * e + w] = offsets[(size_t)pw * e + w] = 0;
    return;
  }
  const size_t j = e - n;
  const unsigned long long v = minw[j];
  bad_link[j] = v == MM_MIN_NONE ? BN254S_MSM_LINK_NONE : (unsigned)(v >> 16);
  bad_step[j] = (unsigned short)(v & 0xFFFF);
  if (drawn && rejected[j]) attempts[j]++;
}

// The predicate of both entry points on their own arguments, every check that needs no device.
bool mm_args_ok(bn254s_ctx* c, const char* tag, int kind, const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m,
                size_t n, const uint64_t* R, const uint64_t* seed, int max_attempts, const void* results, const void* finite,
                const void* offsets, const void* outputs, const void* bad_link) {
  if (kind < 0 || kind > 1 || !scalars || !x || !seg_len || !results || !finite || !offsets || !outputs || !bad_link || (!R && !seed) ||
      m == 0 || n >= (size_t)UINT_MAX)
    return false;
  size_t sum = 0;
  for (size_t j = 0; j < m; j++) {
    if (seg_len[j] == 0 || seg_len[j] > n - sum) return false;
    sum += seg_len[j];
  }
  if (sum != n) return false;
  if (!R && (max_attempts < 1 || max_attempts > DRAW_MAX_ATTEMPTS || !seed_canonical(seed))) return false;
  const char* const* coord = kind == 0 ? COORD_G1 : COORD_G2;
  const int nc = (int)point_words(kind) / 4;
  return coords_below_p(c, tag, "x", coord, nc, x, n) && (!R || coords_below_p(c, tag, "R", coord, nc, R, m));
}

// what the front-end answers, in host memory (bad_step and attempts always, unlike the optional arguments of the entry points)
struct MmOut {
  uint64_t *results, *offsets, *outputs, *R;
  uint8_t *finite, *attempts;
  uint32_t* bad_link;
  uint16_t* bad_step;
};

// The front-end into host memory.  Nothing is written on an error.
template <class M>
int mm_front(bn254s_ctx* c, const char* tag, const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m, size_t n,
             const uint64_t* R, const uint64_t* seed, int max_attempts, const MmOut& o) {
  using C = typename M::Curve;
  constexpr size_t PW = C::PW, JW = 3 * C::FW;
  constexpr bool g2 = std::is_same<typename C::F, fq2>::value;
  constexpr int kind = C::KIND;
  const std::string who = std::string(tag) + ": ";
  const bool drawn = R == nullptr;
  std::vector<unsigned> h_seg(n), h_first(m + 1);
  for (size_t j = 0, i = 0; j < m; j++) {
    h_first[j] = (unsigned)i;
    for (size_t t = 0; t < seg_len[j]; t++) h_seg[i++] = (unsigned)j;
  }
  h_first[m] = (unsigned)n;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const ScanLevels levels(n, JW);  // level 0 = the n products
  const size_t lv_words = levels.words, fl = levels.flags, tot = n + m, mb = (m + 7) / 8 /* words of m bytes */;
  const size_t hw = drawn ? draw_device_words(kind, m) : 0;
  u64* d = c->words("msm.multi", 4 * n /* s */ + PW * n /* x */ + PW * m /* R */ + lv_words + JW * tot /* ob */ +
                                     (g2 ? 2 : 1) * 4 * tot /* [zn,] zi */ + 2 * PW * n /* outputs, offsets */ + PW * m /* results */ +
                                     8 * m /* hash inputs */ + hw + m /* minw */ + (fl + 1) / 2 /* flags */ + (n + 1) / 2 /* seg_of */ +
                                     (m + 2) / 2 /* first */ + 2 * ((m + 1) / 2) /* list, bad_link */ + (n + 3) / 4 /* step */ +
                                     (m + 3) / 4 /* bad_step */ + 4 * mb /* attempts, rejected, fail, finite */ + CTL_WORDS / 2);
  u64* d_pts = c->words(M::POOL_PTS, M::pts_words(products_pcnt<M>(n)));
  if (!d || !d_pts) return BN254S_E_OOM;
  u64 *d_s = d, *d_x = d_s + 4 * n, *d_R = d_x + PW * n, *d_lv = d_R + PW * m, *d_ob = d_lv + lv_words, *d_zn = d_ob + JW * tot;
  u64 *d_zi = d_zn + (g2 ? 4 * tot : 0), *d_out = d_zi + 4 * tot, *d_off = d_out + PW * n, *d_res = d_off + PW * n, *d_in = d_res + PW * m;
  u64* d_hash = d_in + 8 * m;
  unsigned long long* d_min = (unsigned long long*)(d_hash + hw);
  unsigned* d_flags = (unsigned*)(d_min + m);
  unsigned* d_seg = d_flags + 2 * ((fl + 1) / 2);
  unsigned* d_first = d_seg + 2 * ((n + 1) / 2);
  unsigned* d_list = d_first + 2 * ((m + 2) / 2);
  unsigned* d_blink = d_list + 2 * ((m + 1) / 2);
  unsigned short* d_step = (unsigned short*)(d_blink + 2 * ((m + 1) / 2));
  unsigned short* d_bstep = d_step + 4 * ((n + 3) / 4);
  unsigned char* d_att = (unsigned char*)(d_bstep + 4 * ((m + 3) / 4));
  unsigned char *d_rej = d_att + 8 * mb, *d_fail = d_rej + 8 * mb, *d_fin = d_fail + 8 * mb;
  unsigned* d_ctl = (unsigned*)(d_fin + 8 * mb);
  int rc = draw_ctl_clear(c, d_ctl);
  if (rc != BN254S_OK) return rc;
  HIP_TRY(c, hipMemsetAsync(d_att, 0, 3 * 8 * mb, st));  // attempts, rejected and fail
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_seg, h_seg.data(), n * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_first, h_first.data(), (m + 1) * 4, hipMemcpyHostToDevice, st));
  if (!drawn) HIP_TRY(c, hipMemcpyAsync(d_R, R, m * PW * 8, hipMemcpyHostToDevice, st));
  k_mm_check<C><<<(unsigned)((tot + 63) / 64), 64, 0, st>>>(d_x, n, drawn ? nullptr : d_R, m, d_ctl + CTL_BAD);
  k_mm_heads<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_seg, n, d_flags);
  launch_products<M>(d_s, d_x, n, d_pts, d_lv, n, 0, st);
  launch_scan<C, true>(levels, d_lv, d_flags, st);
  HIP_TRY(c, hipGetLastError());
  const char* curve = curve_name(kind);
  const unsigned gt = (unsigned)((tot + 63) / 64);
  // a round: R_j of the listed MSMs (drawn points only), then every link, its affine rows and its job check, and who keeps its R_j
  auto body = [&](int round, const unsigned* list, size_t listed, const HashedPoints& at) -> int {
    const unsigned gl = (unsigned)((listed + 255) / 256);
    if (drawn) k_mm_take<<<gl, 256, 0, st>>>(list, listed, (int)PW, at, d_x, d_first, d_R, d_fail, d_ctl);
    HIP_TRY(c, hipMemsetAsync(d_min, 0xFF, m * 8, st));
    k_mm_link<C><<<gt, 64, 0, st>>>(d_lv, n, m, d_seg, d_first, d_R, d_ob);
    launch_z_inverses<C>(d_ob, tot, d_zn, d_zi, st);
    k_mm_affine<C><<<gt, 64, 0, st>>>(d_ob, d_zi, n, m, d_seg, d_first, d_R, d_out, d_off, d_res, d_fin);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemsetAsync(d_step, 0xFF, n * 2, st));  // (a job k_job_check finds off its curve writes no step)
    const int rc = bn254s_job_check_device(c, kind, d_s, d_x, d_off, n, d_step, d_ctl + CTL_CHK_BAD);
    if (rc != BN254S_OK) return rc;
    k_mm_min<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_step, n, d_seg, d_first, d_min);
    k_mm_accept<<<gl, 256, 0, st>>>(list, listed, d_min, d_fail, d_rej, d_ctl, round);
    HIP_TRY(c, hipGetLastError());
    return BN254S_OK;
  };
  auto check = [&](const unsigned* h_ctl) -> int {
    if (h_ctl[CTL_BAD] != UINT_MAX || h_ctl[CTL_BAD + 1] != UINT_MAX) {  // x before R
      const bool is_x = h_ctl[CTL_BAD] != UINT_MAX;
      c->set_err(who + (is_x ? "x_" : "R_") + std::to_string(h_ctl[CTL_BAD + (is_x ? 0 : 1)]) + " is not on " + curve);
      return BN254S_E_INVALID_ARG;
    }
    if (h_ctl[CTL_ERR]) {
      c->set_err(who + "a drawn offset failed the self-check of its hash-to-curve kernel (device self-check)");
      return BN254S_E_INTERNAL;
    }
    if (h_ctl[CTL_CHK_BAD] != UINT_MAX || h_ctl[CTL_CHK_BAD + 1] != UINT_MAX) {
      const bool is_x = h_ctl[CTL_CHK_BAD] != UINT_MAX;
      c->set_err(who + "the job check found " + (is_x ? "x_" : "the offset of link ") + std::to_string(h_ctl[CTL_CHK_BAD + (is_x ? 0 : 1)]) +
                 " off " + curve + " (device self-check)");
      return BN254S_E_INTERNAL;
    }
    return BN254S_OK;
  };
  rc = draw_rounds(c, who, "MSMs", kind, MM_DOMAIN, drawn ? seed : nullptr, max_attempts, m, DrawBuffers{d_in, d_hash, d_att, d_rej, d_list, d_ctl},
                   body, check);
  if (rc != BN254S_OK) return rc;
  k_mm_final<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(n, m, (int)PW, d_seg, d_rej, d_min, d_out, d_off, d_blink, d_bstep, d_att, drawn);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(o.results, d_res, m * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.finite, d_fin, m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.offsets, d_off, n * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.outputs, d_out, n * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.R, d_R, m * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.attempts, d_att, m, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.bad_link, d_blink, m * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(o.bad_step, d_bstep, m * 2, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

// host copies of everything the front-end answers: the entry points write the caller's arrays only once nothing can fail any more
struct MmHost {
  std::vector<u64> results, offsets, outputs, R;
  std::vector<uint8_t> finite, attempts;
  std::vector<uint32_t> bad_link;
  std::vector<uint16_t> bad_step;
  MmHost(size_t m, size_t n, size_t pw) : results(pw * m), offsets(pw * n), outputs(pw * n), R(pw * m), finite(m), attempts(m), bad_link(m), bad_step(m) {}
  MmOut out() { return {results.data(), offsets.data(), outputs.data(), R.data(), finite.data(), attempts.data(), bad_link.data(), bad_step.data()}; }
  void copy_to(uint64_t* res, uint8_t* fin, uint64_t* off, uint64_t* outp, uint64_t* r, uint8_t* att, uint32_t* bl, uint16_t* bs) const {
    memcpy(res, results.data(), results.size() * 8);
    memcpy(fin, finite.data(), finite.size());
    memcpy(off, offsets.data(), offsets.size() * 8);
    memcpy(outp, outputs.data(), outputs.size() * 8);
    if (r) memcpy(r, R.data(), R.size() * 8);
    if (att) memcpy(att, attempts.data(), attempts.size());
    memcpy(bl, bad_link.data(), bad_link.size() * 4);
    if (bs) memcpy(bs, bad_step.data(), bad_step.size() * 2);
  }
};

int mm_front_kind(bn254s_ctx* c, const char* tag, int kind, const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m,
                  size_t n, const uint64_t* R, const uint64_t* seed, int max_attempts, const MmOut& o) {
  return kind == 0 ? mm_front<MsmG1>(c, tag, scalars, x, seg_len, m, n, R, seed, max_attempts, o)
                   : mm_front<MsmG2>(c, tag, scalars, x, seg_len, m, n, R, seed, max_attempts, o);
}

}  // namespace

extern "C" int bn254s_msm_multi_chain(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m,
                                      size_t n, const uint64_t* R, const uint64_t* seed, int max_attempts, uint64_t* results_out,
                                      uint8_t* finite_out, uint64_t* offsets_out, uint64_t* outputs_out, uint64_t* R_out,
                                      uint8_t* attempts_out, uint32_t* bad_link_out, uint16_t* bad_step_out) {
  if (!mm_args_ok(c, "msm_multi_chain", kind, scalars, x, seg_len, m, n, R, seed, max_attempts, results_out, finite_out, offsets_out,
                  outputs_out, bad_link_out) ||
      !c)
    return BN254S_E_INVALID_ARG;
  MmHost h(m, n, kind == 0 ? 8 : 16);
  const int rc = mm_front_kind(c, "msm_multi_chain", kind, scalars, x, seg_len, m, n, R, seed, max_attempts, h.out());
  if (rc != BN254S_OK) return rc;
  h.copy_to(results_out, finite_out, offsets_out, outputs_out, R_out, attempts_out, bad_link_out, bad_step_out);
  return BN254S_OK;
}

extern "C" int bn254s_msm_multi(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                                const size_t* seg_len, size_t m, size_t n, const uint64_t* R, const uint64_t* seed, int max_attempts,
                                size_t per_proof, uint64_t* results_out, uint8_t* finite_out, uint64_t* offsets_out, uint64_t* outputs_out,
                                uint64_t* R_out, uint8_t* attempts_out, uint32_t* bad_link_out, uint16_t* bad_step_out,
                                bn254s_proof** proofs_out) {
  int rc = proven_args(c, "msm_multi", "proof",
                       mm_args_ok(c, "msm_multi", kind, scalars, x, seg_len, m, n, R, seed, max_attempts, results_out, finite_out,
                                  offsets_out, outputs_out, bad_link_out),
                       params, proofs_out, n, per_proof);
  if (rc != BN254S_OK) return rc;
  const size_t PW = kind == 0 ? 8 : 16;
  MmHost h(m, n, PW);
  rc = mm_front_kind(c, "msm_multi", kind, scalars, x, seg_len, m, n, R, seed, max_attempts, h.out());
  if (rc != BN254S_OK) return rc;
  for (size_t j = 0; j < m; j++)
    if (h.bad_link[j] != BN254S_MSM_LINK_NONE) {
      const unsigned step = h.bad_step[j];
      const std::string hit = step == BN254S_JOB_STEP_NONE ? std::string("the drawn offset is the point at infinity")
                                                           : "link " + std::to_string(h.bad_link[j]) + ", sum == -double at step " +
                                                                 std::to_string(step) + " (row " + std::to_string(2 * step) + " of its frame)";
      c->set_err("msm_multi: msm " + std::to_string(j) + " cannot be proven: " + hit +
                 (R ? std::string(" with the supplied offset")
                    : " with the offset of attempt " + std::to_string(max_attempts - 1) + ", the last of " + std::to_string(max_attempts)));
      return BN254S_E_INVALID_POINT;
    }
  std::vector<u64> proven;
  rc = prove_and_collect(c, "msm_multi", kind, params, scalars, x, h.offsets.data(), n, per_proof, proofs_out, proven);
  if (rc != BN254S_OK) return rc;
  // linkage: the trace generator computes every output bit by bit on its own; it must be the chain's, word for word
  for (size_t i = 0; i < n; i++)
    if (memcmp(proven.data() + PW * i, h.outputs.data() + PW * i, 8 * PW) != 0) {
      c->set_err("msm_multi: the proven output of job " + std::to_string(i) + " is not the chain's");
      release_proofs(proofs_out, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  h.copy_to(results_out, finite_out, offsets_out, outputs_out, R_out, attempts_out, bad_link_out, bad_step_out);
  return BN254S_OK;
}

extern "C" int bn254s_g1_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain<MsmG1>(c, scalars, x, offset, n, offsets_out, result);
}
extern "C" int bn254s_g2_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain<MsmG2>(c, scalars, x, offset, n, offsets_out, result);
}
extern "C" int bn254s_g1_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  return msm<MsmG1>(c, params, scalars, x, offset, n, per_proof, result, offsets_out, proofs);
}
extern "C" int bn254s_g2_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  return msm<MsmG2>(c, params, scalars, x, offset, n, per_proof, result, offsets_out, proofs);
}
