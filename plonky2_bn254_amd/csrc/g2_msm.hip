// g2_msm on the device: the G2 twin of g1_msm.hip, the witness chain of a G2 multi-scalar multiplication written like the
// reference's src/utils/g1_msm.rs:22-36 with the G2 gadgets (G2Target::new_checked, set_random_g2, g2_scalar_mul, G2Target::neg
// and G2Target::add, curves/g2.rs:93-150).  The reference ships these pieces but no g2_msm of its own.
//
//   offset_0 = R,  offset_{i+1} = s_i x_i + offset_i  (one g2_scalar_mul job per link),
//   msm = offset_n + (-R)                              (G2Target::add: a doubling is allowed, infinity is not)
//
// The chain is a prefix sum of points, offset_i = R + sum_{j<i} s_j x_j, computed in the same four steps as g1_msm.hip:
//   1. products P_i = s_i x_i (Jacobian), in chunks of at most MSM_CHUNK inputs: the cooperative G2 doubling chain of trace
//      phase A (k_g2_dbl_chain_coop, trace_g2fq.hip) stores D_k = 2^k x_i, then one 256-lane workgroup per input tree-reduces
//      lane k = (bit_k ? D_k : infinity) with the complete addition law (k_g2_msm_products).  s_i is used as the full 256-bit
//      value, never reduced mod r: a point on the twist need not lie in the r-torsion subgroup (map_to_g2 proves such points
//      before cofactor clearing), and the G2 trace computes s_i x_i bit by bit, so the chain must do the same;
//   2. an inclusive scan over F_0 = R, F_{i+1} = P_i (n + 1 points): blocks of 256 with pt_scan256, the block totals scanned one
//      level up (three levels for n up to 2^24), each block's prefix added back on the way down;
//   3. affine normalisation: the norms of the n + 1 Z coordinates, one batched inversion of the norms, then Z^-1 from the
//      inverse norm (fq2_inv_from_norm_inv); an infinite offset_i (i >= 1) is reported with the first such index;
//   4. msm = offset_n - R (k_g2_msm_finish): offset_n == R is an error (the result would be infinity), offset_n == -R doubles.
// Everything runs on the context's own stream and pooled buffers ("g2msm", "g2msm.pts"), like bn254s_g1_msm_chain.
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "trace_common.h"
#include "chain_scan.h"
#include "trace_g2fq.h"
#include "../../include/bn254_stark.h"

namespace {

// inputs per product launch: D_k (3 x 2 x 4 x NPTS words) and the chain's znorm (4 x NPTS words) are 28 x 514 x 8 B = 115 KB per
// input, 943 MB for a chunk of 8192
constexpr size_t MSM_CHUNK = 8192;
constexpr size_t MSM_PER_PROOF_MAX = 16384;  // 2^23 rows, the largest G2 proof (streaming workspace of bn254s_prove_batch)

// A level of the scan: cnt points in SoA form, component c (0..5 = X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1), word l of element e at
// b[(4 c + l) cnt + e].  The doubling chain's arrays have the same layout (launch_g2_dbl_chain).
__device__ __forceinline__ fq2 ld_f2(const u64* b, size_t cnt, size_t e) {
  fq2 r;
  r.c0 = ld_fq(b, cnt, e);
  r.c1 = ld_fq(b + 4 * cnt, cnt, e);
  return r;
}
__device__ __forceinline__ void st_f2(u64* b, size_t cnt, size_t e, const fq2& v) {
  st_fq(b, cnt, e, v.c0);
  st_fq(b + 4 * cnt, cnt, e, v.c1);
}
__device__ __forceinline__ g2j pa_load(const u64* b, size_t cnt, size_t e) {
  g2j p;
  p.x = ld_f2(b, cnt, e);
  p.y = ld_f2(b + 8 * cnt, cnt, e);
  p.z = ld_f2(b + 16 * cnt, cnt, e);
  return p;
}
__device__ __forceinline__ void pa_store(u64* b, size_t cnt, size_t e, const g2j& p) {
  st_f2(b, cnt, e, p.x);
  st_f2(b + 8 * cnt, cnt, e, p.y);
  st_f2(b + 16 * cnt, cnt, e, p.z);
}
__device__ __forceinline__ fq2 f2_from_canonical(const u64* w) {
  fq2 r;
  r.c0 = fq_from_canonical(w);
  r.c1 = fq_from_canonical(w + 4);
  return r;
}
__device__ __forceinline__ void f2_to_canonical(u64* w, const fq2& a) {
  const fqw c0 = fq_to_canonical(a.c0), c1 = fq_to_canonical(a.c1);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    w[l] = c0.l[l];
    w[4 + l] = c1.l[l];
  }
}

// F_0 = R (canonical affine words -> Jacobian, Montgomery)
__global__ __launch_bounds__(64) void k_g2_msm_init(const u64* __restrict__ R, u64* __restrict__ lv, size_t cnt) {
  if (threadIdx.x != 0) return;
  g2j p;
  p.x = f2_from_canonical(R);
  p.y = f2_from_canonical(R + 8);
  p.z = fq2_one();
  pa_store(lv, cnt, 0, p);
}

// One workgroup per input i of the chunk: lane k holds bit_k(s_i) ? D_k : infinity, a tree reduction leaves s_i x_i in lane 0,
// stored as F_{first + i} of level 0.  D_k at element (257 + k) m + i of pts (count NPTS m, launch_g2_dbl_chain).
__global__ __launch_bounds__(256) void k_g2_msm_products(const u64* __restrict__ scalars, int m, const u64* __restrict__ pts,
                                                         u64* __restrict__ lv, size_t cnt, size_t first) {
  __shared__ u64 sh[24 * 256];
  const int inst = blockIdx.x, k = threadIdx.x;
  const size_t pcnt = (size_t)NPTS * m, e = (size_t)(257 + k) * m + inst;
  const bool bit = (scalars[4 * inst + (k >> 6)] >> (k & 63)) & 1;
  g2j f = bit ? pa_load(pts, pcnt, e) : pt_infinity((const g2j*)nullptr);
#pragma unroll 1
  for (int h = 128; h > 0; h >>= 1) {
    if (k >= h && k < 2 * h) lds_put(sh, k, f);
    __syncthreads();
    if (k < h) {
      g2j q;
      lds_get(sh, k + h, q);
      f = pt_add_complete(f, q);
    }
    __syncthreads();
  }
  if (k == 0) pa_store(lv, cnt, first + inst, f);
}

// Inclusive scan of each block of 256 points of a level in place; lane 255's sum is the block total, element b of the next
// level (up == nullptr at the top level, which is a single block).
__global__ __launch_bounds__(256) void k_g2_msm_scan_blocks(u64* __restrict__ lv, size_t cnt, u64* __restrict__ up, size_t up_cnt) {
  __shared__ u64 sh[24 * 256];
  const int k = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * 256 + k;
  g2j f = e < cnt ? pa_load(lv, cnt, e) : pt_infinity((const g2j*)nullptr);
  pt_scan256(f, sh, k);
  if (e < cnt) pa_store(lv, cnt, e, f);
  if (up && k == 255) pa_store(up, up_cnt, blockIdx.x, f);
}

// After the level above is scanned, its element b is the sum of blocks 0..b of this level: block b + 1 adds it to its elements.
__global__ __launch_bounds__(256) void k_g2_msm_scan_add(u64* __restrict__ lv, size_t cnt, const u64* __restrict__ up, size_t up_cnt) {
  const size_t b = (size_t)blockIdx.x + 1, e = b * 256 + threadIdx.x;
  if (e >= cnt) return;
  const g2j pre = pa_load(up, up_cnt, b - 1), f = pa_load(lv, cnt, e);
  pa_store(lv, cnt, e, pt_add_complete(pre, f));
}

// zn[e] = norm(Z_e) of level 0 (zero exactly when offset_e is infinity), the input of the batched inversion
__global__ __launch_bounds__(64) void k_g2_msm_norms(const u64* __restrict__ lv, size_t cnt, u64* __restrict__ zn) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  st_fq(zn, cnt, e, fq2_norm(ld_f2(lv + 16 * cnt, cnt, e)));
}

// offsets_i in canonical affine words (out[16 i ..]); zni = the batched inverses of the norms.  An infinite offset writes nothing
// and lowers *inf_idx to its index.
__global__ __launch_bounds__(64) void k_g2_msm_affine(const u64* __restrict__ lv, size_t cnt, const u64* __restrict__ zni,
                                                      u64* __restrict__ out, unsigned* __restrict__ inf_idx) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  const fq2 z = ld_f2(lv + 16 * cnt, cnt, e);
  if (fq2_is_zero(z)) {
    atomicMin(inf_idx, (unsigned)e);
    return;
  }
  const fq2 zi = fq2_inv_from_norm_inv(z, ld_fq(zni, cnt, e)), z2 = fq2_sqr(zi);
  f2_to_canonical(out + 16 * e, fq2_mul(ld_f2(lv, cnt, e), z2));
  f2_to_canonical(out + 16 * e + 8, fq2_mul(fq2_mul(ld_f2(lv + 8 * cnt, cnt, e), z2), zi));
}

// result = offset_n - R (affine; offset_n == -R doubles, offset_n == R is reported).  Nothing to do after an infinite offset.
// The doubling needs y1 != 0, i.e. offset_n is not a point of order 2: #E'(Fq2) = r (2p - r) is odd, so the twist has no point
// of order 2, whether or not offset_n lies in the r-torsion subgroup.
__global__ __launch_bounds__(64) void k_g2_msm_finish(const u64* __restrict__ o, const u64* __restrict__ R, u64* __restrict__ res,
                                                      int* __restrict__ err, const unsigned* __restrict__ inf_idx) {
  if (threadIdx.x != 0 || *inf_idx != UINT_MAX) return;
  bool same_x = true, same_y = true;
  for (int l = 0; l < 8; l++) {
    same_x &= o[l] == R[l];
    same_y &= o[8 + l] == R[8 + l];
  }
  if (same_x && same_y) {
    *err = BN254S_E_INVALID_POINT;
    return;
  }
  const fq2 x1 = f2_from_canonical(o), y1 = f2_from_canonical(o + 8);
  const fq2 x2 = f2_from_canonical(R), y2 = fq2_sub(fq2_zero(), f2_from_canonical(R + 8));
  fq2 num, den;
  if (same_x) {  // o == -R: the tangent at o
    const fq2 x1s = fq2_sqr(x1);
    num = fq2_add(fq2_add(x1s, x1s), x1s);
    den = fq2_dbl(y1);
  } else {
    num = fq2_sub(y2, y1);
    den = fq2_sub(x2, x1);
  }
  const fq2 lam = fq2_mul(num, fq2_inv_from_norm_inv(den, fq_inv(fq2_norm(den))));
  const fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), x1), x2);
  const fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(x1, x3)), y1);
  f2_to_canonical(res, x3);
  f2_to_canonical(res + 8, y3);
}

// the arguments other than the context (n < 2^32: the first infinite index travels as a 32-bit word)
bool msm_args_ok(const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n) {
  return scalars && x && offset && n > 0 && n < (size_t)UINT_MAX;
}

// The chain into host memory: offs[(n + 1) x 16], res[16].
int msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* R, size_t n, uint64_t* offs, uint64_t* res) {
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // levels of the scan: level 0 = the n + 1 points F, level l + 1 = the block totals of level l, until one block remains
  std::vector<size_t> cnt{n + 1}, at{0};
  size_t lv_words = 24 * (n + 1);
  while (cnt.back() > 256) {
    cnt.push_back((cnt.back() + 255) / 256);
    at.push_back(lv_words);
    lv_words += 24 * cnt.back();
  }
  const size_t m_max = n < MSM_CHUNK ? n : MSM_CHUNK, pcnt = (size_t)NPTS * m_max;
  u64* d = c->words("g2msm", 4 * n /* s */ + 16 * n /* x */ + 16 /* R */ + lv_words + 2 * 4 * (n + 1) /* zn, zni */ +
                                 16 * (n + 1) /* out */ + 16 /* result */ + 2 /* err, inf_idx */);
  u64* d_pts = c->words("g2msm.pts", 6 * 4 * pcnt /* D_k */ + 4 * pcnt /* znorm */);
  if (!d || !d_pts) return BN254S_E_OOM;
  u64* d_s = d;
  u64* d_x = d_s + 4 * n;
  u64* d_R = d_x + 16 * n;
  u64* d_lv = d_R + 16;
  u64* d_zn = d_lv + lv_words;
  u64* d_zi = d_zn + 4 * (n + 1);
  u64* d_out = d_zi + 4 * (n + 1);
  u64* d_res = d_out + 16 * (n + 1);
  int* d_err = (int*)(d_res + 16);
  unsigned* d_inf = (unsigned*)(d_err + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, st));
  HIP_TRY(c, hipMemsetAsync(d_inf, 0xFF, 4, st));
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * 128, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_R, R, 128, hipMemcpyHostToDevice, st));
  k_g2_msm_init<<<1, 64, 0, st>>>(d_R, d_lv, cnt[0]);
  for (size_t base = 0; base < n; base += MSM_CHUNK) {
    const int m = (int)(n - base < MSM_CHUNK ? n - base : MSM_CHUNK);
    launch_g2_dbl_chain(d_x + 16 * base, m, d_pts, d_pts + 6 * 4 * pcnt, st);
    k_g2_msm_products<<<(unsigned)m, 256, 0, st>>>(d_s + 4 * base, m, d_pts, d_lv, cnt[0], base + 1);
  }
  const size_t top = cnt.size() - 1;
  for (size_t l = 0; l <= top; l++)
    k_g2_msm_scan_blocks<<<(unsigned)((cnt[l] + 255) / 256), 256, 0, st>>>(d_lv + at[l], cnt[l], l < top ? d_lv + at[l + 1] : nullptr,
                                                                         l < top ? cnt[l + 1] : 0);
  for (size_t l = top; l-- > 0;)
    k_g2_msm_scan_add<<<(unsigned)((cnt[l] + 255) / 256 - 1), 256, 0, st>>>(d_lv + at[l], cnt[l], d_lv + at[l + 1], cnt[l + 1]);
  const unsigned g0 = (unsigned)((cnt[0] + 63) / 64);
  k_g2_msm_norms<<<g0, 64, 0, st>>>(d_lv, cnt[0], d_zn);
  launch_fq_batch_inv(d_zn, d_zi, cnt[0], st);
  k_g2_msm_affine<<<g0, 64, 0, st>>>(d_lv, cnt[0], d_zi, d_out, d_inf);
  k_g2_msm_finish<<<1, 64, 0, st>>>(d_out + 16 * n, d_R, d_res, d_err, d_inf);
  HIP_TRY(c, hipGetLastError());
  int h_err[2];
  HIP_TRY(c, hipMemcpyAsync(offs, d_out, (n + 1) * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(res, d_res, 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_err, d_err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const unsigned inf = (unsigned)h_err[1];
  if (inf != UINT_MAX) {
    c->set_err("g2_msm: offset_" + std::to_string(inf) + " = R + s_0 x_0 + ... + s_" + std::to_string(inf - 1) + " x_" +
               std::to_string(inf - 1) + " is the point at infinity");
    return BN254S_E_INVALID_POINT;
  }
  if (h_err[0]) {
    c->set_err("g2_msm: offset_n equals R, the result is the point at infinity");
    return h_err[0];
  }
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g2_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain(c, scalars, x, offset, n, offsets_out, result);
}

extern "C" int bn254s_g2_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  // every check before device work; the context last, so that the shape checks can be exercised without one
  if (!msm_args_ok(scalars, x, offset, n) || !params || !result || !proofs || per_proof == 0 ||
      params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  const size_t n_proofs = (n + per_proof - 1) / per_proof;
  for (size_t i = 0; i < n_proofs; i++) proofs[i] = nullptr;
  if (per_proof > MSM_PER_PROOF_MAX) {
    if (c) c->set_err("g2_msm: per_proof above 16384 (2^23 rows, the largest G2 proof)");
    return BN254S_E_UNSUPPORTED;
  }
  if (!c) return BN254S_E_INVALID_ARG;
  std::vector<u64> offs(16 * (n + 1));
  int rc = msm_chain(c, scalars, x, offset, n, offs.data(), result);
  if (rc != BN254S_OK) return rc;
  rc = bn254s_prove_batch(c, 1, params, scalars, x, offs.data(), n, per_proof, proofs);
  if (rc != BN254S_OK) return rc;  // (the batch has freed its proofs)
  // linkage: the trace generator computes s_i x_i + offset_i on its own; it must land on offset_{i+1}
  size_t pos = 0;
  for (size_t i = 0; i < n_proofs && rc == BN254S_OK; i++) {
    const uint64_t* o;
    size_t len;
    const size_t cnt = n - pos < per_proof ? n - pos : per_proof;
    if (bn254s_proof_outputs(proofs[i], &o, &len) != BN254S_OK || len != 16 * cnt) {
      c->set_err("g2_msm: proof " + std::to_string(i) + " has " + std::to_string(len / 16) + " outputs, expected " +
                 std::to_string(cnt));
      rc = BN254S_E_INTERNAL;
    } else if (memcmp(o, offs.data() + 16 * (pos + 1), len * 8) != 0) {
      size_t j = 0;
      while (memcmp(o + 16 * j, offs.data() + 16 * (pos + 1 + j), 128) == 0) j++;
      c->set_err("g2_msm: output " + std::to_string(pos + j) + " of the proofs differs from offset_" + std::to_string(pos + j + 1) +
                 " of the chain");
      rc = BN254S_E_INTERNAL;
    }
    pos += cnt;
  }
  if (rc != BN254S_OK) {
    for (size_t i = 0; i < n_proofs; i++) {
      bn254s_proof_free(proofs[i]);
      proofs[i] = nullptr;
    }
    return rc;
  }
  if (offsets_out) memcpy(offsets_out, offs.data(), offs.size() * 8);
  return BN254S_OK;
}
