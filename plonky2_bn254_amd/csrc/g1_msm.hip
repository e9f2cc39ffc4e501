// g1_msm on the device: the witness chain of the reference's G1 multi-scalar multiplication (src/utils/g1_msm.rs:22-36).
//
// The reference folds
//   offset_0 = R,  offset_{i+1} = s_i x_i + offset_i  (one G1SingleGenerator::run_once per link, sequential on the CPU),
//   msm = offset_n + (-R)                              (G1Target::add, curves/g1.rs:117-150)
// and proves the n triples (s_i, x_i, offset_i) in one G1 STARK (hook.rs:63-71).  The chain is a prefix sum of points,
// offset_i = R + sum_{j<i} s_j x_j, so it is computed here in parallel:
//   1. products P_i = s_i x_i (Jacobian; s_i is any 256-bit value, P_i may be infinity), in chunks of at most MSM_CHUNK inputs:
//      the cooperative doubling chain of phase A (k_g1_dbl_chain_coop, trace_g1.hip) stores D_k = 2^k x_i, then one 256-lane
//      workgroup per input tree-reduces lane k = (bit_k ? D_k : infinity) with the complete addition law (k_g1_msm_products);
//   2. an inclusive scan over F_0 = R, F_{i+1} = P_i (n + 1 points): blocks of 256 with pt_scan256, the block totals scanned one
//      level up (as many levels as needed: three for n up to 2^24), each block's prefix added back on the way down;
//   3. affine normalisation with one batched inversion of the n + 1 Z coordinates; an infinite offset_i (i >= 1) is reported
//      with the first such index (the reference's G1Target cannot be infinity either);
//   4. msm = offset_n - R (k_g1_msm_finish, the G1 twin of k_m2g_finish): offset_n == R is an error (the result would be
//      infinity), offset_n == -R doubles (the circuit's add allows it).
// The complete addition law is used throughout, so equal partial sums double and opposite ones give infinity exactly where the
// sequential fold meets them.  Everything runs on the context's own stream and pooled buffers, like bn254s_map_to_g2.
//
// The products could also come from a fused double-and-add with one workgroup per input that stores no D_k; the doubling chain
// of phase A is used instead because it is already tuned (four lanes per input, 3 products of latency per doubling) and the
// 256-lane reduction after it is 8 additions deep, where a fused loop is 256 dependent doublings plus additions per input.
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "trace_common.h"
#include "chain_scan.h"
#include "trace_g1.h"
#include "../../include/bn254_stark.h"

namespace {

constexpr size_t MSM_CHUNK = 16384;  // inputs per product launch: 3 x 4 x NPTS words = 49 KB of D_k per input, 808 MB at most
constexpr size_t MSM_PER_PROOF_MAX = 16384;  // 2^23 rows, the largest G1 proof (bn254s_prove_batch)

// A level of the scan: n points in SoA form, coordinate c (0 = X, 1 = Y, 2 = Z), word l of element e at b[(4 c + l) cnt + e].
__device__ __forceinline__ g1j pa_load(const u64* b, size_t cnt, size_t e) {
  g1j p;
  p.x = ld_fq(b, cnt, e);
  p.y = ld_fq(b + 4 * cnt, cnt, e);
  p.z = ld_fq(b + 8 * cnt, cnt, e);
  return p;
}
__device__ __forceinline__ void pa_store(u64* b, size_t cnt, size_t e, const g1j& p) {
  st_fq(b, cnt, e, p.x);
  st_fq(b + 4 * cnt, cnt, e, p.y);
  st_fq(b + 8 * cnt, cnt, e, p.z);
}

// F_0 = R (canonical affine words -> Jacobian, Montgomery)
__global__ __launch_bounds__(64) void k_g1_msm_init(const u64* __restrict__ R, u64* __restrict__ lv, size_t cnt) {
  if (threadIdx.x != 0) return;
  g1j p;
  p.x = fq_from_canonical(R);
  p.y = fq_from_canonical(R + 4);
  p.z = fq_one();
  pa_store(lv, cnt, 0, p);
}

// One workgroup per input i of the chunk: lane k holds bit_k(s_i) ? D_k : infinity, a tree reduction leaves s_i x_i in lane 0,
// stored as F_{first + i} of level 0.  D_k at element (257 + k) m + i of px / py / pz (count NPTS m, launch_g1_dbl_chain).
__global__ __launch_bounds__(256) void k_g1_msm_products(const u64* __restrict__ scalars, int m, const u64* __restrict__ px,
                                                         const u64* __restrict__ py, const u64* __restrict__ pz,
                                                         u64* __restrict__ lv, size_t cnt, size_t first) {
  __shared__ u64 sh[12 * 256];
  const int inst = blockIdx.x, k = threadIdx.x;
  const size_t pcnt = (size_t)NPTS * m, e = (size_t)(257 + k) * m + inst;
  const bool bit = (scalars[4 * inst + (k >> 6)] >> (k & 63)) & 1;
  g1j f;
  if (bit) {
    f.x = ld_fq(px, pcnt, e);
    f.y = ld_fq(py, pcnt, e);
    f.z = ld_fq(pz, pcnt, e);
  } else {
    f = pt_infinity((const g1j*)nullptr);
  }
#pragma unroll 1
  for (int h = 128; h > 0; h >>= 1) {
    if (k >= h && k < 2 * h) lds_put(sh, k, f);
    __syncthreads();
    if (k < h) {
      g1j q;
      lds_get(sh, k + h, q);
      f = pt_add_complete(f, q);
    }
    __syncthreads();
  }
  if (k == 0) pa_store(lv, cnt, first + inst, f);
}

// Inclusive scan of each block of 256 points of a level in place; lane 255's sum is the block total, element b of the next
// level (up == nullptr at the top level, which is a single block).
__global__ __launch_bounds__(256) void k_g1_msm_scan_blocks(u64* __restrict__ lv, size_t cnt, u64* __restrict__ up, size_t up_cnt) {
  __shared__ u64 sh[12 * 256];
  const int k = threadIdx.x;
  const size_t e = (size_t)blockIdx.x * 256 + k;
  g1j f = e < cnt ? pa_load(lv, cnt, e) : pt_infinity((const g1j*)nullptr);
  pt_scan256(f, sh, k);
  if (e < cnt) pa_store(lv, cnt, e, f);
  if (up && k == 255) pa_store(up, up_cnt, blockIdx.x, f);
}

// After the level above is scanned, its element b is the sum of blocks 0..b of this level: block b + 1 adds it to its elements.
__global__ __launch_bounds__(256) void k_g1_msm_scan_add(u64* __restrict__ lv, size_t cnt, const u64* __restrict__ up, size_t up_cnt) {
  const size_t b = (size_t)blockIdx.x + 1, e = b * 256 + threadIdx.x;
  if (e >= cnt) return;
  const g1j pre = pa_load(up, up_cnt, b - 1), f = pa_load(lv, cnt, e);
  pa_store(lv, cnt, e, pt_add_complete(pre, f));
}

// offsets_i in canonical affine words (out[8 i ..]); zi = the batched inverses of the Z words of level 0.  An infinite offset
// writes nothing and lowers *inf_idx to its index.
__global__ __launch_bounds__(64) void k_g1_msm_affine(const u64* __restrict__ lv, size_t cnt, const u64* __restrict__ zi,
                                                      u64* __restrict__ out, unsigned* __restrict__ inf_idx) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cnt) return;
  if (fq_is_zero(ld_fq(lv + 8 * cnt, cnt, e))) {
    atomicMin(inf_idx, (unsigned)e);
    return;
  }
  const fq z = ld_fq(zi, cnt, e), z2 = fq_sqr(z);
  const fqw x = fq_to_canonical(fq_mul(ld_fq(lv, cnt, e), z2));
  const fqw y = fq_to_canonical(fq_mul(fq_mul(ld_fq(lv + 4 * cnt, cnt, e), z2), z));
#pragma unroll
  for (int l = 0; l < 4; l++) {
    out[8 * e + l] = x.l[l];
    out[8 * e + 4 + l] = y.l[l];
  }
}

// result = offset_n - R (affine; offset_n == -R doubles, offset_n == R is reported).  Nothing to do after an infinite offset.
__global__ __launch_bounds__(64) void k_g1_msm_finish(const u64* __restrict__ o, const u64* __restrict__ R, u64* __restrict__ res,
                                                      int* __restrict__ err, const unsigned* __restrict__ inf_idx) {
  if (threadIdx.x != 0 || *inf_idx != UINT_MAX) return;
  bool same_x = true, same_y = true;
  for (int l = 0; l < 4; l++) {
    same_x &= o[l] == R[l];
    same_y &= o[4 + l] == R[4 + l];
  }
  if (same_x && same_y) {
    *err = BN254S_E_INVALID_POINT;
    return;
  }
  const fq x1 = fq_from_canonical(o), y1 = fq_from_canonical(o + 4);
  const fq x2 = fq_from_canonical(R), y2 = fq_neg(fq_from_canonical(R + 4));
  fq lam;
  if (same_x) {  // o == -R: the tangent at o (y1 != 0: G1 has odd order)
    const fq x1s = fq_sqr(x1);
    lam = fq_mul(fq_add(fq_add(x1s, x1s), x1s), fq_inv(fq_add(y1, y1)));
  } else {
    lam = fq_mul(fq_sub(y2, y1), fq_inv(fq_sub(x2, x1)));
  }
  const fq x3 = fq_sub(fq_sub(fq_sqr(lam), x1), x2);
  const fq y3 = fq_sub(fq_mul(lam, fq_sub(x1, x3)), y1);
  const fqw cx = fq_to_canonical(x3), cy = fq_to_canonical(y3);
  for (int l = 0; l < 4; l++) {
    res[l] = cx.l[l];
    res[4 + l] = cy.l[l];
  }
}

// the arguments other than the context (n < 2^32: the first infinite index travels as a 32-bit word)
bool msm_args_ok(const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n) {
  return scalars && x && offset && n > 0 && n < (size_t)UINT_MAX;
}

// The chain into host memory: offs[(n + 1) x 8], res[8].
int msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* R, size_t n, uint64_t* offs, uint64_t* res) {
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // levels of the scan: level 0 = the n + 1 points F, level l + 1 = the block totals of level l, until one block remains
  std::vector<size_t> cnt{n + 1}, at{0};
  size_t lv_words = 12 * (n + 1);
  while (cnt.back() > 256) {
    cnt.push_back((cnt.back() + 255) / 256);
    at.push_back(lv_words);
    lv_words += 12 * cnt.back();
  }
  const size_t m_max = n < MSM_CHUNK ? n : MSM_CHUNK, pcnt = (size_t)NPTS * m_max;
  u64* d = c->words("msm", 4 * n /* s */ + 8 * n /* x */ + 8 /* R */ + lv_words + 4 * (n + 1) /* zi */ + 8 * (n + 1) /* out */ +
                               8 /* result */ + 2 /* err, inf_idx */);
  u64* d_pts = c->words("msm.pts", 3 * 4 * pcnt);
  if (!d || !d_pts) return BN254S_E_OOM;
  u64* d_s = d;
  u64* d_x = d_s + 4 * n;
  u64* d_R = d_x + 8 * n;
  u64* d_lv = d_R + 8;
  u64* d_zi = d_lv + lv_words;
  u64* d_out = d_zi + 4 * (n + 1);
  u64* d_res = d_out + 8 * (n + 1);
  int* d_err = (int*)(d_res + 8);
  unsigned* d_inf = (unsigned*)(d_err + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 4, st));
  HIP_TRY(c, hipMemsetAsync(d_inf, 0xFF, 4, st));
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * 64, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_R, R, 64, hipMemcpyHostToDevice, st));
  k_g1_msm_init<<<1, 64, 0, st>>>(d_R, d_lv, cnt[0]);
  u64 *px = d_pts, *py = px + 4 * pcnt, *pz = py + 4 * pcnt;
  for (size_t base = 0; base < n; base += MSM_CHUNK) {
    const int m = (int)(n - base < MSM_CHUNK ? n - base : MSM_CHUNK);
    launch_g1_dbl_chain(d_x + 8 * base, m, px, py, pz, st);
    k_g1_msm_products<<<(unsigned)m, 256, 0, st>>>(d_s + 4 * base, m, px, py, pz, d_lv, cnt[0], base + 1);
  }
  const size_t top = cnt.size() - 1;
  for (size_t l = 0; l <= top; l++)
    k_g1_msm_scan_blocks<<<(unsigned)((cnt[l] + 255) / 256), 256, 0, st>>>(d_lv + at[l], cnt[l], l < top ? d_lv + at[l + 1] : nullptr,
                                                                         l < top ? cnt[l + 1] : 0);
  for (size_t l = top; l-- > 0;)
    k_g1_msm_scan_add<<<(unsigned)((cnt[l] + 255) / 256 - 1), 256, 0, st>>>(d_lv + at[l], cnt[l], d_lv + at[l + 1], cnt[l + 1]);
  launch_fq_batch_inv(d_lv + 8 * cnt[0], d_zi, cnt[0], st);
  k_g1_msm_affine<<<(unsigned)((cnt[0] + 63) / 64), 64, 0, st>>>(d_lv, cnt[0], d_zi, d_out, d_inf);
  k_g1_msm_finish<<<1, 64, 0, st>>>(d_out + 8 * n, d_R, d_res, d_err, d_inf);
  HIP_TRY(c, hipGetLastError());
  int h_err[2];
  HIP_TRY(c, hipMemcpyAsync(offs, d_out, (n + 1) * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(res, d_res, 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h_err, d_err, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const unsigned inf = (unsigned)h_err[1];
  if (inf != UINT_MAX) {
    c->set_err("g1_msm: offset_" + std::to_string(inf) + " = R + s_0 x_0 + ... + s_" + std::to_string(inf - 1) + " x_" +
               std::to_string(inf - 1) + " is the point at infinity");
    return BN254S_E_INVALID_POINT;
  }
  if (h_err[0]) {
    c->set_err("g1_msm: offset_n equals R, the result is the point at infinity");
    return h_err[0];
  }
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g1_msm_chain(bn254s_ctx* c, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                                   uint64_t* offsets_out, uint64_t* result) {
  if (!c || !msm_args_ok(scalars, x, offset, n) || !offsets_out || !result) return BN254S_E_INVALID_ARG;
  return msm_chain(c, scalars, x, offset, n, offsets_out, result);
}

extern "C" int bn254s_g1_msm(bn254s_ctx* c, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                             bn254s_proof** proofs) {
  // every check before device work; the context last, so that the shape checks can be exercised without one
  if (!msm_args_ok(scalars, x, offset, n) || !params || !result || !proofs || per_proof == 0 ||
      params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  const size_t n_proofs = (n + per_proof - 1) / per_proof;
  for (size_t i = 0; i < n_proofs; i++) proofs[i] = nullptr;
  if (per_proof > MSM_PER_PROOF_MAX) {
    if (c) c->set_err("g1_msm: per_proof above 16384 (2^23 rows, the largest G1 proof)");
    return BN254S_E_UNSUPPORTED;
  }
  if (!c) return BN254S_E_INVALID_ARG;
  std::vector<u64> offs(8 * (n + 1));
  int rc = msm_chain(c, scalars, x, offset, n, offs.data(), result);
  if (rc != BN254S_OK) return rc;
  rc = bn254s_prove_batch(c, 0, params, scalars, x, offs.data(), n, per_proof, proofs);
  if (rc != BN254S_OK) return rc;  // (the batch has freed its proofs)
  // linkage: the trace generator computes s_i x_i + offset_i on its own; it must land on offset_{i+1}
  size_t pos = 0;
  for (size_t i = 0; i < n_proofs && rc == BN254S_OK; i++) {
    const uint64_t* o;
    size_t len;
    const size_t cnt = n - pos < per_proof ? n - pos : per_proof;
    if (bn254s_proof_outputs(proofs[i], &o, &len) != BN254S_OK || len != 8 * cnt) {
      c->set_err("g1_msm: proof " + std::to_string(i) + " has " + std::to_string(len / 8) + " outputs, expected " + std::to_string(cnt));
      rc = BN254S_E_INTERNAL;
    } else if (memcmp(o, offs.data() + 8 * (pos + 1), len * 8) != 0) {
      size_t j = 0;
      while (memcmp(o + 8 * j, offs.data() + 8 * (pos + 1 + j), 64) == 0) j++;
      c->set_err("g1_msm: output " + std::to_string(pos + j) + " of the proofs differs from offset_" + std::to_string(pos + j + 1) +
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
