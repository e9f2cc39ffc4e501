// map_to_g2 on the device: the front-end of BASELINE config 5.
//
// Replaces the witness arithmetic of the reference's `map_to_g2` / `map_to_g2_circuit` (src/utils/hash_to_g2.rs:113-148,
// 150-207: Shallue-van de Woestijne map with Z = 1, RFC 9380 6.6.1) around its two STARK job kinds:
//   k_m2g_candidates: x1, x2, x3 and the 2n Legendre jobs  norm(g(x_i))^((p-1)/2)   (is_square, fields/fq2.rs:235-240)
//   [2n fq_exp proofs]
//   k_m2g_select:     x = first candidate with a square g(x), y = sqrt(g(x)) with sgn(y) = sgn(u)  (hash_to_g2.rs:128-145)
//   [n G2 proofs of cofactor * (x, y) + offset]
//   k_m2g_finish:     output - offset                                                (hash_to_g2.rs:200-205)
// Square roots follow ark-ff 0.4 (Fq: a^((p+1)/4); Fq2: the "complex method" of QuadExtField::sqrt), like the Python
// front-end tools/map_to_g2_ref.py, which is the parity reference of tests/test_map_to_g2.py.
// The same map without the proofs, the reference's native map_to_g2 / hash_to_g2 (bn254s_map_to_g2_batch, bn254s_hash_to_g2_batch):
//   [k_hash_to_fq2]
//   k_m2g_point:          the candidates, the two "is a square" flags and the signed root from the ladders of fq2_root.h
//   k_g2_clear_cofactor:  [h](x, y) by the endomorphism form (g2_cofactor.hip)
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "fq_dev.h"
#include "fq2_root.h"
#include "g2_cofactor.h"
#include "hash_to_fq.h"
#include "job_device.h"
#include "proven_jobs.h"
#include "transcript.h"
#include "../../include/bn254_stark.h"
#include "map_to_g2_constants.inc"

namespace {

struct M2GConsts {
  u64 b2[8], gz[8], nz2[8], tv4[8], tv6[8], leg[4], sq[4], two_inv[4], cof[4];
};
M2GConsts host_consts() {
  M2GConsts c;
  memcpy(c.b2, M2G_B2, 64);
  memcpy(c.gz, M2G_GZ, 64);
  memcpy(c.nz2, M2G_NEG_Z_BY_2, 64);
  memcpy(c.tv4, M2G_TV4, 64);
  memcpy(c.tv6, M2G_TV6, 64);
  memcpy(c.leg, M2G_LEGENDRE_EXP, 32);
  memcpy(c.sq, M2G_SQRT_EXP, 32);
  memcpy(c.two_inv, M2G_TWO_INV, 32);
  memcpy(c.cof, M2G_COFACTOR, 32);
  return c;
}

__device__ __noinline__ fq fq_pow_words(const fq& a, const u64* e) {  // a^e, e < 2^256
  fq r = fq_one();
  for (int i = 255; i >= 0; i--) {
    r = fq_sqr(r);
    if ((e[i >> 6] >> (i & 63)) & 1) r = fq_mul(r, a);
  }
  return r;
}
__device__ __forceinline__ fq2 g_rhs(const fq2& x, const fq2& b2) { return fq2_add(fq2_mul(fq2_sqr(x), x), b2); }
__device__ __forceinline__ bool fq_is_square(const fq& a, const M2GConsts& C) {
  return fq_is_zero(a) || fq_eq(fq_pow_words(a, C.leg), fq_one());
}
// src/fields/sgn.rs:20-27 (sgn_words of fq2_root.h, on the canonical words)
__device__ __forceinline__ bool f2_sgn(const fq2& a) { return sgn_words(fq_to_canonical(a.c0), fq_to_canonical(a.c1)); }
// QuadExtField::sqrt of ark-ff 0.4 for a square a; *ok = false if the candidate does not square back
__device__ __noinline__ fq2 f2_sqrt(const fq2& a, const M2GConsts& C, bool* ok) {
  fq2 r;
  if (fq_is_zero(a.c1)) {
    if (fq_is_square(a.c0, C)) {
      r.c0 = fq_pow_words(a.c0, C.sq);
      r.c1 = fq_zero();
    } else {
      r.c0 = fq_zero();
      r.c1 = fq_pow_words(fq_neg(a.c0), C.sq);
    }
  } else {
    const fq two_inv = fq_from_canonical(C.two_inv);
    const fq alpha = fq_pow_words(fq2_norm(a), C.sq);
    fq delta = fq_mul(fq_add(alpha, a.c0), two_inv);
    if (!fq_is_square(delta, C)) delta = fq_sub(delta, alpha);
    r.c0 = fq_pow_words(delta, C.sq);
    r.c1 = fq_mul(fq_mul(a.c1, two_inv), fq_inv(r.c0));
  }
  *ok = fq2_eq(fq2_sqr(r), a);
  return r;
}

// x1, x2, x3 of hash_to_g2.rs:119-127 for one input u: shared by the proven pipeline (k_m2g_candidates) and the proof-free one
// (k_m2g_point), so that the two cannot diverge - also not where tv1 tv2 = 0, whose inverse both take as fq2_inv gives it.
__device__ __forceinline__ void m2g_candidates(const fq2& uu, const M2GConsts& C, fq2& x1, fq2& x2, fq2& x3) {
  const fq2 gz = fq2_from_canonical(C.gz);
  fq2 tv1 = fq2_mul(fq2_sqr(uu), gz);
  const fq2 tv2 = fq2_add(fq2_one(), tv1);
  tv1 = fq2_sub(fq2_one(), tv1);
  const fq2 tv3 = fq2_inv(fq2_mul(tv1, tv2));
  const fq2 tv5 = fq2_mul(fq2_mul(fq2_mul(uu, tv1), tv3), fq2_from_canonical(C.tv4));
  const fq2 nz2 = fq2_from_canonical(C.nz2);
  x1 = fq2_sub(nz2, tv5);
  x2 = fq2_add(nz2, tv5);
  const fq2 t = fq2_mul(fq2_sqr(tv2), tv3);
  x3 = fq2_add(fq2_one(), fq2_mul(fq2_from_canonical(C.tv6), fq2_sqr(t)));
}

// cand: 3 x 8 words per input (x1, x2, x3 canonical); fq_s / fq_x: the 2n fq_exp jobs
__global__ __launch_bounds__(64) void k_m2g_candidates(const u64* __restrict__ u, size_t n, M2GConsts C, u64* __restrict__ cand,
                                                       u64* __restrict__ fq_s, u64* __restrict__ fq_x) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const fq2 b2 = fq2_from_canonical(C.b2);
  fq2 x[3];
  m2g_candidates(fq2_from_canonical(u + 8 * k), C, x[0], x[1], x[2]);
#pragma unroll 1
  for (int i = 0; i < 3; i++) fq2_store_canonical(cand + (3 * k + i) * 8, x[i]);
#pragma unroll 1
  for (int i = 0; i < 2; i++) {
    const fqw nrm = fq_to_canonical(fq2_norm(g_rhs(x[i], b2)));
    for (int w = 0; w < 4; w++) {
      fq_x[(2 * k + i) * 4 + w] = nrm.l[w];
      fq_s[(2 * k + i) * 4 + w] = C.leg[w];
    }
  }
}

// legendre: the 2n fq_exp outputs (canonical words); g2_s / g2_x: the n cofactor-clearing jobs
__global__ __launch_bounds__(64) void k_m2g_select(const u64* __restrict__ u, const u64* __restrict__ cand,
                                                   const u64* __restrict__ legendre, size_t n, M2GConsts C, u64* __restrict__ g2_s,
                                                   u64* __restrict__ g2_x, int* __restrict__ err) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  auto is_one = [&](const u64* w) { return w[0] == 1 && (w[1] | w[2] | w[3]) == 0; };
  const int pick = is_one(legendre + (2 * k) * 4) ? 0 : is_one(legendre + (2 * k + 1) * 4) ? 1 : 2;
  const fq2 x = fq2_from_canonical(cand + (3 * k + pick) * 8);
  bool ok;
  fq2 y = f2_sqrt(g_rhs(x, fq2_from_canonical(C.b2)), C, &ok);
  if (!ok) atomicCAS(err, 0, BN254S_E_INTERNAL);  // g(x) is not a square: inconsistent Legendre results
  if (f2_sgn(fq2_from_canonical(u + 8 * k)) != f2_sgn(y)) y = fq2_neg(y);
  for (int w = 0; w < 8; w++) g2_x[16 * k + w] = cand[(3 * k + pick) * 8 + w];
  fq2_store_canonical(g2_x + 16 * k + 8, y);
  for (int w = 0; w < 4; w++) g2_s[4 * k + w] = C.cof[w];
}

// out = o - off (affine; o != +-off for a random offset: reported otherwise)
__global__ __launch_bounds__(64) void k_m2g_finish(const u64* __restrict__ o, const u64* __restrict__ off, size_t n, u64* __restrict__ out,
                                                   int* __restrict__ err) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const fq2 x1 = fq2_from_canonical(o + 16 * k), y1 = fq2_from_canonical(o + 16 * k + 8);
  const fq2 x2 = fq2_from_canonical(off + 16 * k), y2 = fq2_neg(fq2_from_canonical(off + 16 * k + 8));
  const fq2 dx = fq2_sub(x2, x1);
  if (fq2_is_zero(dx)) {
    atomicCAS(err, 0, BN254S_E_INVALID_POINT);
    return;
  }
  const fq2 lam = fq2_mul(fq2_sub(y2, y1), fq2_inv(dx));
  const fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), x1), x2);
  const fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(x1, x3)), y1);
  fq2_store_canonical(out + 16 * k, x3);
  fq2_store_canonical(out + 16 * k + 8, y3);
}

// The point (x, y) of hash_to_g2.rs:119-145 without the proven Legendre symbols: the candidates, "g(x1) is a square" and "g(x2) is
// a square" from the norm's exponentiation as G2 recovery decides its flag (fq2_root.h), the choice of x, and y = sqrt(g(x)) with
// sgn(y) = sgn(u).  The two roots +-y have opposite signs under sgn.rs:20-27, so any root followed by the sign fix is the
// reference's y.  Every lane runs the three norm ladders and one root ladder, so that a wave stays together.
// points: n x 16 canonical words; *err: BN254S_E_INTERNAL if g of the chosen x is no square or a root does not square back.
__global__ __launch_bounds__(G1R_LANES) void k_m2g_point(const u64* __restrict__ u, size_t n, M2GConsts C, u64* __restrict__ points,
                                                         int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq2 uu = fq2_from_canonical(u + 8 * k), b2 = fq2_from_canonical(C.b2);
  fq2 x1, x2, x3;
  m2g_candidates(uu, C, x1, x2, x3);
  // from x3 down to x1, so that the first candidate with a square g(x) is the one that stays
  fq2 x = x3, g = g_rhs(x3, b2);
  bool square, bad;
  fq alpha = fq_root(tab, fq2_norm(g), square, bad);
  auto prefer = [&](const fq2& xi) {
    const fq2 gi = g_rhs(xi, b2);
    bool sq, bd;
    const fq ai = fq_root(tab, fq2_norm(gi), sq, bd);
    bad |= bd;
    x.c0 = fq_select(sq, xi.c0, x.c0);
    x.c1 = fq_select(sq, xi.c1, x.c1);
    g.c0 = fq_select(sq, gi.c0, g.c0);
    g.c1 = fq_select(sq, gi.c1, g.c1);
    alpha = fq_select(sq, ai, alpha);
    square |= sq;
  };
  prefer(x2);
  prefer(x1);
  fq2 y = fq2_root_from_alpha(tab, g, alpha, square, bad);
  if (bad || !square) atomicCAS(err, 0, BN254S_E_INTERNAL);
  if (f2_sgn(uu) != f2_sgn(y)) y = fq2_neg(y);
  fq2_store_canonical(points + 16 * k, x);
  fq2_store_canonical(points + 16 * k + 8, y);
}

// hash_to_fq2 for n inputs of `len` Goldilocks elements each, one lane per input (hash_to_g2.rs:76-87): the challenger lane of
// hash_to_fq.h with both coordinates.
__global__ __launch_bounds__(64) void k_hash_to_fq2(const u64* __restrict__ in, size_t n, size_t len, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  hash_to_fq_lane<2>(in + k * len, len, out + 8 * k);
}

}  // namespace

// hash_to_fq2 (src/utils/hash_to_g2.rs:76-87): Challenger::observe_elements(input); each coordinate = the low 32 bits of 16
// challenges as little-endian limbs of a 512-bit integer, reduced modulo p (f_slice_to_biguint, :226-240, then `.into()`).
extern "C" int bn254s_hash_to_fq2(const uint64_t* input, size_t len, uint64_t* out) {
  if ((!input && len) || !out) return BN254S_E_INVALID_ARG;
  hash_to_fq_host(input, len, 2, out);
  return BN254S_OK;
}

// The same for n inputs at once on the device (inputs[n][len] -> out[n][8]): the step before bn254s_map_to_g2 when a circuit hashes
// many messages to G2.
extern "C" int bn254s_hash_to_fq2_batch(bn254s_ctx* c, const uint64_t* inputs, size_t n, size_t len, uint64_t* out) {
  if (!c || !out || (!inputs && len) || n == 0) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d_in = c->words("h2f.in", n * len + 1);
  u64* d_out = c->words("h2f.out", n * 8);
  if (!d_in || !d_out) return BN254S_E_OOM;
  if (len) HIP_TRY(c, hipMemcpyAsync(d_in, inputs, n * len * 8, hipMemcpyHostToDevice, c->stream));
  k_hash_to_fq2<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, n * 64, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

namespace {

constexpr size_t M2G_PER_PROOF = 128;  // instances of a proof, of either kind

// The pipeline of bn254s_map_to_g2 after its argument check; the proofs that exist when it returns an error are the caller's to release.
int m2g_proven(bn254s_ctx* c, const bn254s_params* params, const uint64_t* u, const uint64_t* offsets, size_t n, uint64_t* out_points,
               uint64_t* fq_jobs, uint64_t* g2_jobs, bn254s_proof** fq_proofs, bn254s_proof** g2_proofs) {
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const M2GConsts C = host_consts();
  const unsigned grid = (unsigned)((n + 63) / 64);
  u64* d = c->words("m2g", n * (8 + 24 + 8 + 8 + 8 + 4 + 16 + 16 + 16 + 16) + 16);
  if (!d) return BN254S_E_OOM;
  u64* d_u = d;
  u64* d_cand = d_u + 8 * n;
  u64* d_fq_s = d_cand + 24 * n;
  u64* d_fq_x = d_fq_s + 8 * n;
  u64* d_leg = d_fq_x + 8 * n;
  u64* d_g2_s = d_leg + 8 * n;
  u64* d_g2_x = d_g2_s + 4 * n;
  u64* d_off = d_g2_x + 16 * n;
  u64* d_o = d_off + 16 * n;
  u64* d_out = d_o + 16 * n;
  int* d_err = (int*)(d_out + 16 * n);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_u, u, n * 64, hipMemcpyHostToDevice, st));
  k_m2g_candidates<<<grid, 64, 0, st>>>(d_u, n, C, d_cand, d_fq_s, d_fq_x);
  std::vector<u64> fs(8 * n), fx(8 * n);
  HIP_TRY(c, hipMemcpyAsync(fs.data(), d_fq_s, fs.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(fx.data(), d_fq_x, fx.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // 2n Legendre exponentiations in 128-instance proofs
  std::vector<u64> leg;
  int rc = prove_and_collect(c, "map_to_g2", 2, params, fs.data(), fx.data(), nullptr, 2 * n, M2G_PER_PROOF, fq_proofs, leg);
  if (rc != BN254S_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_leg, leg.data(), leg.size() * 8, hipMemcpyHostToDevice, st));
  k_m2g_select<<<grid, 64, 0, st>>>(d_u, d_cand, d_leg, n, C, d_g2_s, d_g2_x, d_err);
  std::vector<u64> gs(4 * n), gx(16 * n);
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(gs.data(), d_g2_s, gs.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(gx.data(), d_g2_x, gx.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err("map_to_g2: square root self-check failed");
    return h_err;
  }
  // n cofactor-clearing scalar multiplications
  std::vector<u64> outs;
  rc = prove_and_collect(c, "map_to_g2", 1, params, gs.data(), gx.data(), offsets, n, M2G_PER_PROOF, g2_proofs, outs);
  if (rc != BN254S_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(d_o, outs.data(), outs.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_off, offsets, n * 128, hipMemcpyHostToDevice, st));
  k_m2g_finish<<<grid, 64, 0, st>>>(d_o, d_off, n, d_out, d_err);
  HIP_TRY(c, hipMemcpyAsync(out_points, d_out, n * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (fq_jobs) {  // the job arrays (what bn254s_verify needs as claimed inputs): 2n x (scalar 4 | x 4), n x (scalar 4 | x 16)
    for (size_t k = 0; k < 2 * n; k++) {
      memcpy(fq_jobs + 8 * k, fs.data() + 4 * k, 32);
      memcpy(fq_jobs + 8 * k + 4, fx.data() + 4 * k, 32);
    }
  }
  if (g2_jobs) {
    for (size_t k = 0; k < n; k++) {
      memcpy(g2_jobs + 20 * k, gs.data() + 4 * k, 32);
      memcpy(g2_jobs + 20 * k + 4, gx.data() + 16 * k, 128);
    }
  }
  if (h_err) {
    c->set_err("map_to_g2: output equals +-offset");
    return h_err;
  }
  return BN254S_OK;
}

}  // namespace

// On any error after the argument check no proof is left to the caller and every slot of both arrays is NULL.
extern "C" int bn254s_map_to_g2(bn254s_ctx* c, const bn254s_params* params, const uint64_t* u, const uint64_t* offsets, size_t n,
                                uint64_t* out_points, uint64_t* fq_jobs, uint64_t* g2_jobs, bn254s_proof** fq_proofs,
                                bn254s_proof** g2_proofs) {
  if (!c || !params || !u || !offsets || !out_points || !fq_proofs || !g2_proofs || n == 0) return BN254S_E_INVALID_ARG;
  for (size_t i = 0; i < (2 * n + M2G_PER_PROOF - 1) / M2G_PER_PROOF; i++) fq_proofs[i] = nullptr;
  for (size_t i = 0; i < (n + M2G_PER_PROOF - 1) / M2G_PER_PROOF; i++) g2_proofs[i] = nullptr;
  const int rc = m2g_proven(c, params, u, offsets, n, out_points, fq_jobs, g2_jobs, fq_proofs, g2_proofs);
  if (rc != BN254S_OK) {
    release_proofs(fq_proofs, 2 * n, M2G_PER_PROOF);
    release_proofs(g2_proofs, n, M2G_PER_PROOF);
  }
  return rc;
}

namespace {

// k_m2g_point and k_g2_clear_cofactor on the workspace d (m2g_batch_words(n) words on the device: u in its first 8n, then the
// mapped points, their images, err, bad, finite), not waited for
int map_to_g2_launch(bn254s_ctx* c, u64* d, size_t n) {
  hipStream_t st = c->stream;
  u64 *d_pts = d + 8 * n, *d_img = d_pts + 16 * n;
  int* d_err = (int*)(d_img + 16 * n);
  unsigned* d_bad = (unsigned*)(d_img + 16 * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
  k_m2g_point<<<(unsigned)((n + G1R_LANES - 1) / G1R_LANES), G1R_LANES, 0, st>>>(d, n, host_consts(), d_pts, d_err);
  HIP_TRY(c, hipGetLastError());
  return bn254s_g2_clear_cofactor_device(c, d_pts, n, d_img, (unsigned char*)(d_img + 16 * n + 2), d_bad);
}

// d_u (n x 8 canonical words on the device, in the buffer d of 8n + 16n + 16n + 2 + ceil(n/8) words that starts with it) ->
// out_points: k_m2g_point, then k_g2_clear_cofactor on its points.  Nothing is written on an error.
int map_to_g2_on_device(bn254s_ctx* c, const char* tag, u64* d, size_t n, uint64_t* out_points) {
  hipStream_t st = c->stream;
  u64* d_u = d;
  u64* d_pts = d_u + 8 * n;
  u64* d_img = d_pts + 16 * n;
  int* d_err = (int*)(d_img + 16 * n);
  unsigned* d_bad = (unsigned*)(d_img + 16 * n + 1);
  unsigned char* d_fin = (unsigned char*)(d_img + 16 * n + 2);
  const std::string who = std::string(tag) + ": ";
  int rc = map_to_g2_launch(c, d, n);
  if (rc != BN254S_OK) return rc;
  int h_err = 0;
  unsigned h_bad = UINT_MAX;
  std::vector<uint8_t> fin(n);
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(fin.data(), d_fin, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err(who + "g(x) of the chosen candidate is not a square, or a root does not square back (device self-check)");
    return h_err;
  }
  if (h_bad != UINT_MAX) {
    c->set_err(who + "the mapped point " + std::to_string(h_bad) + " is not on the twist curve (device self-check)");
    return BN254S_E_INTERNAL;
  }
  for (size_t i = 0; i < n; i++)
    if (!fin[i]) {
      c->set_err(who + "the image of input " + std::to_string(i) + " is the point at infinity (the order of its mapped point divides the cofactor)");
      return BN254S_E_INVALID_POINT;
    }
  HIP_TRY(c, hipMemcpyAsync(out_points, d_img, n * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}
size_t m2g_batch_words(size_t n) { return 40 * n + 2 + (n + 7) / 8; }

}  // namespace

size_t bn254s_hash_to_g2_device_words(size_t n) { return m2g_batch_words(n); }

int bn254s_hash_to_g2_device(bn254s_ctx* c, const u64* d_in, size_t n, size_t len, u64* d_work, HashedPoints* at) {
  k_hash_to_fq2<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d_work);
  HIP_TRY(c, hipGetLastError());
  *at = {d_work + 24 * n, (const int*)(d_work + 40 * n), (const unsigned*)(d_work + 40 * n + 1),
         (const unsigned char*)(d_work + 40 * n + 2)};
  return map_to_g2_launch(c, d_work, n);
}

// The reference's native map_to_g2 (hash_to_g2.rs:113-148) without proofs: the point bn254s_map_to_g2 reads from its proofs.
extern "C" int bn254s_map_to_g2_batch(bn254s_ctx* c, const uint64_t* u, size_t n, uint64_t* out_points) {
  if (!c || !u || !out_points || n == 0 || n >= (size_t)UINT_MAX) return BN254S_E_INVALID_ARG;
  if (!coords_below_p(c, "map_to_g2_batch", "u", COORD_FQ2, 2, u, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("m2g.batch", m2g_batch_words(n));
  if (!d) return BN254S_E_OOM;
  HIP_TRY(c, hipMemcpyAsync(d, u, n * 64, hipMemcpyHostToDevice, c->stream));
  return map_to_g2_on_device(c, "map_to_g2_batch", d, n, out_points);
}

// hash_to_g2 (hash_to_g2.rs:40-43): k_hash_to_fq2 writes u where k_m2g_point reads it.
extern "C" int bn254s_hash_to_g2_batch(bn254s_ctx* c, const uint64_t* inputs, size_t n, size_t len, uint64_t* out_points) {
  if (!c || !out_points || (!inputs && len) || n == 0 || n >= (size_t)UINT_MAX) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d_in = c->words("h2f.in", n * len + 1);
  u64* d = c->words("m2g.batch", m2g_batch_words(n));
  if (!d_in || !d) return BN254S_E_OOM;
  if (len) HIP_TRY(c, hipMemcpyAsync(d_in, inputs, n * len * 8, hipMemcpyHostToDevice, c->stream));
  k_hash_to_fq2<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d);
  HIP_TRY(c, hipGetLastError());
  return map_to_g2_on_device(c, "hash_to_g2_batch", d, n, out_points);
}
