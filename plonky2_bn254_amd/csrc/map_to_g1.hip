// map_to_g1 / hash_to_g1 on the device: the G1 twin of map_to_g2.hip.
//
// The reference has no map_to_g1.  This is its map_to_g2 (src/utils/hash_to_g2.rs:113-148: Shallue-van de Woestijne with Z = 1)
// read over Fq on E: y^2 = x^3 + 3, the circuit one writes with FqTarget::is_square (src/fields/fq.rs:283-295: one Fq-exp job with
// the exponent (p-1)/2), sqrt_with_sgn (fq.rs:266-281), inv (src/fields/inv.rs: inv(0) = 0), sgn (src/fields/sgn.rs:9-18: the
// parity of the canonical value), select and G1Target::g_circuit (src/curves/g1.rs:43-51):
//   tv1 = 4 u^2;  tv2 = 1 + tv1;  tv1 = 1 - tv1;  tv3 = inv(tv1 tv2)
//   tv5 = u tv1 tv3 tv4;  x1 = nz2 - tv5;  x2 = nz2 + tv5;  t = tv2^2 tv3;  x3 = 1 + tv6 t^2
//   x = x1 if g(x1) is a square, else x2 if g(x2) is a square, else x3;  y = sqrt(g(x)) with the parity of u
// with g(x) = x^3 + 3, nz2 = -1/2, tv4 = sqrt(-12) = (p - 12)^((p+1)/4) and tv6 = -16/3 (map_to_g1_constants.inc).  G1 has the
// cofactor 1: nothing is cleared, no G2 job is made, no offset is needed; the STARK work is the two Legendre jobs per input.
//   k_m2g1_point: the candidates, c_i = g(x_i)^((p+1)/4) by the ladder of sqrt_ladder.h for all three, the flags
//                 "c_i^2 == g(x_i)" of x1 and x2, the choice, y = +-c of the chosen candidate, and the jobs (p-1)/2 | g(x_i)
//   [2n fq_exp proofs of the Legendre symbols, linked to the flags: proven_jobs.h]
// g(x) is never zero (-3 is not a cube modulo p), so c^2 is g or -g, never both, and y is never zero.
//   k_hash_to_fq: hash_to_fq = the first coordinate of hash_to_fq2 (hash_to_g2.rs:76-87; hash_to_fq.h)
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "hash_to_fq.h"
#include "job_device.h"
#include "root_kinds.h"  // m2g1_candidates, curve_rhs, prove_legendre

namespace {

// points: n x 8 words (x, y); flags: 2n bytes; jobs: 2n x 8 words (scalar (p-1)/2 | g(x_i)); job and flag 2k+i belong to x_{i+1}.
// Every lane runs the same three ladders over the one table in LDS, so that a wave stays together; the choice goes through
// fq_select from x3 down to x1, so that the first candidate with a square g(x) is the one that stays, and with it its c: no
// fourth ladder for the root.  *err: BN254S_E_INTERNAL if some c^2 is neither g nor -g, or if no candidate has a square g.
__global__ __launch_bounds__(G1R_LANES) void k_m2g1_point(const u64* __restrict__ u, size_t n, u64* __restrict__ points,
                                                          unsigned char* __restrict__ flags, u64* __restrict__ jobs,
                                                          int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq uu = fq_from_canonical(u + 4 * k);
  const bool u_odd = u[4 * k] & 1;
  fq x1, x2, x3;
  m2g1_candidates(uu, x1, x2, x3);  // root_kinds.h: the checker's, too
  fq x = x3;
  bool any, bad;  // bad: some c^2 is neither g nor -g, the ladder is wrong
  fq c = fq_root(tab, curve_rhs(x3), any, bad);
  auto prefer = [&](const fq& xi, int i) {
    const fq gi = curve_rhs(xi);
    bool sq, bd;
    const fq ci = fq_root(tab, gi, sq, bd);  // overwrites the lane's own table entries: no barrier
    bad |= bd;
    x = fq_select(sq, xi, x);
    c = fq_select(sq, ci, c);
    any |= sq;
    const fqw gc = fq_to_canonical(gi);
#pragma unroll
    for (int w = 0; w < 4; w++) {
      jobs[8 * (2 * k + i) + w] = G1R_LEGENDRE_EXP[w];
      jobs[8 * (2 * k + i) + 4 + w] = gc.l[w];
    }
    flags[2 * k + i] = sq ? 1 : 0;
  };
  prefer(x2, 1);
  prefer(x1, 0);
  if (bad || !any) atomicCAS(err, 0, BN254S_E_INTERNAL);
  fqw y = fq_to_canonical(c);
  if ((bool)(y.l[0] & 1) != u_odd) y = fq_to_canonical(fq_neg(c));  // p - y: the other parity, as p is odd and y != 0
  const fqw xc = fq_to_canonical(x);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    points[8 * k + w] = xc.l[w];
    points[8 * k + 4 + w] = y.l[w];
  }
}

// hash_to_fq for n inputs of `len` Goldilocks elements each, one lane per input: the challenger lane of k_hash_to_fq2 with one
// coordinate.  out: n x 4 canonical words.
__global__ __launch_bounds__(64) void k_hash_to_fq(const u64* __restrict__ in, size_t n, size_t len, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  hash_to_fq_lane<1>(in + k * len, len, out + 4 * k);
}

// words of the front-end's device buffer: u (4n), points (8n), jobs (16n), err (1), flags (2n bytes)
size_t m2g1_words(size_t n) { return 28 * n + 1 + (2 * n + 7) / 8; }

// k_m2g1_point on the workspace d (m2g1_words(n) words on the device, u in its first 4n, then points, jobs, err, flags), not waited for
int m2g1_launch(bn254s_ctx* c, u64* d, size_t n) {
  u64 *d_pts = d + 4 * n, *d_jobs = d_pts + 8 * n;
  int* d_err = (int*)(d_jobs + 16 * n);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, c->stream));
  k_m2g1_point<<<(unsigned)((n + G1R_LANES - 1) / G1R_LANES), G1R_LANES, 0, c->stream>>>(d, n, d_pts, (unsigned char*)(d_jobs + 16 * n + 1),
                                                                                        d_jobs, d_err);
  HIP_TRY(c, hipGetLastError());
  return BN254S_OK;
}

// d (m2g1_words(n) words on the device, u in its first 4n) -> points[n x 8], flags[2n], jobs[2n x 8] in host memory (flags and
// jobs may be NULL).  Nothing is written on an error.
int m2g1_on_device(bn254s_ctx* c, const char* tag, u64* d, size_t n, uint64_t* points, uint8_t* flags, uint64_t* jobs) {
  hipStream_t st = c->stream;
  u64* d_u = d;
  u64* d_pts = d_u + 4 * n;
  u64* d_jobs = d_pts + 8 * n;
  int* d_err = (int*)(d_jobs + 16 * n);
  unsigned char* d_flags = (unsigned char*)(d_jobs + 16 * n + 1);
  const int rc = m2g1_launch(c, d, n);
  if (rc != BN254S_OK) return rc;
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err(std::string(tag) + ": g(x)^((p+1)/4) squares to neither g(x) nor -g(x), or no candidate has a square g(x) (device self-check)");
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(points, d_pts, n * 64, hipMemcpyDeviceToHost, st));
  if (flags) HIP_TRY(c, hipMemcpyAsync(flags, d_flags, 2 * n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

// The front-end for u in host memory; the first u_i >= p is reported before any device work.
int m2g1_front(bn254s_ctx* c, const char* tag, const uint64_t* u, size_t n, uint64_t* points, uint8_t* flags, uint64_t* jobs) {
  if (!coords_below_p(c, tag, "u", nullptr, 1, u, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("m2g1", m2g1_words(n));
  if (!d) return BN254S_E_OOM;
  HIP_TRY(c, hipMemcpyAsync(d, u, n * 32, hipMemcpyHostToDevice, c->stream));
  return m2g1_on_device(c, tag, d, n, points, flags, jobs);
}

}  // namespace

size_t bn254s_hash_to_g1_device_words(size_t n) { return m2g1_words(n); }

int bn254s_hash_to_g1_device(bn254s_ctx* c, const u64* d_in, size_t n, size_t len, u64* d_work, HashedPoints* at) {
  k_hash_to_fq<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d_work);
  HIP_TRY(c, hipGetLastError());
  *at = {d_work + 4 * n, (const int*)(d_work + 28 * n), nullptr, nullptr};
  return m2g1_launch(c, d_work, n);
}

extern "C" int bn254s_hash_to_fq(const uint64_t* input, size_t len, uint64_t* out) {
  if ((!input && len) || !out) return BN254S_E_INVALID_ARG;
  hash_to_fq_host(input, len, 1, out);
  return BN254S_OK;
}

extern "C" int bn254s_hash_to_fq_batch(bn254s_ctx* c, const uint64_t* inputs, size_t n, size_t len, uint64_t* out) {
  if (!c || !out || (!inputs && len) || n == 0 || n >= ((size_t)1 << 32)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d_in = c->words("h2f1.in", n * len + 1);
  u64* d_out = c->words("h2f1.out", n * 4);
  if (!d_in || !d_out) return BN254S_E_OOM;
  if (len) HIP_TRY(c, hipMemcpyAsync(d_in, inputs, n * len * 8, hipMemcpyHostToDevice, c->stream));
  k_hash_to_fq<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

extern "C" int bn254s_map_to_g1_batch(bn254s_ctx* c, const uint64_t* u, size_t n, uint64_t* out_points, uint8_t* sq_flags,
                                      uint64_t* fq_jobs) {
  if (!c || !u || !out_points || n == 0 || n >= ((size_t)1 << 32)) return BN254S_E_INVALID_ARG;
  return m2g1_front(c, "map_to_g1_batch", u, n, out_points, sq_flags, fq_jobs);
}

// hash_to_g1: k_hash_to_fq writes u where k_m2g1_point reads it (u is below p by construction).
extern "C" int bn254s_hash_to_g1_batch(bn254s_ctx* c, const uint64_t* inputs, size_t n, size_t len, uint64_t* out_points) {
  if (!c || !out_points || (!inputs && len) || n == 0 || n >= ((size_t)1 << 32)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d_in = c->words("h2f1.in", n * len + 1);
  u64* d = c->words("m2g1", m2g1_words(n));
  if (!d_in || !d) return BN254S_E_OOM;
  if (len) HIP_TRY(c, hipMemcpyAsync(d_in, inputs, n * len * 8, hipMemcpyHostToDevice, c->stream));
  k_hash_to_fq<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_in, n, len, d);
  HIP_TRY(c, hipGetLastError());
  return m2g1_on_device(c, "hash_to_g1_batch", d, n, out_points, nullptr, nullptr);
}

extern "C" int bn254s_map_to_g1(bn254s_ctx* c, const bn254s_params* params, const uint64_t* u, size_t n, size_t per_proof,
                                uint64_t* out_points, uint8_t* sq_flags, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  const size_t n_jobs = 2 * n;
  int rc = proven_args(c, "map_to_g1", "Fq-exp proof", u && out_points && n > 0 && n < ((size_t)1 << 31), params, fq_proofs, n_jobs,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> points(8 * n), jobs(8 * n_jobs);
  std::vector<uint8_t> flags(n_jobs);
  rc = m2g1_front(c, "map_to_g1", u, n, points.data(), flags.data(), jobs.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_legendre(c, "map_to_g1", params, jobs, flags.data(), n_jobs, per_proof, fq_proofs);
  if (rc != BN254S_OK) return rc;
  memcpy(out_points, points.data(), points.size() * 8);
  if (sq_flags) memcpy(sq_flags, flags.data(), flags.size());
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}
