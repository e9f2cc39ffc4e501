// The field gadgets of the reference's src/fields/ on the device, for values that are not the right-hand side of a curve equation:
//   k_fq_sqrt:  FqTarget::is_square (fq.rs:283-295) and FqTarget::sqrt_with_sgn (fq.rs:266-281, generator :357-365)
//   k_fq2_sqrt: Fq2Target::is_square (fq2.rs:228-241) and Fq2Target::sqrt_with_sgn (fq2.rs:209-226, generator :305-313; sign
//               rule sgn.rs:20-27)
//   k_fq_inv, k_fq2_inv: FqTarget::inv (fq.rs:241-255) and Fq2Target::inv (fq2.rs:190-204; native inv.rs), inv(0) = 0
//   [n fq_exp proofs of the Legendre symbols x^((p-1)/2) | norm(x)^((p-1)/2) for the proven forms]
// The arithmetic is that of g1_recover.hip and g2_recover.hip (sqrt_ladder.h, fq2_root.h); what is new is the input that a curve
// equation never produces:
//   x = 0.  Fq: c = 0^((p+1)/4) = 0 squares to x AND to -x, so the flags come from fq_is_zero(x): is_square is the gadget's
//     "Legendre symbol == 1" and the symbol of 0 is 0, so square = 0; a root with the wanted sign exists for sgn 0 only (the one
//     root 0 is even).  Fq2: norm = 0 (only for x = 0: -1 is a non-residue, p = 3 mod 4), alpha = 0 "is a root", g.c1 == 0 picks
//     delta = g.c0 = 0, t = 0, plus holds, o = g.c1 * fq_inv(0) = 0 * (a canonical value) = 0 whatever fq_inv makes of 0 (it makes
//     0: with g = 0 no divstep ever swaps, every round's matrix is (2^30 0; 0 1), so d stays 0 and f = p > 0), y = (0, 0).
//   c1 == 0, c0 a residue:     norm = c0^2, delta = c0 (NOT (alpha + c0)/2, which vanishes for alpha = -c0), t^2 = c0:  y = (t, 0).
//   c1 == 0, c0 a non-residue: delta = c0, t^2 = -c0, the !plus branch with o = 0: y = (0, t), y^2 = -t^2 = c0; sgn falls to c1.
// Every lane runs every ladder and inversion; the zero cases are selected, never branched around.
#include <cstring>
#include <string>
#include <vector>
#include "proven_jobs.h"
#include "fq2_root.h"

namespace {

// xs, roots: n x 4 words; sgns, square, ok: n bytes; jobs: n x 8 words ((p-1)/2 | x)
__global__ __launch_bounds__(G1R_LANES) void k_fq_sqrt(const u64* __restrict__ xs, const unsigned char* __restrict__ sgns, size_t n,
                                                       u64* __restrict__ roots, unsigned char* __restrict__ square,
                                                       unsigned char* __restrict__ ok, u64* __restrict__ jobs, int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq x = fq_from_canonical(xs + 4 * k);
  const bool zero = fq_is_zero(x);
  const fq c = sqrt_ladder(tab, x);  // sqrt_ladder.h; 0 for x = 0
  const fq c2 = fq_sqr(c);
  const bool root = fq_eq(c2, x);  // also true for x = 0, like the comparison with -x
  if (!root && !fq_eq(c2, fq_neg(x))) atomicCAS(err, 0, BN254S_E_INTERNAL);  // neither root nor non-residue: the ladder is wrong
  const bool want = sgns[k] != 0;
  fqw y = fq_to_canonical(c);
  if ((bool)(y.l[0] & 1) != want) y = fq_to_canonical(fq_neg(c));  // p - y flips the parity of y != 0, as p is odd; -0 = 0
  const bool has = zero ? !want : root;                               // the one root of 0 is even
#pragma unroll
  for (int w = 0; w < 4; w++) {
    roots[4 * k + w] = has ? y.l[w] : 0;
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = xs[4 * k + w];
  }
  square[k] = root && !zero ? 1 : 0;
  ok[k] = has ? 1 : 0;
}

// xs, roots: n x 8 words (c0, c1); sgns, square, ok: n bytes; jobs: n x 8 words ((p-1)/2 | norm(x))
__global__ __launch_bounds__(G1R_LANES) void k_fq2_sqrt(const u64* __restrict__ xs, const unsigned char* __restrict__ sgns, size_t n,
                                                        u64* __restrict__ roots, unsigned char* __restrict__ square,
                                                        unsigned char* __restrict__ ok, u64* __restrict__ jobs, int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq2 x = fq2_from_canonical(xs + 8 * k);
  const fq nrm = fq2_norm(x);
  const bool zero = fq_is_zero(nrm);  // norm(x) = 0 only for x = 0
  bool root, bad;
  const fq2 y = fq2_root(tab, x, nrm, root, bad);  // fq2_root.h; root holds and y = (0, 0) for x = 0 (the head of this file)
  if (bad) atomicCAS(err, 0, BN254S_E_INTERNAL);
  const bool want = sgns[k] != 0;
  fqw y0 = fq_to_canonical(y.c0), y1 = fq_to_canonical(y.c1);
  if (sgn_words(y0, y1) != want) {  // -y: p - c for a non-zero coordinate, which flips its parity as p is odd
    y0 = fq_to_canonical(fq_neg(y.c0));
    y1 = fq_to_canonical(fq_neg(y.c1));
  }
  const bool has = zero ? !want : root;  // sgn(0) = 0
  const fqw nc = fq_to_canonical(nrm);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    roots[8 * k + w] = has ? y0.l[w] : 0;
    roots[8 * k + 4 + w] = has ? y1.l[w] : 0;
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = nc.l[w];
  }
  square[k] = root && !zero ? 1 : 0;
  ok[k] = has ? 1 : 0;
}

// a^-1, 0 for a = 0.  fq_inv maps 0 to 0 by itself (the head of this file), but nothing pins that, so the divsteps see 1 in place
// of 0 and the result is selected: the zero case does not depend on how the inversion treats it.
__device__ __forceinline__ fq inv_or_zero(const fq& a) {
  const bool zero = fq_is_zero(a);
  return fq_select(zero, fq_zero(), fq_inv(fq_select(zero, fq_one(), a)));
}

// xs, out: n x 4 words
__global__ __launch_bounds__(G1R_LANES) void k_fq_inv(const u64* __restrict__ xs, size_t n, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  fe_store_canonical(out + 4 * k, inv_or_zero(fq_from_canonical(xs + 4 * k)));
}

// xs, out: n x 8 words (c0, c1): (c0, -c1) / norm; for x = 0 the norm is 0, its "inverse" 0 and both products vanish
__global__ __launch_bounds__(G1R_LANES) void k_fq2_inv(const u64* __restrict__ xs, size_t n, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq2 x = fq2_from_canonical(xs + 8 * k);
  fq2_store_canonical(out + 8 * k, fq2_inv_from_norm_inv(x, inv_or_zero(fq2_norm(x))));
}

// W: words of an element, 4 (Fq) or 8 (Fq2)
const char* sqrt_tag(int W) { return W == 4 ? "fq_sqrt" : "fq2_sqrt"; }
const char* inv_tag(int W) { return W == 4 ? "fq_inv" : "fq2_inv"; }

// the arguments that both entry points of a root share, other than the context
bool sqrt_args_ok(const uint64_t* xs, size_t n, const uint64_t* roots_out, const uint8_t* square_out, const uint8_t* root_ok_out) {
  return xs && roots_out && square_out && root_ok_out && n > 0 && n < ((size_t)1 << 32);
}

// The front-end of a root into host memory: roots[n x W], square[n], ok[n], jobs[n x 8] (jobs may be NULL).  Nothing is written
// on an error.
int sqrt_front(bn254s_ctx* c, int W, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots, uint8_t* square, uint8_t* ok,
               uint64_t* jobs) {
  const std::string tag = sqrt_tag(W);
  // the first input with a coordinate that is not below p or a sign byte above 1 is reported, the coordinates before the sign
  size_t s = 0;
  while (s < n && (!sgns || sgns[s] <= 1)) s++;
  if (!coords_below_p(c, tag, "x", COORD_FQ2, W / 4, xs, s < n ? s + 1 : n)) return BN254S_E_INVALID_ARG;
  if (s < n) {
    c->set_err(tag + ": sgn_" + std::to_string(s) + " is " + std::to_string(sgns[s]) + ", neither 0 nor 1");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words(W == 4 ? "fqsqrt" : "fq2sqrt",
                    W * n /* xs */ + W * n /* roots */ + 8 * n /* jobs */ + 1 /* err */ + 3 * nb /* square, ok, sgns */);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d;
  u64* d_roots = d_xs + W * n;
  u64* d_jobs = d_roots + W * n;
  int* d_err = (int*)(d_jobs + 8 * n);
  unsigned char* d_square = (unsigned char*)(d_jobs + 8 * n + 1);
  unsigned char* d_ok = d_square + 8 * nb;
  unsigned char* d_sgns = d_ok + 8 * nb;
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * W * 8, hipMemcpyHostToDevice, st));
  if (sgns)
    HIP_TRY(c, hipMemcpyAsync(d_sgns, sgns, n, hipMemcpyHostToDevice, st));
  else
    HIP_TRY(c, hipMemsetAsync(d_sgns, 0, n, st));
  const unsigned blocks = (unsigned)((n + G1R_LANES - 1) / G1R_LANES);
  if (W == 4) k_fq_sqrt<<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_roots, d_square, d_ok, d_jobs, d_err);
  else k_fq2_sqrt<<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_roots, d_square, d_ok, d_jobs, d_err);
  HIP_TRY(c, hipGetLastError());
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err(tag + (W == 4 ? ": x^((p+1)/4) squares to neither x nor -x (device self-check)"
                             : ": a square root does not square back (device self-check)"));
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(roots, d_roots, n * W * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(square, d_square, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

int sqrt_batch(bn254s_ctx* c, int W, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots_out, uint8_t* square_out,
               uint8_t* root_ok_out, uint64_t* fq_jobs) {
  if (!c || !sqrt_args_ok(xs, n, roots_out, square_out, root_ok_out)) return BN254S_E_INVALID_ARG;
  return sqrt_front(c, W, xs, sgns, n, roots_out, square_out, root_ok_out, fq_jobs);
}

// The proven form: the front-end into buffers of its own, the Fq-exp proofs of the n jobs, the three-valued linkage
// (prove_legendre with zero_bases: 1 | p - 1 | 0 for a square, a non-square, a zero base); the outputs are written on success only.
int sqrt_proven(bn254s_ctx* c, int W, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n, size_t per_proof,
                uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  int rc = proven_args(c, sqrt_tag(W), "Fq-exp proof", sqrt_args_ok(xs, n, roots_out, square_out, root_ok_out), params, fq_proofs, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> roots((size_t)W * n), jobs(8 * n);
  std::vector<uint8_t> square(n), ok(n);
  rc = sqrt_front(c, W, xs, sgns, n, roots.data(), square.data(), ok.data(), jobs.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_legendre(c, sqrt_tag(W), params, jobs, square.data(), n, per_proof, fq_proofs, /*zero_bases=*/true);
  if (rc != BN254S_OK) return rc;
  memcpy(roots_out, roots.data(), roots.size() * 8);
  memcpy(square_out, square.data(), n);
  memcpy(root_ok_out, ok.data(), n);
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}

int inv_batch(bn254s_ctx* c, int W, const uint64_t* xs, size_t n, uint64_t* out) {
  if (!c || !xs || !out || n == 0 || n >= ((size_t)1 << 32)) return BN254S_E_INVALID_ARG;
  if (!coords_below_p(c, inv_tag(W), "x", COORD_FQ2, W / 4, xs, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("fqinv", 2 * W * n /* xs, out */);
  if (!d) return BN254S_E_OOM;
  u64 *d_xs = d, *d_out = d + W * n;
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * W * 8, hipMemcpyHostToDevice, st));
  const unsigned blocks = (unsigned)((n + G1R_LANES - 1) / G1R_LANES);
  if (W == 4) k_fq_inv<<<blocks, G1R_LANES, 0, st>>>(d_xs, n, d_out);
  else k_fq2_inv<<<blocks, G1R_LANES, 0, st>>>(d_xs, n, d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));  // a failed kernel must not reach the caller's memory
  HIP_TRY(c, hipMemcpyAsync(out, d_out, n * W * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_fq_sqrt_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots_out,
                                    uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs) {
  return sqrt_batch(c, 4, xs, sgns, n, roots_out, square_out, root_ok_out, fq_jobs);
}
extern "C" int bn254s_fq2_sqrt_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots_out,
                                     uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs) {
  return sqrt_batch(c, 8, xs, sgns, n, roots_out, square_out, root_ok_out, fq_jobs);
}
extern "C" int bn254s_fq_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                              size_t per_proof, uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs,
                              bn254s_proof** fq_proofs) {
  return sqrt_proven(c, 4, params, xs, sgns, n, per_proof, roots_out, square_out, root_ok_out, fq_jobs, fq_proofs);
}
extern "C" int bn254s_fq2_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                               size_t per_proof, uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs,
                               bn254s_proof** fq_proofs) {
  return sqrt_proven(c, 8, params, xs, sgns, n, per_proof, roots_out, square_out, root_ok_out, fq_jobs, fq_proofs);
}
extern "C" int bn254s_fq_inv_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* out) { return inv_batch(c, 4, xs, n, out); }
extern "C" int bn254s_fq2_inv_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* out) { return inv_batch(c, 8, xs, n, out); }
