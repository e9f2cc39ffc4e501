// G1 point recovery from x on the device: the witness arithmetic of the reference's G1Target::is_recoverable_from_x /
// recover_from_x (src/curves/g1.rs:76-95; native form src/fields/recover.rs) around their one STARK job kind:
//   k_g1_recover: g = x^3 + 3, the Legendre job g^((p-1)/2) (is_square, src/fields/fq.rs:283-295), the flag "g is a square" and
//                 y = sqrt(g) with an even low bit (sqrt_with_sgn with sgn = false, fq.rs:266-281)
//   [n fq_exp proofs of the Legendre symbols]
// One exponentiation per input: p = 3 (mod 4), so c = g^((p+1)/4) has c^2 = g g^((p-1)/2) = +-g: c^2 == g says that g is a square
// and c is its root, c^2 == -g that it is none.  g is never zero (-3 is not a cube modulo p: pow(p - 3, (p - 1)/3, p) != 1), so
// the native definition of "recoverable" (g.sqrt().is_some(), true for 0) and the circuit's (Legendre symbol == 1) agree, and
// the two cases exclude each other.
#include <cstring>
#include <string>
#include <vector>
#include "proven_jobs.h"
#include "sqrt_ladder.h"

namespace {

// points: n x 8 words (x, y); flags: n bytes; jobs: n x 8 words (scalar (p-1)/2 | g)
__global__ __launch_bounds__(G1R_LANES) void k_g1_recover(const u64* __restrict__ xs, size_t n, u64* __restrict__ points,
                                                          unsigned char* __restrict__ flags, u64* __restrict__ jobs,
                                                          int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq x = fq_from_canonical(xs + 4 * k);
  const fq one = fq_one();
  const fq g = fq_add(fq_mul(fq_sqr(x), x), fq_add(fq_dbl(one), one));
  const fq c = sqrt_ladder(tab, g);  // sqrt_ladder.h
  const fq c2 = fq_sqr(c);
  const bool square = fq_eq(c2, g);
  if (!square && !fq_eq(c2, fq_neg(g))) atomicCAS(err, 0, BN254S_E_INTERNAL);  // neither root nor non-residue: the ladder is wrong
  fqw y = fq_to_canonical(c);
  if (y.l[0] & 1) y = fq_to_canonical(fq_neg(c));  // p - y: even, as p is odd and y != 0
  const fqw gc = fq_to_canonical(g);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    points[8 * k + w] = xs[4 * k + w];
    points[8 * k + 4 + w] = square ? y.l[w] : 0;
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = gc.l[w];
  }
  flags[k] = square ? 1 : 0;
}

// the arguments that both entry points share, other than the context
bool recover_args_ok(const uint64_t* xs, size_t n, const uint64_t* points_out, const uint8_t* flags_out) {
  return xs && points_out && flags_out && n > 0 && n < ((size_t)1 << 32);
}

// The front-end into host memory: points[n x 8], flags[n], jobs[n x 8] (jobs may be NULL).  Nothing is written on an error.
int recover_front(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* points, uint8_t* flags, uint64_t* jobs) {
  if (!coords_below_p(c, "g1_recover_from_x", "x", nullptr, 1, xs, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("g1rec", 4 * n /* xs */ + 8 * n /* points */ + 8 * n /* jobs */ + 1 /* err */ + (n + 7) / 8 /* flags */);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d;
  u64* d_pts = d_xs + 4 * n;
  u64* d_jobs = d_pts + 8 * n;
  int* d_err = (int*)(d_jobs + 8 * n);
  unsigned char* d_flags = (unsigned char*)(d_jobs + 8 * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * 32, hipMemcpyHostToDevice, st));
  k_g1_recover<<<(unsigned)((n + G1R_LANES - 1) / G1R_LANES), G1R_LANES, 0, st>>>(d_xs, n, d_pts, d_flags, d_jobs, d_err);
  HIP_TRY(c, hipGetLastError());
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err("g1_recover_from_x: g^((p+1)/4) squares to neither g nor -g (device self-check)");
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(points, d_pts, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g1_recover_from_x_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* points_out, uint8_t* flags_out,
                                              uint64_t* fq_jobs) {
  if (!c || !recover_args_ok(xs, n, points_out, flags_out)) return BN254S_E_INVALID_ARG;
  return recover_front(c, xs, n, points_out, flags_out, fq_jobs);
}

extern "C" int bn254s_g1_recover_from_x(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, size_t n, size_t per_proof,
                                        uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  int rc = proven_args(c, "g1_recover_from_x", "Fq-exp proof", recover_args_ok(xs, n, points_out, flags_out), params, fq_proofs, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> jobs(8 * n);
  rc = recover_front(c, xs, n, points_out, flags_out, jobs.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_legendre(c, "g1_recover_from_x", params, jobs, flags_out, n, per_proof, fq_proofs);
  if (rc != BN254S_OK) return rc;
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}
