// G2 point recovery from x on the device: the witness arithmetic of the reference's G2Target::g_circuit (src/curves/g2.rs:42-54),
// Fq2Target::is_square (src/fields/fq2.rs:228-241) and Fq2Target::sqrt_with_sgn (fq2.rs:209-226; sign rule src/fields/sgn.rs:20-27)
// around their one STARK job kind:
//   k_g2_recover: g = x^3 + b' in Fq2, the Legendre job norm(g)^((p-1)/2), the flag "g is a square" and y = sqrt(g) with the
//                 wanted sign
//   [n fq_exp proofs of the Legendre symbols]
// An Fq2 square root in two Fq exponentiations, both with the exponent (p+1)/4 of sqrt_ladder.h (p = 3 mod 4); the code is
// fq2_root.h, shared with map_to_g2.hip:
//   1. N = g.c0^2 + g.c1^2, alpha = N^((p+1)/4): alpha^2 == N says that N, and with it g, is a square; alpha^2 == -N that it is none.
//   2. delta = (alpha + g.c0)/2 satisfies delta (delta - alpha) = -g.c1^2/4.  t = delta^((p+1)/4) has t^2 = +-delta:
//        t^2 ==  delta: y = (t, g.c1/(2t)),   since (g.c1/(2t))^2 = alpha - delta and t^2 - (alpha - delta) = g.c0;
//        t^2 == -delta: y = (g.c1/(2t), t),   since (g.c1/(2t))^2 = delta - alpha and (delta - alpha) - t^2 = g.c0.
//      For g.c1 == 0 delta could vanish (alpha = -g.c0), so delta = g.c0 there: the same two formulas give (t, 0) and (0, t).
// g is never zero (the twist has odd order: no point with y = 0; equivalently -b' is not a cube in Fq2), and -1 is a non-residue
// of Fq, so N is never zero either: "N is a square" and "the Legendre symbol of N is 1" agree, and delta, t are never zero.
#include "proven_jobs.h"
#include "fq2_root.h"

namespace {

// xs: n x 8 words (x.c0, x.c1); sgns: n bytes; points: n x 16 words (x, y); flags: n bytes; jobs: n x 8 words ((p-1)/2 | norm(g))
__global__ __launch_bounds__(G1R_LANES) void k_g2_recover(const u64* __restrict__ xs, const unsigned char* __restrict__ sgns, size_t n,
                                                          u64* __restrict__ points, unsigned char* __restrict__ flags,
                                                          u64* __restrict__ jobs, int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq2 x = fq2_from_canonical(xs + 8 * k);
  fq2 b;
  b.c0 = fq_from_limbs(G2R_B_C0);
  b.c1 = fq_from_limbs(G2R_B_C1);
  const fq2 g = fq2_add(fq2_mul(fq2_sqr(x), x), b);
  const fq nrm = fq2_norm(g);
  bool square, bad;
  const fq2 y = fq2_root(tab, g, nrm, square, bad);
  if (bad) atomicCAS(err, 0, BN254S_E_INTERNAL);
  fqw y0 = fq_to_canonical(y.c0), y1 = fq_to_canonical(y.c1);
  if (sgn_words(y0, y1) != (sgns[k] != 0)) {  // -y: p - c for a non-zero coordinate, which flips its parity as p is odd
    y0 = fq_to_canonical(fq_neg(y.c0));
    y1 = fq_to_canonical(fq_neg(y.c1));
  }
  const fqw nc = fq_to_canonical(nrm);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    points[16 * k + w] = xs[8 * k + w];
    points[16 * k + 4 + w] = xs[8 * k + 4 + w];
    points[16 * k + 8 + w] = square ? y0.l[w] : 0;
    points[16 * k + 12 + w] = square ? y1.l[w] : 0;
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = nc.l[w];
  }
  flags[k] = square ? 1 : 0;
}

// the arguments that both entry points share, other than the context
bool recover_args_ok(const uint64_t* xs, size_t n, const uint64_t* points_out, const uint8_t* flags_out) {
  return xs && points_out && flags_out && n > 0 && n < ((size_t)1 << 32);
}

// The front-end into host memory: points[n x 16], flags[n], jobs[n x 8] (jobs may be NULL).  Nothing is written on an error.
int recover_front(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* points, uint8_t* flags, uint64_t* jobs) {
  // the first input with a coordinate that is not below p or a sign byte above 1 is reported, the coordinates before the sign
  size_t s = 0;
  while (s < n && (!sgns || sgns[s] <= 1)) s++;
  if (!coords_below_p(c, "g2_recover_from_x", "x", COORD_FQ2, 2, xs, s < n ? s + 1 : n)) return BN254S_E_INVALID_ARG;
  if (s < n) {
    c->set_err("g2_recover_from_x: sgn_" + std::to_string(s) + " is " + std::to_string(sgns[s]) + ", neither 0 nor 1");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words("g2rec", 8 * n /* xs */ + 16 * n /* points */ + 8 * n /* jobs */ + 1 /* err */ + nb /* flags */ + nb /* sgns */);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d;
  u64* d_pts = d_xs + 8 * n;
  u64* d_jobs = d_pts + 16 * n;
  int* d_err = (int*)(d_jobs + 8 * n);
  unsigned char* d_flags = (unsigned char*)(d_jobs + 8 * n + 1);
  unsigned char* d_sgns = d_flags + 8 * nb;
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * 64, hipMemcpyHostToDevice, st));
  if (sgns)
    HIP_TRY(c, hipMemcpyAsync(d_sgns, sgns, n, hipMemcpyHostToDevice, st));
  else
    HIP_TRY(c, hipMemsetAsync(d_sgns, 0, n, st));
  k_g2_recover<<<(unsigned)((n + G1R_LANES - 1) / G1R_LANES), G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_pts, d_flags, d_jobs, d_err);
  HIP_TRY(c, hipGetLastError());
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err("g2_recover_from_x: a square root does not square back (device self-check)");
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(points, d_pts, n * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g2_recover_from_x_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* points_out,
                                              uint8_t* flags_out, uint64_t* fq_jobs) {
  if (!c || !recover_args_ok(xs, n, points_out, flags_out)) return BN254S_E_INVALID_ARG;
  return recover_front(c, xs, sgns, n, points_out, flags_out, fq_jobs);
}

extern "C" int bn254s_g2_recover_from_x(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                                        size_t per_proof, uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs,
                                        bn254s_proof** fq_proofs) {
  int rc = proven_args(c, "g2_recover_from_x", "Fq-exp proof", recover_args_ok(xs, n, points_out, flags_out), params, fq_proofs, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> jobs(8 * n);
  rc = recover_front(c, xs, sgns, n, points_out, flags_out, jobs.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_legendre(c, "g2_recover_from_x", params, jobs, flags_out, n, per_proof, fq_proofs);
  if (rc != BN254S_OK) return rc;
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}
