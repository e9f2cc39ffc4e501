// The four one-job root front-ends on the device: one kernel (k_root<WHAT>), one host front (root_front) and one proven body
// (root_proven) over the table of root_kinds.h.  Each input gives one root with a wanted sign, its flag(s) and one Legendre job
// (p-1)/2 | base, the one STARK job kind of the gadgets it replaces:
//   G1 recovery, G2 recovery: the root of the right-hand side of the curve at x, in a row (x, y)
//   fq_sqrt, fq2_sqrt:        the root of x itself, for values that are not the right-hand side of a curve equation
//   [n fq_exp proofs of the Legendre symbols for the proven forms]
//
// G1 point recovery from x: the witness arithmetic of the reference's G1Target::is_recoverable_from_x /
// recover_from_x (src/curves/g1.rs:76-95; native form src/fields/recover.rs) around their one STARK job kind:
//   k_root<G1_RECOVER>: g = x^3 + 3, the Legendre job g^((p-1)/2) (is_square, src/fields/fq.rs:283-295), the flag "g is a square"
//                 and y = sqrt(g) with an even low bit (sqrt_with_sgn with sgn = false, fq.rs:266-281)
// One exponentiation per input: p = 3 (mod 4), so c = g^((p+1)/4) has c^2 = g g^((p-1)/2) = +-g: c^2 == g says that g is a square
// and c is its root, c^2 == -g that it is none.  g is never zero (-3 is not a cube modulo p: pow(p - 3, (p - 1)/3, p) != 1), so
// the native definition of "recoverable" (g.sqrt().is_some(), true for 0) and the circuit's (Legendre symbol == 1) agree, and
// the two cases exclude each other.
//
// G2 point recovery from x: the witness arithmetic of the reference's G2Target::g_circuit (src/curves/g2.rs:42-54),
// Fq2Target::is_square (src/fields/fq2.rs:228-241) and Fq2Target::sqrt_with_sgn (fq2.rs:209-226; sign rule src/fields/sgn.rs:20-27)
// around their one STARK job kind:
//   k_root<G2_RECOVER>: g = x^3 + b' in Fq2, the Legendre job norm(g)^((p-1)/2), the flag "g is a square" and y = sqrt(g) with the
//                 wanted sign
// An Fq2 square root in two Fq exponentiations, both with the exponent (p+1)/4 of sqrt_ladder.h (p = 3 mod 4); the code is
// fq2_root.h, shared with map_to_g2.hip:
//   1. N = g.c0^2 + g.c1^2, alpha = N^((p+1)/4): alpha^2 == N says that N, and with it g, is a square; alpha^2 == -N that it is none.
//   2. delta = (alpha + g.c0)/2 satisfies delta (delta - alpha) = -g.c1^2/4.  t = delta^((p+1)/4) has t^2 = +-delta:
//        t^2 ==  delta: y = (t, g.c1/(2t)),   since (g.c1/(2t))^2 = alpha - delta and t^2 - (alpha - delta) = g.c0;
//        t^2 == -delta: y = (g.c1/(2t), t),   since (g.c1/(2t))^2 = delta - alpha and (delta - alpha) - t^2 = g.c0.
//      For g.c1 == 0 delta could vanish (alpha = -g.c0), so delta = g.c0 there: the same two formulas give (t, 0) and (0, t).
// g is never zero (the twist has odd order: no point with y = 0; equivalently -b' is not a cube in Fq2), and -1 is a non-residue
// of Fq, so N is never zero either: "N is a square" and "the Legendre symbol of N is 1" agree, and delta, t are never zero.
//
// The field gadgets of the reference's src/fields/, for values that are not the right-hand side of a curve equation:
//   k_root<FQ_SQRT>:  FqTarget::is_square (fq.rs:283-295) and FqTarget::sqrt_with_sgn (fq.rs:266-281, generator :357-365)
//   k_root<FQ2_SQRT>: Fq2Target::is_square (fq2.rs:228-241) and Fq2Target::sqrt_with_sgn (fq2.rs:209-226, generator :305-313; sign
//               rule sgn.rs:20-27)
// The arithmetic is that of the recovery kinds (sqrt_ladder.h, fq2_root.h); what is new is the input that a curve equation never
// produces:
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
#include "root_kinds.h"

namespace {

// the canonical words of the one of +-c that has the sign `want`: p - y flips the parity of y != 0, as p is odd; -0 = 0
__device__ __forceinline__ void signed_words(const fq& c, bool want, fqw (&y)[1]) {
  y[0] = fq_to_canonical(c);
  if ((bool)(y[0].l[0] & 1) != want) y[0] = fq_to_canonical(fq_neg(c));
}
__device__ __forceinline__ void signed_words(const fq2& c, bool want, fqw (&y)[2]) {
  y[0] = fq_to_canonical(c.c0);
  y[1] = fq_to_canonical(c.c1);
  if (sgn_words(y[0], y[1]) != want) {  // -y: p - c for a non-zero coordinate
    y[0] = fq_to_canonical(fq_neg(c.c0));
    y[1] = fq_to_canonical(fq_neg(c.c1));
  }
}

// xs: n x IW words; sgns: n bytes, not read for G1 recovery (the even root); out: n x OW words, (x, y) for the recovery kinds and
// the root alone for the sqrt kinds, zero words where there is no root; flags: n bytes, "the base's Legendre symbol is 1";
// root_ok: n bytes, sqrt kinds only, "a root with the wanted sign exists"; jobs: n x 8 words ((p-1)/2 | base)
template <int WHAT>
__global__ __launch_bounds__(G1R_LANES) void k_root(const u64* __restrict__ xs, const unsigned char* __restrict__ sgns, size_t n,
                                                    u64* __restrict__ out, unsigned char* __restrict__ flags,
                                                    unsigned char* __restrict__ root_ok, u64* __restrict__ jobs, int* __restrict__ err) {
  constexpr int IW = (int)root_in_words(WHAT), OW = (int)root_out_words(WHAT), AT = (int)root_at(WHAT), NC = IW / 4;
  using F = root_field<WHAT>;
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  F x, g;
  fq base;
  fe_from_canonical(xs + IW * k, x);
  root_radicand_base<WHAT>(x, g, base);
  const bool zero = root_is_sqrt(WHAT) ? fq_is_zero(base) : false;  // a curve's g(x) and its norm are never zero
  bool root, bad;  // root: c^2 == g, also for g = 0; bad: a self-check of the ladders fails
  F c;             // any root of g, or what squares to -g
  if constexpr (NC == 1) c = fq_root(tab, g, root, bad);  // sqrt_ladder.h; 0 for g = 0
  else c = fq2_root(tab, g, base, root, bad);             // fq2_root.h; root holds and c = (0, 0) for g = 0 (the head of this file)
  if (bad) atomicCAS(err, 0, BN254S_E_INTERNAL);
  const bool want = root_has_sgns(WHAT) ? sgns[k] != 0 : false;
  fqw y[NC];
  signed_words(c, want, y);
  const bool has = zero ? !want : root;  // the one root of 0 has the sign 0
  const fqw bc = fq_to_canonical(base);
#pragma unroll
  for (int w = 0; w < 4; w++) {
#pragma unroll
    for (int j = 0; j < NC; j++) {
      if constexpr (!root_is_sqrt(WHAT)) out[OW * k + 4 * j + w] = xs[IW * k + 4 * j + w];
      out[OW * k + AT + 4 * j + w] = has ? y[j].l[w] : 0;
    }
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = root_base_word<WHAT>(xs + IW * k, bc, w);
  }
  flags[k] = root && !zero ? 1 : 0;
  if constexpr (root_is_sqrt(WHAT)) root_ok[k] = has ? 1 : 0;
}

// what a kind brings to the host front besides its shape: the tag of its texts, the name of its pooled buffer, its self-check
struct RootFront {
  const char *tag, *pool, *self_check;
};
constexpr RootFront ROOT_FRONT[4] = {
    {"g1_recover_from_x", "g1rec", ": g^((p+1)/4) squares to neither g nor -g (device self-check)"},
    {"g2_recover_from_x", "g2rec", ": a square root does not square back (device self-check)"},
    {"fq_sqrt", "fqsqrt", ": x^((p+1)/4) squares to neither x nor -x (device self-check)"},
    {"fq2_sqrt", "fq2sqrt", ": a square root does not square back (device self-check)"},
};

// the arguments that both entry points of a kind share, other than the context (root_ok: sqrt kinds only)
bool root_args_ok(int what, const uint64_t* xs, size_t n, const uint64_t* out, const uint8_t* flags, const uint8_t* root_ok) {
  return xs && out && flags && (root_ok || !root_is_sqrt(what)) && n > 0 && n < ((size_t)1 << 32);
}

// The front-end into host memory: out[n x OW], flags[n], root_ok[n] (sqrt kinds), jobs[n x 8] (jobs may be NULL; sgns may be
// NULL, all zero, and is not looked at for G1 recovery).  Nothing is written on an error.
int root_front(bn254s_ctx* c, int what, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* out, uint8_t* flags,
               uint8_t* root_ok, uint64_t* jobs) {
  if (!c || !root_args_ok(what, xs, n, out, flags, root_ok)) return BN254S_E_INVALID_ARG;
  const RootFront& K = ROOT_FRONT[what];
  const std::string tag = K.tag;
  const size_t IW = root_in_words(what), OW = root_out_words(what);
  const bool sqrt = root_is_sqrt(what), has_sgns = root_has_sgns(what);
  if (!has_sgns) sgns = nullptr;
  // the first input with a coordinate that is not below p or a sign byte above 1 is reported, the coordinates before the sign
  size_t s = 0;
  while (s < n && (!sgns || sgns[s] <= 1)) s++;
  if (!coords_below_p(c, tag, "x", COORD_FQ2, (int)IW / 4, xs, s < n ? s + 1 : n)) return BN254S_E_INVALID_ARG;
  if (s < n) {
    c->set_err(tag + ": sgn_" + std::to_string(s) + " is " + std::to_string(sgns[s]) + ", neither 0 nor 1");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words(K.pool, IW * n /* xs */ + OW * n /* out */ + 8 * n /* jobs */ + 1 /* err */ +
                                ((size_t)1 + sqrt + has_sgns) * nb /* flags, root_ok, sgns */);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d;
  u64* d_out = d_xs + IW * n;
  u64* d_jobs = d_out + OW * n;
  int* d_err = (int*)(d_jobs + 8 * n);
  unsigned char* d_flags = (unsigned char*)(d_jobs + 8 * n + 1);
  unsigned char* d_ok = sqrt ? d_flags + 8 * nb : nullptr;
  unsigned char* d_sgns = has_sgns ? d_flags + 8 * nb * (1 + sqrt) : nullptr;
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * IW * 8, hipMemcpyHostToDevice, st));
  if (sgns)
    HIP_TRY(c, hipMemcpyAsync(d_sgns, sgns, n, hipMemcpyHostToDevice, st));
  else if (has_sgns)
    HIP_TRY(c, hipMemsetAsync(d_sgns, 0, n, st));
  const unsigned blocks = (unsigned)((n + G1R_LANES - 1) / G1R_LANES);
  switch (what) {
    case ROOT_G1_RECOVER: k_root<ROOT_G1_RECOVER><<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_out, d_flags, d_ok, d_jobs, d_err); break;
    case ROOT_G2_RECOVER: k_root<ROOT_G2_RECOVER><<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_out, d_flags, d_ok, d_jobs, d_err); break;
    case ROOT_FQ_SQRT: k_root<ROOT_FQ_SQRT><<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_out, d_flags, d_ok, d_jobs, d_err); break;
    default: k_root<ROOT_FQ2_SQRT><<<blocks, G1R_LANES, 0, st>>>(d_xs, d_sgns, n, d_out, d_flags, d_ok, d_jobs, d_err); break;
  }
  HIP_TRY(c, hipGetLastError());
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err(tag + K.self_check);
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(out, d_out, n * OW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, st));
  if (sqrt) HIP_TRY(c, hipMemcpyAsync(root_ok, d_ok, n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

// The proven form: the front-end into buffers of its own, the Fq-exp proofs of the n jobs, the linkage of every proven symbol to
// its flag (prove_legendre; three-valued for the sqrt kinds, whose bases may be zero: 1 | p - 1 | 0 for a square, a non-square, a
// zero base); the caller's arrays are written on success only.
int root_proven(bn254s_ctx* c, int what, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                size_t per_proof, uint64_t* out, uint8_t* flags_out, uint8_t* root_ok_out, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  const char* tag = ROOT_FRONT[what].tag;
  int rc = proven_args(c, tag, "Fq-exp proof", root_args_ok(what, xs, n, out, flags_out, root_ok_out), params, fq_proofs, n, per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<u64> rows(root_out_words(what) * n), jobs(8 * n);
  std::vector<uint8_t> flags(n), ok(n);
  rc = root_front(c, what, xs, sgns, n, rows.data(), flags.data(), ok.data(), jobs.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_legendre(c, tag, params, jobs, flags.data(), n, per_proof, fq_proofs, /*zero_bases=*/root_is_sqrt(what));
  if (rc != BN254S_OK) return rc;
  memcpy(out, rows.data(), rows.size() * 8);
  memcpy(flags_out, flags.data(), n);
  if (root_ok_out) memcpy(root_ok_out, ok.data(), n);
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g1_recover_from_x_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* points_out, uint8_t* flags_out,
                                              uint64_t* fq_jobs) {
  return root_front(c, ROOT_G1_RECOVER, xs, nullptr, n, points_out, flags_out, nullptr, fq_jobs);
}
extern "C" int bn254s_g2_recover_from_x_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* points_out,
                                              uint8_t* flags_out, uint64_t* fq_jobs) {
  return root_front(c, ROOT_G2_RECOVER, xs, sgns, n, points_out, flags_out, nullptr, fq_jobs);
}
extern "C" int bn254s_fq_sqrt_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots_out,
                                    uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs) {
  return root_front(c, ROOT_FQ_SQRT, xs, sgns, n, roots_out, square_out, root_ok_out, fq_jobs);
}
extern "C" int bn254s_fq2_sqrt_batch(bn254s_ctx* c, const uint64_t* xs, const uint8_t* sgns, size_t n, uint64_t* roots_out,
                                     uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs) {
  return root_front(c, ROOT_FQ2_SQRT, xs, sgns, n, roots_out, square_out, root_ok_out, fq_jobs);
}
extern "C" int bn254s_g1_recover_from_x(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, size_t n, size_t per_proof,
                                        uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  return root_proven(c, ROOT_G1_RECOVER, params, xs, nullptr, n, per_proof, points_out, flags_out, nullptr, fq_jobs, fq_proofs);
}
extern "C" int bn254s_g2_recover_from_x(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                                        size_t per_proof, uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs,
                                        bn254s_proof** fq_proofs) {
  return root_proven(c, ROOT_G2_RECOVER, params, xs, sgns, n, per_proof, points_out, flags_out, nullptr, fq_jobs, fq_proofs);
}
extern "C" int bn254s_fq_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                              size_t per_proof, uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs,
                              bn254s_proof** fq_proofs) {
  return root_proven(c, ROOT_FQ_SQRT, params, xs, sgns, n, per_proof, roots_out, square_out, root_ok_out, fq_jobs, fq_proofs);
}
extern "C" int bn254s_fq2_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                               size_t per_proof, uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs,
                               bn254s_proof** fq_proofs) {
  return root_proven(c, ROOT_FQ2_SQRT, params, xs, sgns, n, per_proof, roots_out, square_out, root_ok_out, fq_jobs, fq_proofs);
}
