// The one description of a root kind: what the kernels that make a root (k_root of root_front.hip, k_m2g1_point of map_to_g1.hip)
// and the kernel that checks one (k_root_links of root_links.hip) must agree on, so that neither can be edited alone.
//   the kinds and their shapes: words of an input, words of a row of points / roots, where the root starts in it, jobs per
//     input, "is a sqrt kind", "takes sign bytes"
//   curve_rhs: x^3 + b on G1 and on the twist
//   root_radicand_base / root_base_word[s]: what the root is taken of and what the Legendre job exponentiates, for the four
//     one-job kinds
//   m2g1_candidates: the SvdW candidates x1, x2, x3 of map_to_g1
// and, host code, the linkage of Legendre jobs to their flags: legendre_output is the output that a flag demands, prove_legendre
// compares the proven outputs against it and verify_roots (root_links.hip) fills the claimed outputs from it.
#pragma once
#include <type_traits>
#include "fq2_root.h"  // fq_select, fq_from_limbs, the constants of the twist
#include "map_to_g1_constants.inc"
#include "proven_jobs.h"

namespace {

// the values of `what` in bn254s_root_links_check_batch (bn254_stark.h)
enum { ROOT_G1_RECOVER = 0, ROOT_G2_RECOVER = 1, ROOT_FQ_SQRT = 2, ROOT_FQ2_SQRT = 3, ROOT_MAP_TO_G1 = 4, ROOT_KINDS = 5 };
// words of an input, words of a row of points / roots, the words of such a row before its y / root, jobs per input
constexpr size_t root_in_words(int what) { return what == ROOT_G2_RECOVER || what == ROOT_FQ2_SQRT ? 8 : 4; }
constexpr size_t root_out_words(int what) { return what == ROOT_G2_RECOVER ? 16 : what == ROOT_FQ_SQRT ? 4 : 8; }
constexpr size_t root_at(int what) { return what == ROOT_FQ_SQRT || what == ROOT_FQ2_SQRT ? 0 : what == ROOT_G2_RECOVER ? 8 : 4; }
constexpr size_t root_jobs(int what) { return what == ROOT_MAP_TO_G1 ? 2 : 1; }
// a sqrt kind has no x in its rows, a root_ok beside its flag, and zero among its inputs
constexpr bool root_is_sqrt(int what) { return what == ROOT_FQ_SQRT || what == ROOT_FQ2_SQRT; }
// the wanted sign is an argument (G1 recovery takes the even root, map_to_g1 the parity of u)
constexpr bool root_has_sgns(int what) { return what != ROOT_G1_RECOVER && what != ROOT_MAP_TO_G1; }
template <int WHAT>
using root_field = std::conditional_t<root_in_words(WHAT) == 8, fq2, fq>;

// x^3 + b on G1 and on the twist
__device__ __forceinline__ fq curve_rhs(const fq& x) {
  const fq one = fq_one();
  return fq_add(fq_mul(fq_sqr(x), x), fq_add(fq_dbl(one), one));
}
__device__ __forceinline__ fq2 curve_rhs(const fq2& x) {
  fq2 b;
  b.c0 = fq_from_limbs(G2R_B_C0);
  b.c1 = fq_from_limbs(G2R_B_C1);
  return fq2_add(fq2_mul(fq2_sqr(x), x), b);
}

// Input x of a one-job kind: the radicand, whose root is made or checked, and the base of its Legendre job - the radicand over
// Fq, its norm over Fq2 (a square in Fq2 iff its norm is one in Fq).
template <int WHAT>
__device__ __forceinline__ void root_radicand_base(const root_field<WHAT>& x, root_field<WHAT>& radicand, fq& base) {
  static_assert(WHAT != ROOT_MAP_TO_G1, "two jobs per input: m2g1_candidates and curve_rhs");
  if constexpr (root_is_sqrt(WHAT)) radicand = x;
  else radicand = curve_rhs(x);
  if constexpr (root_in_words(WHAT) == 8) base = fq2_norm(radicand);
  else base = radicand;
}
// Word w of the job's base, canonical: of fq_to_canonical(base), or for fq_sqrt of the input words xw themselves, which are
// canonical already.  Word by word, so that a kernel that only stores them loads each where it stores it.
template <int WHAT>
__device__ __forceinline__ u64 root_base_word(const u64* __restrict__ xw, const fqw& canonical, int w) {
  return WHAT == ROOT_FQ_SQRT ? xw[w] : canonical.l[w];
}
template <int WHAT>
__device__ __forceinline__ fqw root_base_words(const u64* __restrict__ xw, const fq& base) {
  const fqw canonical = fq_to_canonical(base);  // unused, and dropped, for fq_sqrt
  fqw r;
#pragma unroll
  for (int w = 0; w < 4; w++) r.l[w] = root_base_word<WHAT>(xw, canonical, w);
  return r;
}

// The candidates of map_to_g1 for one input u (the head of map_to_g1.hip): shared by the kernel that makes the point and the one
// that checks it, so that the two cannot diverge - also not at u = +-1/2, where tv1 tv2 = 0 and tv3 is 0 by the select, whatever
// fq_inv makes of 0.
__device__ __forceinline__ void m2g1_candidates(const fq& u, fq& x1, fq& x2, fq& x3) {
  const fq one = fq_one();
  fq tv1 = fq_dbl(fq_dbl(fq_sqr(u)));  // u^2 g(Z), g(Z) = 4
  const fq tv2 = fq_add(one, tv1);
  tv1 = fq_sub(one, tv1);
  const fq prod = fq_mul(tv1, tv2);  // zero only for u = +-1/2 (-1 is no square); fq_inv gives 0 there, the select says so
  const fq tv3 = fq_select(fq_is_zero(prod), fq_zero(), fq_inv(prod));
  const fq tv5 = fq_mul(fq_mul(fq_mul(u, tv1), tv3), fq_from_limbs(M2G1_TV4));
  const fq nz2 = fq_from_limbs(M2G1_NEG_Z_BY_2);
  x1 = fq_sub(nz2, tv5);
  x2 = fq_add(nz2, tv5);
  const fq t = fq_mul(fq_sqr(tv2), tv3);
  x3 = fq_add(one, fq_mul(fq_from_limbs(M2G1_TV6), fq_sqr(t)));
}

// The output base^((p-1)/2) that a flag demands of a Legendre job, as four words: 1 where the flag is set; where it is clear,
// p - 1, or 0 for a zero base (the symbol of 0 is 0: sqrt kinds only, a curve equation's bases never are zero).
inline const u64* legendre_output(bool flag, bool zero_base) {
  static const u64 ONE[4] = {1, 0, 0, 0}, ZERO[4] = {0, 0, 0, 0}, PM1[4] = {G1R_P[0] - 1, G1R_P[1], G1R_P[2], G1R_P[3]};  // p is odd
  return flag ? ONE : zero_base ? ZERO : PM1;
}
inline bool words_are_zero(const u64* w) { return (w[0] | w[1] | w[2] | w[3]) == 0; }

// Proves the n Legendre jobs (8 words each: (p-1)/2 | base) as Fq-exp proofs and checks every proven output against its flag:
// the trace generator computes base_i^((p-1)/2) on its own; it must be what legendre_output says.
// zero_bases: the bases may be zero (the sqrt kinds; a curve equation's never are), and the rule is three-valued.
// fq_proofs: ceil(n / per_proof) slots; on any error every proof is freed and its slot is NULL.
inline int prove_legendre(bn254s_ctx* c, const std::string& tag, const bn254s_params* params, const std::vector<u64>& jobs,
                          const uint8_t* flags, size_t n, size_t per_proof, bn254s_proof** fq_proofs, bool zero_bases = false) {
  std::vector<u64> s(4 * n), g(4 * n), outs;
  for (size_t i = 0; i < n; i++) {
    memcpy(s.data() + 4 * i, jobs.data() + 8 * i, 32);
    memcpy(g.data() + 4 * i, jobs.data() + 8 * i + 4, 32);
  }
  int rc = prove_and_collect(c, tag, 2, params, s.data(), g.data(), nullptr, n, per_proof, fq_proofs, outs);
  if (rc != BN254S_OK) return rc;
  for (size_t i = 0; i < n; i++) {
    const bool zero = zero_bases && words_are_zero(g.data() + 4 * i);
    if (memcmp(outs.data() + 4 * i, legendre_output(flags[i], zero), 32) != 0) {
      c->set_err(tag + ": the proven Legendre symbol of input " + std::to_string(i) + " is not " +
                 (flags[i] ? "1, but its flag is set" : zero ? "0, but its base is zero" : "p - 1, but its flag is clear"));
      release_proofs(fq_proofs, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  }
  return BN254S_OK;
}

}  // namespace
