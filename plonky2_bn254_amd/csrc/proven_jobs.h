// Host half of the proven front-ends (msm.hip, job_outputs.hip, job_check.hip, scalar_mul.hip, root_front.hip, g2_subgroup.hip, g2_cofactor.hip,
// map_to_g1.hip, map_to_g2.hip, field_gadgets.hip): the range check of coordinates, the argument ladder of the full calls, "prove the jobs and collect
// their outputs" and the release of the proofs on an error (the linkage of Legendre jobs to their flags: root_kinds.h); and of the statement
// verifiers (point_sum.hip, root_links.hip): their shared argument predicate verifier_args_ok and verify_proof_runs,
// "bn254s_verify_batch once per run of consecutive proofs of one height and size, every verdict kept".  Host code only.
// A front-end brings its kernel, its own pointer / n predicate and its linkage rule: a flat loop over the collected outputs
// that calls release_proofs when it fails.
#pragma once
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "../../include/bn254_stark.h"
#include "g1_recover_constants.inc"  // p

namespace {

constexpr size_t PER_PROOF_MAX = 16384;  // 2^23 rows, the largest proof of every kind (bn254s_prove_batch)

// four canonical words below p
inline bool fq_below_p(const uint64_t* w) {
  for (int j = 3; j >= 0; j--)
    if (w[j] != G1R_P[j]) return w[j] < G1R_P[j];
  return false;
}

// the names of the coordinates of an Fq2 element and of a G1 / G2 point, four words each
constexpr const char* const COORD_FQ2[2] = {"c0", "c1"};
constexpr const char* const COORD_G1[2] = {"x", "y"};
constexpr const char* const COORD_G2[4] = {"x.c0", "x.c1", "y.c0", "y.c1"};

// w: n items of ncoord coordinates.  The first coordinate that is not below p names itself in the context's error text,
// "<tag>: <name>_<i> has <coord> not below p" ("<tag>: <name>_<i> is not below p" for ncoord == 1); true if all are fine.
// c == nullptr (the shape checks of a call without a context): the same answer without a text.
inline bool coords_below_p(bn254s_ctx* c, const std::string& tag, const char* name, const char* const* coord, int ncoord,
                           const uint64_t* w, size_t n) {
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < ncoord; k++)
      if (!fq_below_p(w + 4 * (ncoord * i + k))) {
        if (c) c->set_err(tag + ": " + name + "_" + std::to_string(i) + (ncoord > 1 ? std::string(" has ") + coord[k] : " is") + " not below p");
        return false;
      }
  return true;
}

// The argument ladder of a full call, every check before device work and the context last, so that the shape checks can be
// exercised without one.  own_ok: the caller's predicate on its own pointers and n.  The ceil(n_jobs / per_proof) slots are NULL
// from the second rung on.  largest: the proof that the limit is named after ("G2 proof").
inline int proven_args(bn254s_ctx* c, const std::string& tag, const char* largest, bool own_ok, const bn254s_params* params,
                       bn254s_proof** proofs, size_t n_jobs, size_t per_proof) {
  if (!own_ok || !params || !proofs || per_proof == 0 || params->struct_size != sizeof(bn254s_params)) return BN254S_E_INVALID_ARG;
  for (size_t i = 0; i < (n_jobs + per_proof - 1) / per_proof; i++) proofs[i] = nullptr;
  if (per_proof > PER_PROOF_MAX) {
    if (c) c->set_err(tag + ": per_proof above 16384 (2^23 rows, the largest " + largest + ")");
    return BN254S_E_UNSUPPORTED;
  }
  return c ? BN254S_OK : BN254S_E_INVALID_ARG;
}

// Frees the ceil(n_jobs / per_proof) proofs and leaves their slots NULL: what every error after the proofs exist does.
inline void release_proofs(bn254s_proof** proofs, size_t n_jobs, size_t per_proof) {
  for (size_t i = 0; i < (n_jobs + per_proof - 1) / per_proof; i++) {
    bn254s_proof_free(proofs[i]);
    proofs[i] = nullptr;
  }
}

// bn254s_prove_batch of the n jobs, cut by per_proof, and the outputs of all proofs one after the other in outs (n x PW words,
// PW = 8 | 16 | 4 for kind 0 | 1 | 2).  On any error no proof is left and every slot is NULL.
inline int prove_and_collect(bn254s_ctx* c, const std::string& tag, int kind, const bn254s_params* params, const uint64_t* scalars,
                             const uint64_t* x, const uint64_t* offset, size_t n, size_t per_proof, bn254s_proof** proofs,
                             std::vector<u64>& outs) {
  const size_t PW = kind == 0 ? 8 : kind == 1 ? 16 : 4, n_proofs = (n + per_proof - 1) / per_proof;
  int rc = bn254s_prove_batch(c, kind, params, scalars, x, offset, n, per_proof, proofs);
  if (rc != BN254S_OK) return rc;  // (the batch has freed its proofs)
  outs.resize(PW * n);
  for (size_t i = 0, pos = 0; i < n_proofs; i++) {
    const uint64_t* o;
    size_t len = 0;
    const size_t cnt = n - pos < per_proof ? n - pos : per_proof;
    if (bn254s_proof_outputs(proofs[i], &o, &len) != BN254S_OK || len != PW * cnt) {
      c->set_err(tag + ": proof " + std::to_string(i) + " has " + std::to_string(len / PW) + " outputs, expected " + std::to_string(cnt));
      release_proofs(proofs, n, per_proof);
      return BN254S_E_INTERNAL;
    }
    memcpy(outs.data() + PW * pos, o, 8 * len);
    pos += cnt;
  }
  return BN254S_OK;
}

// The arguments that the statement verifiers (point_sum.hip, root_links.hip) share, in the order of the header; n: the jobs of
// the call; the context is the caller's last rung.
inline bool verifier_args_ok(int kind, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                             const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, size_t n) {
  if (!params || !words || !n_words || !degree_bits) return false;
  if (n == 0 || n >= (size_t)UINT_MAX || per_proof == 0 || n_proofs != (n + per_proof - 1) / per_proof) return false;
  for (size_t k = 0; k < n_proofs; k++)
    if (!words[k]) return false;
  return true;
}

// bn254s_verify_batch of the proofs, one call per run of consecutive proofs of one height and size, against the jobs
// (scalars, x, offsets, outputs) cut by per_proof; offsets == nullptr for kind 2, which has none.  status [n_proofs]; text:
// "proof k: ..." of the lowest rejected proof, or empty.  Returns BN254S_OK, BN254S_E_VERIFY, or the code of a call that failed
// itself.
inline int verify_proof_runs(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                             const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* scalars,
                             const uint64_t* x, const uint64_t* offsets, const uint64_t* outputs, size_t n, int32_t* status,
                             std::string& text) {
  constexpr size_t STRIDE = 160;
  const size_t PW = kind == 0 ? 8 : kind == 1 ? 16 : 4;
  std::vector<size_t> n_jobs(n_proofs);
  for (size_t k = 0; k < n_proofs; k++) n_jobs[k] = (k + 1) * per_proof <= n ? per_proof : n - k * per_proof;
  std::vector<char> err(n_proofs * STRIDE);
  int ret = BN254S_OK;
  for (size_t lo = 0, hi; lo < n_proofs; lo = hi) {
    for (hi = lo + 1; hi < n_proofs && degree_bits[hi] == degree_bits[lo] && n_words[hi] == n_words[lo];) hi++;
    const size_t j = lo * per_proof;
    const int rc = bn254s_verify_batch(c, kind, params, degree_bits[lo], words + lo, n_words[lo], scalars + 4 * j, x + PW * j,
                                       offsets ? offsets + PW * j : nullptr, outputs + PW * j, n_jobs.data() + lo, hi - lo,
                                       status + lo, err.data() + lo * STRIDE, STRIDE);
    if (rc != BN254S_OK && rc != BN254S_E_VERIFY) return rc;
    if (rc == BN254S_E_VERIFY) ret = rc;
  }
  text.clear();
  for (size_t k = 0; k < n_proofs && text.empty(); k++)
    if (status[k] != BN254S_OK) text = "proof " + std::to_string(k) + ": " + (err.data() + k * STRIDE);
  return ret;
}

}  // namespace
