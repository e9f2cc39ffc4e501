// Host half that the point-recovery entry points share (g1_recover.hip, g2_recover.hip): the range check of a coordinate and
// the Fq-exp proofs of the Legendre jobs with their linkage to the flags.
#pragma once
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "../../include/bn254_stark.h"
#include "sqrt_ladder.h"  // (g1_recover_constants.inc: p)

namespace {

constexpr size_t G1R_PER_PROOF_MAX = 16384;  // 2^23 rows: the largest Fq-exp proof (bn254s_prove_batch)

// four canonical words below p
inline bool recover_below_p(const uint64_t* w) {
  for (int j = 3; j >= 0; j--)
    if (w[j] != G1R_P[j]) return w[j] < G1R_P[j];
  return false;
}

// Proves the n Legendre jobs (8 words each: (p-1)/2 | base) with bn254s_prove_batch(kind 2), cut by per_proof, and checks every
// proven output against its flag.  fq_proofs: ceil(n / per_proof) slots, all NULL on entry; on any error every proof is freed
// and its slot is NULL again.  `tag` starts the error texts.
inline int recover_prove_legendre(bn254s_ctx* c, const char* tag, const bn254s_params* params, const std::vector<u64>& jobs,
                                  const uint8_t* flags, size_t n, size_t per_proof, bn254s_proof** fq_proofs) {
  const std::string who = std::string(tag) + ": ";
  const size_t n_proofs = (n + per_proof - 1) / per_proof;
  std::vector<u64> s(4 * n), g(4 * n);
  for (size_t i = 0; i < n; i++) {
    memcpy(s.data() + 4 * i, jobs.data() + 8 * i, 32);
    memcpy(g.data() + 4 * i, jobs.data() + 8 * i + 4, 32);
  }
  int rc = bn254s_prove_batch(c, 2, params, s.data(), g.data(), nullptr, n, per_proof, fq_proofs);
  if (rc != BN254S_OK) return rc;  // (the batch has freed its proofs)
  // linkage: the trace generator computes base_i^((p-1)/2) on its own; it must be 1 where the flag is set and p - 1 where it is not
  u64 pm1[4];
  memcpy(pm1, G1R_P, 32);
  pm1[0] -= 1;
  static const u64 ONE[4] = {1, 0, 0, 0};
  size_t pos = 0;
  for (size_t i = 0; i < n_proofs && rc == BN254S_OK; i++) {
    const uint64_t* o;
    size_t len = 0;
    const size_t cnt = n - pos < per_proof ? n - pos : per_proof;
    if (bn254s_proof_outputs(fq_proofs[i], &o, &len) != BN254S_OK || len != 4 * cnt) {
      c->set_err(who + "proof " + std::to_string(i) + " has " + std::to_string(len / 4) + " outputs, expected " + std::to_string(cnt));
      rc = BN254S_E_INTERNAL;
    }
    for (size_t j = 0; j < cnt && rc == BN254S_OK; j++) {
      if (memcmp(o + 4 * j, flags[pos + j] ? ONE : pm1, 32) != 0) {
        c->set_err(who + "the proven Legendre symbol of input " + std::to_string(pos + j) + " is not " +
                   (flags[pos + j] ? "1, but its flag is set" : "p - 1, but its flag is clear"));
        rc = BN254S_E_INTERNAL;
      }
    }
    pos += cnt;
  }
  if (rc != BN254S_OK) {
    for (size_t i = 0; i < n_proofs; i++) {
      bn254s_proof_free(fq_proofs[i]);
      fq_proofs[i] = nullptr;
    }
  }
  return rc;
}

}  // namespace
