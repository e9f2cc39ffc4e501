// The transforms of the provers' stages: shared by prover.hip (the stages) and ntt_selftest.hip (bn254s_selftest_transforms runs
// these members on caller data).
#pragma once
#include <algorithm>
#include "ctx.h"
#include "merkle.h"
#include "proof_plan.h"

// iNTT / LDE / coset iNTT of a proof's columns on the plan of its height (ntt.h: the decomposition and the scratch layout are
// decided there).  What is decided here is the chunking: the compact and the streaming workspace work in chunks of CH columns,
// whose scratch `tmp` (ProofPlan::ntt_tmp_words) is sized for.
struct Transforms {
  static constexpr int CH = ProofPlan::CH;
  const NttPlan& np;
  hipStream_t st;
  const ProofPlan& pl;  // N, M2, log_m2, log_s, lowmem
  u64 *tmp, *ldechunk, *sponge;

  // from_values of a whole commitment; in chunks in the compact workspace (which every split height has)
  void commit_ntt(const u64* vals, u64* coef, u64* lde, int nc) const {
    const size_t N = pl.N, M2 = pl.M2;
    const int step = pl.lowmem ? CH : nc;
    for (int c0 = 0; c0 < nc; c0 += step) {
      const int cn = std::min(step, nc - c0);
      ntt_commit(np, vals + (size_t)c0 * N, coef + (size_t)c0 * N, lde + (size_t)c0 * M2, M2, tmp, cn, st);
    }
  }
  // in chunks only under the split level (the provers give a tall transform in the compact workspace at most 6 columns)
  void lde(const u64* coef, u64* out, int nc) const {
    const size_t N = pl.N, M2 = pl.M2;
    const int step = pl.log_s ? CH : nc;
    for (int c0 = 0; c0 < nc; c0 += step) {
      const int cn = std::min(step, nc - c0);
      ntt_lde(np, coef + (size_t)c0 * N, out + (size_t)c0 * M2, M2, tmp, cn, st);
    }
  }
  // stream mode: the LDE of ONE column chunk (coefficients at `coef`, cn <= CH columns) into ldechunk
  // (coset_mask: 1 / 2 = only coset 0 / 1 of the output, 3 = both)
  void lde_chunk(const u64* coef, int cn, int coset_mask = 3) const { ntt_lde(np, coef, ldechunk, pl.M2, tmp, cn, st, coset_mask); }
  // stream mode: one pass of chunk LDEs over the nc columns at `coef`; use(c0, cn) takes what it needs out of ldechunk
  template <class F>
  void for_lde_chunks(const u64* coef, int nc, int coset_mask, F use) const {
    for (int c0 = 0; c0 < nc; c0 += CH) {
      const int cn = std::min(CH, nc - c0);
      lde_chunk(coef + (size_t)c0 * pl.N, cn, coset_mask);
      use(c0, cn);
    }
  }
  // stream mode: from_values of a commitment, chunk by chunk: coefficients stay, the chunk's LDE is absorbed by the leaf hash
  void commit_stream(const u64* vals, u64* coef, int nc, u64* tree) const {
    const size_t N = pl.N, M2 = pl.M2;
    for (int c0 = 0; c0 < nc; c0 += CH) {
      const int cn = std::min(CH, nc - c0);
      ntt_commit(np, vals + (size_t)c0 * N, coef + (size_t)c0 * N, ldechunk, M2, tmp, cn, st);
      merkle_absorb(ldechunk, M2, cn, (int)pl.log_m2, sponge, c0 == 0, c0 + cn == nc ? tree : nullptr, st);
    }
  }
  // quotient values qv[2 alphas][2 cosets][N] (natural order on each coset) -> their coset interpolants ab, same layout
  void quotient_coset_inverse(const u64* qv, u64* ab) const {
    const size_t N = pl.N;
    for (int a = 0; a < 2; a++)
      for (int h = 0; h < 2; h++) ntt_coset_inverse(np, h, qv + (size_t)(a * 2 + h) * N, ab + (size_t)(a * 2 + h) * N, tmp, 1, st);
  }
};
