// The transform dispatch of the provers and the per-height table caches of the context: shared by prover.hip (the stages) and
// ntt_selftest.hip (bn254s_selftest_transforms runs these members on caller data).
#pragma once
#include <algorithm>
#include <mutex>
#include "ctx.h"
#include "merkle.h"
#include "proof_plan.h"

// Per-degree tables of the tall-trace NTT, built on first use.
// `half_of_split`: the tables of the H-point halves under the radix-2 level of ntt.hip (cosets g^2, g^2 w_2H instead of g, g w_2H)
inline const NttTallTables* get_tall_tables(bn254s_ctx* c, unsigned log_n, bool half_of_split = false) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  const unsigned key = log_n + (half_of_split ? 100 : 0);
  auto it = c->tall.find(key);
  if (it != c->tall.end()) return it->second;
  NttTallTables* t = new NttTallTables();
  if (ntt_tall_tables_init(t, log_n, half_of_split ? gl_mul(GL_GEN, GL_GEN) : GL_GEN) != 0) {
    delete t;
    return nullptr;
  }
  c->tall[key] = t;
  return t;
}
inline const NttSplitTables* get_split_tables(bn254s_ctx* c, unsigned log_n) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  auto it = c->split.find(log_n);
  if (it != c->split.end()) return it->second;
  NttSplitTables* t = new NttSplitTables();
  if (ntt_split_tables_init(t, log_n) != 0) {
    delete t;
    return nullptr;
  }
  c->split[log_n] = t;
  return t;
}

// ---- transforms -------------------------------------------------------------------------------------------------
// iNTT / LDE / coset iNTT dispatch: 2^16-row traces use the four-step kernels directly, taller ones add the outer pass, the split
// level one radix-2 level above that; the compact and the streaming workspace work in chunks of CH columns.
struct Transforms {
  static constexpr int CH = ProofPlan::CH;
  bn254s_ctx* c;
  hipStream_t st;
  const NttTallTables* TT;
  const NttSplitTables* SP;
  const ProofPlan& pl;
  u64 *tmp, *ldechunk, *sponge;
  // split level, per chunk: values -> [Pe | Po] (radix-2 level), the tall transform of the 2 CH half columns, halves' LDEs -> LDE
  u64* eo() const { return tmp; }                              // [CH][2][N]
  u64* ntmp() const { return tmp + (size_t)CH * 2 * pl.N; }    // [2 CH][NH]

  // from_values of a whole commitment: the fused four-launch form for 2^16 rows, iNTT then LDE otherwise
  void commit_ntt(const u64* vals, u64* coef, u64* lde, int nc) const {
    const size_t N = pl.N, M2 = pl.M2;
    if (pl.log_s) {
      for (int c0 = 0; c0 < nc; c0 += CH) {
        const int cn = std::min(CH, nc - c0);
        ntt_split_inverse(SP, vals + (size_t)c0 * N, coef + (size_t)c0 * N, cn, st);
        ntt_inverse_lde_tall(&c->ntt, TT, coef + (size_t)c0 * N, coef + (size_t)c0 * N, eo(), ntmp(), 2 * cn, st);
        ntt_split_forward(SP, eo(), lde + (size_t)c0 * M2, M2, cn, st);
      }
    } else if (pl.log_r && pl.lowmem) {
      for (int c0 = 0; c0 < nc; c0 += CH) {
        const int cn = std::min(CH, nc - c0);
        ntt_inverse_lde_tall(&c->ntt, TT, vals + (size_t)c0 * N, coef + (size_t)c0 * N, lde + (size_t)c0 * M2, tmp, cn, st);
      }
    } else if (pl.log_r) {
      ntt_inverse_lde_tall(&c->ntt, TT, vals, coef, lde, tmp, nc, st);
    } else {
      ntt_inverse_lde(&c->ntt, vals, coef, lde, tmp, tmp + (size_t)nc * N, nc, st);
    }
  }
  void lde(const u64* coef, u64* out, int nc) const {
    const size_t N = pl.N, M2 = pl.M2;
    if (pl.log_s) {
      for (int c0 = 0; c0 < nc; c0 += CH) {
        const int cn = std::min(CH, nc - c0);
        ntt_lde_tall(&c->ntt, TT, coef + (size_t)c0 * N, eo(), ntmp(), 2 * cn, st);
        ntt_split_forward(SP, eo(), out + (size_t)c0 * M2, M2, cn, st);
      }
    } else if (pl.log_r) ntt_lde_tall(&c->ntt, TT, coef, out, tmp, nc, st);
    else ntt_lde(&c->ntt, coef, out, tmp, nc, st);
  }
  // stream mode: the LDE of ONE column chunk (coefficients at `coef`, cn <= CH columns) into ldechunk
  // (coset_mask: 1 / 2 = only coset 0 / 1 of the output, 3 = both; under the split level coset h of the N-point domain comes from
  // coset h of both half transforms)
  void lde_chunk(const u64* coef, int cn, int coset_mask = 3) const {
    if (pl.log_s) {
      ntt_lde_tall(&c->ntt, TT, coef, eo(), ntmp(), 2 * cn, st, coset_mask);
      ntt_split_forward(SP, eo(), ldechunk, pl.M2, cn, st, coset_mask);
    } else {
      ntt_lde_tall(&c->ntt, TT, coef, ldechunk, tmp, cn, st, coset_mask);
    }
  }
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
      if (pl.log_s) {
        ntt_split_inverse(SP, vals + (size_t)c0 * N, coef + (size_t)c0 * N, cn, st);
        ntt_inverse_lde_tall(&c->ntt, TT, coef + (size_t)c0 * N, coef + (size_t)c0 * N, eo(), ntmp(), 2 * cn, st);
        ntt_split_forward(SP, eo(), ldechunk, M2, cn, st);
      } else {
        ntt_inverse_lde_tall(&c->ntt, TT, vals + (size_t)c0 * N, coef + (size_t)c0 * N, ldechunk, tmp, cn, st);
      }
      merkle_absorb(ldechunk, M2, cn, (int)pl.log_m2, sponge, c0 == 0, c0 + cn == nc ? tree : nullptr, st);
    }
  }
  // quotient values qv[2 alphas][2 cosets][N] (natural order on each coset) -> their coset interpolants ab, same layout
  void quotient_coset_inverse(const u64* qv, u64* ab) const {
    const size_t N = pl.N;
    for (int a = 0; a < 2; a++)
      for (int h = 0; h < 2; h++)
        if (pl.log_s) ntt_coset_inverse_split(&c->ntt, TT, SP, h, qv + (size_t)(a * 2 + h) * N, ab + (size_t)(a * 2 + h) * N, tmp, 1, st);
        else if (pl.log_r) ntt_coset_inverse_tall(&c->ntt, TT, h, qv + (size_t)(a * 2 + h) * N, ab + (size_t)(a * 2 + h) * N, tmp, 1, st);
        else ntt_coset_inverse(&c->ntt, h, qv + (size_t)(a * 2 + h) * N, ab + (size_t)(a * 2 + h) * N, tmp, 1, st);
  }
};
