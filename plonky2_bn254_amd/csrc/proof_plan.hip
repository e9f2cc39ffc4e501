// proof_plan(): the host arithmetic in front of a proof (proof_plan.h), and the debug entry point that shows it to a test.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "proof_plan.h"
#include "merkle.h"
#include "prover.h"

static bool env_flag(const char* name) { return getenv(name) && atoi(getenv(name)); }
PlanOverrides plan_overrides_from_env() {
  PlanOverrides ov;
  ov.force_split = env_flag("BN254S_FORCE_SPLIT");
  ov.force_lowmem = env_flag("BN254S_FORCE_LOWMEM");
  ov.force_stream = env_flag("BN254S_FORCE_STREAM");
  if (const char* e = getenv("BN254S_STREAM_WIN_LOG")) ov.stream_win_log = atoi(e) < 0 ? 99 : atoi(e);  // (clamped by the plan)
  return ov;
}

size_t rows_for(size_t n, uint32_t min_rows_log2) {
  size_t r = std::max((size_t)1 << min_rows_log2, n * 512), p = 1;
  while (p < r) p <<= 1;
  return p;
}

int proof_plan(int kind, size_t n, const bn254s_params& P, size_t dev_total_bytes, const PlanOverrides& ov, ProofPlan& pl,
               std::string& err) {
  const StarkKind& sk = stark_kind(kind);
  pl.kind = kind;
  pl.n = n;
  pl.P = P;
  const StarkShape& sh = pl.sh = sk.shape;
  const int W = pl.W = sh.W, A = pl.A = sh.n_aux(), K = pl.K = sh.n_total_constraints(), PW = pl.PW = sk.point_words;
  const int NQ = ProofPlan::NQ, CH = ProofPlan::CH;
  const size_t N = pl.N = rows_for(n, P.min_rows_log2);
  unsigned log_n = 0;
  while (((size_t)1 << log_n) < N) log_n++;
  pl.log_n = log_n;
  if (log_n < 16 || log_n > 23) {
    err = "supported trace heights: 2^16 .. 2^23 rows (up to 16384 instances in one proof)";
    return BN254S_E_UNSUPPORTED;
  }
  if (P.num_challenges != 2 || P.rate_bits != 1 || P.cap_height != 4 || P.arity_bits != 4 || P.min_rows_log2 < 16 ||
      P.pow_bits == 0 || P.pow_bits > 32 || P.num_queries == 0 || P.num_queries > 256) {
    err = "unsupported StarkConfig (only standard_fast_config shapes)";
    return BN254S_E_UNSUPPORTED;
  }
  // 2^23 rows: one radix-2 level above the tall transforms (ntt.hip), and the workspace is laid out to fit one GPU: the NTT
  // stage runs in column chunks (its scratch is a chunk, not a commitment), the auxiliary coefficients overwrite their values,
  // and the trace values are released before the auxiliary LDE is allocated.  BN254S_FORCE_SPLIT=1 takes
  // the same path from 2^18 rows on (tests: word-for-word against the oracle at 2^18).
  const unsigned log_s = pl.log_s = (log_n == 23 || (ov.force_split && log_n >= 18)) ? 1 : 0;
  const unsigned log_m2 = pl.log_m2 = log_n + 1, log_r = pl.log_r = log_n - 16 - log_s;
  const size_t R = pl.R = (size_t)1 << log_r;
  const size_t M2 = pl.M2 = 2 * N;
  pl.NH = N >> log_s;             // NH: words of one half (= N without the extra level)
  const int NSPL = pl.NSPL = 1 << log_s;  // coefficient arrays hold NSPL halves per polynomial
  // The compact workspace (NTT stage in column chunks, auxiliary commitment in place, auxiliary LDE in the memory of the dead
  // trace values) is used whenever the plain layout would not fit: 2^23 rows, and G2 from 2^22 rows on (339 GB plain, 211 GB
  // compact).  BN254S_FORCE_LOWMEM=1 selects it for any tall proof (tests).
  const double plain_bytes = 8.0 * (double)N * (4.0 * sh.W + 4.0 * sh.n_aux() + std::max(sh.W, sh.n_aux()));
  // "stream": even the compact workspace does not fit (G2 at 2^23 rows: its two LDEs alone are 296 GB).  Only the coefficients
  // stay resident; a commitment streams 16-column chunks through the NTT into a leaf hash that absorbs into resident sponge
  // states, and wherever LDE rows are needed they are recomputed from the coefficients: the quotient runs over windows of
  // consecutive rows of a coset (natural order, QArgs window mode), the FRI batch polynomial is formed on the coefficient
  // vectors (it is linear in them) and extended once, the query rows are gathered from one more pass of chunk LDEs.
  // BN254S_FORCE_STREAM=1 takes this path for any proof above 2^16 rows (tests: word for word against the oracle at 2^17 / 2^18);
  // BN254S_STREAM_WIN_LOG = log2 of the rows per window (default: at most 2^22, at least two windows per coset).
  const double compact_bytes = 8.0 * ((double)std::max((size_t)sh.W * N, (size_t)sh.n_aux() * 2 * N) + (double)sh.W * N * 3.0 + (double)sh.n_aux() * N);
  const bool stream = pl.stream =
      log_n > 16 && (ov.force_stream || (dev_total_bytes > 0 && compact_bytes + 20e9 > (double)dev_total_bytes));
  const bool lowmem = pl.lowmem = stream || log_s || (log_n > 16 && (ov.force_lowmem || plain_bytes > 200e9));
  pl.log_bk = std::min(22u, log_n - 1);
  if (ov.stream_win_log >= 0) pl.log_bk = std::min(log_n, std::max(8u, (unsigned)ov.stream_win_log));
  pl.BK = (size_t)1 << pl.log_bk;
  const size_t WROWS = pl.WROWS = pl.BK + 1;  // rows per quotient window (+ the next row of the last one)
  const std::vector<int> arities = fri_arities(P, log_n);
  const int L = pl.L = (int)arities.size();
  if (L > FRI_MAX_LAYERS) return BN254S_E_UNSUPPORTED;
  std::copy(arities.begin(), arities.end(), pl.arities);

  // ---- buffers ----------------------------------------------------------------------------------------------
  PlanBuffers& b = pl.words = PlanBuffers{};
  pl.in_words = n * (4 + 2 * (size_t)PW);
  b.in = pl.in_words + 16;
  // compact workspace: the trace values are dead once the auxiliary values exist, the auxiliary LDE takes their place
  b.tvals = lowmem && !stream ? std::max((size_t)W * N, (size_t)A * M2) : (size_t)W * N;
  b.tcoef = (size_t)W * N;
  b.hist = 65536 / 2;
  b.tmp = pl.ntt_tmp_words(std::max(W, A));
  b.ldechunk = stream ? (size_t)CH * M2 : 0;  // the LDE of one column chunk
  b.sponge = stream ? (size_t)12 * M2 : 0;    // sponge states of the streaming leaf hash
  b.comb = (size_t)6 * N + (size_t)6 * M2;    // FRI batch polynomial: coefficients | LDE
  b.tlde = stream ? 0 : (size_t)W * M2;
  pl.tree_words = merkle_tree_digests(log_m2, P.cap_height) * 4;
  b.trees = 3 * pl.tree_words;
  b.avals = (size_t)A * N;
  b.acoef = lowmem ? 0 : (size_t)A * N;  // compact workspace: the commitment runs in place
  b.alde = lowmem ? 0 : (size_t)A * M2;  // (stream: the chunk buffer; compact: the memory of the trace values)
  b.scratch = std::max(sk.trace_scratch_words(n), aux_scratch_words(sh, N));
  b.quot = (size_t)(3 * NQ) * N + (size_t)NQ * M2 + (size_t)QUOTIENT_MAX_PARTS * 2 * (stream ? WROWS : M2);  // qv, ab, qcoef, qlde, partials
  b.tabs = QUOTIENT_W_WORDS(K) + QUOTIENT_MZT_WORDS + 4 * (size_t)(W + A + NQ);  // W, mzt, apow (8 u32 per power)
  b.open = std::max((size_t)(W + A + NQ) * NSPL * R * 5 + FRI_OPENING_TABLE_WORDS, n * (size_t)PW);
  // FRI layer values (extension, 2 words) and trees
  pl.fri_words = pl.fri_tree_words = 0;
  {
    size_t m = M2;
    for (int l = 0; l <= L; l++) {
      pl.fri_words += 2 * m;
      if (l < L) pl.fri_tree_words += merkle_tree_digests((int)log_m2 - 4 * (l + 1), P.cap_height) * 4;
      m >>= 4;
    }
  }
  b.fri = pl.fri_words;
  b.fritrees = pl.fri_tree_words;
  // per-query proof words
  pl.wpq = (size_t)(W + A + NQ) + 3 * 4 * (log_m2 - P.cap_height);
  {
    int lg = log_m2;
    for (int l = 0; l < L; l++) {
      lg -= arities[l];
      pl.wpq += 32 + 4 * (lg - P.cap_height);
    }
  }
  b.qout = pl.n_q() + 64;
  // stream: all columns x WROWS rows of a quotient window, the window's point tables and the leaf rows of the queries
  b.win = stream ? (size_t)(W + A) * WROWS + 3 * WROWS + (size_t)(W + A) * P.num_queries : 0;
  pl.pinned_bytes = std::max(pl.n_part(), pl.n_q()) * 8;
  return BN254S_OK;
}

extern "C" int bn254s_selftest_proof_plan(int kind, size_t n, const bn254s_params* params, uint64_t dev_total_bytes, int force_split,
                                          int force_lowmem, int force_stream, int stream_win_log, uint64_t* out, char* err,
                                          size_t err_len) {
  if (kind < 0 || kind > 2 || n == 0 || !params || params->struct_size != sizeof(bn254s_params) || !out) return BN254S_E_INVALID_ARG;
  PlanOverrides ov;
  ov.force_split = force_split != 0;
  ov.force_lowmem = force_lowmem != 0;
  ov.force_stream = force_stream != 0;
  ov.stream_win_log = stream_win_log;
  ProofPlan pl;
  std::string msg;
  const int rc = proof_plan(kind, n, *params, (size_t)dev_total_bytes, ov, pl, msg);
  if (err && err_len) {
    strncpy(err, msg.c_str(), err_len - 1);
    err[err_len - 1] = 0;
  }
  if (rc != BN254S_OK) return rc;
  const PlanBuffers& b = pl.words;
  const uint64_t head[] = {(uint64_t)pl.kind, pl.n, (uint64_t)pl.W, (uint64_t)pl.A, (uint64_t)pl.K, (uint64_t)pl.PW, pl.N, pl.log_n, pl.log_s,
                           pl.log_r, pl.R, pl.NH, (uint64_t)pl.NSPL, pl.stream, pl.lowmem, pl.log_bk, pl.BK, pl.WROWS, (uint64_t)pl.L};
  const uint64_t tail[] = {pl.wpq, pl.tree_words, pl.fri_words, pl.fri_tree_words, pl.in_words,
                           b.in, b.tvals, b.tcoef, b.hist, b.tmp, b.ldechunk, b.sponge, b.comb, b.tlde, b.trees, b.avals, b.acoef,
                           b.alde, b.scratch, b.quot, b.tabs, b.open, b.fri, b.fritrees, b.qout, b.win, pl.pinned_bytes};
  static_assert(sizeof(head) / 8 + FRI_MAX_LAYERS + sizeof(tail) / 8 == BN254S_PLAN_WORDS, "bn254s_selftest_proof_plan layout");
  for (uint64_t v : head) *out++ = v;
  for (int l = 0; l < FRI_MAX_LAYERS; l++) *out++ = (uint64_t)pl.arities[l];
  for (uint64_t v : tail) *out++ = v;
  return BN254S_OK;
}
