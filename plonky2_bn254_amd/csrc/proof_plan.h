// The plan of one proof: everything the prover decides before it touches memory - the shape, the transform decomposition, which of
// the three workspace layouts the proof gets, the FRI layers and the word count of every named buffer.  Pure host arithmetic (no HIP
// call): prover.hip acquires the workspace from it (workspace_acquire), bn254s_selftest_proof_plan shows it to a test without a GPU.
#pragma once
#include <string>
#include "aux.h"
#include "fri.h"
#include "ntt.h"

// The test overrides, read from the environment per call by the caller (plan_overrides_from_env):
// BN254S_FORCE_SPLIT / BN254S_FORCE_LOWMEM / BN254S_FORCE_STREAM, and BN254S_STREAM_WIN_LOG (-1: not set).
struct PlanOverrides {
  bool force_split = false, force_lowmem = false, force_stream = false;
  int stream_win_log = -1;
};
PlanOverrides plan_overrides_from_env();

// Word counts of the named buffers of a slot's BufPool, in the order they are allocated.  0: the proof has no buffer of that name
// (in the compact and the streaming workspace several pointers alias another buffer; see workspace_acquire).
struct PlanBuffers {
  size_t in, tvals, tcoef, hist, tmp, ldechunk, sponge, comb, tlde, trees, avals, acoef, alde, scratch, quot, tabs, open, fri,
      fritrees, qout;
  size_t win;  // allocated in the middle of a streaming proof, in the memory of its dead trace values
};

struct ProofPlan {
  static constexpr int NQ = 4, CAPW = 64;  // quotient chunk polynomials; words of a Merkle cap (cap_height 4)
  static constexpr int CH = 16;            // columns per chunk of the chunked / streamed commitment
  int kind = 0;
  size_t n = 0;  // instances
  bn254s_params P;
  StarkShape sh;
  int W = 0, A = 0, K = 0, PW = 0;  // trace / auxiliary width, constraints in all, words per point
  size_t N = 0, M2 = 0;             // rows, LDE points
  unsigned log_n = 0, log_m2 = 0;
  // 2^16-row transforms are the four-step kernels; taller ones add an outer pass over R = 2^log_r blocks; log_s = 1 puts one
  // radix-2 level above that: coefficient arrays then hold NSPL = 2 halves of NH words per polynomial
  unsigned log_s = 0, log_r = 0;
  size_t R = 1, NH = 0;
  int NSPL = 1;
  bool stream = false, lowmem = false;  // streaming workspace (implies lowmem); compact workspace
  unsigned log_bk = 0;
  size_t BK = 0, WROWS = 0;  // stream: rows per quotient window (+ the next row of the last one)
  int L = 0, arities[FRI_MAX_LAYERS] = {0};
  size_t wpq = 0;  // proof words per query round
  size_t tree_words = 0, fri_words = 0, fri_tree_words = 0, in_words = 0;
  PlanBuffers words = {};
  size_t pinned_bytes = 0;  // staging for the two larger device -> host copies (opening partials, query rounds)
  // words of the transforms' scratch for commitments of at most `width` columns (needs log_n, log_s, lowmem): the compact and
  // the streaming workspace transform one chunk of columns at a time
  size_t ntt_tmp_words(int width) const { return ntt_scratch_words(log_n, log_s != 0, lowmem ? CH : width); }
  size_t n_part() const { return (size_t)(W + A + NQ) * NSPL * R * 5; }  // words of the opening partials
  size_t n_q() const { return wpq * P.num_queries; }                     // words of the query rounds
};

// Fills `pl` for a proof of n instances of `kind` on a device of dev_total_bytes of memory (0: unknown - never streams on that
// account).  BN254S_OK, or BN254S_E_UNSUPPORTED with the reason in `err` (none for more FRI layers than FRI_MAX_LAYERS).
int proof_plan(int kind, size_t n, const bn254s_params& P, size_t dev_total_bytes, const PlanOverrides& ov, ProofPlan& pl,
               std::string& err);
size_t rows_for(size_t n, uint32_t min_rows_log2);  // (512 n).next_power_of_two(), at least 2^min_rows_log2
