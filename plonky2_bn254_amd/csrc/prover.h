// Host-side pieces shared by the prover (prover.hip), its plan (proof_plan.hip) and the native verifier (verify.hip).
#pragma once
#include <vector>
#include "aux.h"
#include "layout.h"
#include "quotient.h"

// What differs between the three STARKs (kind = KIND_G1 / KIND_G2 / KIND_FQ), in one table.
struct StarkKind {
  StarkShape shape;  // Stark::lookups, looked CTL tables and constraint counts of the AIR
  int point_words;   // words per input point: 8 (G1), 16 (G2), 4 (Fq element)
  bool has_offset;   // the jobs carry an offset point (not Fq-exp)
  size_t (*trace_scratch_words)(size_t n);
  // device pointers; trace column-major [W][N]; outputs n x point_words canonical words (d_off is ignored without has_offset)
  int (*generate_trace)(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N, u64* d_scratch,
                        u64* d_outputs, int* d_err, hipStream_t st, bool with_range);
  int (*mz_blocks)(const int** e0);  // first constraint indices of the eval_modulus_zero blocks (for quotient_host_tables)
  void (*quotient_launch)(const QArgs& A, const StarkShape& sh, hipStream_t st);
};
const StarkKind& stark_kind(int kind);
// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits) for a polynomial of 2^degree_bits coefficients
std::vector<int> fri_arities(const bn254s_params& P, int degree_bits);
