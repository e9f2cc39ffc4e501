// Host interface of the Goldilocks NTT / LDE kernels (ntt.hip).
#pragma once
#include <vector>
#include "gl_dev.h"

static constexpr size_t NTT_N = 65536;  // kernel transform size; trace height of one 128-instance proof

struct NttTables {
  u64 *tw256_fwd = nullptr, *tw256_inv = nullptr;  // w_256^e
  u64 *twmat_fwd = nullptr, *twmat_inv = nullptr;  // w_N^(i2*k1) at [k1*256+i2]
  u64* twmat_inv_ninv = nullptr;                   // (1/N) w_N^-(i2*k1)
  u64* coset_pow[2] = {nullptr, nullptr};          // shift_h^i
  u64* coset_inv_pow[2] = {nullptr, nullptr};      // (1/N) shift_h^-k
  u64 n_inv = 0;
};

int ntt_tables_init(NttTables* T);  // frees what it allocated when it fails
void ntt_tables_free(NttTables* T);

// N = R * 2^16 (tall traces): the tables of the outer pass over the R blocks of a column
struct NttTallTables {
  unsigned log_n = 0;
  u64* wn_inv_pow = nullptr;              // w_N^-i2, i2 < 2^16
  u64* wn_pow_br = nullptr;               // w_N^bitrev16(p)
  u64* block_coset_pow[2] = {nullptr, nullptr};  // (shift_h^R)^i2
  u64 shift[2] = {0, 0};                  // g, g*w_2N
  u64 r_inv = 0;
};
// one radix-2 level above the tall transforms (2^23 rows; see ntt.hip)
struct NttSplitTables {
  unsigned log_n = 0;
  u64 *fwd_lo = nullptr, *fwd_hi = nullptr, *inv_lo = nullptr, *inv_hi = nullptr;  // w_N^(+-b), w_N^(+-2048 a)
  u64 shift[2] = {0, 0};  // g, g*w_2N
  u64 half = 0;
};

// Everything the transforms of one trace height need.  2^16 rows: the four-step kernels on `base`; taller: an outer pass over
// R = 2^log_r blocks (coefficient k1 + R*k2 is stored at k1*2^16 + k2, the "transposed" layout); log_s = 1: one radix-2 level above
// that, a column of coefficients then holds the two halves [Pe | Po] of N/2 words, each in the transposed layout.
struct NttPlan {
  unsigned log_n = 0, log_s = 0, log_r = 0;  // log_r = log_n - 16 - log_s
  const NttTables* base = nullptr;           // the context's 2^16 tables
  NttTallTables tall;                        // used iff log_r (under the split level: of the halves, cosets g^2, g^2 w_N)
  NttSplitTables split;                      // used iff log_s
};
int ntt_plan_init(NttPlan* P, const NttTables* base, unsigned log_n, bool split);  // frees what it allocated when it fails
void ntt_plan_free(NttPlan* P);
// words of `scratch` below for ncols columns (host arithmetic only): [tmp | y0 | y1] of the fused commitment at 2^16 rows, one tmp
// for a tall transform, [E, O LDEs | tmp] under the split level
size_t ntt_scratch_words(unsigned log_n, bool split, int ncols);
// lde: [C][lde_stride] in bit-reversed order (both cosets).  lde_stride is 2 N except under the split level, whose last kernel
// writes rows of any stride.  coset_mask: bit h set = compute coset h (the lower / upper half of the output); 3 = both (the only
// value at 2^16 rows).
// from_values: values[C][N] -> stored coefficients[C][N] and their LDE; values == coef allowed
void ntt_commit(const NttPlan& P, const u64* vals, u64* coef, u64* lde, size_t lde_stride, u64* scratch, int ncols, hipStream_t s);
// stored coefficients[C][N] -> LDE
void ntt_lde(const NttPlan& P, const u64* coef, u64* lde, size_t lde_stride, u64* scratch, int ncols, hipStream_t s, int coset_mask = 3);
// values on coset h (natural order) -> stored coefficients of the interpolant
void ntt_coset_inverse(const NttPlan& P, int h, const u64* vals, u64* coef, u64* scratch, int ncols, hipStream_t s);

// debug: runs the hand-written field sequences of gl_asm.h on n operand pairs (bn254s_selftest_field)
static constexpr int FIELD_SELFTEST_OUTS = 17;
void field_selftest(const u64* a, const u64* b, u64* out, size_t n, hipStream_t s);
// debug: the shift table and the R-point DFT of the outer passes on caller data (bn254s_selftest_mul_2exp, _outer_dft)
void mul_2exp_selftest(const u64* x, u64* out, size_t n, hipStream_t s);                                   // out[n][64]
void outer_dft_selftest(int log_r, bool inverse, const u64* in, u64* out, size_t n, hipStream_t s);       // in, out [n][2^log_r], 1 <= log_r <= 6
