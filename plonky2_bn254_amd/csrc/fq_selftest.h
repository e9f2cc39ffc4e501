// Debug (bn254s_selftest_fq): the BN254 Fq / Fq2 device arithmetic of fq_dev.h and the cooperative pieces of chain_coop.h on
// caller-chosen RAW register contents, one lane per row.  Operands are loaded with fq_unpack and results stored with fq_pack:
// nothing is converted to or from Montgomery form on the way, so the caller decides which limbs the multiplier sees and sees
// whether a result is canonical.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

constexpr int FQ_SELFTEST_GROUPS = 4;
// u64 words per row, by group: 0 Fq (a b c d), 1 Fq2 (x = (a, b), y = (c, d)), 2 cooperative pieces (e0 .. e7), 3 curve (G1 P, Q as
// X Y Z; G2 P, Q as X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1)
constexpr int FQ_SELFTEST_IN[FQ_SELFTEST_GROUPS] = {16, 16, 32, 72};
constexpr int FQ_SELFTEST_OUT[FQ_SELFTEST_GROUPS] = {68, 60, 92, 74};

// in[n][FQ_SELFTEST_IN[group]] -> out[n][FQ_SELFTEST_OUT[group]] (device buffers); every operand below p, see bn254_stark.h
void launch_fq_selftest(int group, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st);
