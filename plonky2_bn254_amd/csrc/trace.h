// Trace generation of the three STARKs on the device: the drivers (trace_g1.hip, trace_g2fq.hip) and the launchers of the
// kernels they share (trace_shared.hip).  Column layouts: layout.h.
#pragma once
#include "gl_dev.h"
#include "layout.h"
#include "../../include/bn254_stark.h"

// Words of scratch a driver needs for n instances.
size_t g1_trace_scratch_words(size_t n);
size_t g2_trace_scratch_words(size_t n);
size_t fq_trace_scratch_words(size_t n);
// All pointers are device pointers; the trace is column-major [W][N]; outputs n x 8 (G1) / n x 16 (G2) / n x 4 (Fq) canonical
// words.
int g1_generate_trace_device(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N,
                             u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range = true);
int g2_generate_trace_device(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N,
                             u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range = true);
int fq_generate_trace_device(const u64* d_scalars, const u64* d_x, size_t n, u64* d_trace, size_t N, u64* d_scratch,
                             u64* d_outputs, int* d_err, hipStream_t st, bool with_range = true);

// The cooperative doubling chain of phase A alone: D_k = 2^k x_i (k = 0..256, Jacobian, Montgomery) at point index 257 + k,
// element (257 + k) * n + i of SoA Fq vectors of 4 * NPTS * n words each; msm.hip uses it for the products s_i x_i.
// G1: the vectors px / py / pz.  G2: pts holds six of them one after the other, X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1, and znorm
// is one more (the norms of Z).
void launch_g1_dbl_chain(const u64* d_x, int n, u64* px, u64* py, u64* pz, hipStream_t st);
void launch_g2_dbl_chain(const u64* d_x, int n, u64* pts, u64* znorm, hipStream_t st);

// ---- trace_shared.hip ---------------------------------------------------------------------------------------------------
// out[e] = in[e]^-1 (0 -> 0) over SoA Fq vectors of `count` elements
void launch_fq_batch_inv(const u64* in, u64* out, size_t count, hipStream_t st);
// Goldilocks inverses of counter and counter - 511 for counter in [0, 512): tbl[2][512]
void launch_round_flag_table(u64* tbl, hipStream_t st);
// generate_range_checks on a finished trace: histogram of columns [rc_begin, rc_end) -> frequency column, and the range
// counter column (hist = 65536 u32 of scratch)
void launch_range_columns(u64* trace, size_t N, int rc_begin, int rc_end, int freq_col, int range_col, u32* hist, int* err,
                          hipStream_t st);
void launch_fq_inv_selftest(const u64* in, u64* out, size_t n, hipStream_t st);
