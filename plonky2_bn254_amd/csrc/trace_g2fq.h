// Trace-generation drivers of the G2 scalar-mul and Fq-exp STARKs (trace_g2fq.hip).
#pragma once
#include "gl_dev.h"
#include "layout.h"
size_t g2_trace_scratch_words(size_t n);
size_t fq_trace_scratch_words(size_t n);
// device pointers; trace column-major [W][N]; outputs n x 16 (G2) / n x 4 (Fq) canonical words
int g2_generate_trace_device(const u64* d_scalars, const u64* d_x, const u64* d_off, size_t n, u64* d_trace, size_t N,
                             u64* d_scratch, u64* d_outputs, int* d_err, hipStream_t st, bool with_range = true);
int fq_generate_trace_device(const u64* d_scalars, const u64* d_x, size_t n, u64* d_trace, size_t N, u64* d_scratch,
                             u64* d_outputs, int* d_err, hipStream_t st, bool with_range = true);
// the cooperative doubling chain of phase A alone: D_k = 2^k x_i (k = 0..256, Jacobian, Montgomery) at point index 257 + k.  pts
// holds six SoA Fq vectors of 4 * NPTS * n words each, X.c0, X.c1, Y.c0, Y.c1, Z.c0, Z.c1 one after the other (element
// (257 + k) * n + i), znorm one more (the norms of Z); msm.hip uses it for the products s_i x_i
void launch_g2_dbl_chain(const u64* d_x, int n, u64* pts, u64* znorm, hipStream_t st);
