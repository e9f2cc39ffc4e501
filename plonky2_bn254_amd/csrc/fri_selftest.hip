// Debug entry points for the openings / FRI kernels of fri.hip and the un-reduced accumulators of quotient_common.h
// (bn254s_selftest_acc, _openings, _fri_combine, _fri_fold, _fri_rows; include/bn254_stark.h).  Each runs the launchers of fri.h
// that the provers run, on caller data, in named scratch of the context on its stream: no kernel of fri.hip is repeated here.
// Only the accumulators, which are inline device functions without a launcher, get a small kernel of their own.  Every argument
// is checked on the host (pointers, sizes, every field word below p) before anything is launched.
#include <cstring>
#include <vector>
#include "ctx.h"
#include "fri.h"

// One lane per row: the T terms of the row go through ONE Acc and ONE Acc3, as a constraint sum of the quotient kernels does.
// w3[8 t ..] = the weight t as fri_weight_record cuts it (limbs w0 w1 w2 of w3_split at 0..2); the value is cut as accw_mad cuts it.
__global__ __launch_bounds__(64) void k_acc_selftest(const u64* __restrict__ values, const u64* __restrict__ weights,
                                                     const u32* __restrict__ w3, size_t T, size_t rows, u64* __restrict__ out) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  Acc a;
  Acc3 a3;
  acc_init(a);
  acc3_init(a3);
  const u64* v = values + r * T;
  for (size_t t = 0; t < T; t++) {
    const u64 x = v[t];
    acc_mad(a, x, weights[t]);
    const u32 v0 = (u32)x & M22, v1 = (u32)(x >> 22) & M22, v2 = (u32)(x >> 44);
    const u32* e = w3 + 8 * t;
    acc3_mad(a3, v0, v1, v2, e[0], e[1], e[2]);
  }
  out[2 * r] = acc_red(a);
  out[2 * r + 1] = acc3_red(a3);
}

static bool all_canonical(const uint64_t* w, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (w[k] >= GL_P) return false;
  return true;
}

extern "C" {

int bn254s_selftest_acc(bn254s_ctx* c, const uint64_t* values, const uint64_t* weights, size_t T, size_t rows, uint64_t* out) {
  if (!c || !values || !weights || !out) return BN254S_E_INVALID_ARG;
  if (T < 1 || T > ((size_t)1 << 17) || rows < 1 || rows > 4096) return BN254S_E_INVALID_ARG;
  if (!all_canonical(values, rows * T) || !all_canonical(weights, T)) return BN254S_E_INVALID_ARG;
  std::vector<u32> rec(8 * T);
  for (size_t t = 0; t < T; t++) fri_weight_record(&rec[8 * t], gl2_make(weights[t], 0));
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("fs.acc", rows * T + T + 4 * T + 2 * rows);
  if (!d) return BN254S_E_OOM;
  u64* d_w = d + rows * T;
  u64* d_rec = d_w + T;
  u64* d_out = d_rec + 4 * T;
  HIP_TRY(c, hipMemcpyAsync(d, values, 8 * rows * T, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_w, weights, 8 * T, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_rec, rec.data(), 32 * T, hipMemcpyHostToDevice, c->stream));
  k_acc_selftest<<<(unsigned)((rows + 63) / 64), 64, 0, c->stream>>>(d, d_w, reinterpret_cast<const u32*>(d_rec), T, rows, d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 16 * rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (rec is read by the copy above until here)
  return BN254S_OK;
}

int bn254s_selftest_openings(bn254s_ctx* c, const uint64_t* coeffs, int npolys, int log_r, const uint64_t zeta[2],
                             const uint64_t zeta_next[2], uint64_t* out) {
  if (!c || !coeffs || !zeta || !zeta_next || !out) return BN254S_E_INVALID_ARG;
  if (npolys < 1 || npolys > 64 || log_r < 0 || log_r > 2) return BN254S_E_INVALID_ARG;
  const size_t N = (size_t)1 << (16 + log_r), R = (size_t)1 << log_r;
  if (!all_canonical(zeta, 2) || !all_canonical(zeta_next, 2) || !all_canonical(coeffs, (size_t)npolys * N)) return BN254S_E_INVALID_ARG;
  const size_t n_part = 5 * R * (size_t)npolys;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("fs.open", (size_t)npolys * N + FRI_OPENING_TABLE_WORDS + n_part);
  if (!d) return BN254S_E_OOM;
  u64* d_tab = d + (size_t)npolys * N;
  u64* d_out = d_tab + FRI_OPENING_TABLE_WORDS;
  HIP_TRY(c, hipMemcpyAsync(d, coeffs, 8 * (size_t)npolys * N, hipMemcpyHostToDevice, c->stream));
  fri_opening_tables((unsigned)log_r, gl2_make(zeta[0], zeta[1]), gl2_make(zeta_next[0], zeta_next[1]), d_tab, c->stream);
  fri_openings(d, N, (unsigned)log_r, npolys, d_tab, d_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 8 * n_part, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

int bn254s_selftest_fri_combine(bn254s_ctx* c, int mode, int W, int n_rc, int n_ctl, size_t n, const uint64_t* cols,
                                const uint64_t* aux_in, const uint64_t* points, uint64_t* out) {
  if (!c || !cols || !aux_in || !out || mode < 0 || mode > 1 || (mode == 1 && !points)) return BN254S_E_INVALID_ARG;
  if (W < 1 || W > 4096 || n_rc < 1 || n_rc > W || (n_ctl != 0 && n_ctl != 2)) return BN254S_E_INVALID_ARG;
  if (n < 1 || n > (mode == 0 ? (size_t)1 << 16 : (size_t)1 << 20)) return BN254S_E_INVALID_ARG;
  StarkShape sh;  // (as bn254s_selftest_logup builds it: the combine kernels read the widths only)
  sh.W = W;
  sh.rc_begin = 0;
  sh.rc_end = n_rc;
  sh.table_col = 0;
  sh.freq_col = 0;
  sh.n_ctl = n_ctl;
  memset(&sh.ctl, 0, sizeof(sh.ctl));
  const size_t A = (size_t)sh.n_aux(), n_polys = (size_t)W + A + 4;
  if (mode == 0) {
    if (!all_canonical(cols, n_polys * n) || !all_canonical(aux_in, 2 * n_polys)) return BN254S_E_INVALID_ARG;
    std::vector<u32> rec(8 * n_polys);
    for (size_t p = 0; p < n_polys; p++) fri_weight_record(&rec[8 * p], gl2_make(aux_in[2 * p], aux_in[2 * p + 1]));
    HIP_TRY(c, hipSetDevice(c->device));
    u64* d = c->words("fs.comb", n_polys * n + 4 * n_polys + 6 * n);
    if (!d) return BN254S_E_OOM;
    u64* d_rec = d + n_polys * n;
    u64* d_out = d_rec + 4 * n_polys;
    HIP_TRY(c, hipMemcpyAsync(d, cols, 8 * n_polys * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_rec, rec.data(), 32 * n_polys, hipMemcpyHostToDevice, c->stream));
    fri_combine_coeffs(sh, d, d + (size_t)W * n, d + ((size_t)W + A) * n, d_rec, n, d_out, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, 8 * 6 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return BN254S_OK;
  }
  if (!all_canonical(cols, 6 * n) || !all_canonical(aux_in, n) || !all_canonical(points, 12)) return BN254S_E_INVALID_ARG;
  auto pt = [&](int k) { return gl2_make(points[2 * k], points[2 * k + 1]); };
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("fs.comb", 6 * n + n + 1 + 2 * n);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d + 6 * n;
  u64* d_out = d_xs + n + (n & 1);  // the kernel stores an extension value as one 16-byte word: an even word offset for every n
  HIP_TRY(c, hipMemcpyAsync(d, cols, 8 * 6 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_xs, aux_in, 8 * n, hipMemcpyHostToDevice, c->stream));
  fri_combine_final(sh, d, d_xs, pt(0), pt(1), pt(2), pt(3), pt(4), pt(5), n, d_out, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 16 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

int bn254s_selftest_fri_fold(bn254s_ctx* c, const uint64_t* in, int log_m, uint64_t shift, const uint64_t beta[2], uint64_t* out) {
  if (!c || !in || !beta || !out) return BN254S_E_INVALID_ARG;
  // log_m = 4 would make the kernel reverse the bits of its one coset index over 0 bits (a shift by 32); the provers stop folding
  // at 2^5 values (final_poly_bits + rate_bits)
  if (log_m < 5 || log_m > 20 || shift == 0 || shift >= GL_P) return BN254S_E_INVALID_ARG;
  const size_t M = (size_t)1 << log_m, Mo = M >> 4;
  if (!all_canonical(beta, 2) || !all_canonical(in, 2 * M)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("fs.fold", 2 * M + 2 * Mo);
  if (!d) return BN254S_E_OOM;
  HIP_TRY(c, hipMemcpyAsync(d, in, 16 * M, hipMemcpyHostToDevice, c->stream));
  fri_fold(d, d + 2 * M, (unsigned)log_m, shift, gl2_make(beta[0], beta[1]), gl_inv(16), c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d + 2 * M, 16 * Mo, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

int bn254s_selftest_fri_rows(bn254s_ctx* c, const uint64_t* lde, int ncols, int log_n, int h, size_t k0, size_t rows,
                             const uint32_t* indices, int nq, uint64_t* window, uint64_t* gathered) {
  if (!c || !lde || !indices || !window || !gathered) return BN254S_E_INVALID_ARG;
  if (ncols < 1 || ncols > 4096 || log_n < 1 || log_n > 20 || h < 0 || h > 1 || nq < 1 || nq > 4096) return BN254S_E_INVALID_ARG;
  const size_t N = (size_t)1 << log_n, M2 = 2 * N;
  if (k0 >= N || rows < 1 || rows > ((size_t)1 << 20)) return BN254S_E_INVALID_ARG;
  for (int q = 0; q < nq; q++)
    if (indices[q] >= M2) return BN254S_E_INVALID_ARG;
  if (!all_canonical(lde, (size_t)ncols * M2)) return BN254S_E_INVALID_ARG;
  const size_t lw = (size_t)ncols * M2, ww = (size_t)ncols * rows, gw = (size_t)ncols * (size_t)nq, iw = ((size_t)nq + 1) / 2;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("fs.rows", lw + ww + gw + iw);
  if (!d) return BN254S_E_OOM;
  u64* d_win = d + lw;
  u64* d_gat = d_win + ww;
  u32* d_idx = reinterpret_cast<u32*>(d_gat + gw);
  HIP_TRY(c, hipMemcpyAsync(d, lde, 8 * lw, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_idx, indices, 4 * (size_t)nq, hipMemcpyHostToDevice, c->stream));
  fri_extract_window(d, M2, (unsigned)log_n, h, k0, rows, ncols, d_win, c->stream);
  fri_gather_rows(d, M2, ncols, d_idx, nq, d_gat, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(window, d_win, 8 * ww, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(gathered, d_gat, 8 * gw, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

}  // extern "C"
