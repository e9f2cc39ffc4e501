// Debug entry points for the quotient (AIR constraint) kernels of quotient_g1.hip / quotient_g2fq.hip / quotient_sched.h and
// the auxiliary columns of aux.hip with the kind's real shape, CTLs included (bn254s_selftest_quotient, _point_tables, _aux;
// include/bn254_stark.h).  Each runs what the provers and the device verifier run - quotient_host_tables, quotient_fill_args,
// quotient_window_args, stark_kind(kind).quotient_launch, quotient_point_tables[_window], aux_build - on caller data, in named
// scratch of the context on its stream: no kernel is repeated here.  Every argument is checked on the host (pointers, ranges,
// every field word below p) before anything is launched.
#include <string>
#include <vector>
#include "ctx.h"
#include "prover.h"

static bool qs_canonical(const uint64_t* w, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (w[k] >= GL_P) return false;
  return true;
}

// the sizes the entry points accept: whole domain 2^3 .. 2^12 rows, windows of at most 4096 rows of a domain of up to 2^20
static constexpr int QS_LOG_MIN = 3, QS_LOG_WHOLE_MAX = 12, QS_LOG_WINDOW_MAX = 20;
static constexpr size_t QS_STRIDE_MAX = 8192;
static_assert(QUOTIENT_MAX_PARTS == BN254S_QS_MAX_PARTS, "the part buffer of bn254s_selftest_quotient");

extern "C" {

int bn254s_selftest_quotient(bn254s_ctx* c, int kind, int log_n, int flags, int h, size_t k0, size_t count, size_t stride,
                             const uint64_t* trace, const uint64_t* aux, const uint64_t alphas[2], const uint64_t betas[2],
                             const uint64_t gammas[2], const uint64_t* x, const uint64_t* lfirst, const uint64_t* llast, uint64_t* out,
                             uint64_t* part) {
  if (!c || !trace || !aux || !alphas || !betas || !gammas || !out || !part) return BN254S_E_INVALID_ARG;
  if (kind < 0 || kind > 2 || (flags & ~(BN254S_QS_WINDOW | BN254S_QS_RAW))) return BN254S_E_INVALID_ARG;
  const bool window = flags & BN254S_QS_WINDOW, raw = flags & BN254S_QS_RAW;
  if (log_n < QS_LOG_MIN || log_n > (window ? QS_LOG_WINDOW_MAX : QS_LOG_WHOLE_MAX)) return BN254S_E_INVALID_ARG;
  const size_t N = (size_t)1 << log_n;
  if (window) {
    if (h < 0 || h > 1 || count < 1 || count > N || k0 > N - count || stride < count + 1 || stride > QS_STRIDE_MAX)
      return BN254S_E_INVALID_ARG;
  } else {
    count = stride = 2 * N;
  }
  const bool own_tables = x || lfirst || llast;
  if (own_tables && !(x && lfirst && llast)) return BN254S_E_INVALID_ARG;
  const StarkKind& sk = stark_kind(kind);
  const StarkShape& sh = sk.shape;
  const size_t W = (size_t)sh.W, A = (size_t)sh.n_aux();
  const int K = sh.n_total_constraints();
  if (!qs_canonical(alphas, 2) || !qs_canonical(betas, 2) || !qs_canonical(gammas, 2)) return BN254S_E_INVALID_ARG;
  if (!qs_canonical(trace, W * stride) || !qs_canonical(aux, A * stride)) return BN254S_E_INVALID_ARG;
  if (own_tables && (!qs_canonical(x, count) || !qs_canonical(lfirst, count) || !qs_canonical(llast, count))) return BN254S_E_INVALID_ARG;

  std::vector<u64> hW, hmzt;
  const int* mz_e0 = nullptr;
  const int nblk = sk.mz_blocks(&mz_e0);
  quotient_host_tables(K, alphas, mz_e0, nblk, hW, hmzt);

  const size_t pw = (size_t)QUOTIENT_MAX_PARTS * 2 * stride;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d_tl = c->words("qs.tl", W * stride);
  u64* d_al = c->words("qs.al", A * stride);
  u64* d_pt = c->words("qs.pt", 3 * count);
  u64* d_W = c->words("qs.W", hW.size());
  u64* d_mzt = c->words("qs.mzt", hmzt.size());
  u64* d_out = c->words("qs.out", 4 * N);
  u64* d_part = c->words("qs.part", pw);
  if (!d_tl || !d_al || !d_pt || !d_W || !d_mzt || !d_out || !d_part) return BN254S_E_OOM;
  hipStream_t st = c->stream;
  HIP_TRY(c, hipMemcpyAsync(d_tl, trace, 8 * W * stride, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_al, aux, 8 * A * stride, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_W, hW.data(), 8 * hW.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_mzt, hmzt.data(), 8 * hmzt.size(), hipMemcpyHostToDevice, st));
  // out and part go in as the caller filled them: what no lane writes comes back unchanged
  HIP_TRY(c, hipMemcpyAsync(d_out, out, 8 * 4 * N, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_part, part, 8 * pw, hipMemcpyHostToDevice, st));
  QPointTables pt;
  pt.x = d_pt;
  pt.lfirst = d_pt + count;
  pt.llast = d_pt + 2 * count;
  if (own_tables) {
    HIP_TRY(c, hipMemcpyAsync(d_pt, x, 8 * count, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_pt + count, lfirst, 8 * count, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_pt + 2 * count, llast, 8 * count, hipMemcpyHostToDevice, st));
  } else if (window) {
    quotient_point_tables_window(d_pt, d_pt + count, d_pt + 2 * count, (unsigned)log_n, h, k0, count, st);
  } else {
    quotient_point_tables(d_pt, d_pt + count, d_pt + 2 * count, (unsigned)log_n, st);
  }
  QArgs QA;
  quotient_fill_args(QA, sh, d_tl, d_al, d_W, d_mzt, pt, betas, gammas, (unsigned)log_n, d_out, d_part);
  if (window) quotient_window_args(QA, d_tl, d_al, pt, d_part, stride, count, k0, h);
  if (raw) {  // as vanishing_on_gpu of verify.hip
    QA.zh_inv[0] = QA.zh_inv[1] = 1;
    QA.w_inv = 0;
  }
  sk.quotient_launch(QA, sh, st);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_out, 8 * 4 * N, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(part, d_part, 8 * pw, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // (hW, hmzt are read by the copies above until here)
  return BN254S_OK;
}

int bn254s_selftest_point_tables(bn254s_ctx* c, int log_n, int window, int h, size_t k0, size_t count, uint64_t* out) {
  if (!c || !out || log_n < QS_LOG_MIN || log_n > QS_LOG_WINDOW_MAX || window < 0 || window > 1) return BN254S_E_INVALID_ARG;
  const size_t N = (size_t)1 << log_n;
  if (window) {
    if (h < 0 || h > 1 || count < 1 || count > N || k0 >= N) return BN254S_E_INVALID_ARG;
  } else {
    count = 2 * N;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("qs.pt", 3 * count);
  if (!d) return BN254S_E_OOM;
  if (window) quotient_point_tables_window(d, d + count, d + 2 * count, (unsigned)log_n, h, k0, count, c->stream);
  else quotient_point_tables(d, d + count, d + 2 * count, (unsigned)log_n, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d, 8 * 3 * count, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

int bn254s_selftest_aux(bn254s_ctx* c, int kind, const uint64_t* trace, size_t rows, const uint64_t betas[2], const uint64_t gammas[2],
                        uint64_t* out) {
  if (!c || !trace || !betas || !gammas || !out || kind < 0 || kind > 2) return BN254S_E_INVALID_ARG;
  if (rows < 64 || rows > ((size_t)1 << 16) || (rows & (rows - 1))) return BN254S_E_INVALID_ARG;
  const StarkShape& sh = stark_kind(kind).shape;
  const size_t tw = (size_t)sh.W * rows, aw = (size_t)sh.n_aux() * rows, sw = aux_scratch_words(sh, rows);
  if (!qs_canonical(betas, 2) || !qs_canonical(gammas, 2) || !qs_canonical(trace, tw)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("qs.aux", tw + aw + sw + 2);
  if (!d) return BN254S_E_OOM;
  u64* d_aux = d + tw;
  u64* d_scr = d_aux + aw;
  int* d_err = (int*)(d_scr + sw);
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(d, trace, 8 * tw, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, c->stream));
  aux_build(sh, d, rows, betas, gammas, d_aux, d_scr, d_err, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d_aux, 8 * aw, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (h_err) {
    c->set_err("auxiliary columns: device error " + std::to_string(h_err) +
               " (a range-checked or table value above 65535, or a CTL filter that is neither 0 nor 1)");
    return h_err;
  }
  return BN254S_OK;
}

}  // extern "C"
