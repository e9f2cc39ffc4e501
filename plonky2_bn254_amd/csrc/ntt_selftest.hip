// Debug entry points for the NTT / LDE stage above 2^16 rows (bn254s_selftest_transforms, _mul_2exp, _outer_dft;
// include/bn254_stark.h).  bn254s_selftest_transforms runs the members of Transforms (transforms.h) that the provers' stages run,
// on caller data, in named scratch of the context on its stream, on the context's plan of the height: the chunking by workspace
// is the provers' own, the dispatch by height is ntt.hip's, nothing of either is repeated here.  The two small ones run the shift table and
// the R-point DFT of the outer passes through the kernels beside k_field_selftest in ntt.hip.  Every argument is checked on the
// host (pointers, sizes, every field word below p) before anything is launched.
#include "ctx.h"
#include "transforms.h"

static bool all_canonical(const uint64_t* w, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (w[k] >= GL_P) return false;
  return true;
}

extern "C" {

int bn254s_selftest_transforms(bn254s_ctx* c, int op, int log_n, int flags, int ncols, int coset_mask, const uint64_t* in,
                               uint64_t* out0, uint64_t* out1) {
  if (!c || !in || !out0 || (op == 0 && !out1)) return BN254S_E_INVALID_ARG;
  if (op < 0 || op > 3 || log_n < 16 || log_n > 23 || flags < 0 || flags > 3 || ncols < 1 || ncols > 64) return BN254S_E_INVALID_ARG;
  const bool split = flags & 1, compact = flags & 2;
  if ((split && log_n < 18) || (!split && log_n == 23) || (compact && log_n == 16)) return BN254S_E_INVALID_ARG;
  if (op == 2 && (log_n == 16 || ncols > Transforms::CH || coset_mask < 1 || coset_mask > 3)) return BN254S_E_INVALID_ARG;
  if (op == 3 && ncols != 2 * 2) return BN254S_E_INVALID_ARG;
  // Transforms::lde runs a tall transform over all its columns at once (the provers give it at most 6 in the compact workspace),
  // while the compact plan sizes tmp for one chunk: more columns than a chunk would not fit
  if (op == 1 && compact && !split && ncols > Transforms::CH) return BN254S_E_INVALID_ARG;
  // the plan fields the transforms read, as proof_plan() derives them from the height and the overrides
  ProofPlan pl;
  pl.log_n = (unsigned)log_n;
  const size_t N = pl.N = (size_t)1 << log_n, M2 = pl.M2 = 2 * N;
  pl.log_m2 = pl.log_n + 1;
  pl.log_s = split ? 1 : 0;
  pl.lowmem = op == 2 || split || compact;  // (op 2: lde_chunk is a member of the streaming workspace, which is a compact one)
  const size_t n_in = (size_t)ncols * N;
  if (!all_canonical(in, n_in)) return BN254S_E_INVALID_ARG;

  HIP_TRY(c, hipSetDevice(c->device));
  const NttPlan* np = c->ntt_plan(pl.log_n, split);
  if (!np) {
    c->set_err("NTT tables");
    return BN254S_E_OOM;
  }
  const size_t n_lde = (size_t)ncols * M2;
  u64* d_in = c->words("ns.in", n_in);
  u64* d_coef = op == 0 || op == 3 ? c->words("ns.coef", n_in) : nullptr;
  u64* d_lde = op != 3 ? c->words("ns.lde", n_lde) : nullptr;
  u64* d_tmp = c->words("ns.tmp", pl.ntt_tmp_words(ncols));
  if (!d_in || !d_tmp || (!d_coef && (op == 0 || op == 3)) || (!d_lde && op != 3)) return BN254S_E_OOM;
  hipStream_t st = c->stream;
  HIP_TRY(c, hipMemcpyAsync(d_in, in, 8 * n_in, hipMemcpyHostToDevice, st));
  const Transforms tf{*np, st, pl, d_tmp, d_lde, nullptr};
  switch (op) {
    case 0: tf.commit_ntt(d_in, d_coef, d_lde, ncols); break;
    case 1: tf.lde(d_in, d_lde, ncols); break;
    case 2:
      HIP_TRY(c, hipMemsetAsync(d_lde, 0xFF, 8 * n_lde, st));  // a half the mask leaves out stays ~0, which is no field element
      tf.lde_chunk(d_in, ncols, coset_mask);
      break;
    default: tf.quotient_coset_inverse(d_in, d_coef); break;
  }
  HIP_TRY(c, hipGetLastError());
  if (op == 0 || op == 3) HIP_TRY(c, hipMemcpyAsync(out0, d_coef, 8 * n_in, hipMemcpyDeviceToHost, st));
  if (op != 3) HIP_TRY(c, hipMemcpyAsync(op == 0 ? out1 : out0, d_lde, 8 * n_lde, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

int bn254s_selftest_mul_2exp(bn254s_ctx* c, const uint64_t* x, size_t n, uint64_t* out) {
  if (!c || !x || !out || n < 1 || n > ((size_t)1 << 20) || !all_canonical(x, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("ns.shift", n + 64 * n);
  if (!d) return BN254S_E_OOM;
  HIP_TRY(c, hipMemcpyAsync(d, x, 8 * n, hipMemcpyHostToDevice, c->stream));
  mul_2exp_selftest(d, d + n, n, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d + n, 8 * 64 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

int bn254s_selftest_outer_dft(bn254s_ctx* c, int log_r, int inverse, const uint64_t* in, size_t n, uint64_t* out) {
  if (!c || !in || !out || log_r < 1 || log_r > 6 || inverse < 0 || inverse > 1 || n < 1 || n > ((size_t)1 << 16)) return BN254S_E_INVALID_ARG;
  const size_t words = n << log_r;
  if (!all_canonical(in, words)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  u64* d = c->words("ns.dft", 2 * words);
  if (!d) return BN254S_E_OOM;
  HIP_TRY(c, hipMemcpyAsync(d, in, 8 * words, hipMemcpyHostToDevice, c->stream));
  outer_dft_selftest(log_r, inverse != 0, d, d + words, n, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, d + words, 8 * words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return BN254S_OK;
}

}  // extern "C"
