// The inversions of the reference's src/fields/ on the device (the roots of the same gadget family are root_front.hip):
//   k_fq_inv, k_fq2_inv: FqTarget::inv (fq.rs:241-255) and Fq2Target::inv (fq2.rs:190-204; native inv.rs), inv(0) = 0
// Every lane runs the inversion; the zero case is selected, never branched around.
#include "proven_jobs.h"
#include "fq2_root.h"  // fq_select, G1R_LANES

namespace {

// a^-1, 0 for a = 0.  fq_inv maps 0 to 0 by itself (the head of root_front.hip), but nothing pins that, so the divsteps see 1 in place
// of 0 and the result is selected: the zero case does not depend on how the inversion treats it.
__device__ __forceinline__ fq inv_or_zero(const fq& a) {
  const bool zero = fq_is_zero(a);
  return fq_select(zero, fq_zero(), fq_inv(fq_select(zero, fq_one(), a)));
}

// xs, out: n x 4 words
__global__ __launch_bounds__(G1R_LANES) void k_fq_inv(const u64* __restrict__ xs, size_t n, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  fe_store_canonical(out + 4 * k, inv_or_zero(fq_from_canonical(xs + 4 * k)));
}

// xs, out: n x 8 words (c0, c1): (c0, -c1) / norm; for x = 0 the norm is 0, its "inverse" 0 and both products vanish
__global__ __launch_bounds__(G1R_LANES) void k_fq2_inv(const u64* __restrict__ xs, size_t n, u64* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq2 x = fq2_from_canonical(xs + 8 * k);
  fq2_store_canonical(out + 8 * k, fq2_inv_from_norm_inv(x, inv_or_zero(fq2_norm(x))));
}

const char* inv_tag(int W) { return W == 4 ? "fq_inv" : "fq2_inv"; }  // W: words of an element, 4 (Fq) or 8 (Fq2)

int inv_batch(bn254s_ctx* c, int W, const uint64_t* xs, size_t n, uint64_t* out) {
  if (!c || !xs || !out || n == 0 || n >= ((size_t)1 << 32)) return BN254S_E_INVALID_ARG;
  if (!coords_below_p(c, inv_tag(W), "x", COORD_FQ2, W / 4, xs, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("fqinv", 2 * W * n /* xs, out */);
  if (!d) return BN254S_E_OOM;
  u64 *d_xs = d, *d_out = d + W * n;
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * W * 8, hipMemcpyHostToDevice, st));
  const unsigned blocks = (unsigned)((n + G1R_LANES - 1) / G1R_LANES);
  if (W == 4) k_fq_inv<<<blocks, G1R_LANES, 0, st>>>(d_xs, n, d_out);
  else k_fq2_inv<<<blocks, G1R_LANES, 0, st>>>(d_xs, n, d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(st));  // a failed kernel must not reach the caller's memory
  HIP_TRY(c, hipMemcpyAsync(out, d_out, n * W * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_fq_inv_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* out) { return inv_batch(c, 4, xs, n, out); }
extern "C" int bn254s_fq2_inv_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* out) { return inv_batch(c, 8, xs, n, out); }
