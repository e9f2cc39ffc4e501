// G1 point recovery from x on the device: the witness arithmetic of the reference's G1Target::is_recoverable_from_x /
// recover_from_x (src/curves/g1.rs:76-95; native form src/fields/recover.rs) around their one STARK job kind:
//   k_g1_recover: g = x^3 + 3, the Legendre job g^((p-1)/2) (is_square, src/fields/fq.rs:283-295), the flag "g is a square" and
//                 y = sqrt(g) with an even low bit (sqrt_with_sgn with sgn = false, fq.rs:266-281)
//   [n fq_exp proofs of the Legendre symbols]
// One exponentiation per input: p = 3 (mod 4), so c = g^((p+1)/4) has c^2 = g g^((p-1)/2) = +-g: c^2 == g says that g is a square
// and c is its root, c^2 == -g that it is none.  g is never zero (-3 is not a cube modulo p: pow(p - 3, (p - 1)/3, p) != 1), so
// the native definition of "recoverable" (g.sqrt().is_some(), true for 0) and the circuit's (Legendre symbol == 1) agree, and
// the two cases exclude each other.
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "fq_dev.h"
#include "../../include/bn254_stark.h"
#include "g1_recover_constants.inc"

namespace {

constexpr size_t G1R_PER_PROOF_MAX = 16384;  // 2^23 rows: the largest Fq-exp proof (bn254s_prove_batch)
constexpr int G1R_LANES = 64, G1R_ENTRIES = (1 << G1R_WINDOW) - 1;  // g^1 .. g^15 (a zero digit multiplies by nothing)

// g^((p+1)/4) by a fixed-window ladder over the compile-time digits of the exponent: 4 x 62 squarings and one product per non-zero
// digit, against 256 squarings and 109 products of a bit-at-a-time ladder.  The lane's powers g^1 .. g^15 (150 words: too many to
// keep in registers beside a product's working set) live in LDS as tab[entry][limb][lane]: a wave's 64 lanes read 64 consecutive
// words, one per bank, whatever the entry.  A lane only ever reads what it wrote itself: no barrier.
__device__ __forceinline__ void tab_store(u32 (*tab)[FQ_NL][G1R_LANES], int e, const fq& a) {
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) tab[e][j][threadIdx.x] = a.l[j];
}
__device__ __forceinline__ fq tab_load(const u32 (*tab)[FQ_NL][G1R_LANES], int e) {
  fq r;
#pragma unroll
  for (int j = 0; j < FQ_NL; j++) r.l[j] = tab[e][j][threadIdx.x];
  return r;
}

// points: n x 8 words (x, y); flags: n bytes; jobs: n x 8 words (scalar (p-1)/2 | g)
__global__ __launch_bounds__(G1R_LANES) void k_g1_recover(const u64* __restrict__ xs, size_t n, u64* __restrict__ points,
                                                          unsigned char* __restrict__ flags, u64* __restrict__ jobs,
                                                          int* __restrict__ err) {
  __shared__ u32 tab[G1R_ENTRIES][FQ_NL][G1R_LANES];
  const size_t k = (size_t)blockIdx.x * G1R_LANES + threadIdx.x;
  if (k >= n) return;
  const fq x = fq_from_canonical(xs + 4 * k);
  const fq one = fq_one();
  const fq g = fq_add(fq_mul(fq_sqr(x), x), fq_add(fq_dbl(one), one));
  fq t = g;
#pragma unroll 1
  for (int e = 0; e < G1R_ENTRIES; e++) {
    tab_store(tab, e, t);
    if (e + 1 < G1R_ENTRIES) t = fq_mul(t, g);
  }
  fq c = tab_load(tab, G1R_SQRT_DIGITS[0] - 1);
#pragma unroll 1
  for (int i = 1; i < G1R_NDIGITS; i++) {
#pragma unroll 1
    for (int s = 0; s < G1R_WINDOW; s++) c = fq_sqr(c);
    const int d = G1R_SQRT_DIGITS[i];  // the same in every lane; 32-bit entries, so that it is a scalar load
    if (d) c = fq_mul(c, tab_load(tab, d - 1));
  }
  const fq c2 = fq_sqr(c);
  const bool square = fq_eq(c2, g);
  if (!square && !fq_eq(c2, fq_neg(g))) atomicCAS(err, 0, BN254S_E_INTERNAL);  // neither root nor non-residue: the ladder is wrong
  fqw y = fq_to_canonical(c);
  if (y.l[0] & 1) y = fq_to_canonical(fq_neg(c));  // p - y: even, as p is odd and y != 0
  const fqw gc = fq_to_canonical(g);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    points[8 * k + w] = xs[4 * k + w];
    points[8 * k + 4 + w] = square ? y.l[w] : 0;
    jobs[8 * k + w] = G1R_LEGENDRE_EXP[w];
    jobs[8 * k + 4 + w] = gc.l[w];
  }
  flags[k] = square ? 1 : 0;
}

// index of the first x_i >= p, or n
size_t first_unreduced(const uint64_t* xs, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const uint64_t* w = xs + 4 * i;
    bool below = false;
    for (int j = 3; j >= 0; j--) {
      if (w[j] != G1R_P[j]) {
        below = w[j] < G1R_P[j];
        break;
      }
    }
    if (!below) return i;
  }
  return n;
}

// the arguments that both entry points share, other than the context
bool recover_args_ok(const uint64_t* xs, size_t n, const uint64_t* points_out, const uint8_t* flags_out) {
  return xs && points_out && flags_out && n > 0 && n < ((size_t)1 << 32);
}

// The front-end into host memory: points[n x 8], flags[n], jobs[n x 8] (jobs may be NULL).  Nothing is written on an error.
int recover_front(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* points, uint8_t* flags, uint64_t* jobs) {
  const size_t bad = first_unreduced(xs, n);
  if (bad != n) {
    c->set_err("g1_recover_from_x: x_" + std::to_string(bad) + " is not below p");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("g1rec", 4 * n /* xs */ + 8 * n /* points */ + 8 * n /* jobs */ + 1 /* err */ + (n + 7) / 8 /* flags */);
  if (!d) return BN254S_E_OOM;
  u64* d_xs = d;
  u64* d_pts = d_xs + 4 * n;
  u64* d_jobs = d_pts + 8 * n;
  int* d_err = (int*)(d_jobs + 8 * n);
  unsigned char* d_flags = (unsigned char*)(d_jobs + 8 * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_err, 0, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_xs, xs, n * 32, hipMemcpyHostToDevice, st));
  k_g1_recover<<<(unsigned)((n + G1R_LANES - 1) / G1R_LANES), G1R_LANES, 0, st>>>(d_xs, n, d_pts, d_flags, d_jobs, d_err);
  HIP_TRY(c, hipGetLastError());
  int h_err = 0;
  HIP_TRY(c, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_err) {
    c->set_err("g1_recover_from_x: g^((p+1)/4) squares to neither g nor -g (device self-check)");
    return h_err;
  }
  HIP_TRY(c, hipMemcpyAsync(points, d_pts, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(jobs, d_jobs, n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g1_recover_from_x_batch(bn254s_ctx* c, const uint64_t* xs, size_t n, uint64_t* points_out, uint8_t* flags_out,
                                              uint64_t* fq_jobs) {
  if (!c || !recover_args_ok(xs, n, points_out, flags_out)) return BN254S_E_INVALID_ARG;
  return recover_front(c, xs, n, points_out, flags_out, fq_jobs);
}

extern "C" int bn254s_g1_recover_from_x(bn254s_ctx* c, const bn254s_params* params, const uint64_t* xs, size_t n, size_t per_proof,
                                        uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs, bn254s_proof** fq_proofs) {
  // every check before device work; the context last, so that the shape checks can be exercised without one
  if (!recover_args_ok(xs, n, points_out, flags_out) || !params || !fq_proofs || per_proof == 0 ||
      params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  const size_t n_proofs = (n + per_proof - 1) / per_proof;
  for (size_t i = 0; i < n_proofs; i++) fq_proofs[i] = nullptr;
  if (per_proof > G1R_PER_PROOF_MAX) {
    if (c) c->set_err("g1_recover_from_x: per_proof above 16384 (2^23 rows, the largest Fq-exp proof)");
    return BN254S_E_UNSUPPORTED;
  }
  if (!c) return BN254S_E_INVALID_ARG;
  std::vector<u64> jobs(8 * n);
  int rc = recover_front(c, xs, n, points_out, flags_out, jobs.data());
  if (rc != BN254S_OK) return rc;
  std::vector<u64> s(4 * n), g(4 * n);
  for (size_t i = 0; i < n; i++) {
    memcpy(s.data() + 4 * i, jobs.data() + 8 * i, 32);
    memcpy(g.data() + 4 * i, jobs.data() + 8 * i + 4, 32);
  }
  rc = bn254s_prove_batch(c, 2, params, s.data(), g.data(), nullptr, n, per_proof, fq_proofs);
  if (rc != BN254S_OK) return rc;  // (the batch has freed its proofs)
  // linkage: the trace generator computes g_i^((p-1)/2) on its own; it must be 1 where the flag is set and p - 1 where it is not
  u64 pm1[4];
  memcpy(pm1, G1R_P, 32);
  pm1[0] -= 1;
  static const u64 ONE[4] = {1, 0, 0, 0};
  size_t pos = 0;
  for (size_t i = 0; i < n_proofs && rc == BN254S_OK; i++) {
    const uint64_t* o;
    size_t len = 0;
    const size_t cnt = n - pos < per_proof ? n - pos : per_proof;
    if (bn254s_proof_outputs(fq_proofs[i], &o, &len) != BN254S_OK || len != 4 * cnt) {
      c->set_err("g1_recover_from_x: proof " + std::to_string(i) + " has " + std::to_string(len / 4) + " outputs, expected " +
                 std::to_string(cnt));
      rc = BN254S_E_INTERNAL;
    }
    for (size_t j = 0; j < cnt && rc == BN254S_OK; j++) {
      if (memcmp(o + 4 * j, flags_out[pos + j] ? ONE : pm1, 32) != 0) {
        c->set_err("g1_recover_from_x: the proven Legendre symbol of input " + std::to_string(pos + j) + " is not " +
                   (flags_out[pos + j] ? "1, but its flag is set" : "p - 1, but its flag is clear"));
        rc = BN254S_E_INTERNAL;
      }
    }
    pos += cnt;
  }
  if (rc != BN254S_OK) {
    for (size_t i = 0; i < n_proofs; i++) {
      bn254s_proof_free(fq_proofs[i]);
      fq_proofs[i] = nullptr;
    }
    return rc;
  }
  if (fq_jobs) memcpy(fq_jobs, jobs.data(), jobs.size() * 8);
  return BN254S_OK;
}
