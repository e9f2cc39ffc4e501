// G2 cofactor clearing on the device: P -> [h]P for points of the twist curve E'(Fq2), h = 2p - r = p - 1 + t the cofactor of
// the r-torsion subgroup.  It is the last step of the reference's map_to_g2 (mul_by_cofactor, src/utils/hash_to_g2.rs:113-148) and,
// in its circuit, the job (h, P, R) of the G2 STARK with the output R + [h]P (g2_scalar_mul with the constant scalar h).
//   k_g2_clear_cofactor: the on-curve test y^2 == x^3 + b', the affine image [h]P and the byte "[h]P is finite" of every point
//   [n G2 proofs of the jobs (h, P_i, R_i)]
//   k_g2c_link:          proven output - R_i == image_i (or the output is R_i where the image is O)
// The image does not cost 254 doublings.  psi = twist^-1 o Frobenius_p o twist satisfies psi^2 - t psi + p = 0 on every point of
// E'(Fq2), t = 6 x0^2 + 1 (DESIGN.md "G2 cofactor clearing"), so [p] = [t]psi - psi^2 and, with T = [6 x0^2]P,
//   [h]P = [p - 1 + t]P = [t]psi(P) - psi^2(P) - P + [t]P = T + psi(T + P) - psi^2(P),
// exactly, on the whole twist and not only on the subgroup.  T is two chained ladders: Q = [x0]P (63 bits, the ladder of
// k_g2_subgroup), Q made affine, T = [6 x0]Q (65 bits).  Then one psi, three additions, psi^2 of P and one inversion.
//
// Which additions are ordinary (distinct, non-opposite, finite operands), and which are not known to be:
//  - the two ladders.  Their bases P and Q = [x0]P are finite points of the curve: x0 is not 0 modulo a prime of r h, so Q is O
//    for no P (and Z of Q can be inverted).  The accumulator is [k]B for the prefixes k of the multiplier; [2k]B is O, B or -B only
//    if a prime of r h divides 2k, 2k - 1 or 2k + 1, and no prefix of x0 or of 6 x0 has that (the two large primes exceed
//    12 x0 + 1; the three small ones are checked by tests/test_g2_cofactor_cpu.py).  g2_madd still answers every case;
//  - T + P, psi(T + P) + T and the last sum with -psi^2(P): nothing is known about these operands (the result is O for every
//    P whose order divides h).  g2_madd and g2_add_lean, the complete laws of g2_endo.h.
// One lane per point, like k_g2_subgroup; the multipliers are compile-time constants, so every lane of a wave doubles and adds in
// the same steps.  The bases stay affine through the ladders (mixed addition, Z2 = 1); P is read again from memory after them
// rather than kept in registers beside Q.
#include <climits>
#include "g2_endo.h"
#include "proven_jobs.h"
#include "g2_cofactor.h"
#include "g2_cofactor_constants.inc"

namespace {

constexpr int G2C_LANES = 64;

// (X, Y, Z) -> (X/Z^2, Y/Z^3, 1) for a finite point
__device__ __forceinline__ g2j g2_normalise(const g2j& p) {
  const fq2 zi = fq2_inv(p.z), zi2 = fq2_sqr(zi);
  g2j r;
  r.x = fq2_mul(p.x, zi2);
  r.y = fq2_mul(fq2_mul(p.y, zi), zi2);
  r.z = fq2_one();
  return r;
}

// points: n x 16 canonical words (x.c0, x.c1, y.c0, y.c1), every coordinate below p; images: n x 16 canonical words, zeros
// where [h]P = O; finite: n bytes.  A point off the curve writes nothing and lowers *bad_idx to its index.
__global__ __launch_bounds__(G2C_LANES) void k_g2_clear_cofactor(const u64* __restrict__ points, size_t n, u64* __restrict__ images,
                                                                 unsigned char* __restrict__ finite, unsigned* __restrict__ bad_idx) {
  const size_t k = (size_t)blockIdx.x * G2C_LANES + threadIdx.x;
  if (k >= n) return;
  g2j q, b;  // the accumulator and the (affine) base of a ladder
  b.x = fq2_from_canonical(points + 16 * k);
  b.y = fq2_from_canonical(points + 16 * k + 8);
  if (!g2_on_twist(b.x, b.y)) {
    atomicMin(bad_idx, (unsigned)k);
    return;
  }
  // pass 0: Q = [x0]P; pass 1: T = [6 x0]Q.  The top bit of the multiplier is the base itself, then one step per lower bit.
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    const u64 m = pass ? G2C_6X0_LO : G2S_X0;
    if (pass) b = g2_normalise(q);
    q.x = b.x;
    q.y = b.y;
    q.z = fq2_one();
#pragma unroll 1
    for (int i = (pass ? G2C_6X0_TOP : 62) - 1; i >= 0; i--) {
      q = g2_double(q);
      if ((m >> i) & 1) q = g2_madd(q, b.x, b.y);  // the same branch in every lane
    }
  }
  // T + psi(T + P) - psi^2(P); b becomes P, then -psi^2(P)
  b.x = fq2_from_canonical(points + 16 * k);
  b.y = fq2_from_canonical(points + 16 * k + 8);
  b.z = fq2_one();
  q = g2_add_lean(g2_psi(g2_madd(q, b.x, b.y)), q);
  b = g2_psi(g2_psi(b));
  q = g2_madd(q, b.x, fq2_neg(b.y));
  const bool inf = pt_inf(q);
  if (!inf) q = g2_normalise(q);
  const fqw x0 = fq_to_canonical(q.x.c0), x1 = fq_to_canonical(q.x.c1), y0 = fq_to_canonical(q.y.c0), y1 = fq_to_canonical(q.y.c1);
#pragma unroll
  for (int w = 0; w < 4; w++) {
    images[16 * k + w] = inf ? 0 : x0.l[w];
    images[16 * k + 4 + w] = inf ? 0 : x1.l[w];
    images[16 * k + 8 + w] = inf ? 0 : y0.l[w];
    images[16 * k + 12 + w] = inf ? 0 : y1.l[w];
  }
  finite[k] = inf ? 0 : 1;
}

// The linkage of the proven jobs: outs[i] = R_i + [h]P_i as the trace generator computed it, offs[i] = R_i, both canonical.
// Where finite[i] is 0 the output must be R_i word for word; where it is 1, output - R_i (the subtraction of k_m2g_finish,
// map_to_g2.hip) must be images[i] word for word: the first i that fails lowers bad[0].  An output with the x of R_i beside a
// finite image (output == +-R_i) cannot be subtracted that way and lowers bad[1].
__global__ __launch_bounds__(G2C_LANES) void k_g2c_link(const u64* __restrict__ outs, const u64* __restrict__ offs,
                                                        const u64* __restrict__ images, const unsigned char* __restrict__ finite, size_t n,
                                                        unsigned* __restrict__ bad) {
  const size_t k = (size_t)blockIdx.x * G2C_LANES + threadIdx.x;
  if (k >= n) return;
  bool same = true;
  for (int w = 0; w < 16; w++) same = same && outs[16 * k + w] == offs[16 * k + w];
  if (!finite[k]) {
    if (!same) atomicMin(bad, (unsigned)k);
    return;
  }
  const fq2 x1 = fq2_from_canonical(outs + 16 * k), y1 = fq2_from_canonical(outs + 16 * k + 8);
  const fq2 x2 = fq2_from_canonical(offs + 16 * k), y2 = fq2_neg(fq2_from_canonical(offs + 16 * k + 8));
  const fq2 dx = fq2_sub(x2, x1);
  if (fq2_is_zero(dx)) {
    atomicMin(bad + 1, (unsigned)k);
    return;
  }
  const fq2 lam = fq2_mul(fq2_sub(y2, y1), fq2_inv(dx));
  const fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), x1), x2);
  const fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(x1, x3)), y1);
  const fqw c[4] = {fq_to_canonical(x3.c0), fq_to_canonical(x3.c1), fq_to_canonical(y3.c0), fq_to_canonical(y3.c1)};
  bool eq = true;
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int w = 0; w < 4; w++) eq = eq && c[j].l[w] == images[16 * k + 4 * j + w];
  if (!eq) atomicMin(bad, (unsigned)k);
}

bool front_args_ok(const uint64_t* points, size_t n, const uint64_t* images_out, const uint8_t* finite_out) {
  return points && images_out && finite_out && n > 0 && n < (size_t)UINT_MAX;  // the first bad index travels as a 32-bit word
}

// The front-end into host memory: images[n x 16], finite[n].  Nothing is written on an error.
int cofactor_front(bn254s_ctx* c, const uint64_t* points, size_t n, uint64_t* images, uint8_t* finite) {
  if (!coords_below_p(c, "g2_clear_cofactor", "point", COORD_G2, 4, points, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words("g2cof", 16 * n /* points */ + 16 * n /* images */ + 1 /* bad_idx */ + nb /* finite */);
  if (!d) return BN254S_E_OOM;
  u64* d_pts = d;
  u64* d_img = d + 16 * n;
  unsigned* d_bad = (unsigned*)(d + 32 * n);
  unsigned char* d_fin = (unsigned char*)(d + 32 * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_pts, points, n * 128, hipMemcpyHostToDevice, st));
  int rc = bn254s_g2_clear_cofactor_device(c, d_pts, n, d_img, d_fin, d_bad);
  if (rc != BN254S_OK) return rc;
  unsigned h_bad = UINT_MAX;
  HIP_TRY(c, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_bad != UINT_MAX) {
    c->set_err("g2_clear_cofactor: point_" + std::to_string(h_bad) + " is not on the twist curve y^2 = x^3 + b'");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipMemcpyAsync(images, d_img, n * 128, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(finite, d_fin, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

// k_g2_clear_cofactor on n points that are on the device already (d_points: n x 16 canonical words below p), on the context's
// stream, without waiting for it: d_images n x 16 words, d_finite n bytes, *d_bad_idx (preset to UINT_MAX) lowered to the first
// point off the curve.  n < UINT_MAX.
int bn254s_g2_clear_cofactor_device(bn254s_ctx* c, const u64* d_points, size_t n, u64* d_images, unsigned char* d_finite,
                                    unsigned* d_bad_idx) {
  k_g2_clear_cofactor<<<(unsigned)((n + G2C_LANES - 1) / G2C_LANES), G2C_LANES, 0, c->stream>>>(d_points, n, d_images, d_finite, d_bad_idx);
  HIP_TRY(c, hipGetLastError());
  return BN254S_OK;
}

extern "C" int bn254s_g2_clear_cofactor_batch(bn254s_ctx* c, const uint64_t* points, size_t n, uint64_t* images_out,
                                              uint8_t* finite_out) {
  if (!c || !front_args_ok(points, n, images_out, finite_out)) return BN254S_E_INVALID_ARG;
  return cofactor_front(c, points, n, images_out, finite_out);
}

extern "C" int bn254s_g2_clear_cofactor(bn254s_ctx* c, const bn254s_params* params, const uint64_t* points, const uint64_t* offsets,
                                        size_t n, size_t per_proof, uint64_t* images_out, uint8_t* finite_out, uint64_t* g2_jobs,
                                        bn254s_proof** g2_proofs) {
  int rc = proven_args(c, "g2_clear_cofactor", "G2 proof", front_args_ok(points, n, images_out, finite_out) && offsets, params,
                       g2_proofs, n, per_proof);
  if (rc != BN254S_OK) return rc;
  // (the trace generator takes canonical words)
  if (!coords_below_p(c, "g2_clear_cofactor", "offset", COORD_G2, 4, offsets, n)) return BN254S_E_INVALID_ARG;
  std::vector<u64> images(16 * n), outs;
  std::vector<uint8_t> finite(n);
  rc = cofactor_front(c, points, n, images.data(), finite.data());
  if (rc != BN254S_OK) return rc;
  std::vector<u64> h(4 * n);
  for (size_t i = 0; i < n; i++) memcpy(h.data() + 4 * i, G2C_H, 32);
  rc = prove_and_collect(c, "g2_clear_cofactor", 1, params, h.data(), points, offsets, n, per_proof, g2_proofs, outs);
  if (rc != BN254S_OK) return rc;  // (BN254S_E_INVALID_POINT: the caller draws another offset)
  // linkage: the trace generator computes R_i + [h]P_i bit by bit on its own; minus R_i it must be the front-end's image
  auto link = [&]() -> int {
    // (the proofs used the pool meanwhile: the operands travel again, in a buffer of their own)
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nb = (n + 7) / 8;
    u64* d = c->words("g2cof.link", 48 * n + 1 + nb);
    if (!d) return BN254S_E_OOM;
    u64 *d_outs = d, *d_offs = d + 16 * n, *d_img = d + 32 * n;
    unsigned* d_bad = (unsigned*)(d + 48 * n);
    unsigned char* d_fin = (unsigned char*)(d + 48 * n + 1);
    HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
    HIP_TRY(c, hipMemcpyAsync(d_outs, outs.data(), n * 128, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_offs, offsets, n * 128, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_img, images.data(), n * 128, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_fin, finite.data(), n, hipMemcpyHostToDevice, st));
    k_g2c_link<<<(unsigned)((n + G2C_LANES - 1) / G2C_LANES), G2C_LANES, 0, st>>>(d_outs, d_offs, d_img, d_fin, n, d_bad);
    HIP_TRY(c, hipGetLastError());
    unsigned h_bad[2] = {UINT_MAX, UINT_MAX};
    HIP_TRY(c, hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h_bad[0] != UINT_MAX) {
      c->set_err("g2_clear_cofactor: the proven R + [h]P of point " + std::to_string(h_bad[0]) +
                 (finite[h_bad[0]] ? " minus R is not the front-end's image" : " is not R, but the front-end's image is infinite"));
      return BN254S_E_INTERNAL;
    }
    if (h_bad[1] != UINT_MAX) {
      c->set_err("g2_clear_cofactor: output " + std::to_string(h_bad[1]) + " equals +-offset");
      return BN254S_E_INVALID_POINT;
    }
    return BN254S_OK;
  };
  rc = link();
  if (rc != BN254S_OK) {
    release_proofs(g2_proofs, n, per_proof);
    return rc;
  }
  memcpy(images_out, images.data(), n * 128);
  memcpy(finite_out, finite.data(), n);
  if (g2_jobs)
    for (size_t i = 0; i < n; i++) {
      memcpy(g2_jobs + 20 * i, G2C_H, 32);
      memcpy(g2_jobs + 20 * i + 4, points + 16 * i, 128);
    }
  return BN254S_OK;
}
