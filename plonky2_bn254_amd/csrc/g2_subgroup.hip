// G2 subgroup check on the device: is a point of the twist curve E'(Fq2) in the r-torsion subgroup, [r]P = O?  The reference
// has no such gadget; it is the circuit one writes with its pieces (G2Target::new_checked, set_random_g2 for the offset R,
// g2_scalar_mul with the constant scalar r, connect): the job (r, P, R) of the G2 STARK has the output R + [r]P, which is R
// exactly for a member.
//   k_g2_subgroup: the on-curve test y^2 == x^3 + b' and the flag "[r]P == O" of every point
//   [n G2 proofs of the jobs (r, P_i, R_i)]
// The flag does not cost 254 doublings.  With psi = twist^-1 o Frobenius_p o twist, psi(x, y) = (conj(x) xi^((p-1)/3),
// conj(y) xi^((p-1)/2)), and the BN parameter x0 (63 bits, weight 28), P is a member iff
//   [x0 + 1]P + psi([x0]P) + psi^2([x0]P) == psi^3([2 x0]P)
// (El Housni, Guillevic, Piellard: "Co-factor clearing and subgroup membership testing on pairing-friendly curves"; why this is
// sound on the whole of E'(Fq2), cofactor part included: DESIGN.md "G2 subgroup check").  In Horner form, with Q = [x0]P:
//   T = -psi(2Q);  U = Q + T, T = psi(U);  U = Q + T, T = psi(U);  U = Q + T;   member iff U == -P,
// since Q + psi(Q + psi(Q - psi(2Q))) = Q + psi(Q) + psi^2(Q) - psi^3(2Q): one 63-bit ladder, one doubling, three psi, three
// additions and one comparison, and the three additions are one loop body, so the kernel holds one copy of the full addition.
// (The loop applies psi after the last addition too and the comparison is psi(U) == -psi(P).)
//
// Which additions are ordinary (distinct, non-opposite, finite operands), and which are not known to be:
//  - the ladder.  The accumulator is [k]P for the prefixes k of x0, a step doubles it and adds P where the bit is set.  Every
//    point of E'(Fq2) other than O has an order d > 1 that divides r h, h = 2p - r = 10069 * 5864401 * 1875725156269 * (a
//    178-bit prime).  [2k]P is O, P or -P only if d divides 2k, 2k - 1 or 2k + 1, and then so does a prime of r h; no prefix k of
//    x0 has 2k = 0 or +-1 modulo one of the five primes (the two large ones exceed 2 x0 + 1; the three small ones are checked by
//    tests/test_g2_subgroup_cpu.py), so on points of the curve the ladder never meets an exceptional case.  g2_madd still
//    answers all of them (an infinite accumulator, equal and opposite points): the ladder does not rest on the argument;
//  - 2Q: E'(Fq2) has odd order, so no point has y = 0 and a doubling of a finite point is finite; g2_double keeps Z = 0 for O;
//  - Q + T (three times) and the comparison: the operands depend on P through psi, nothing is known about them - T is O
//    for instance whenever psi(2Q) is, and U == -P is the very question.  g2_add_lean, the complete law of pt_add_complete
//    (chain_scan.h), and a comparison that cross-multiplies and knows O (P and psi(P) are finite).
// One lane per point, like k_root; x0 is a compile-time constant, so every lane of a wave doubles and adds in the same
// steps.  P stays affine through the ladder (mixed addition, Z2 = 1).
#include <climits>
#include "g2_endo.h"
#include "proven_jobs.h"

namespace {

constexpr int G2S_LANES = 64;

// points: n x 16 canonical words (x.c0, x.c1, y.c0, y.c1), every coordinate below p; flags: n bytes.  A point off the curve
// writes no flag and lowers *bad_idx to its index.
__global__ __launch_bounds__(G2S_LANES) void k_g2_subgroup(const u64* __restrict__ points, size_t n, unsigned char* __restrict__ flags,
                                                           unsigned* __restrict__ bad_idx) {
  const size_t k = (size_t)blockIdx.x * G2S_LANES + threadIdx.x;
  if (k >= n) return;
  fq2 px = fq2_from_canonical(points + 16 * k), py = fq2_from_canonical(points + 16 * k + 8);
  if (!g2_on_twist(px, py)) {
    atomicMin(bad_idx, (unsigned)k);
    return;
  }
  g2j q;  // [x0]P: the top bit of x0, then 62 steps
  q.x = px;
  q.y = py;
  q.z = fq2_one();
#pragma unroll 1
  for (int i = 61; i >= 0; i--) {
    q = g2_double(q);
    if ((G2S_X0 >> i) & 1) q = g2_madd(q, px, py);  // the same branch in every lane
  }
  g2j t = g2_psi(g2_double(q));
  t.y = fq2_neg(t.y);
  // three times T = psi(Q + T): the last psi is one too many for the Horner form, so the comparison happens in its image,
  // psi(U) == -psi(P) (psi is injective: psi^2 - t psi + p = 0 gives (t - psi) psi = p, and E'(Fq2) has no p-torsion).  Only T
  // lives across the loop that way, not U beside it.
#pragma unroll 1
  for (int i = 0; i < 3; i++) t = g2_psi(g2_add_lean(t, q));
  q.x = px;
  q.y = py;
  q = g2_psi(q);  // (Z is not used)
  flags[k] = g2_is_neg_of_affine(t, q.x, q.y) ? 1 : 0;
}

bool front_args_ok(const uint64_t* points, size_t n, const uint8_t* flags_out) {
  return points && flags_out && n > 0 && n < (size_t)UINT_MAX;  // the first bad index travels as a 32-bit word
}

// The front-end into host memory: flags[n].  Nothing is written on an error.
int subgroup_front(bn254s_ctx* c, const uint64_t* points, size_t n, uint8_t* flags) {
  if (!coords_below_p(c, "g2_subgroup_check", "point", COORD_G2, 4, points, n)) return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words("g2sub", 16 * n /* points */ + 1 /* bad_idx */ + nb /* flags */);
  if (!d) return BN254S_E_OOM;
  u64* d_pts = d;
  unsigned* d_bad = (unsigned*)(d_pts + 16 * n);
  unsigned char* d_flags = (unsigned char*)(d_pts + 16 * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_pts, points, n * 128, hipMemcpyHostToDevice, st));
  k_g2_subgroup<<<(unsigned)((n + G2S_LANES - 1) / G2S_LANES), G2S_LANES, 0, st>>>(d_pts, n, d_flags, d_bad);
  HIP_TRY(c, hipGetLastError());
  unsigned h_bad = UINT_MAX;
  HIP_TRY(c, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_bad != UINT_MAX) {
    c->set_err("g2_subgroup_check: point_" + std::to_string(h_bad) + " is not on the twist curve y^2 = x^3 + b'");
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_g2_subgroup_check_batch(bn254s_ctx* c, const uint64_t* points, size_t n, uint8_t* flags_out) {
  if (!c || !front_args_ok(points, n, flags_out)) return BN254S_E_INVALID_ARG;
  return subgroup_front(c, points, n, flags_out);
}

extern "C" int bn254s_g2_subgroup_check(bn254s_ctx* c, const bn254s_params* params, const uint64_t* points, const uint64_t* offsets,
                                        size_t n, size_t per_proof, uint8_t* flags_out, uint64_t* g2_jobs, bn254s_proof** g2_proofs) {
  int rc = proven_args(c, "g2_subgroup_check", "G2 proof", front_args_ok(points, n, flags_out) && offsets, params, g2_proofs, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  // (the trace generator takes canonical words; before any output is written)
  if (!coords_below_p(c, "g2_subgroup_check", "offset", COORD_G2, 4, offsets, n)) return BN254S_E_INVALID_ARG;
  std::vector<uint8_t> flags(n);
  rc = subgroup_front(c, points, n, flags.data());
  if (rc != BN254S_OK) return rc;
  std::vector<u64> r(4 * n), outs;
  for (size_t i = 0; i < n; i++) memcpy(r.data() + 4 * i, G2S_R, 32);
  rc = prove_and_collect(c, "g2_subgroup_check", 1, params, r.data(), points, offsets, n, per_proof, g2_proofs, outs);
  if (rc != BN254S_OK) return rc;  // (BN254S_E_INVALID_POINT: the caller draws another offset)
  // linkage: the trace generator computes R_i + [r]P_i bit by bit on its own; it must be R_i exactly where the flag is set
  for (size_t j = 0; j < n; j++) {
    const bool back = memcmp(outs.data() + 16 * j, offsets + 16 * j, 128) == 0;
    if (back != (flags[j] != 0)) {
      c->set_err("g2_subgroup_check: the proven R + [r]P of point " + std::to_string(j) +
                 (back ? " is R, but its flag is clear" : " is not R, but its flag is set"));
      release_proofs(g2_proofs, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  }
  memcpy(flags_out, flags.data(), n);
  if (g2_jobs)
    for (size_t i = 0; i < n; i++) {
      memcpy(g2_jobs + 20 * i, G2S_R, 32);
      memcpy(g2_jobs + 20 * i + 4, points + 16 * i, 128);
    }
  return BN254S_OK;
}
