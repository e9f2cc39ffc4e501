// Job outputs without a proof: s_i x_i + offset_i on G1 and on the twist curve E'(Fq2), x_i^s_i in Fq, for n independent jobs
// that each bring their own 256-bit scalar.  It is what the reference's G1SingleGenerator / G2SingleGenerator / FqSingleGenerator
// compute with arkworks, one call after the other on one host thread (src/generators/{g1,g2,fq}/single.rs:48-52), so that the rest
// of the circuit can go on before the STARK of the same jobs is proven.
//   k_job_outputs<G1 | G2 | FqExp>: one lane per job, blocks of 64 lanes: the on-curve test of x_i and offset_i, the fixed-window
//                                   ladder of window_ladder.h over the lane's scalar, + offset_i, one inversion, canonical words
//   [bn254s_job_outputs only: bn254s_prove_batch of the same jobs, then the outputs of the proofs against the kernel's, word for word]
// The scalar is used as the 256-bit value it is, never reduced modulo r: on the twist s x != (s mod r) x for a point outside the
// r-torsion subgroup, and the G2 trace walks all 256 bits.  (On G1 a reduction would give the same point; none is made.)
//
// Windows.  The lane's table [1]x .. [2^W - 1]x is LDS, tab[entry][limb][lane], 4 (2^W - 1) NL 64 bytes for a block:
//   G1     W = 3   7 x 30 limbs   53 760 B        86 windows (the first one bit), 255 doublings + 85 additions
//   G2     W = 2   3 x 60 limbs   46 080 B       128 windows,                     254 doublings + 127 additions
//   Fq     W = 4  15 x 10 limbs   38 400 B        64 windows,                     252 squarings + 63 products
// (the largest windows whose table stays below the 64 KB of static LDS a block may have).
//
// Which additions are ordinary (distinct, non-opposite, finite operands), and which are not known to be:
//  - the table, [e]x = [e - 1]x + x for 3 <= e <= 2^W - 1 <= 7 after [2]x = the doubling of x.  x is a finite point of its curve.
//    G1 has the prime order r and the twist the odd order r (2p - r) whose smallest prime is 10069, so [k]x is O for no
//    0 < k <= 8: every entry is finite, and [e - 1]x = +-x would make [e - 2]x or [e]x vanish.  Ordinary; the complete law is
//    called all the same, it is the one addition this file has;
//  - the ladder, acc + [d]x with acc = [2^W m]x for the prefix m of the scalar: NOT ordinary.  acc is O while m = 0 (small
//    scalars, and the first window of every scalar below 2^(256 - W0) for its W0 = 1, 2 bits: 2^255 on G1, 2^254 on G2) and whenever the order of x divides 2^W m (s a multiple of r on
//    G1; a twist point of order 10069 with m = 10069); the digit d = 0 adds O; acc = [d]x where 2^W m = d modulo the order
//    (a doubling) and acc = -[d]x where 2^W m + d = 0 modulo the order (s = r on G1 ends that way: [r - 1]x + x).  The complete
//    law pt_add_lean, which branches on exactly these cases and on nothing else;
//  - the last addition, [s]x + offset: NOT ordinary.  [s]x may be O (the output is the offset), equal to the offset (s = 1 with
//    offset = x: a doubling) or its negative (offset = -[s]x: the output is O, finite = 0, zero words).  pt_add_lean again, with
//    the offset as a Jacobian point of Z = 1.  A mixed addition would save 3 of its 11 products and 2 of its 5 squarings
//    (g2_madd of g2_endo.h fits on the twist as it is), once in about 128 additions and 255 doublings per job; G1 has no
//    mixed law yet, and a second addition law inlined beside the first is more code for the one kernel than that is worth.
// The doublings need no care: no point of either curve has y = 0 (both orders are odd), and the doubling of Z = 0 has Z = 0.
// Fq-exp has no exceptional case: a zero digit multiplies by 1, 0^0 = 1 as the trace has it (a = 1 in its first row).
// Control flow depends on the lane's scalar only inside pt_add_lean; digits select table entries as data.
#include <cstring>
#include <string>
#include <vector>
#include "job_curve.h"
#include "job_device.h"
#include "proven_jobs.h"

namespace {

struct FqExp {
  using E = fq;
  static constexpr bool IS_CURVE = false;
  static constexpr int W = 4, NL = FQ_NL, KIND = 2, FW = 4, PW = 4;
  static __device__ __forceinline__ E dbl(const E& a) { return fq_sqr(a); }
  static __device__ __forceinline__ E add(const E& a, const E& b) { return fq_mul(a, b); }
  static __device__ __forceinline__ void identity_if(E& q, bool flag) {
#pragma unroll
    for (int j = 0; j < FQ_NL; j++) q.l[j] = flag ? FQ_ONE[j] : q.l[j];
  }
};

// scalars: n x 4 words; x, offset: n x PW canonical words, every coordinate below p (offset is not read by Fq-exp); out: n x PW
// canonical words, zeros where the output is O; finite: n bytes.  A job whose x (offset) is off its curve writes nothing and
// lowers bad[0] (bad[1]) to its index.
template <class C>
__global__ __launch_bounds__(WL_LANES) void k_job_outputs(const u64* __restrict__ scalars, const u64* __restrict__ x,
                                                          const u64* __restrict__ offset, size_t n, u64* __restrict__ out,
                                                          unsigned char* __restrict__ finite, unsigned* __restrict__ bad) {
  __shared__ u32 tab[(1 << C::W) - 1][C::NL][WL_LANES];
  const size_t k = (size_t)blockIdx.x * WL_LANES + threadIdx.x;
  if (k >= n) return;
  typename C::E acc;
  if constexpr (C::IS_CURVE) {
    typename C::E r;  // (the offset is read again after the ladder rather than kept in registers beside it)
    const bool x_ok = C::load(x + C::PW * k, acc), off_ok = C::load(offset + C::PW * k, r);
    if (!x_ok) atomicMin(bad, (unsigned)k);
    if (!off_ok) atomicMin(bad + 1, (unsigned)k);
    if (!x_ok || !off_ok) return;
  } else {
    acc = fq_from_canonical(x + C::PW * k);
  }
  u64 s[4] = {scalars[4 * k], scalars[4 * k + 1], scalars[4 * k + 2], scalars[4 * k + 3]};
  acc = wl_ladder<C>(tab, acc, s);
  u64* o = out + C::PW * k;
  if constexpr (C::IS_CURVE) {
    typename C::E r;
    C::load(offset + C::PW * k, r);
    acc = pt_add_lean(acc, r);
    const bool inf = pt_inf(acc);
    finite[k] = inf ? 0 : 1;
    if (inf) {
#pragma unroll
      for (int w = 0; w < C::PW; w++) o[w] = 0;
      return;
    }
    const auto zi = fe_inv(acc.z), zi2 = fe_sqr(zi);
    fe_store_canonical(o, fe_mul(acc.x, zi2));
    fe_store_canonical(o + C::FW, fe_mul(fe_mul(acc.y, zi), zi2));
  } else {
    finite[k] = 1;
    fe_store_canonical(o, acc);
  }
}

}  // namespace

int bn254s_job_outputs_device(bn254s_ctx* c, int kind, const u64* d_scalars, const u64* d_x, const u64* d_offset, size_t n, u64* d_out,
                              unsigned char* d_finite, unsigned* d_bad) {
  const unsigned blocks = (unsigned)((n + WL_LANES - 1) / WL_LANES);
  hipStream_t st = c->stream;
  if (kind == 0) k_job_outputs<G1><<<blocks, WL_LANES, 0, st>>>(d_scalars, d_x, d_offset, n, d_out, d_finite, d_bad);
  else if (kind == 1) k_job_outputs<G2><<<blocks, WL_LANES, 0, st>>>(d_scalars, d_x, d_offset, n, d_out, d_finite, d_bad);
  else k_job_outputs<FqExp><<<blocks, WL_LANES, 0, st>>>(d_scalars, d_x, d_offset, n, d_out, d_finite, d_bad);
  HIP_TRY(c, hipGetLastError());
  return BN254S_OK;
}

namespace {

// The front-end into host memory: outputs[n x PW], finite[n].  Nothing is written on an error.
int jobout_front(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                 uint64_t* outputs, uint8_t* finite) {
  const char* const* coord = kind == 0 ? COORD_G1 : COORD_G2;  // (not read for the one coordinate of kind 2)
  const size_t PW = point_words(kind);
  const bool curve = kind != 2;
  if (!coords_below_p(c, "job_outputs", "x", coord, (int)PW / 4, x, n) ||
      (curve && !coords_below_p(c, "job_outputs", "offset", coord, (int)PW / 4, offset, n)))
    return BN254S_E_INVALID_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t nb = (n + 7) / 8;  // words that hold n bytes
  u64* d = c->words("jobout", 4 * n /* scalars */ + 3 * PW * n /* x, offset, outputs */ + 1 /* bad */ + nb /* finite */);
  if (!d) return BN254S_E_OOM;
  u64 *d_s = d, *d_x = d + 4 * n, *d_off = d_x + PW * n, *d_out = d_off + PW * n;
  unsigned* d_bad = (unsigned*)(d_out + PW * n);
  unsigned char* d_fin = (unsigned char*)(d_out + PW * n + 1);
  HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  if (curve) HIP_TRY(c, hipMemcpyAsync(d_off, offset, n * PW * 8, hipMemcpyHostToDevice, st));
  const int rc = bn254s_job_outputs_device(c, kind, d_s, d_x, d_off, n, d_out, d_fin, d_bad);
  if (rc != BN254S_OK) return rc;
  unsigned h_bad[2] = {UINT_MAX, UINT_MAX};
  HIP_TRY(c, hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h_bad[0] != UINT_MAX || h_bad[1] != UINT_MAX) {
    const bool is_x = h_bad[0] <= h_bad[1];  // the smaller index; x before offset at the same one
    c->set_err(std::string("job_outputs: ") + (is_x ? "x_" : "offset_") + std::to_string(is_x ? h_bad[0] : h_bad[1]) +
               (kind == 0 ? " is not on the curve y^2 = x^3 + 3" : " is not on the twist curve y^2 = x^3 + b'"));
    return BN254S_E_INVALID_ARG;
  }
  HIP_TRY(c, hipMemcpyAsync(outputs, d_out, n * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(finite, d_fin, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_job_outputs_batch(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset,
                                        size_t n, uint64_t* outputs_out, uint8_t* finite_out) {
  if (!c || !finite_out || !batch_args_ok(kind, scalars, x, offset, n, outputs_out)) return BN254S_E_INVALID_ARG;
  return jobout_front(c, kind, scalars, x, offset, n, outputs_out, finite_out);
}

extern "C" int bn254s_job_outputs(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                                  const uint64_t* offset, size_t n, size_t per_proof, uint64_t* outputs_out, bn254s_proof** proofs_out) {
  int rc = proven_args(c, "job_outputs", "proof", batch_args_ok(kind, scalars, x, offset, n, outputs_out), params, proofs_out, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  const size_t PW = point_words(kind);
  std::vector<u64> outs(PW * n), proven;
  std::vector<uint8_t> finite(n);
  rc = jobout_front(c, kind, scalars, x, offset, n, outs.data(), finite.data());
  if (rc != BN254S_OK) return rc;
  for (size_t i = 0; i < n; i++)
    if (!finite[i]) {  // the reference's targets cannot hold the point at infinity: no such job can be proven
      c->set_err("job_outputs: the output of job " + std::to_string(i) + " is the point at infinity");
      return BN254S_E_INVALID_POINT;
    }
  rc = prove_and_collect(c, "job_outputs", kind, params, scalars, x, offset, n, per_proof, proofs_out, proven);
  if (rc != BN254S_OK) return rc;
  // linkage: the trace generator computes every output bit by bit on its own; it must be the front-end's, word for word
  for (size_t j = 0; j < n; j++)
    if (memcmp(proven.data() + PW * j, outs.data() + PW * j, 8 * PW) != 0) {
      c->set_err("job_outputs: the proven output of job " + std::to_string(j) + " is not the front-end's");
      release_proofs(proofs_out, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  memcpy(outputs_out, outs.data(), 8 * PW * n);
  return BN254S_OK;
}
