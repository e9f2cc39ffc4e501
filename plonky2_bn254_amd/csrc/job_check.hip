// Which curve jobs can be proven: the double-and-add walk of the scalar-multiplication traces (trace_common.h: k_sum_scan; the
// reference's generate_one_set, scalar_mul_stark.rs:92-213) adds sum_k + dbl_k in every adding row, whether or not bit k of the
// scalar is set, and the addition gadget cannot take opposite points (add.rs:49-51).  With dbl_0 = x, sum_0 = offset:
//   step k hits iff sum_k == -dbl_k;  otherwise sum_{k+1} = sum_k + dbl_k where bit k is set (equal points double: provable),
//   sum_k where it is clear;  dbl_{k+1} = 2 dbl_k.
// A job is provable iff none of its 256 steps hits (DESIGN.md "Job check"); a prover meets the first hit in row 2k of the job's
// 512-row frame and can only answer BN254S_E_INVALID_POINT for the whole proof.
//   k_job_check<G1 | G2>: one lane per job, blocks of 64 lanes: the on-curve test of x_i and offset_i as k_job_outputs makes it,
//                         then the walk in Jacobian coordinates without an inversion; the first hitting k, or 0xFFFF
//   [bn254s_prove_batch_checked only: bn254s_prove_batch of the same jobs if every one of them is provable]
// The scalar is the 256-bit value it is, never reduced: the trace walks all 256 bits.
//
// The hit is what g1_add / g2_add (fq_dev.h) report as code 2, from the cross-multiplied coordinates they compute anyway.  The
// whole addition is made in every step and kept where the bit is set: lanes of a wave differ in their bits, so a cheaper test
// for clear bits would only run beside the additions of the other lanes, not instead of them.
// No operand is ever the point at infinity: the offset is finite, a sum becomes infinite only in a hit, which ends the lane,
// and no doubling is infinite (both group orders are odd).
//
// Both points live in LDS between their uses, pts[sum | dbl][limb][lane] as window_ladder.h keeps its table (a wave touches
// 64 consecutive words, a lane reads only what it wrote: no barrier): 2 x 30 x 64 x 4 = 15 360 B on G1, 30 720 B on G2.  Two
// Jacobian points of the twist beside the temporaries of an addition do not fit in 256 registers; held this way the addition
// has its two operands and the doubling its one, and nothing else is alive across them but the scalar and the step.
#include <cstring>
#include <string>
#include <vector>
#include "job_curve.h"
#include "job_device.h"
#include "proven_jobs.h"

namespace {

constexpr unsigned STEP_NONE = BN254S_JOB_STEP_NONE;

// scalars: n x 4 words; x, offset: n x PW canonical words, every coordinate below p; step: n half-words.  A job whose x (offset)
// is off its curve writes nothing and lowers bad[0] (bad[1]) to its index.
template <class C>
__global__ __launch_bounds__(WL_LANES) void k_job_check(const u64* __restrict__ scalars, const u64* __restrict__ x,
                                                        const u64* __restrict__ offset, size_t n, unsigned short* __restrict__ step,
                                                        unsigned* __restrict__ bad) {
  using E = typename C::E;
  __shared__ u32 pts[2][C::NL][WL_LANES];  // 0: the running sum, 1: the doubling
  const size_t i = (size_t)blockIdx.x * WL_LANES + threadIdx.x;
  if (i >= n) return;
  {
    E d, sum;
    const bool x_ok = C::load(x + C::PW * i, d), off_ok = C::load(offset + C::PW * i, sum);
    if (!x_ok) atomicMin(bad, (unsigned)i);
    if (!off_ok) atomicMin(bad + 1, (unsigned)i);
    if (!x_ok || !off_ok) return;
    wl_put(pts, 0, sum);
    wl_put(pts, 1, d);
  }
  u64 s[4] = {scalars[4 * i], scalars[4 * i + 1], scalars[4 * i + 2], scalars[4 * i + 3]};
  unsigned hit = STEP_NONE;
#pragma unroll 1
  for (int k = 0; k < 256; k++) {
    E d;
    {
      E sum, r;
      wl_get(pts, 0, sum);
      wl_get(pts, 1, d);
      if (pt_add(sum, d, r) == 2) {
        hit = k;
        break;
      }
      if (s[0] & 1) wl_put(pts, 0, r);
    }
    s[0] = (s[0] >> 1) | (s[1] << 63);  // bit k + 1 comes down to bit 0
    s[1] = (s[1] >> 1) | (s[2] << 63);
    s[2] = (s[2] >> 1) | (s[3] << 63);
    s[3] >>= 1;
    wl_get(pts, 1, d);
    wl_put(pts, 1, pt_double(d));
  }
  step[i] = (unsigned short)hit;
}

}  // namespace

int bn254s_job_check_device(bn254s_ctx* c, int kind, const u64* d_scalars, const u64* d_x, const u64* d_offset, size_t n,
                            unsigned short* d_step, unsigned* d_bad) {
  const unsigned blocks = (unsigned)((n + WL_LANES - 1) / WL_LANES);
  if (kind == 0) k_job_check<G1><<<blocks, WL_LANES, 0, c->stream>>>(d_scalars, d_x, d_offset, n, d_step, d_bad);
  else k_job_check<G2><<<blocks, WL_LANES, 0, c->stream>>>(d_scalars, d_x, d_offset, n, d_step, d_bad);
  HIP_TRY(c, hipGetLastError());
  return BN254S_OK;
}

namespace {

// The front-end into host memory: provable[n] and, where it is asked for, step[n].  Nothing is written on an error.
int jobchk_front(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, size_t n,
                 uint8_t* provable, uint16_t* step) {
  const char* const* coord = kind == 0 ? COORD_G1 : COORD_G2;  // (not read for the one coordinate of kind 2)
  const size_t PW = point_words(kind);
  const bool curve = kind != 2;
  if (!coords_below_p(c, "job_check", "x", coord, (int)PW / 4, x, n) ||
      (curve && !coords_below_p(c, "job_check", "offset", coord, (int)PW / 4, offset, n)))
    return BN254S_E_INVALID_ARG;
  std::vector<uint16_t> h_step(n, (uint16_t)STEP_NONE);
  if (curve) {  // (an Fq exponentiation has no exceptional case: every job is provable, nothing is launched)
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    u64* d = c->words("jobchk", 4 * n /* scalars */ + 2 * PW * n /* x, offset */ + 1 /* bad */ + (n + 3) / 4 /* steps */);
    if (!d) return BN254S_E_OOM;
    u64 *d_s = d, *d_x = d + 4 * n, *d_off = d_x + PW * n;
    unsigned* d_bad = (unsigned*)(d_off + PW * n);
    unsigned short* d_step = (unsigned short*)(d_off + PW * n + 1);
    HIP_TRY(c, hipMemsetAsync(d_bad, 0xFF, 8, st));
    HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_off, offset, n * PW * 8, hipMemcpyHostToDevice, st));
    const int rc = bn254s_job_check_device(c, kind, d_s, d_x, d_off, n, d_step, d_bad);
    if (rc != BN254S_OK) return rc;
    unsigned h_bad[2] = {UINT_MAX, UINT_MAX};
    HIP_TRY(c, hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h_step.data(), d_step, n * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (h_bad[0] != UINT_MAX || h_bad[1] != UINT_MAX) {
      const bool is_x = h_bad[0] <= h_bad[1];  // the smaller index; x before offset at the same one
      c->set_err(std::string("job_check: ") + (is_x ? "x_" : "offset_") + std::to_string(is_x ? h_bad[0] : h_bad[1]) +
                 (kind == 0 ? " is not on the curve y^2 = x^3 + 3" : " is not on the twist curve y^2 = x^3 + b'"));
      return BN254S_E_INVALID_ARG;
    }
  }
  for (size_t i = 0; i < n; i++) provable[i] = h_step[i] == STEP_NONE;
  if (step) memcpy(step, h_step.data(), n * 2);
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_job_check_batch(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset,
                                      size_t n, uint8_t* provable_out, uint16_t* step_out) {
  if (!c || !batch_args_ok(kind, scalars, x, offset, n, provable_out)) return BN254S_E_INVALID_ARG;
  return jobchk_front(c, kind, scalars, x, offset, n, provable_out, step_out);
}

extern "C" int bn254s_prove_batch_checked(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars,
                                          const uint64_t* x, const uint64_t* offset, size_t n, size_t per_proof, uint8_t* provable_out,
                                          uint16_t* step_out, bn254s_proof** proofs_out) {
  int rc = proven_args(c, "prove_batch_checked", "proof", batch_args_ok(kind, scalars, x, offset, n, scalars), params, proofs_out, n,
                       per_proof);
  if (rc != BN254S_OK) return rc;
  std::vector<uint8_t> provable(n);
  std::vector<uint16_t> step(n);
  rc = jobchk_front(c, kind, scalars, x, offset, n, provable.data(), step.data());
  if (rc != BN254S_OK) return rc;
  // the answer of the check is the caller's whether or not anything is proven
  if (provable_out) memcpy(provable_out, provable.data(), n);
  if (step_out) memcpy(step_out, step.data(), n * 2);
  for (size_t i = 0; i < n; i++)
    if (!provable[i]) {
      c->set_err("prove_batch_checked: job " + std::to_string(i) + " cannot be proven: sum == -double at step " + std::to_string(step[i]) +
                 " (row " + std::to_string(2 * step[i]) + " of its frame)");
      return BN254S_E_INVALID_POINT;
    }
  std::vector<u64> outs;
  return prove_and_collect(c, "prove_batch_checked", kind, params, scalars, x, offset, n, per_proof, proofs_out, outs);
}
