// Scalar multiplication without an offset argument: s_i x_i for n independent jobs on G1 and on the twist curve E'(Fq2), with
// the offset that the statement s x + offset needs drawn, checked and, where the job cannot be proven with it, drawn again on
// the device.  The reference does this by hand around every scalar multiplication (src/utils/g1_msm.rs:22-36, the tail of
// map_to_g2 in src/utils/hash_to_g2.rs:184-201, src/generators/g{1,2}/random.rs): set_random_g{1,2} for an offset R, the
// multiplication, then minus R.  Here (DESIGN.md "Scalar multiplication without an offset"):
//   offset_i^(a) = hash_to_g1 | hash_to_g2 (seed[0..3], i mod 2^32, i >> 32, a, 0x62736D00 + kind),  a = 0, 1, ...
//   job i takes the smallest a < max_attempts whose (s_i, x_i, offset_i^(a)) the traces can prove (job_check.hip)
//   output_i = s_i x_i + offset_i,  product_i = output_i - offset_i
// Rounds, one per attempt, over a list of jobs (round 0: all of them; later: the jobs just rejected, a handful at most), run by
// draw_rounds (offset_draw.h: k_draw_inputs, the hash, k_draw_compact), which msm.hip uses for its MSMs too.  A round here:
//   k_smul_gather    rounds after the first: the scalars and x of the listed jobs side by side
//   [k_job_check of the listed jobs with the drawn points as their offsets: job_check.hip]
//   k_smul_accept    a provable job keeps its drawn point as its offset; every other one is marked and counted
// then
//   [k_job_outputs: s x + offset by the window ladder, job_outputs.hip]
//   k_smul_sub       output - offset: equal (O), opposite (a doubling) and general, one inversion, canonical words, on-curve self-check
// Scalars, points, offsets, steps and flags stay on the device between these steps; the final arrays are copied out once.
//
// The inversion of k_smul_sub is one fe_inv per lane, not the batched inversion of msm.hip: the subtraction follows a ladder of
// 255 doublings and 85 (G1) / 127 (G2) additions per lane, beside which one Fermat inversion is about a tenth; a batched one
// would share it among the 64 lanes of a block at the price of a scan through LDS and two barriers in a kernel that has none.
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "job_curve.h"
#include "job_device.h"
#include "offset_draw.h"
#include "proven_jobs.h"

namespace {

constexpr u64 SMUL_DOMAIN = 0x62736D00;  // "bsm\0" + kind: the last hash input
constexpr unsigned SMUL_STEP_UNSET = 0xFEFE;  // what the step of a job is before k_job_check writes it (it writes none for a bad point)

// CTL_ERR beyond CTL_ERR_DRAW (offset_draw.h)
enum { SMUL_ERR_DRAW_INF = 2 /* a drawn G2 point is O */, SMUL_ERR_OUT_INF = 3 /* the output of a provable job is O */,
       SMUL_ERR_OPPOSITE = 4 /* equal x, y neither equal nor opposite */, SMUL_ERR_CURVE = 5 /* the product is off its curve */ };

// cs, cx: m x 4, m x pw words, the scalars and x of the listed jobs
__global__ __launch_bounds__(256) void k_smul_gather(const unsigned* __restrict__ list, size_t m, int pw, const u64* __restrict__ scalars,
                                                     const u64* __restrict__ x, u64* __restrict__ cs, u64* __restrict__ cx) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const size_t i = list[j];
  for (int w = 0; w < 4; w++) cs[4 * j + w] = scalars[4 * i + w];
  for (int w = 0; w < pw; w++) cx[(size_t)pw * j + w] = x[(size_t)pw * i + w];
}

// step: the m steps k_job_check found for the listed jobs with the drawn points `at.points` as their offsets.  A provable job
// copies its point to offset[i]; a job with a hit is marked in rejected[i], keeps the step in last_step[i] and is counted in
// *count, as is a job whose step was never written (k_job_check has lowered bad[] for it: the host reads on).
__global__ __launch_bounds__(256) void k_smul_accept(const unsigned* __restrict__ list, size_t m, int pw, const unsigned short* __restrict__ step,
                                                     HashedPoints at, u64* __restrict__ offset, unsigned char* __restrict__ rejected,
                                                     unsigned short* __restrict__ last_step, unsigned* __restrict__ ctl, int round) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  if (j == 0) draw_self_check(at, ctl);
  if (at.finite && !at.finite[j]) atomicCAS(ctl + CTL_ERR, 0u, (unsigned)SMUL_ERR_DRAW_INF);
  const size_t i = list ? list[j] : j;
  const unsigned st = step[j];
  if (st == BN254S_JOB_STEP_NONE) {
    for (int w = 0; w < pw; w++) offset[(size_t)pw * i + w] = at.points[(size_t)pw * j + w];
    rejected[i] = 0;
    return;
  }
  rejected[i] = st == SMUL_STEP_UNSET ? 0 : 1;
  last_step[i] = (unsigned short)st;
  atomicAdd(ctl + CTL_COUNT + round, 1u);
}

// product = output - offset for affine, canonical points of the curve C (pt_sub_slope, pt_sub_point: job_curve.h); out_finite: what
// k_job_outputs said of the output.  output == offset: the product is O, zero words and finite = 0 (s x = O).  Otherwise the
// product must be on the curve again.
template <class C>
__global__ __launch_bounds__(64) void k_smul_sub(const u64* __restrict__ output, const u64* __restrict__ offset,
                                                 const unsigned char* __restrict__ out_finite, size_t n, u64* __restrict__ product,
                                                 unsigned char* __restrict__ finite, unsigned* __restrict__ ctl) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  u64* o = product + C::PW * k;
  if (!out_finite[k]) {  // (a provable job has a finite output: its last sum is one)
    atomicCAS(ctl + CTL_ERR, 0u, (unsigned)SMUL_ERR_OUT_INF);
    return;
  }
  typename C::F x1, y1, x2, y2, num, den, x3, y3;
  fe_from_canonical(output + C::PW * k, x1);
  fe_from_canonical(output + C::PW * k + C::FW, y1);
  fe_from_canonical(offset + C::PW * k, x2);
  fe_from_canonical(offset + C::PW * k + C::FW, y2);
  const int which = pt_sub_slope(x1, y1, x2, y2, num, den);
  if (which == SUB_EQUAL) {
    finite[k] = 0;
#pragma unroll
    for (int w = 0; w < C::PW; w++) o[w] = 0;
    return;
  }
  if (which == SUB_SAME_X) {
    atomicCAS(ctl + CTL_ERR, 0u, (unsigned)SMUL_ERR_OPPOSITE);
    return;
  }
  pt_sub_point(x1, y1, x2, num, den, x3, y3);
  if (!on_curve(x3, y3)) {
    atomicCAS(ctl + CTL_ERR, 0u, (unsigned)SMUL_ERR_CURVE);
    return;
  }
  finite[k] = 1;
  fe_store_canonical(o, x3);
  fe_store_canonical(o + C::FW, y3);
}

const char* smul_err_text(unsigned e) {
  switch (e) {
    case CTL_ERR_DRAW: return "a drawn offset failed the self-check of its hash-to-curve kernel";
    case SMUL_ERR_DRAW_INF: return "a drawn offset is the point at infinity";
    case SMUL_ERR_OUT_INF: return "the output of a provable job is the point at infinity";
    case SMUL_ERR_OPPOSITE: return "an output shares x with its offset and is neither it nor its negative";
    default: return "a product is not on its curve";
  }
}

// The predicate of both entry points on their own arguments, every check that needs no device.  The first coordinate of x that
// is not below p names itself where there is a context to hold the text.
bool smul_args_ok(bn254s_ctx* c, const char* tag, int kind, const uint64_t* scalars, const uint64_t* x, size_t n, const uint64_t* seed,
                  int max_attempts, const void* products, const void* finite, const void* offsets) {
  if (kind < 0 || kind > 1 || !scalars || !x || !seed || !products || !finite || !offsets || n == 0 || n >= (size_t)UINT_MAX ||
      max_attempts < 1 || max_attempts > DRAW_MAX_ATTEMPTS || !seed_canonical(seed))
    return false;
  return coords_below_p(c, tag, "x", kind == 0 ? COORD_G1 : COORD_G2, (int)point_words(kind) / 4, x, n);
}

// The front-end into host memory: products, offsets, outputs [n x PW], finite and attempts [n].  Nothing is written on an error.
int smul_front(bn254s_ctx* c, const char* tag, int kind, const uint64_t* scalars, const uint64_t* x, size_t n, const uint64_t* seed,
               int max_attempts, uint64_t* products, uint8_t* finite, uint64_t* offsets, uint64_t* outputs, uint8_t* attempts) {
  const std::string who = std::string(tag) + ": ";
  const size_t PW = point_words(kind), nb = (n + 7) / 8 /* words that hold n bytes */;
  const size_t hw = draw_device_words(kind, n);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("smul", 2 * (4 + PW) * n /* scalars, x and their gathered copies */ + 3 * PW * n /* offset, output, product */ +
                                8 * n /* hash inputs */ + hw + 4 * nb /* attempts, rejected, out_finite, finite */ +
                                2 * ((n + 3) / 4) /* step, last_step */ + (n + 1) / 2 /* list */ + CTL_WORDS / 2);
  if (!d) return BN254S_E_OOM;
  u64 *d_s = d, *d_x = d_s + 4 * n, *d_cs = d_x + PW * n, *d_cx = d_cs + 4 * n, *d_off = d_cx + PW * n, *d_out = d_off + PW * n;
  u64 *d_prod = d_out + PW * n, *d_in = d_prod + PW * n, *d_hash = d_in + 8 * n, *d_bytes = d_hash + hw;
  unsigned char *d_att = (unsigned char*)d_bytes, *d_rej = (unsigned char*)(d_bytes + nb);
  unsigned char *d_ofin = (unsigned char*)(d_bytes + 2 * nb), *d_fin = (unsigned char*)(d_bytes + 3 * nb);
  unsigned short *d_step = (unsigned short*)(d_bytes + 4 * nb), *d_last = d_step + 4 * ((n + 3) / 4);
  unsigned* d_list = (unsigned*)(d_last + 4 * ((n + 3) / 4));
  unsigned* d_ctl = d_list + 2 * ((n + 1) / 2);
  int rc = draw_ctl_clear(c, d_ctl);  // (CTL_CHK_BAD is not used here and stays at UINT_MAX)
  if (rc != BN254S_OK) return rc;
  HIP_TRY(c, hipMemsetAsync(d_att, 0, 2 * nb * 8, st));  // attempts and rejected
  HIP_TRY(c, hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_x, x, n * PW * 8, hipMemcpyHostToDevice, st));
  const char* curve = curve_name(kind);
  auto fail_ctl = [&](const unsigned* h_ctl) -> int {  // what the control words say beyond a count; BN254S_OK if nothing
    if (h_ctl[CTL_BAD] != UINT_MAX) {
      c->set_err(who + "x_" + std::to_string(h_ctl[CTL_BAD]) + " is not on " + curve);
      return BN254S_E_INVALID_ARG;
    }
    if (h_ctl[CTL_BAD + 1] != UINT_MAX) {
      c->set_err(who + "the offset drawn for job " + std::to_string(h_ctl[CTL_BAD + 1]) + " is not on " + curve + " (device self-check)");
      return BN254S_E_INTERNAL;
    }
    if (h_ctl[CTL_ERR]) {
      c->set_err(who + smul_err_text(h_ctl[CTL_ERR]) + " (device self-check)");
      return h_ctl[CTL_ERR] == SMUL_ERR_DRAW_INF ? BN254S_E_INVALID_POINT : BN254S_E_INTERNAL;
    }
    return BN254S_OK;
  };
  // a round: the job check of the listed jobs with the drawn points as their offsets, then who keeps its point.  A job with a
  // point off its curve never gets a step and is counted, so that the round does not end the loop before check() has named it.
  auto body = [&](int round, const unsigned* list, size_t m, const HashedPoints& at) -> int {
    const unsigned grid = (unsigned)((m + 255) / 256);
    if (round) {
      k_smul_gather<<<grid, 256, 0, st>>>(list, m, (int)PW, d_s, d_x, d_cs, d_cx);
      HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemsetAsync(d_step, SMUL_STEP_UNSET & 0xFF, m * 2, st));
    const int rc = bn254s_job_check_device(c, kind, round ? d_cs : d_s, round ? d_cx : d_x, at.points, m, d_step, d_ctl + CTL_BAD);
    if (rc != BN254S_OK) return rc;
    k_smul_accept<<<grid, 256, 0, st>>>(list, m, (int)PW, d_step, at, d_off, d_rej, d_last, d_ctl, round);
    HIP_TRY(c, hipGetLastError());
    return BN254S_OK;
  };
  unsigned count = 0;
  rc = draw_rounds(c, who, "jobs", kind, SMUL_DOMAIN, seed, max_attempts, n, DrawBuffers{d_in, d_hash, d_att, d_rej, d_list, d_ctl}, body,
                   fail_ctl, &count);
  if (rc != BN254S_OK) return rc;
  if (count != 0) {  // out of attempts: the smallest job that is still rejected, with the step of this, its last attempt
    std::vector<uint8_t> rej(n);
    std::vector<uint16_t> last(n);
    HIP_TRY(c, hipMemcpyAsync(rej.data(), d_rej, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(last.data(), d_last, n * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    size_t i = 0;
    while (i < n && !rej[i]) i++;
    if (i == n) {
      c->set_err(who + "a round counted rejected jobs and marked none");
      return BN254S_E_INTERNAL;
    }
    c->set_err(who + "job " + std::to_string(i) + " cannot be proven: sum == -double at step " + std::to_string(last[i]) + " (row " +
               std::to_string(2 * last[i]) + " of its frame) with the offset of attempt " + std::to_string(max_attempts - 1) + ", the last of " +
               std::to_string(max_attempts));
    return BN254S_E_INVALID_POINT;
  }
  rc = bn254s_job_outputs_device(c, kind, d_s, d_x, d_off, n, d_out, d_ofin, d_ctl + CTL_BAD);
  if (rc != BN254S_OK) return rc;
  const unsigned blocks = (unsigned)((n + 63) / 64);
  if (kind == 0) k_smul_sub<G1><<<blocks, 64, 0, st>>>(d_out, d_off, d_ofin, n, d_prod, d_fin, d_ctl);
  else k_smul_sub<G2><<<blocks, 64, 0, st>>>(d_out, d_off, d_ofin, n, d_prod, d_fin, d_ctl);
  HIP_TRY(c, hipGetLastError());
  unsigned h_ctl[CTL_WORDS];
  HIP_TRY(c, hipMemcpyAsync(h_ctl, d_ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  rc = fail_ctl(h_ctl);
  if (rc != BN254S_OK) return rc;
  HIP_TRY(c, hipMemcpyAsync(products, d_prod, n * PW * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(finite, d_fin, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(offsets, d_off, n * PW * 8, hipMemcpyDeviceToHost, st));
  if (outputs) HIP_TRY(c, hipMemcpyAsync(outputs, d_out, n * PW * 8, hipMemcpyDeviceToHost, st));
  if (attempts) HIP_TRY(c, hipMemcpyAsync(attempts, d_att, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

}  // namespace

extern "C" int bn254s_scalar_mul_batch(bn254s_ctx* c, int kind, const uint64_t* scalars, const uint64_t* x, size_t n,
                                       const uint64_t seed[4], int max_attempts, uint64_t* products_out, uint8_t* finite_out,
                                       uint64_t* offsets_out, uint64_t* outputs_out, uint8_t* attempts_out) {
  if (!smul_args_ok(c, "scalar_mul_batch", kind, scalars, x, n, seed, max_attempts, products_out, finite_out, offsets_out) || !c)
    return BN254S_E_INVALID_ARG;
  return smul_front(c, "scalar_mul_batch", kind, scalars, x, n, seed, max_attempts, products_out, finite_out, offsets_out, outputs_out,
                    attempts_out);
}

extern "C" int bn254s_scalar_mul(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                                 size_t n, size_t per_proof, const uint64_t seed[4], int max_attempts, uint64_t* products_out,
                                 uint8_t* finite_out, uint64_t* offsets_out, uint64_t* outputs_out, uint8_t* attempts_out,
                                 bn254s_proof** proofs_out) {
  int rc = proven_args(c, "scalar_mul", "proof",
                       smul_args_ok(c, "scalar_mul", kind, scalars, x, n, seed, max_attempts, products_out, finite_out, offsets_out), params,
                       proofs_out, n, per_proof);
  if (rc != BN254S_OK) return rc;
  const size_t PW = point_words(kind);
  std::vector<u64> prods(PW * n), offs(PW * n), outs(PW * n), proven;
  std::vector<uint8_t> finite(n), attempts(n);
  rc = smul_front(c, "scalar_mul", kind, scalars, x, n, seed, max_attempts, prods.data(), finite.data(), offs.data(), outs.data(),
                  attempts.data());
  if (rc != BN254S_OK) return rc;
  rc = prove_and_collect(c, "scalar_mul", kind, params, scalars, x, offs.data(), n, per_proof, proofs_out, proven);
  if (rc != BN254S_OK) return rc;
  // linkage: the trace generator computes every output bit by bit on its own; it must be the front-end's, word for word
  for (size_t j = 0; j < n; j++)
    if (memcmp(proven.data() + PW * j, outs.data() + PW * j, 8 * PW) != 0) {
      c->set_err("scalar_mul: the proven output of job " + std::to_string(j) + " is not the front-end's");
      release_proofs(proofs_out, n, per_proof);
      return BN254S_E_INTERNAL;
    }
  memcpy(products_out, prods.data(), 8 * PW * n);
  memcpy(finite_out, finite.data(), n);
  memcpy(offsets_out, offs.data(), 8 * PW * n);
  if (outputs_out) memcpy(outputs_out, outs.data(), 8 * PW * n);
  if (attempts_out) memcpy(attempts_out, attempts.data(), n);
  return BN254S_OK;
}
