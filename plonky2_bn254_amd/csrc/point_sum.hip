// Statement verifiers: what a caller of bn254s_scalar_mul / bn254s_msm_multi wants to know is products[i] == s_i x_i, or
// results[j] == the sum of s x over MSM j.  The proofs carry s x + offset == output; the statement follows from them only with the
// linkage between the arrays: product + offset == output, the offset chain inside an MSM, result + R == the last output.  The
// linkage is curve arithmetic and is checked here, on the device, next to k_smul_sub which made it (DESIGN.md "Statement verifiers"):
//   k_point_sum<G1 | G2>        one lane per relation "c == a + b", a possibly O: a code 0..7 per relation as a byte, and the
//                               smallest failing index in a control word
//   k_points_on_curve<G1 | G2>  one lane per point: a byte per point, and the smallest index off the curve in a control word
// and the two verifiers are host code over these and bn254s_verify_batch.
//
// No inversion.  With d = x_b - x_a, e = y_b - y_a (the tangent d = 2 y_a, e = 3 x_a^2 where a == b; d != 0, both group orders are
// odd) the chord law reads lambda = e / d, x_3 = lambda^2 - x_a - x_b, y_3 = lambda (x_a - x_3) - y_a.  Multiplied through by d^2
// and by d, c == a + b holds exactly when
//   x_c d^2 == e^2 - (x_a + x_b) d^2          (taken as (x_a + x_b + x_c) d^2 == e^2: one product by d^2 for the two)
//   (y_c + y_a) d == e (x_a - x_c)
// which is 3 products and 2 squarings against the ~380 of a Fermat inversion.  Where x agrees and y does not, c is on the curve
// with the x of the sum: it is minus the sum, code 7.  The case (a = O, a == b, a == -b, general) is decided by comparisons before
// any product that the case does not need, and the x equation is finished before the y equation starts.
//
// Where the offsets or the R of a call come from (the seed, the attempts) is deliberately not checked: s x + offset == output is
// proven for the offset at hand and the same offset is subtracted, whatever point it is.  Drawing the offsets again would double
// the device work and verify nothing about the statement.
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "job_curve.h"
#include "proven_jobs.h"

namespace {

enum { PS_FIRST_SUM = 0 /* the smallest relation with a code */, PS_FIRST_X = 1 /* the smallest x off its curve */, PS_CTL_WORDS = 2 };

template <class C>
__device__ __forceinline__ unsigned point_sum_code(const u64* __restrict__ aw, bool a_fin, const u64* __restrict__ bw,
                                                   const u64* __restrict__ cw) {
  using F = typename C::F;
  F xa, ya, xb, yb, xc, yc;
  if (!a_fin) {
    u64 any = 0;
#pragma unroll
    for (int w = 0; w < C::PW; w++) any |= aw[w];
    if (any) return BN254S_SUM_A_NOT_ZERO;
  } else {
    fe_from_canonical(aw, xa);
    fe_from_canonical(aw + C::FW, ya);
    if (!on_curve(xa, ya)) return BN254S_SUM_A_OFF_CURVE;
  }
  fe_from_canonical(bw, xb);
  fe_from_canonical(bw + C::FW, yb);
  if (!on_curve(xb, yb)) return BN254S_SUM_B_OFF_CURVE;
  fe_from_canonical(cw, xc);
  fe_from_canonical(cw + C::FW, yc);
  if (!on_curve(xc, yc)) return BN254S_SUM_C_OFF_CURVE;
  if (!a_fin) {  // O + b: c == b, x first
    if (!fe_is_zero(fe_sub(xb, xc))) return BN254S_SUM_X;
    return fe_is_zero(fe_sub(yb, yc)) ? BN254S_SUM_OK : BN254S_SUM_Y;
  }
  F d = fe_sub(xb, xa), e = fe_sub(yb, ya);
  if (fe_is_zero(d)) {
    if (!fe_is_zero(e)) return BN254S_SUM_INFINITE;  // two points of the curve with one x and another y: a == -b
    pt_tangent(xa, ya, e, d);
  }
  const F dd = fe_sqr(d);
  if (!fe_is_zero(fe_sub(fe_mul(fe_add(fe_add(xa, xb), xc), dd), fe_sqr(e)))) return BN254S_SUM_X;
  if (!fe_is_zero(fe_sub(fe_mul(fe_add(yc, ya), d), fe_mul(e, fe_sub(xa, xc))))) return BN254S_SUM_Y;
  return BN254S_SUM_OK;
}

// a, b, c: n x PW canonical words, every coordinate below p but for the rows of a with a_finite == 0, which are only compared with
// zero; code: n bytes; first: preset to UINT_MAX
template <class C>
__global__ __launch_bounds__(64) void k_point_sum(const u64* __restrict__ a, const unsigned char* __restrict__ a_finite,
                                                  const u64* __restrict__ b, const u64* __restrict__ c, size_t n,
                                                  unsigned char* __restrict__ code, unsigned* __restrict__ first) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const unsigned r = point_sum_code<C>(a + C::PW * k, a_finite[k] != 0, b + C::PW * k, c + C::PW * k);
  code[k] = (unsigned char)r;
  if (r) atomicMin(first, (unsigned)k);
}

// x: n x PW canonical words below p; ok: n bytes, 1 for a point of the curve; first: preset to UINT_MAX
template <class C>
__global__ __launch_bounds__(64) void k_points_on_curve(const u64* __restrict__ x, size_t n, unsigned char* __restrict__ ok,
                                                        unsigned* __restrict__ first) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  typename C::F px, py;
  fe_from_canonical(x + C::PW * k, px);
  fe_from_canonical(x + C::PW * k + C::FW, py);
  const bool on = on_curve(px, py);
  ok[k] = on ? 1 : 0;
  if (!on) atomicMin(first, (unsigned)k);
}

// The n relations and, where x != nullptr, the nx points, from host memory into host memory: codes [n], x_ok [nx] and the two
// control words.  One pooled buffer, the context's stream, one wait.  The caller has checked ranges and counts.
int psum_run(bn254s_ctx* c, int kind, const uint64_t* a, const uint8_t* a_finite, const uint64_t* b, const uint64_t* cc, size_t n,
             const uint64_t* x, size_t nx, uint8_t* codes, uint8_t* x_ok, unsigned first[PS_CTL_WORDS]) {
  if (!x) nx = 0;
  const size_t PW = point_words(kind), nb = (n + 7) / 8, nxb = (nx + 7) / 8;  // words that hold n, nx bytes
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("psum", 3 * PW * n /* a, b, c */ + PW * nx /* x */ + 2 * nb /* a_finite, codes */ + nxb /* x_ok */ + 1 /* control */);
  if (!d) return BN254S_E_OOM;
  u64 *d_a = d, *d_b = d_a + PW * n, *d_c = d_b + PW * n, *d_x = d_c + PW * n, *d_bytes = d_x + PW * nx;
  unsigned char *d_fin = (unsigned char*)d_bytes, *d_code = (unsigned char*)(d_bytes + nb), *d_ok = (unsigned char*)(d_bytes + 2 * nb);
  unsigned* d_ctl = (unsigned*)(d_bytes + 2 * nb + nxb);
  HIP_TRY(c, hipMemsetAsync(d_ctl, 0xFF, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_a, a, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_b, b, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_c, cc, n * PW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_fin, a_finite, n, hipMemcpyHostToDevice, st));
  const unsigned blocks = (unsigned)((n + 63) / 64);
  if (kind == 0) k_point_sum<G1><<<blocks, 64, 0, st>>>(d_a, d_fin, d_b, d_c, n, d_code, d_ctl + PS_FIRST_SUM);
  else k_point_sum<G2><<<blocks, 64, 0, st>>>(d_a, d_fin, d_b, d_c, n, d_code, d_ctl + PS_FIRST_SUM);
  HIP_TRY(c, hipGetLastError());
  if (nx) {
    HIP_TRY(c, hipMemcpyAsync(d_x, x, nx * PW * 8, hipMemcpyHostToDevice, st));
    const unsigned xblocks = (unsigned)((nx + 63) / 64);
    if (kind == 0) k_points_on_curve<G1><<<xblocks, 64, 0, st>>>(d_x, nx, d_ok, d_ctl + PS_FIRST_X);
    else k_points_on_curve<G2><<<xblocks, 64, 0, st>>>(d_x, nx, d_ok, d_ctl + PS_FIRST_X);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(x_ok, d_ok, nx, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipMemcpyAsync(codes, d_code, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(first, d_ctl, PS_CTL_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

// coords_below_p of the rows of a whose flag is set (a row with a clear flag is compared with zero on the device and never
// read as a point)
bool finite_coords_below_p(bn254s_ctx* c, const std::string& tag, const char* name, int kind, const uint64_t* a, const uint8_t* fin,
                           size_t n) {
  const size_t PW = point_words(kind);
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; fin[i] && k < PW / 4; k++)
      if (!fq_below_p(a + PW * i + 4 * k)) {
        if (c) c->set_err(tag + ": " + name + "_" + std::to_string(i) + " has " + (kind == 0 ? COORD_G1 : COORD_G2)[k] + " not below p");
        return false;
      }
  return true;
}

bool all_coords_below_p(bn254s_ctx* c, const std::string& tag, const char* name, int kind, const uint64_t* w, size_t n) {
  return coords_below_p(c, tag, name, kind == 0 ? COORD_G1 : COORD_G2, (int)point_words(kind) / 4, w, n);
}

// What a code 1..7 says of the relation a + b == c, with the names of the three arrays as the call has them
std::string sum_text(unsigned code, const std::string& a, const std::string& b, const std::string& cc, int kind) {
  switch (code) {
    case BN254S_SUM_A_NOT_ZERO: return "finite is 0 and " + a + " is not zero words";
    case BN254S_SUM_A_OFF_CURVE: return a + " is not on " + curve_name(kind);
    case BN254S_SUM_B_OFF_CURVE: return b + " is not on " + curve_name(kind);
    case BN254S_SUM_C_OFF_CURVE: return cc + " is not on " + curve_name(kind);
    case BN254S_SUM_INFINITE: return a + " == -" + b + ": their sum is the point at infinity";
    case BN254S_SUM_X: return a + " + " + b + " != " + cc + " (x)";
    default: return a + " + " + b + " != " + cc + " (y)";
  }
}

}  // namespace

extern "C" int bn254s_point_sum_check_batch(bn254s_ctx* c, int kind, const uint64_t* a, const uint8_t* a_finite, const uint64_t* b,
                                            const uint64_t* cc, size_t n, uint8_t* code_out) {
  const char* tag = "point_sum_check";
  if (!a || !a_finite || !b || !cc || !code_out || n == 0 || n >= (size_t)UINT_MAX || kind < 0 || kind > 1) return BN254S_E_INVALID_ARG;
  if (!finite_coords_below_p(c, tag, "a", kind, a, a_finite, n) || !all_coords_below_p(c, tag, "b", kind, b, n) ||
      !all_coords_below_p(c, tag, "c", kind, cc, n) || !c)
    return BN254S_E_INVALID_ARG;
  std::vector<uint8_t> codes(n);
  unsigned first[PS_CTL_WORDS];
  const int rc = psum_run(c, kind, a, a_finite, b, cc, n, nullptr, 0, codes.data(), nullptr, first);
  if (rc != BN254S_OK) return rc;
  memcpy(code_out, codes.data(), n);
  return BN254S_OK;
}

extern "C" int bn254s_verify_scalar_mul(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* const* words,
                                        const size_t* n_words, const uint32_t* degree_bits, size_t n_proofs, size_t per_proof,
                                        const uint64_t* scalars, const uint64_t* x, size_t n, const uint64_t* products,
                                        const uint8_t* finite, const uint64_t* offsets, const uint64_t* outputs, uint8_t* link_out,
                                        int32_t* proof_status) {
  const std::string tag = "verify_scalar_mul";
  if (!scalars || !x || !products || !finite || !offsets || !outputs ||
      !verifier_args_ok(kind, params, words, n_words, degree_bits, n_proofs, per_proof, n) || kind < 0 || kind > 1 ||
      params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  if (!all_coords_below_p(c, tag, "x", kind, x, n) || !finite_coords_below_p(c, tag, "products", kind, products, finite, n) ||
      !all_coords_below_p(c, tag, "offsets", kind, offsets, n) || !all_coords_below_p(c, tag, "outputs", kind, outputs, n) || !c)
    return BN254S_E_INVALID_ARG;
  std::vector<uint8_t> link(n), x_ok(n);
  std::vector<int32_t> status(n_proofs);
  unsigned first[PS_CTL_WORDS];
  int rc = psum_run(c, kind, products, finite, offsets, outputs, n, x, n, link.data(), x_ok.data(), first);
  if (rc != BN254S_OK) return rc;
  for (size_t i = 0; i < n; i++)
    if (!x_ok[i]) link[i] = BN254S_SUM_X_OFF_CURVE;
  std::string text;
  rc = verify_proof_runs(c, kind, params, words, n_words, degree_bits, n_proofs, per_proof, scalars, x, offsets, outputs, n,
                         status.data(), text);
  if (rc != BN254S_OK && rc != BN254S_E_VERIFY) return rc;
  if (link_out) memcpy(link_out, link.data(), n);
  if (proof_status) memcpy(proof_status, status.data(), n_proofs * sizeof(int32_t));
  const unsigned bad = first[PS_FIRST_SUM] < first[PS_FIRST_X] ? first[PS_FIRST_SUM] : first[PS_FIRST_X];  // the control words
  if (bad != UINT_MAX) {
    c->set_err(tag + ": job " + std::to_string(bad) + ": " +
               (link[bad] == BN254S_SUM_X_OFF_CURVE ? std::string("x is not on ") + curve_name(kind)
                                                    : sum_text(link[bad], "products", "offsets", "outputs", kind)));
    return BN254S_E_VERIFY;
  }
  if (rc == BN254S_E_VERIFY) c->set_err(text);  // "proof k: ...", k counted over the whole call
  return rc;
}

extern "C" int bn254s_verify_msm_multi(bn254s_ctx* c, int kind, const bn254s_params* params, const uint64_t* const* words,
                                       const size_t* n_words, const uint32_t* degree_bits, size_t n_proofs, size_t per_proof,
                                       const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m, size_t n,
                                       const uint64_t* R, const uint64_t* results, const uint8_t* finite, const uint64_t* offsets,
                                       const uint64_t* outputs, uint8_t* link_out, int32_t* proof_status) {
  const std::string tag = "verify_msm_multi";
  if (!scalars || !x || !seg_len || !R || !results || !finite || !offsets || !outputs || m == 0 ||
      !verifier_args_ok(kind, params, words, n_words, degree_bits, n_proofs, per_proof, n))
    return BN254S_E_INVALID_ARG;
  size_t sum = 0;
  for (size_t j = 0; j < m; j++) {
    if (seg_len[j] == 0 || seg_len[j] > n - sum) return BN254S_E_INVALID_ARG;
    sum += seg_len[j];
  }
  if (sum != n || kind < 0 || kind > 1 || params->struct_size != sizeof(bn254s_params)) return BN254S_E_INVALID_ARG;
  if (!all_coords_below_p(c, tag, "x", kind, x, n) || !all_coords_below_p(c, tag, "R", kind, R, m) ||
      !finite_coords_below_p(c, tag, "results", kind, results, finite, m) || !all_coords_below_p(c, tag, "offsets", kind, offsets, n) ||
      !all_coords_below_p(c, tag, "outputs", kind, outputs, n) || !c)
    return BN254S_E_INVALID_ARG;
  const size_t PW = point_words(kind);
  std::vector<u64> last(PW * m);  // outputs[l_j]
  for (size_t j = 0, f = 0; j < m; f += seg_len[j++]) memcpy(last.data() + PW * j, outputs + PW * (f + seg_len[j] - 1), 8 * PW);
  std::vector<uint8_t> link(m), x_ok(n);
  std::vector<int32_t> status(n_proofs);
  unsigned first[PS_CTL_WORDS];
  int rc = psum_run(c, kind, results, finite, R, last.data(), m, x, n, link.data(), x_ok.data(), first);
  if (rc != BN254S_OK) return rc;
  // the first failing check of every MSM in the order 8, 9, 10, then the relation's own code; the message of the smallest such MSM
  std::string why;
  for (size_t j = 0, f = 0; j < m; f += seg_len[j++]) {
    const size_t l = f + seg_len[j] - 1;
    std::string t;
    size_t i = f;
    if (first[PS_FIRST_X] <= l)  // (no MSM before the one that holds the smallest such x needs the walk)
      while (i <= l && x_ok[i]) i++;
    else i = l + 1;
    if (i <= l) {
      link[j] = BN254S_SUM_X_OFF_CURVE;
      t = "x_" + std::to_string(i) + " is not on " + curve_name(kind);
    } else if (memcmp(offsets + PW * f, R + PW * j, 8 * PW) != 0) {
      link[j] = BN254S_SUM_HEAD;
      t = "offsets[" + std::to_string(f) + "] != R_" + std::to_string(j) + " (the head)";
    } else {
      for (i = f; i < l && memcmp(offsets + PW * (i + 1), outputs + PW * i, 8 * PW) == 0;) i++;
      if (i < l) {
        link[j] = BN254S_SUM_CHAIN;
        t = "offsets[" + std::to_string(i + 1) + "] != outputs[" + std::to_string(i) + "] (link " + std::to_string(i - f) + " -> " +
            std::to_string(i - f + 1) + ")";
      } else if (link[j]) {
        t = sum_text(link[j], "results", "R", "outputs[" + std::to_string(l) + "]", kind);
      }
    }
    if (link[j] && why.empty()) why = tag + ": msm " + std::to_string(j) + ": " + t;
  }
  std::string text;
  rc = verify_proof_runs(c, kind, params, words, n_words, degree_bits, n_proofs, per_proof, scalars, x, offsets, outputs, n,
                         status.data(), text);
  if (rc != BN254S_OK && rc != BN254S_E_VERIFY) return rc;
  if (link_out) memcpy(link_out, link.data(), m);
  if (proof_status) memcpy(proof_status, status.data(), n_proofs * sizeof(int32_t));
  if (!why.empty()) {
    c->set_err(why);
    return BN254S_E_VERIFY;
  }
  if (rc == BN254S_E_VERIFY) c->set_err(text);  // "proof k: ...", k counted over the whole call
  return rc;
}
