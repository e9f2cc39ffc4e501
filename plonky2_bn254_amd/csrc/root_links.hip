// Statement verifiers of the Legendre-proven front-ends (root_front.hip, map_to_g1.hip).  Their
// Fq-exp proofs say base^((p-1)/2) == output and nothing else.  What a caller wants to know - flags[i] says whether g(x_i) is a
// square and points[i] is the root with the wanted sign; points[i] is the map_to_g1 image of u_i - follows from the proofs only
// with the linkage: the base of job i is really x_i^3 + 3 (norm(x_i^3 + b'), x_i, norm(x_i), g of the SvdW candidate), the proven
// symbol matches the flag, the root squares back and has the right sign, the flags select the point's x.  The field part of that
// is checked here, on the device, next to the kernels that made it (DESIGN.md "Root statement verifiers"):
//   k_root_links<what>   one lane per input, blocks of 64: the canonical base words, a code 0..7 per input as a byte, and the
//                        smallest index with a code in a control word
// and the five verifiers are host code over it and bn254s_verify_batch.
//
// No LDS table, no ladder, no exponentiation: a root is CHECKED, y^2 == radicand, never computed.  The cost is a few products per
// input; map_to_g1 adds the one inversion of its tv3, in the m2g1_candidates that k_m2g1_point calls.  What a kind's rows hold,
// its radicand, its base and the output that a flag demands are those of the producers: root_kinds.h.  A lane's code depends on
// its own input alone (no cross-lane operation), so it does not matter how a wave diverges on the early returns.  The base and
// its comparison with the job are finished before the root equation starts.
//
// The symbol itself is never computed here either: the verifiers hand bn254s_verify_batch the base from the device and the output
// that the FLAG demands (1 | p - 1 | 0), so that an accepted proof proves the flag.  fq_jobs of the caller is only compared.
#include <climits>
#include <cstring>
#include <string>
#include <vector>
#include "root_kinds.h"

namespace {

template <int N>
__device__ __forceinline__ bool words_differ(const u64* __restrict__ a, const u64* __restrict__ b) {
  u64 d = 0;
#pragma unroll
  for (int w = 0; w < N; w++) d |= a[w] ^ b[w];
  return d != 0;
}
template <int N>
__device__ __forceinline__ bool words_any(const u64* __restrict__ a) {
  u64 d = 0;
#pragma unroll
  for (int w = 0; w < N; w++) d |= a[w];
  return d != 0;
}
// a job (8 words: scalar | base) against (p-1)/2 and the base computed here
__device__ __forceinline__ bool job_scalar_differs(const u64* __restrict__ job) {
  u64 d = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) d |= job[w] ^ G1R_LEGENDRE_EXP[w];
  return d != 0;
}
__device__ __forceinline__ bool job_base_differs(const u64* __restrict__ job, const fqw& base) {
  u64 d = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) d |= job[4 + w] ^ base.l[w];
  return d != 0;
}
__device__ __forceinline__ fqw words_load(const u64* __restrict__ w) {
  fqw r;
#pragma unroll
  for (int k = 0; k < 4; k++) r.l[k] = w[k];
  return r;
}
__device__ __forceinline__ void words_store(u64* __restrict__ w, const fqw& a) {
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = a.l[k];
}
// the sign of canonical words: Fq the parity, Fq2 the rule of sgn.rs:20-27
__device__ __forceinline__ bool sgn_of(const u64* __restrict__ w, const fq&) { return w[0] & 1; }
__device__ __forceinline__ bool sgn_of(const u64* __restrict__ w, const fq2&) { return sgn_words(words_load(w), words_load(w + 4)); }
// The claimed root yw (canonical words below p) of the radicand: codes 6, 7, 0
template <class F>
__device__ __forceinline__ unsigned root_code(const F& radicand, const u64* __restrict__ yw, bool want) {
  F y;
  fe_from_canonical(yw, y);
  if (!fe_is_zero(fe_sub(fe_sqr(y), radicand))) return BN254S_ROOT_SQUARE;
  return sgn_of(yw, y) != want ? BN254S_ROOT_SIGN : BN254S_ROOT_OK;
}

// Input k of a call: its base words into `bases` (where given) and its code, the first that applies (bn254_stark.h).
template <int WHAT>
__device__ __forceinline__ unsigned root_links_code(size_t k, const u64* __restrict__ in, const unsigned char* __restrict__ sgns,
                                                    const u64* __restrict__ out, const unsigned char* __restrict__ flags,
                                                    const unsigned char* __restrict__ root_ok, const u64* __restrict__ jobs,
                                                    u64* __restrict__ bases) {
  constexpr int IW = (int)root_in_words(WHAT), OW = (int)root_out_words(WHAT);
  using F = root_field<WHAT>;
  const u64* xw = in + IW * k;
  const u64* ow = out + OW * k;
  if constexpr (WHAT == ROOT_MAP_TO_G1) {
    fq x1, x2, x3;
    m2g1_candidates(fq_from_canonical(xw), x1, x2, x3);
    {
      const fqw b1 = fq_to_canonical(curve_rhs(x1)), b2 = fq_to_canonical(curve_rhs(x2));
      if (bases) {
        words_store(bases + 8 * k, b1);
        words_store(bases + 8 * k + 4, b2);
      }
      if (jobs) {
        const u64 *j1 = jobs + 16 * k, *j2 = j1 + 8;
        if (job_scalar_differs(j1) || job_scalar_differs(j2)) return BN254S_ROOT_JOB_SCALAR;
        if (job_base_differs(j1, b1) || job_base_differs(j2, b2)) return BN254S_ROOT_JOB_BASE;
      }
    }
    const unsigned f1 = flags[2 * k], f2 = flags[2 * k + 1];
    if (f1 > 1 || f2 > 1) return BN254S_ROOT_FLAG;
    const fq x = fq_select(f1 != 0, x1, fq_select(f2 != 0, x2, x3));
    const fqw xc = fq_to_canonical(x);
    if (words_differ<4>(ow, xc.l)) return BN254S_ROOT_CARRY;
    return root_code<fq>(curve_rhs(x), ow + 4, xw[0] & 1);
  } else {
    F x;
    fe_from_canonical(xw, x);
    F radicand;
    fq b;
    root_radicand_base<WHAT>(x, radicand, b);
    const fqw base = root_base_words<WHAT>(xw, b);
    if (bases) words_store(bases + 4 * k, base);
    if (jobs) {
      if (job_scalar_differs(jobs + 8 * k)) return BN254S_ROOT_JOB_SCALAR;
      if (job_base_differs(jobs + 8 * k, base)) return BN254S_ROOT_JOB_BASE;
    }
    const unsigned flag = flags[k], sgn = WHAT == ROOT_G1_RECOVER ? 0u : (unsigned)sgns[k];  // G1: the even root
    if (flag > 1 || sgn > 1) return BN254S_ROOT_FLAG;
    if constexpr (root_is_sqrt(WHAT)) {
      const unsigned ok = root_ok[k];
      const bool zero = (base.l[0] | base.l[1] | base.l[2] | base.l[3]) == 0;
      if (ok > 1 || (flag && zero) || (ok != 0) != (zero ? sgn == 0 : flag != 0)) return BN254S_ROOT_FLAG;
      if (!ok) return words_any<IW>(ow) ? BN254S_ROOT_NOT_ZERO : BN254S_ROOT_OK;
      return root_code<F>(radicand, ow, sgn != 0);
    } else {
      if (words_differ<IW>(ow, xw)) return BN254S_ROOT_CARRY;
      if (!flag) return words_any<IW>(ow + IW) ? BN254S_ROOT_NOT_ZERO : BN254S_ROOT_OK;
      return root_code<F>(radicand, ow + IW, sgn != 0);
    }
  }
}

// in: n x IW canonical words below p; out: n x OW words, the y / root of a row whose root is claimed below p, the other rows and
// the x of a point only compared; sgns, root_ok: n bytes (read for what 1..3 | 2, 3); flags: n bytes, 2n for map_to_g1; jobs: the
// caller's n (2n) x 8 words or nullptr; bases: n (2n) x 4 words or nullptr; code: n bytes; first: preset to UINT_MAX
template <int WHAT>
__global__ __launch_bounds__(64) void k_root_links(const u64* __restrict__ in, const unsigned char* __restrict__ sgns, size_t n,
                                                   const u64* __restrict__ out, const unsigned char* __restrict__ flags,
                                                   const unsigned char* __restrict__ root_ok, const u64* __restrict__ jobs,
                                                   u64* __restrict__ bases, unsigned char* __restrict__ code,
                                                   unsigned* __restrict__ first) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const unsigned r = root_links_code<WHAT>(k, in, sgns, out, flags, root_ok, jobs, bases);
  code[k] = (unsigned char)r;
  if (r) atomicMin(first, (unsigned)k);
}

// The n inputs from host memory into host memory: codes [n], bases [n (2n) x 4] and the control word.  One pooled buffer, the
// context's stream, one wait.  The caller has checked ranges and counts.
int root_run(bn254s_ctx* c, int what, const uint64_t* in, const uint8_t* sgns, size_t n, const uint64_t* out, const uint8_t* flags,
             const uint8_t* root_ok, const uint64_t* jobs, uint8_t* codes, uint64_t* bases, unsigned* first) {
  const size_t IW = root_in_words(what), OW = root_out_words(what), nj = root_jobs(what) * n;
  const size_t nb = (n + 7) / 8, njb = (nj + 7) / 8;  // words that hold n, nj bytes
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  u64* d = c->words("rootlinks", IW * n + OW * n + 8 * nj /* jobs */ + 4 * nj /* bases */ + 3 * nb /* sgns, root_ok, codes */ +
                                     njb /* flags */ + 1 /* control */);
  if (!d) return BN254S_E_OOM;
  u64 *d_in = d, *d_out = d_in + IW * n, *d_jobs = d_out + OW * n, *d_bases = d_jobs + 8 * nj, *d_bytes = d_bases + 4 * nj;
  unsigned char *d_sgns = (unsigned char*)d_bytes, *d_ok = (unsigned char*)(d_bytes + nb), *d_code = (unsigned char*)(d_bytes + 2 * nb),
                *d_flags = (unsigned char*)(d_bytes + 3 * nb);
  unsigned* d_ctl = (unsigned*)(d_bytes + 3 * nb + njb);
  HIP_TRY(c, hipMemsetAsync(d_ctl, 0xFF, 8, st));
  HIP_TRY(c, hipMemcpyAsync(d_in, in, n * IW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_out, out, n * OW * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_flags, flags, nj, hipMemcpyHostToDevice, st));
  if (jobs) HIP_TRY(c, hipMemcpyAsync(d_jobs, jobs, nj * 64, hipMemcpyHostToDevice, st));
  if (root_has_sgns(what)) {
    if (sgns)
      HIP_TRY(c, hipMemcpyAsync(d_sgns, sgns, n, hipMemcpyHostToDevice, st));
    else
      HIP_TRY(c, hipMemsetAsync(d_sgns, 0, n, st));
  }
  if (root_is_sqrt(what)) HIP_TRY(c, hipMemcpyAsync(d_ok, root_ok, n, hipMemcpyHostToDevice, st));
  const unsigned blocks = (unsigned)((n + 63) / 64);
  const u64* dj = jobs ? d_jobs : nullptr;
  switch (what) {
    case ROOT_G1_RECOVER: k_root_links<ROOT_G1_RECOVER><<<blocks, 64, 0, st>>>(d_in, d_sgns, n, d_out, d_flags, d_ok, dj, d_bases, d_code, d_ctl); break;
    case ROOT_G2_RECOVER: k_root_links<ROOT_G2_RECOVER><<<blocks, 64, 0, st>>>(d_in, d_sgns, n, d_out, d_flags, d_ok, dj, d_bases, d_code, d_ctl); break;
    case ROOT_FQ_SQRT: k_root_links<ROOT_FQ_SQRT><<<blocks, 64, 0, st>>>(d_in, d_sgns, n, d_out, d_flags, d_ok, dj, d_bases, d_code, d_ctl); break;
    case ROOT_FQ2_SQRT: k_root_links<ROOT_FQ2_SQRT><<<blocks, 64, 0, st>>>(d_in, d_sgns, n, d_out, d_flags, d_ok, dj, d_bases, d_code, d_ctl); break;
    default: k_root_links<ROOT_MAP_TO_G1><<<blocks, 64, 0, st>>>(d_in, d_sgns, n, d_out, d_flags, d_ok, dj, d_bases, d_code, d_ctl); break;
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(codes, d_code, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(bases, d_bases, nj * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(first, d_ctl, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return BN254S_OK;
}

const char* in_name(int what) { return what == ROOT_MAP_TO_G1 ? "u" : "x"; }
const char* out_name(int what) { return root_is_sqrt(what) ? "roots" : "points"; }

// The shape of a call, without the context: pointers, n, what
bool links_shape_ok(int what, const uint64_t* in, size_t n, const uint64_t* out, const uint8_t* flags, const uint8_t* root_ok) {
  if (what < 0 || what >= ROOT_KINDS || !in || !out || !flags || (root_is_sqrt(what) && !root_ok)) return false;
  return n > 0 && n < (what == ROOT_MAP_TO_G1 ? (size_t)1 << 31 : (size_t)UINT_MAX);  // the first bad index travels as a 32-bit word
}

// Every coordinate that the device reads as a field element is below p: all of `in`, and the y / root of the rows whose root is
// claimed (recover: the flag is set; sqrt: root_ok is set; map_to_g1: every row).  The other rows, and the x of a point, are only
// compared.  The first that is not names itself like coords_below_p.
bool links_coords_below_p(bn254s_ctx* c, const std::string& tag, int what, const uint64_t* in, size_t n, const uint64_t* out,
                          const uint8_t* flags, const uint8_t* root_ok) {
  const size_t IW = root_in_words(what), OW = root_out_words(what), at = root_at(what);
  if (!coords_below_p(c, tag, in_name(what), COORD_FQ2, (int)IW / 4, in, n)) return false;
  const uint8_t* claimed = what == ROOT_MAP_TO_G1 ? nullptr : root_is_sqrt(what) ? root_ok : flags;
  const char* const* coord = what == ROOT_G2_RECOVER ? COORD_G2 + 2 : what == ROOT_FQ2_SQRT ? COORD_FQ2 : COORD_G1 + 1;
  const size_t ncoord = (what == ROOT_G2_RECOVER || what == ROOT_FQ2_SQRT) ? 2 : 1;
  for (size_t i = 0; i < n; i++)
    for (size_t k = 0; (!claimed || claimed[i]) && k < ncoord; k++)
      if (!fq_below_p(out + OW * i + at + 4 * k)) {
        if (c)
          c->set_err(tag + ": " + out_name(what) + "_" + std::to_string(i) + (what == ROOT_FQ_SQRT ? " is" : std::string(" has ") + coord[k]) +
                     " not below p");
        return false;
      }
  return true;
}

// (p - 1)/2 in words
void legendre_exp(u64 e[4]) {
  u64 pm1[4];
  memcpy(pm1, G1R_P, 32);
  pm1[0] -= 1;  // p is odd
  for (int w = 0; w < 4; w++) e[w] = (pm1[w] >> 1) | (w < 3 ? pm1[w + 1] << 63 : 0);
}

const char* base_name(int what, size_t job) {
  switch (what) {
    case ROOT_G1_RECOVER: return "x^3 + 3";
    case ROOT_G2_RECOVER: return "norm(x^3 + b')";
    case ROOT_FQ_SQRT: return "x";
    case ROOT_FQ2_SQRT: return "norm(x)";
    default: return job % 2 ? "g(x2)" : "g(x1)";
  }
}
const char* radicand_name(int what) {
  switch (what) {
    case ROOT_G1_RECOVER: return "x^3 + 3";
    case ROOT_G2_RECOVER: return "x^3 + b'";
    case ROOT_MAP_TO_G1: return "g of the candidate that the flags select";
    default: return "x";
  }
}

// What a code 1..7 says of input i, from the arrays of the call (the job and the byte that a job code or code 3 means are found
// again here, on the host: one input per call at the most)
std::string link_text(unsigned code, int what, size_t i, const uint8_t* sgns, const uint8_t* flags, const uint8_t* root_ok,
                      const uint64_t* jobs, const uint64_t* bases) {
  const std::string root = root_is_sqrt(what) ? "the root" : "y of the point";
  const size_t nj = root_jobs(what);
  u64 e[4];
  legendre_exp(e);
  switch (code) {
    case BN254S_ROOT_JOB_SCALAR:
      for (size_t j = nj * i; j < nj * (i + 1); j++)
        if (memcmp(jobs + 8 * j, e, 32) != 0)
          return "the scalar of job " + std::to_string(j) + (what == ROOT_MAP_TO_G1 ? std::string(" (") + base_name(what, j) + ")" : "") +
                 " is not (p - 1)/2";
      break;
    case BN254S_ROOT_JOB_BASE:
      for (size_t j = nj * i; j < nj * (i + 1); j++)
        if (memcmp(jobs + 8 * j + 4, bases + 4 * j, 32) != 0) return "the base of job " + std::to_string(j) + " is not " + base_name(what, j);
      break;
    case BN254S_ROOT_FLAG: {
      for (size_t j = nj * i; j < nj * (i + 1); j++)
        if (flags[j] > 1)
          return std::string(root_is_sqrt(what) ? "square" : what == ROOT_MAP_TO_G1 ? (j % 2 ? "the flag of g(x2)" : "the flag of g(x1)") : "the flag") +
                 " is " + std::to_string(flags[j]) + ", neither 0 nor 1";
      const unsigned sgn = sgns ? sgns[i] : 0;
      if (sgn > 1) return "the sign is " + std::to_string(sgn) + ", neither 0 nor 1";
      if (!root_is_sqrt(what)) break;
      if (root_ok[i] > 1) return "root_ok is " + std::to_string(root_ok[i]) + ", neither 0 nor 1";
      const bool zero = words_are_zero(bases + 4 * i);
      if (flags[i] && zero) return "square is set on the base zero, whose Legendre symbol is 0";
      return std::string("root_ok is ") + (root_ok[i] ? "set" : "clear") + ", but a root with the sign " + std::to_string(sgn) +
             (root_ok[i] ? " does not exist" : " exists") + (zero ? " (the one root of zero has the sign 0)" : " by the flag square");
    }
    case BN254S_ROOT_CARRY:
      return what == ROOT_MAP_TO_G1 ? "x of the point is not the candidate that the flags select" : "the point does not carry x";
    case BN254S_ROOT_NOT_ZERO:
      return std::string(root_is_sqrt(what) ? "root_ok" : "the flag") + " is clear and " + root + " is not zero words";
    case BN254S_ROOT_SQUARE: return root + " does not square to " + radicand_name(what);
    case BN254S_ROOT_SIGN: return root + " squares to " + radicand_name(what) + " but has the other sign";
  }
  return "code " + std::to_string(code);
}

// The five verifiers: the argument ladder of bn254s_verify_scalar_mul, the kernel once, bn254s_verify_batch of the proofs against
// jobs made here - (p-1)/2, the base from the device, and the output that the flag demands (legendre_output of root_kinds.h; on a
// zero base, sqrt kinds only, a set flag is code 3 and the proof is judged for what the base is, 0) - and both verdicts reported.
int verify_roots(bn254s_ctx* c, int what, const std::string& tag, const bn254s_params* params, const uint64_t* const* words,
                 const size_t* n_words, const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* in,
                 const uint8_t* sgns, size_t n, const uint64_t* out, const uint8_t* flags, const uint8_t* root_ok, const uint64_t* fq_jobs,
                 uint8_t* link_out, int32_t* proof_status) {
  if (!links_shape_ok(what, in, n, out, flags, root_ok)) return BN254S_E_INVALID_ARG;
  const size_t nj = root_jobs(what) * n;
  if (!verifier_args_ok(2, params, words, n_words, degree_bits, n_proofs, per_proof, nj) || params->struct_size != sizeof(bn254s_params))
    return BN254S_E_INVALID_ARG;
  if (!links_coords_below_p(c, tag, what, in, n, out, flags, root_ok) || !c) return BN254S_E_INVALID_ARG;
  std::vector<uint8_t> link(n);
  std::vector<int32_t> status(n_proofs);
  std::vector<u64> bases(4 * nj), scalars(4 * nj), outputs(4 * nj);
  unsigned first = UINT_MAX;
  int rc = root_run(c, what, in, sgns, n, out, flags, root_ok, fq_jobs, link.data(), bases.data(), &first);
  if (rc != BN254S_OK) return rc;
  u64 e[4];
  legendre_exp(e);
  for (size_t j = 0; j < nj; j++) {
    const bool zero = root_is_sqrt(what) && words_are_zero(bases.data() + 4 * j);  // the flag does not count there
    memcpy(scalars.data() + 4 * j, e, 32);
    memcpy(outputs.data() + 4 * j, legendre_output(flags[j] && !zero, zero), 32);
  }
  std::string text;
  rc = verify_proof_runs(c, 2, params, words, n_words, degree_bits, n_proofs, per_proof, scalars.data(), bases.data(), nullptr,
                         outputs.data(), nj, status.data(), text);
  if (rc != BN254S_OK && rc != BN254S_E_VERIFY) return rc;
  if (link_out) memcpy(link_out, link.data(), n);
  if (proof_status) memcpy(proof_status, status.data(), n_proofs * sizeof(int32_t));
  if (first != UINT_MAX) {
    c->set_err(tag + ": input " + std::to_string(first) + ": " + link_text(link[first], what, first, sgns, flags, root_ok, fq_jobs, bases.data()));
    return BN254S_E_VERIFY;
  }
  if (rc == BN254S_E_VERIFY) c->set_err(text);  // "proof k: ...", k counted over the whole call
  return rc;
}

}  // namespace

extern "C" int bn254s_root_links_check_batch(bn254s_ctx* c, int what, const uint64_t* in, const uint8_t* sgns, size_t n,
                                             const uint64_t* out, const uint8_t* flags, const uint8_t* root_ok, const uint64_t* fq_jobs,
                                             uint8_t* code_out, uint64_t* bases_out) {
  if (!code_out || !links_shape_ok(what, in, n, out, flags, root_ok)) return BN254S_E_INVALID_ARG;
  if (!links_coords_below_p(c, "root_links_check", what, in, n, out, flags, root_ok) || !c) return BN254S_E_INVALID_ARG;
  std::vector<uint8_t> codes(n);
  std::vector<u64> bases(4 * root_jobs(what) * n);
  unsigned first;
  const int rc = root_run(c, what, in, sgns, n, out, flags, root_ok, fq_jobs, codes.data(), bases.data(), &first);
  if (rc != BN254S_OK) return rc;
  memcpy(code_out, codes.data(), n);
  if (bases_out) memcpy(bases_out, bases.data(), bases.size() * 8);
  return BN254S_OK;
}

extern "C" int bn254s_verify_g1_recover(bn254s_ctx* c, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                                        const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs, size_t n,
                                        const uint64_t* points, const uint8_t* flags, const uint64_t* fq_jobs, uint8_t* link_out,
                                        int32_t* proof_status) {
  return verify_roots(c, ROOT_G1_RECOVER, "verify_g1_recover", params, words, n_words, degree_bits, n_proofs, per_proof, xs, nullptr, n,
                      points, flags, nullptr, fq_jobs, link_out, proof_status);
}
extern "C" int bn254s_verify_g2_recover(bn254s_ctx* c, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                                        const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                                        const uint8_t* sgns, size_t n, const uint64_t* points, const uint8_t* flags,
                                        const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status) {
  return verify_roots(c, ROOT_G2_RECOVER, "verify_g2_recover", params, words, n_words, degree_bits, n_proofs, per_proof, xs, sgns, n,
                      points, flags, nullptr, fq_jobs, link_out, proof_status);
}
extern "C" int bn254s_verify_fq_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                                     const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                                     const uint8_t* sgns, size_t n, const uint64_t* roots, const uint8_t* square, const uint8_t* root_ok,
                                     const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status) {
  return verify_roots(c, ROOT_FQ_SQRT, "verify_fq_sqrt", params, words, n_words, degree_bits, n_proofs, per_proof, xs, sgns, n, roots,
                      square, root_ok, fq_jobs, link_out, proof_status);
}
extern "C" int bn254s_verify_fq2_sqrt(bn254s_ctx* c, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                                      const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                                      const uint8_t* sgns, size_t n, const uint64_t* roots, const uint8_t* square, const uint8_t* root_ok,
                                      const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status) {
  return verify_roots(c, ROOT_FQ2_SQRT, "verify_fq2_sqrt", params, words, n_words, degree_bits, n_proofs, per_proof, xs, sgns, n, roots,
                      square, root_ok, fq_jobs, link_out, proof_status);
}
extern "C" int bn254s_verify_map_to_g1(bn254s_ctx* c, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                                       const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* u, size_t n,
                                       const uint64_t* points, const uint8_t* sq_flags, const uint64_t* fq_jobs, uint8_t* link_out,
                                       int32_t* proof_status) {
  return verify_roots(c, ROOT_MAP_TO_G1, "verify_map_to_g1", params, words, n_words, degree_bits, n_proofs, per_proof, u, nullptr, n,
                      points, sq_flags, nullptr, fq_jobs, link_out, proof_status);
}
