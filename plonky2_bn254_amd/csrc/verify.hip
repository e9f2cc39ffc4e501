// Native verification of a proof: bn254s_verify.
//
// Replaces the reference's `verify` (src/starks/common/verifier.rs:32-98: challenges from the transcript, starky's
// verify_stark_proof_with_challenges, verify_cross_table_lookups with only extra looking values, ctl_values.rs:28-47) and
// plonky2's verify_fri_proof, on the flat word layout of include/bn254_stark.h.
//
// The transcript, the FRI checks (Merkle paths, initial combination, arity-16 folds, final polynomial) and the CTL sums
// run on the host.  The vanishing check needs sum_e alpha^(K-1-e) c_e(local(zeta), next(zeta)) * selector_e with the
// openings in the quadratic extension.  The AIR exists once in this library, as the quotient kernels over the base
// field, so it is evaluated there: every constraint has degree <= 3 in the opened values and base-field coefficients
// (alpha, beta, gamma are base-field challenges), hence along the line v(t) = v0 + t v1 through the opening v0 + v1 X the
// weighted sum is a cubic in t.  The kernels evaluate it at t = 0..4 on a tiny synthetic "LDE" (the fifth point checks
// the degree bound), once per selector class (plain / transition / first row / last row, chosen through custom point
// tables), the cubic is interpolated and X^2 = 7 substituted.  Prover and verifier therefore share one statement of the
// AIR; the independent restatement lives in oracle/ and is what the tests compare against.
//
// The verifier is cut in three parts - verify_front, the query rounds (verify_query.h: host/device functions, one query at a
// time), verify_ctl - which verify_impl runs in that order for one proof and bn254s_verify_batch (verify_batch.hip) for many.
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "prover.h"
#include "quotient.h"
#include "transcript.h"
#include "verify_air_host.h"
#include "verify_query.h"

namespace {

inline gl2 ext(const u64* w) { return gl2_make(w[0], w[1]); }
inline gl2 base(u64 x) { return gl2_make(x, 0); }

// ---- vanishing sum through the quotient kernels (see the header comment) -------------------------------------------
constexpr unsigned VLOG = 7;  // synthetic domain: N = 128, 2N = 256 points = one workgroup
constexpr int VT = 5, VS = 4, VPTS = VT * VS;

#define VCHK(call)                                             \
  do {                                                         \
    hipError_t e_ = (call);                                    \
    if (e_ != hipSuccess) {                                    \
      err = std::string(#call) + ": " + hipGetErrorString(e_); \
      return BN254S_E_HIP;                                     \
    }                                                          \
  } while (0)

int vanishing_on_gpu(bn254s_ctx* c, int kind, const StarkShape& sh, const u64* words, const View& v, const u64 alphas[2],
                     const u64 betas[2], const u64 gammas[2], gl2 z_last, gl2 l_first, gl2 l_last, gl2 out[2], std::string& err) {
  const size_t M2 = (size_t)2 << VLOG, N = (size_t)1 << VLOG;
  const int W = v.W, A = v.A, K = sh.n_total_constraints();
  hipStream_t st = c->stream;
  // synthetic LDE: point j = 5 s + t holds local(t) = v0 + t v1; its "next" position holds next(t)
  std::vector<u64> tl((size_t)W * M2, 0), al((size_t)A * M2, 0), px(M2, 0), pf(M2, 0), pl(M2, 0);
  size_t jn[VPTS];
  for (int j = 0; j < VPTS; j++) {
    u32 k = bitrev32((u32)j, VLOG);
    jn[j] = bitrev32((k + 1) & (u32)(N - 1), VLOG);
    if (jn[j] < (size_t)VPTS) {
      err = "internal: synthetic next position collides";
      return BN254S_E_INTERNAL;
    }
  }
  auto fill = [&](std::vector<u64>& buf, int ncols, size_t off_local, size_t off_next) {
    for (int col = 0; col < ncols; col++) {
      const u64 *lv = words + off_local + 2 * (size_t)col, *nv = words + off_next + 2 * (size_t)col;
      for (int j = 0; j < VPTS; j++) {
        u64 t = (u64)(j % VT);
        buf[(size_t)col * M2 + j] = gl_add(lv[0], gl_mul(t, lv[1]));
        buf[(size_t)col * M2 + jn[j]] = gl_add(nv[0], gl_mul(t, nv[1]));
      }
    }
  };
  fill(tl, W, v.local, v.next);
  fill(al, A, v.aux, v.aux_next);
  for (int t = 0; t < VT; t++) {  // selector classes: s = 1 transition (x - w^-1 with w^-1 := 0), 2 first row, 3 last row
    px[VT * 1 + t] = 1;
    pf[VT * 2 + t] = 1;
    pl[VT * 3 + t] = 1;
  }
  std::vector<u64> hW, hmzt;
  const int* mz_e0 = nullptr;
  int nblk = stark_kind(kind).mz_blocks(&mz_e0);
  quotient_host_tables(K, alphas, mz_e0, nblk, hW, hmzt);

  u64* d_tl = c->words("vf_tl", tl.size());
  u64* d_al = c->words("vf_al", al.size());
  u64* d_pt = c->words("vf_pt", 3 * M2);
  u64* d_W = c->words("vf_W", hW.size());
  u64* d_mzt = c->words("vf_mzt", hmzt.size());
  u64* d_out = c->words("vf_out", 4 * N);
  u64* d_part = c->words("vf_part", (size_t)QUOTIENT_MAX_PARTS * 2 * M2);
  if (!d_tl || !d_al || !d_pt || !d_W || !d_mzt || !d_out || !d_part) {
    err = c->BufPool::err;
    return BN254S_E_OOM;
  }
  VCHK(hipMemcpyAsync(d_tl, tl.data(), tl.size() * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_al, al.data(), al.size() * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_pt, px.data(), M2 * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_pt + M2, pf.data(), M2 * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_pt + 2 * M2, pl.data(), M2 * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_W, hW.data(), hW.size() * 8, hipMemcpyHostToDevice, st));
  VCHK(hipMemcpyAsync(d_mzt, hmzt.data(), hmzt.size() * 8, hipMemcpyHostToDevice, st));
  QPointTables pt;
  pt.x = d_pt;
  pt.lfirst = d_pt + M2;
  pt.llast = d_pt + 2 * M2;
  QArgs QA;
  quotient_fill_args(QA, sh, d_tl, d_al, d_W, d_mzt, pt, betas, gammas, VLOG, d_out, d_part);
  QA.zh_inv[0] = QA.zh_inv[1] = 1;  // no division by Z_H
  QA.w_inv = 0;                     // transition selector = the x table itself
  stark_kind(kind).quotient_launch(QA, sh, st);
  std::vector<u64> ho(4 * N);
  VCHK(hipMemcpyAsync(ho.data(), d_out, ho.size() * 8, hipMemcpyDeviceToHost, st));
  VCHK(hipStreamSynchronize(st));
  VCHK(hipGetLastError());
  const u64 inv2 = gl_inv(2), inv6 = gl_inv(6);
  const gl2 sel[VS] = {gl2_make(1, 0), z_last, l_first, l_last};
  for (int a = 0; a < 2; a++) {
    gl2 tot = gl2_make(0, 0);
    u64 plain[VT];
    for (int s = 0; s < VS; s++) {
      u64 y[VT];
      for (int t = 0; t < VT; t++) {
        int j = VT * s + t;
        u64 e = ho[(size_t)(a * 2 + 0) * N + bitrev32((u32)j, VLOG)];  // coset 0, natural index
        if (s == 0) plain[t] = e;
        y[t] = s == 0 ? e : gl_sub(e, plain[t]);
      }
      // Newton form on t = 0..3: y0 + d1 t + d2 t(t-1)/2 + d3 t(t-1)(t-2)/6
      u64 d1 = gl_sub(y[1], y[0]);
      u64 d2 = gl_add(gl_sub(y[2], gl_dbl(y[1])), y[0]);
      u64 d3 = gl_sub(gl_add(gl_sub(y[3], gl_mul(3, y[2])), gl_mul(3, y[1])), y[0]);
      u64 p4 = gl_add(gl_add(y[0], gl_mul(4, d1)), gl_add(gl_mul(6, d2), gl_mul(4, d3)));
      if (p4 != y[4]) {
        err = "internal: a constraint class is not cubic in the openings";
        return BN254S_E_INTERNAL;
      }
      // t -> X with X^2 = 7: t(t-1) = 7 - X, t(t-1)(t-2) = 9X - 21
      u64 h2 = gl_mul(d2, inv2), h3 = gl_mul(d3, inv6);
      gl2 g = gl2_make(gl_sub(gl_add(y[0], gl_mul(7, h2)), gl_mul(21, h3)), gl_add(gl_sub(d1, h2), gl_mul(9, h3)));
      tot = gl2_add(tot, gl2_mul(sel[s], g));
    }
    out[a] = tot;
  }
  return BN254S_OK;
}

// value columns of the two cross-table lookups for instance k (scalar_mul_ctl.rs:57-80, g2 twin, exp_ctl.rs:54-75)
void limbs16(const u64* words4, u64* out) {
  for (int i = 0; i < 16; i++) out[i] = (words4[i >> 2] >> (16 * (i & 3))) & 0xFFFF;
}
void ctl_rows(int kind, const u64* scalars, const u64* x, const u64* off, const u64* outputs, size_t k, std::vector<u64>& in,
              std::vector<u64>& out) {
  const int PW = stark_kind(kind).point_words, PL = 4 * PW;  // 16-bit limbs per point
  in.assign((kind == KIND_FQ ? PL : 2 * PL) + 17, 0);
  out.assign(PL + 1, 0);
  size_t m = 0;
  for (int w = 0; w < PW; w += 4, m += 16) limbs16(x + PW * k + w, &in[m]);
  if (kind != KIND_FQ)
    for (int w = 0; w < PW; w += 4, m += 16) limbs16(off + PW * k + w, &in[m]);
  limbs16(scalars + 4 * k, &in[m]);
  m += 16;
  in[m] = k;
  m = 0;
  for (int w = 0; w < PW; w += 4, m += 16) limbs16(outputs + PW * k + w, &out[m]);
  out[m] = k;
}

}  // namespace

// ---- the verifier in three parts (declared in verify_query.h; bn254s_verify_batch runs them for many proofs) -----------
// Part 1: the shape, the transcript, the vanishing polynomial at zeta and the proof of work.  Leaves the front record of the
// query round (verify_query.h) and the CTL challenges.  c == nullptr: the AIR at zeta on the host (pure host code, no shared
// state: safe on any thread); with a context the quotient kernels evaluate it (named buffers of the context: one call at a time).
int verify_front(bn254s_ctx* c, int kind, const bn254s_params& P, int degree_bits, const u64* w, size_t n_words, View& v, u64* rec,
                 u64 ctl_ch[4], std::string& err) {
  if (!make_view(kind, P, degree_bits, v) || v.total != n_words) {
    err = "bad proof shape";
    return BN254S_E_VERIFY;
  }
  const StarkShape& sh = stark_kind(kind).shape;
  const size_t N = (size_t)1 << degree_bits, M2 = (size_t)1 << v.log_m2;
  const int W = v.W, A = v.A, NQ = v.NQ;
  for (size_t i = 0; i < n_words; i++)
    if (w[i] >= GL_P && i != v.pow) {
      err = "non-canonical field element";
      return BN254S_E_VERIFY;
    }
  // ---- challenges (prover.rs:40-54 / verifier.rs:47-74 + starky get_challenges) ---------------------------------
  Challenger ch;
  ch.observe_n(w + v.caps, 64);
  u64 betas[2], gammas[2], alphas[2];
  for (int i = 0; i < 2; i++) {
    betas[i] = ch.challenge();
    gammas[i] = ch.challenge();
  }
  ctl_ch[0] = betas[0], ctl_ch[1] = betas[1], ctl_ch[2] = gammas[0], ctl_ch[3] = gammas[1];
  u64 st12[12];
  ch.compact(st12);
  if (memcmp(st12, w + v.init, sizeof(st12))) {
    err = "init_challenger_state mismatch";
    return BN254S_E_VERIFY;
  }
  ch.observe_n(w + v.caps + 64, 64);
  for (int i = 0; i < 2; i++) alphas[i] = ch.challenge();
  ch.observe_n(w + v.caps + 128, 64);
  gl2 zeta = ch.challenge_ext();
  ch.observe_n(w + v.local, 2 * (size_t)W);
  ch.observe_n(w + v.aux, 2 * (size_t)A);
  ch.observe_n(w + v.quot, 2 * (size_t)NQ);
  ch.observe_n(w + v.next, 2 * (size_t)W);
  ch.observe_n(w + v.aux_next, 2 * (size_t)A);
  for (int i = 0; i < v.NCTLZ; i++) {
    ch.observe(w[v.ctlz + i]);
    ch.observe(0);
  }
  gl2 fri_alpha = ch.challenge_ext();
  for (size_t i = 0; i < vq_record_words(P.num_queries); i++) rec[i] = 0;
  for (int l = 0; l < v.L; l++) {
    ch.observe_n(w + v.fri_caps + 64 * (size_t)l, 64);
    gl2 b = ch.challenge_ext();
    rec[VQ_REC_BETAS + 2 * l] = b.c0;
    rec[VQ_REC_BETAS + 2 * l + 1] = b.c1;
  }
  ch.observe_n(w + v.final_poly, 2 * v.final_len);
  ch.observe(w[v.pow]);
  u64 pow_response = ch.challenge();
  for (uint32_t q = 0; q < P.num_queries; q++) rec[VQ_REC_QUERIES + q] = ch.challenge() % M2;

  // ---- vanishing polynomial at zeta --------------------------------------------------------------------------------
  const u64 g = gl_root_of_unity(degree_bits);
  gl2 zeta_pow = zeta;
  for (int i = 0; i < degree_bits; i++) zeta_pow = gl2_mul(zeta_pow, zeta_pow);
  const gl2 one = gl2_make(1, 0);
  gl2 z_h = gl2_sub(zeta_pow, one);
  if (gl2_eq(z_h, gl2_make(0, 0))) {
    err = "Opening point is in the subgroup.";
    return BN254S_E_VERIFY;
  }
  const u64 nF = (u64)N % GL_P;
  gl2 l_first = gl2_mul(z_h, gl2_inv(gl2_mul_base(gl2_sub(zeta, one), nF)));
  gl2 l_last = gl2_mul(z_h, gl2_inv(gl2_mul_base(gl2_sub(gl2_mul_base(zeta, g), one), nF)));
  gl2 z_last = gl2_sub(zeta, base(gl_inv(g)));
  gl2 van[2];
  if (c) {  // batched hosts with a context: the constraint sum through the quotient kernels
    int rc = vanishing_on_gpu(c, kind, sh, w, v, alphas, betas, gammas, z_last, l_first, l_last, van, err);
    if (rc != BN254S_OK) return rc;
  } else {  // no context: the independent host statement of the AIR (verify_air_host.h), no GPU involved
    if (!host_air::vanishing_on_host(kind, sh, w + v.local, w + v.next, w + v.aux, w + v.aux_next, alphas, betas, gammas, z_last,
                                     l_first, l_last, van, err))
      return BN254S_E_INTERNAL;
  }
  for (int j = 0; j < 2; j++) {
    gl2 t = gl2_add(ext(w + v.quot + 4 * j), gl2_mul(ext(w + v.quot + 4 * j + 2), zeta_pow));
    if (!gl2_eq(van[j], gl2_mul(z_h, t))) {
      err = "Mismatch between evaluation and opening of quotient polynomial";
      return BN254S_E_VERIFY;
    }
  }

  // ---- verify_fri_proof: proof of work, then what the query rounds need of the openings --------------------------------
  if (pow_response >> (64 - P.pow_bits)) {
    err = "Invalid proof of work witness";
    return BN254S_E_VERIFY;
  }
  // batches of fri_instance: zeta (trace | aux | quotient), g zeta (trace | aux), 1 (CTL Z columns of the aux oracle)
  std::vector<gl2> opened[3];
  for (int p = 0; p < W; p++) opened[0].push_back(ext(w + v.local + 2 * (size_t)p));
  for (int p = 0; p < A; p++) opened[0].push_back(ext(w + v.aux + 2 * (size_t)p));
  for (int p = 0; p < NQ; p++) opened[0].push_back(ext(w + v.quot + 2 * (size_t)p));
  for (int p = 0; p < W; p++) opened[1].push_back(ext(w + v.next + 2 * (size_t)p));
  for (int p = 0; p < A; p++) opened[1].push_back(ext(w + v.aux_next + 2 * (size_t)p));
  for (int p = 0; p < v.NCTLZ; p++) opened[2].push_back(base(w[v.ctlz + p]));
  auto put = [&](int at, gl2 x) { rec[at] = x.c0, rec[at + 1] = x.c1; };
  put(VQ_REC_ALPHA, fri_alpha);
  put(VQ_REC_ZETA, zeta);
  put(VQ_REC_ZETA_NEXT, gl2_mul_base(zeta, g));
  for (int b = 0; b < 3; b++) {
    gl2 acc = gl2_make(0, 0);
    for (size_t j = opened[b].size(); j-- > 0;) acc = gl2_add(gl2_mul(acc, fri_alpha), opened[b][j]);
    put(VQ_REC_REDUCED + 2 * b, acc);
    put(VQ_REC_ALPHA_LEN + 2 * b, gl2_pow(fri_alpha, opened[b].size()));
  }
  return BN254S_OK;
}

// Part 2 on the host: the code of query q (verify_query.h).  The checks run in the verifier's order and stop at the first failure.
int verify_query_host(const View& v, const u64* w, const u64* rec, uint32_t q) {
  for (int t = 0; t < 3; t++)
    if (!vq_merkle_check(v, w, rec, q, t)) return 1 + t;
  const int fri = vq_fri_round(v, w, rec, q);
  return vq_merge_code(v.L, [&](int which) { return which < 3 || vq_merkle_check(v, w, rec, q, which); }, fri);
}

// Part 3: cross-table lookups against the claimed inputs / outputs (ctl_values.rs:28-47)
int verify_ctl(int kind, const View& v, const u64* w, const u64 ctl_ch[4], const u64* scalars, const u64* x, const u64* off,
               const u64* outputs, size_t n, std::string& err) {
  const u64 *betas = ctl_ch, *gammas = ctl_ch + 2;
  u64 sums[2][2] = {{0, 0}, {0, 0}};
  std::vector<u64> in, out;
  for (size_t k = 0; k < n; k++) {
    ctl_rows(kind, scalars, x, off, outputs, k, in, out);
    const std::vector<u64>* rows[2] = {&in, &out};
    for (int t = 0; t < 2; t++)
      for (int cidx = 0; cidx < 2; cidx++) {
        u64 acc = 0;
        for (size_t m = rows[t]->size(); m-- > 0;) acc = gl_add(gl_mul(acc, betas[cidx]), (*rows[t])[m]);
        acc = gl_add(acc, gammas[cidx]);
        if (acc == 0) {
          err = "CTL denominator vanishes";
          return BN254S_E_VERIFY;
        }
        sums[t][cidx] = gl_add(sums[t][cidx], gl_inv(acc));
      }
  }
  for (int t = 0; t < 2; t++)
    for (int cidx = 0; cidx < 2; cidx++)
      if (sums[t][cidx] != w[v.ctlz + 2 * t + cidx]) {
        err = "CTL sum mismatch";
        return BN254S_E_VERIFY;
      }
  return BN254S_OK;
}

static int verify_impl(bn254s_ctx* c, int kind, const bn254s_params& P, int degree_bits, const u64* w, size_t n_words,
                       const u64* scalars, const u64* x, const u64* off, const u64* outputs, size_t n, std::string& err) {
  View v;
  u64 ctl_ch[4];
  std::vector<u64> rec(vq_record_words(P.num_queries));
  int rc = verify_front(c, kind, P, degree_bits, w, n_words, v, rec.data(), ctl_ch, err);
  if (rc != BN254S_OK) return rc;
  for (uint32_t q = 0; q < P.num_queries; q++) {
    const int code = verify_query_host(v, w, rec.data(), q);
    if (code) {
      err = vq_code_text(v.L, code);
      return BN254S_E_VERIFY;
    }
  }
  return verify_ctl(kind, v, w, ctl_ch, scalars, x, off, outputs, n, err);
}

extern "C" int bn254s_ctl_values(int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* off, const uint64_t* outputs,
                                 size_t n, uint64_t* in_rows, uint64_t* out_rows) {
  if (kind < 0 || kind > 2 || !scalars || !x || (kind != KIND_FQ && !off) || !outputs || !in_rows || !out_rows)
    return BN254S_E_INVALID_ARG;
  std::vector<u64> in, out;
  for (size_t k = 0; k < n; k++) {
    ctl_rows(kind, scalars, x, off, outputs, k, in, out);
    memcpy(in_rows + k * in.size(), in.data(), in.size() * 8);
    memcpy(out_rows + k * out.size(), out.data(), out.size() * 8);
  }
  return BN254S_OK;
}

extern "C" int bn254s_verify_host(int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words, size_t n_words,
                                  const uint64_t* scalars, const uint64_t* x, const uint64_t* off, const uint64_t* outputs, size_t n,
                                  char* err_buf, size_t err_cap) {
  if (err_buf && err_cap) err_buf[0] = 0;
  if (kind < 0 || kind > 2 || !params || params->struct_size != sizeof(bn254s_params) || !words || !scalars || !x ||
      (kind != KIND_FQ && !off) || !outputs || n == 0 || degree_bits < 7 || degree_bits > 30)
    return BN254S_E_INVALID_ARG;
  std::string err;
  int rc;
  if (params->num_challenges != 2 || params->rate_bits != 1) {
    err = "only num_challenges = 2, rate_bits = 1 are supported";
    rc = BN254S_E_UNSUPPORTED;
  } else {
    rc = verify_impl(nullptr, kind, *params, (int)degree_bits, words, n_words, scalars, x, off, outputs, n, err);
  }
  if (rc != BN254S_OK && err_buf && err_cap) {
    strncpy(err_buf, err.c_str(), err_cap - 1);
    err_buf[err_cap - 1] = 0;
  }
  return rc;
}

extern "C" int bn254s_verify(bn254s_ctx* c, int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words,
                             size_t n_words, const uint64_t* scalars, const uint64_t* x, const uint64_t* off, const uint64_t* outputs,
                             size_t n) {
  if (!c || kind < 0 || kind > 2 || !params || params->struct_size != sizeof(bn254s_params) || !words || !scalars || !x ||
      (kind != KIND_FQ && !off) || !outputs || n == 0 || degree_bits < 7 || degree_bits > 30)
    return BN254S_E_INVALID_ARG;
  if (params->num_challenges != 2 || params->rate_bits != 1) {
    c->set_err("only num_challenges = 2, rate_bits = 1 are supported");
    return BN254S_E_UNSUPPORTED;
  }
  if (hipSetDevice(c->device) != hipSuccess) return BN254S_E_HIP;
  std::string err;
  int rc = verify_impl(c, kind, *params, (int)degree_bits, words, n_words, scalars, x, off, outputs, n, err);
  if (rc != BN254S_OK) c->set_err(err);
  return rc;
}
