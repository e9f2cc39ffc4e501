// One FRI query round of the native verifier as host/device functions, shared by verify.hip (bn254s_verify, bn254s_verify_host: one
// proof on the host) and verify_batch.hip (bn254s_verify_batch: the rounds of many proofs as kernels).
//
// A query round is everything verify_fri_proof does per query index: the Merkle paths of the three initial trees, the combination
// of the opened leaves (fri_combine_initial), per FRI layer the consistency check, the arity-2^ab interpolation at the layer's
// beta (compute_evaluation) and the layer's Merkle path, and the final polynomial.  It needs the proof words and a handful of
// transcript values, which the host part of the verifier (verify_front in verify.hip) leaves in a flat per-proof FRONT RECORD of
// u64 words (an extension element is two words c0, c1):
//
//   word  0 ..  1   fri_alpha
//         2 ..  7   reduced[3]     the alpha-reduced openings of the three batches (zeta | g zeta | 1)
//         8 .. 13   alpha_len[3]   fri_alpha ^ (polynomials in the batch)
//        14 .. 15   zeta           first opening point
//        16 .. 17   g zeta         second opening point (the third is 1)
//        18 .. 33   fri_betas[FRI_MAX_LAYERS]   (unused layers are zero)
//        34 ..      num_queries query indices, each below 2^(degree_bits + rate_bits)
//
// Per-query code = the first failing check in the verifier's own order, counted from 1 (L = number of FRI layers):
//   0 pass | 1, 2, 3 initial tree 0, 1, 2 | 4 + 2l consistency at layer l | 5 + 2l Merkle path of layer l | 4 + 2L final polynomial
// vq_merkle_check and vq_fri_round report their halves of it; vq_merge_code puts them together.
//
// Bounds: both functions index the untrusted word array by offsets computed from the View alone (make_view; the caller has
// checked that the array holds view.total words) and by the record's query index, which the caller has checked to be below
// 2^log_m2.  No proof word is used as an index.
#pragma once
#include <string>
#include <vector>
#include "fri.h"
#include "poseidon_dev.h"
#include "prover.h"

static constexpr int VQ_REC_ALPHA = 0, VQ_REC_REDUCED = 2, VQ_REC_ALPHA_LEN = 8, VQ_REC_ZETA = 14, VQ_REC_ZETA_NEXT = 16,
                     VQ_REC_BETAS = 18, VQ_REC_QUERIES = VQ_REC_BETAS + 2 * FRI_MAX_LAYERS;
inline size_t vq_record_words(uint32_t num_queries) { return (size_t)VQ_REC_QUERIES + num_queries; }

struct View {  // offsets into the word layout (plain data: passed to the kernels by value)
  int W, A, NQ, NCTLZ, L, log_n, log_m2, cap_h, P, num_lookup, num_queries;
  int layer_path[FRI_MAX_LAYERS], arity_bits[FRI_MAX_LAYERS];
  size_t caps, local, next, aux, aux_next, ctlz, quot, fri_caps, queries, wpq, final_poly, final_len, pow, init, total;
};

// false: a shape the word layout cannot hold.  Arities above 16, more than FRI_MAX_LAYERS layers and caps of more than the 16
// digests the layout reserves count as such (the provers refuse those parameter sets, proof_plan.hip).
inline bool make_view(int kind, const bn254s_params& P, int degree_bits, View& v) {
  const StarkShape& sh = stark_kind(kind).shape;
  v.W = sh.W;
  v.A = sh.n_aux();
  v.NQ = 4;
  v.NCTLZ = 4;
  v.num_lookup = sh.n_lookup_cols();
  v.num_queries = (int)P.num_queries;
  v.log_n = degree_bits;
  v.log_m2 = degree_bits + P.rate_bits;
  v.cap_h = P.cap_height;
  v.P = v.log_m2 - v.cap_h;
  if (P.arity_bits < 1 || P.arity_bits > 4 || P.cap_height > 4 || v.P < 0) return false;
  std::vector<int> ar = fri_arities(P, degree_bits);
  if (ar.size() > (size_t)FRI_MAX_LAYERS) return false;
  v.L = (int)ar.size();
  size_t o = 0;
  v.caps = o; o += 3 * 64;
  v.local = o; o += 2 * (size_t)v.W;
  v.next = o; o += 2 * (size_t)v.W;
  v.aux = o; o += 2 * (size_t)v.A;
  v.aux_next = o; o += 2 * (size_t)v.A;
  v.ctlz = o; o += v.NCTLZ;
  v.quot = o; o += 2 * (size_t)v.NQ;
  v.fri_caps = o; o += (size_t)v.L * 64;
  v.queries = o;
  v.wpq = (size_t)(v.W + v.A + v.NQ) + 3 * (size_t)v.P * 4;
  int bits = v.log_m2, sum = 0;
  for (int l = 0; l < FRI_MAX_LAYERS; l++) v.layer_path[l] = v.arity_bits[l] = 0;
  for (int l = 0; l < v.L; l++) {
    bits -= ar[l];
    sum += ar[l];
    int pl = bits - v.cap_h;
    if (pl < 0) return false;
    v.layer_path[l] = pl;
    v.arity_bits[l] = ar[l];
    v.wpq += 2 * ((size_t)1 << ar[l]) + (size_t)pl * 4;
  }
  o += v.wpq * P.num_queries;
  v.final_len = (size_t)1 << (degree_bits - sum);
  v.final_poly = o; o += 2 * v.final_len;
  v.pow = o; o += 1;
  v.init = o; o += 12;
  v.total = o;
  return true;
}

GL_HD gl2 vq_ext(const u64* w) { return gl2_make(w[0], w[1]); }
GL_HD u32 vq_rev_bits(u32 x, int bits) { return bits ? bitrev32(x, (unsigned)bits) : 0; }

// PoseidonHash::hash_or_noop: a leaf of at most 4 words is its own digest (zero padded), a longer one goes through the sponge
GL_HD void vq_hash_or_noop(const u64* in, int n, u64 out[4]) {
  if (n <= 4) {
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = i < n ? in[i] : 0;
    return;
  }
  u64 st[12];
#pragma unroll
  for (int i = 0; i < 12; i++) st[i] = 0;
  for (int i = 0; i < n; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (i + k < n) st[k] = in[i + k];
    poseidon_permute(st);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) out[i] = st[i];
}

// Merkle check `which` of query q: 0..2 = initial tree (trace | aux | quotient) at the query index, 3 + l = FRI layer l at
// x_index >> (sum of the arity bits up to and including layer l).  hash_or_noop of the leaf, the path with two_to_one, the
// compare with the cap.  The number of permutations depends on (view, which) only, never on the data: lanes of a wave that
// share `which` stay uniform.
GL_HD bool vq_merkle_check(const View& v, const u64* w, const u64* rec, u32 q, int which) {
  size_t index = (size_t)rec[VQ_REC_QUERIES + q];
  const u64* r = w + v.queries + v.wpq * q;
  const u64* cap;
  int leaf_len, path_len;
  if (which < 3) {
    const int widths[3] = {v.W, v.A, v.NQ};
    for (int t = 0; t < which; t++) r += widths[t] + 4 * v.P;
    leaf_len = widths[which];
    path_len = v.P;
    cap = w + v.caps + 64 * (size_t)which;
  } else {
    const int l = which - 3;
    r += (size_t)(v.W + v.A + v.NQ) + 12 * (size_t)v.P;
    for (int m = 0; m < l; m++) r += ((size_t)2 << v.arity_bits[m]) + 4 * (size_t)v.layer_path[m];
    for (int m = 0; m <= l; m++) index >>= v.arity_bits[m];
    leaf_len = 2 << v.arity_bits[l];
    path_len = v.layer_path[l];
    cap = w + v.fri_caps + 64 * (size_t)l;
  }
  const u64* path = r + leaf_len;
  u64 cur[4];
  vq_hash_or_noop(r, leaf_len, cur);
  for (int i = 0; i < path_len; i++) {
    const u64* sib = path + 4 * i;
    const bool right = index & 1;  // the running digest is the right child
    u64 s[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      s[k] = right ? sib[k] : cur[k];
      s[4 + k] = right ? cur[k] : sib[k];
      s[8 + k] = 0;
    }
    poseidon_permute(s);
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = s[k];
    index >>= 1;
  }
  const u64* c = cap + 4 * index;  // index < 2^cap_h: the query index is below 2^log_m2
  return cur[0] == c[0] && cur[1] == c[1] && cur[2] == c[2] && cur[3] == c[3];
}

// acc = acc * alpha + x over the columns col0 + n - 1 .. col0 of a leaf (the reduction runs from the last polynomial down)
GL_HD gl2 vq_reduce_leaf(gl2 acc, gl2 alpha, const u64* leaf, int col0, int n) {
  for (int j = n; j-- > 0;) {
    acc = gl2_mul(acc, alpha);
    acc.c0 = gl_add(acc.c0, leaf[col0 + j]);
  }
  return acc;
}

// The arithmetic of query q: fri_combine_initial, per layer the consistency check and compute_evaluation, the final polynomial.
// Returns 0, 1 + l for the consistency check of layer l, or L + 1 for the final polynomial: the first that fails.
//
// compute_evaluation interpolates the 2^ab values of the coset x0 <gg> (x0 = the coset's first point, gg of order n = 2^ab) at
// beta in Lagrange form.  The points are p_i = x0 gg^i, so prod_{k != i} (p_i - p_k) = n p_i^(n-1) = n x0^n / p_i: one inversion
// per layer, and no division by (beta - p_k), so the result is the interpolant for every beta.
GL_HD int vq_fri_round(const View& v, const u64* w, const u64* rec, u32 q) {
  const size_t x_index = (size_t)rec[VQ_REC_QUERIES + q];
  const gl2 alpha = vq_ext(rec + VQ_REC_ALPHA);
  const u64* r = w + v.queries + v.wpq * q;
  const u64* trace = r;
  const u64* auxl = trace + v.W + 4 * v.P;
  const u64* quot = auxl + v.A + 4 * v.P;
  r = quot + v.NQ + 4 * v.P;
  u64 subgroup_x = gl_mul(GL_GEN, gl_pow(gl_root_of_unity((unsigned)v.log_m2), vq_rev_bits((u32)x_index, v.log_m2)));
  // batches of fri_instance: zeta (trace | aux | quotient), g zeta (trace | aux), 1 (CTL Z columns of the aux oracle)
  gl2 sum = gl2_make(0, 0);
  for (int b = 0; b < 3; b++) {
    gl2 acc = gl2_make(0, 0);
    gl2 point;
    if (b == 0) {
      acc = vq_reduce_leaf(acc, alpha, quot, 0, v.NQ);
      acc = vq_reduce_leaf(acc, alpha, auxl, 0, v.A);
      acc = vq_reduce_leaf(acc, alpha, trace, 0, v.W);
      point = vq_ext(rec + VQ_REC_ZETA);
    } else if (b == 1) {
      acc = vq_reduce_leaf(acc, alpha, auxl, 0, v.A);
      acc = vq_reduce_leaf(acc, alpha, trace, 0, v.W);
      point = vq_ext(rec + VQ_REC_ZETA_NEXT);
    } else {
      acc = vq_reduce_leaf(acc, alpha, auxl, v.num_lookup, v.NCTLZ);
      point = gl2_make(1, 0);
    }
    const gl2 num = gl2_sub(acc, vq_ext(rec + VQ_REC_REDUCED + 2 * b));
    const gl2 den = gl2_sub(gl2_make(subgroup_x, 0), point);
    sum = gl2_add(gl2_mul(sum, vq_ext(rec + VQ_REC_ALPHA_LEN + 2 * b)), gl2_mul(num, gl2_inv(den)));
  }
  gl2 old_eval = sum;
  size_t xi = x_index;
  for (int l = 0; l < v.L; l++) {
    const int ab = v.arity_bits[l];
    const size_t arity = (size_t)1 << ab;
    const u64* evals = r;
    r += 2 * arity + 4 * (size_t)v.layer_path[l];
    const size_t within = xi & (arity - 1);
    if (!gl2_eq(vq_ext(evals + 2 * within), old_eval)) return 1 + l;
    const gl2 beta = vq_ext(rec + VQ_REC_BETAS + 2 * l);
    const u64 gg = gl_root_of_unity((unsigned)ab);
    const u64 x0 = gl_mul(subgroup_x, gl_pow(gg, arity - vq_rev_bits((u32)within, ab)));
    u64 x0n = x0;
    for (int k = 0; k < ab; k++) x0n = gl_mul(x0n, x0n);
    const u64 cinv = gl_inv(gl_mul((u64)arity, x0n));  // 1 / (n x0^n)
    gl2 res = gl2_make(0, 0);
    u64 pi = x0;
    for (size_t i = 0; i < arity; i++) {
      gl2 num = gl2_make(1, 0);
      u64 pk = x0;
      for (size_t k = 0; k < arity; k++) {
        if (k != i) num = gl2_mul(num, gl2_sub(beta, gl2_make(pk, 0)));
        pk = gl_mul(pk, gg);
      }
      const gl2 ev = vq_ext(evals + 2 * (size_t)vq_rev_bits((u32)i, ab));  // the layer stores its coset in bit-reversed order
      res = gl2_add(res, gl2_mul(ev, gl2_mul_base(num, gl_mul(pi, cinv))));
      pi = gl_mul(pi, gg);
    }
    old_eval = res;
    for (int k = 0; k < ab; k++) subgroup_x = gl_mul(subgroup_x, subgroup_x);
    xi >>= ab;
  }
  gl2 fin = gl2_make(0, 0);
  for (size_t i = v.final_len; i-- > 0;) fin = gl2_add(gl2_mul_base(fin, subgroup_x), vq_ext(w + v.final_poly + 2 * i));
  return gl2_eq(fin, old_eval) ? 0 : v.L + 1;
}

// The code of a query from its Merkle results (mk(which) = 1 where the path checks out, which = 0 .. 2 + L) and vq_fri_round's
// result: inside a query the Merkle result of layer l counts after the consistency check of layer l, as verify_fri_proof runs.
template <class MK>
GL_HD int vq_merge_code(int L, MK mk, int fri) {
  for (int t = 0; t < 3; t++)
    if (!mk(t)) return 1 + t;
  for (int l = 0; l < L; l++) {
    if (fri == 1 + l) return 4 + 2 * l;
    if (!mk(3 + l)) return 5 + 2 * l;
  }
  return fri == L + 1 ? 4 + 2 * L : 0;
}

// the reference's error text of a non-zero code
inline const char* vq_code_text(int L, int code) {
  if (code <= 3) return "Invalid Merkle proof (initial tree)";
  if (code == 4 + 2 * L) return "Final polynomial evaluation is invalid";
  return (code & 1) ? "Invalid Merkle proof (FRI layer)" : "FRI consistency check failed";
}

// ---- the three parts of the verifier (verify.hip) -----------------------------------------------------------------------------
struct bn254s_ctx;
// everything up to and including the proof-of-work check; writes the front record (vq_record_words(num_queries) words) and the
// CTL challenges (beta0 beta1 gamma0 gamma1).  c == nullptr: pure host code without shared state.
int verify_front(bn254s_ctx* c, int kind, const bn254s_params& P, int degree_bits, const u64* w, size_t n_words, View& v, u64* rec,
                 u64 ctl_ch[4], std::string& err);
int verify_query_host(const View& v, const u64* w, const u64* rec, uint32_t q);  // the code of query q, on the host
int verify_ctl(int kind, const View& v, const u64* w, const u64 ctl_ch[4], const u64* scalars, const u64* x, const u64* off,
               const u64* outputs, size_t n, std::string& err);
