/*
 * bn254_stark.h - C ABI of the MI355X-native prover for the BN254 scalar-multiplication STARKs.
 *
 * Drop-in boundary: one call replaces the body of the reference's witness generator
 *   G1StarkProofGenerator::run_once   src/generators/g1/stark_proof.rs:136-179
 * namely lines :143-163 (outputs = s*x+offset, generate_trace, starks::common::prover::prove).  The caller
 * (a Rust shim) keeps get_witness / set_witness / verify / set_stark_proof_target.
 * G2 (src/generators/g2/stark_proof.rs:136-179) and Fq-exp (src/generators/fq/stark_proof.rs:135-178)
 * entry points have the same shape.
 *
 * Wire formats (all little-endian u64 words, canonical = reduced, non-Montgomery):
 *   scalar  : 4 words, any 256-bit value (NOT reduced modulo the group order; common/utils.rs:21-25)
 *   Fq      : 4 words, value < p
 *   G1 point: 8 words = x, y (affine, never infinity; src/curves/g1.rs:170-174)
 *   G2 point: 16 words = x.c0, x.c1, y.c0, y.c1
 *   Goldilocks element: 1 word < 2^64 - 2^32 + 1; extension element: 2 words (c0, c1)
 *   Poseidon digest: 4 words
 *
 * Proof layout returned by bn254s_proof_words() - field order of starky's StarkProofWithMetadata
 * (reference src/starks/common/prover.rs:66-71), W = trace width, A = auxiliary polys, L = FRI layers,
 * P = lde_bits - cap_height Merkle path length of the initial trees:
 *   trace_cap[16*4] aux_cap[16*4] quotient_cap[16*4]
 *   openings: local_values[W*2] next_values[W*2] auxiliary_polys[A*2] auxiliary_polys_next[A*2]
 *             ctl_zs_first[4] quotient_polys[4*2]
 *   commit_phase_merkle_caps[L][16*4]
 *   query_round_proofs[84]: for oracle in (trace, aux, quotient): leaf[width] path[P*4];
 *                           for layer l: evals[16*2] path[P_l*4]
 *   final_poly[len*2]  pow_witness[1]  init_challenger_state[12]
 *
 * Errors: every function returns 0 on success or a negative BN254S_E_* code; the reference panics
 * (unwrap at stark_proof.rs:163,172), the Rust shim maps non-zero to panic!.
 * Threading: one call at a time per context (one host thread enters the context at a time); any number of contexts (one per
 * GPU / per host thread).  A batch opened with bn254s_prove_batch_begin stays in flight after _begin returns: until its _end
 * the context may still be entered, one call at a time, and every proving entry point (bn254s_prove_g1 / _g2 / _fq_exp /
 * _batch* / bn254s_map_to_g2 / bn254s_g1_msm / bn254s_g2_msm / bn254s_g1_recover_from_x / bn254s_g2_recover_from_x /
 * bn254s_g2_subgroup_check / bn254s_g2_clear_cofactor / bn254s_job_outputs / bn254s_map_to_g1 / bn254s_fq_sqrt /
 * bn254s_fq2_sqrt / bn254s_prove_batch_checked / bn254s_scalar_mul / bn254s_msm_multi) queues behind the open batches on the same worker pool and runs on a free slot (stream + workspace) of its
 * own, so it can never share device state with a proof of the open batch; bn254s_verify_batch uses the context's own stream and device memory that it allocates
 * and frees itself, so it is independent of open batches too; bn254s_verify, _commit_values, _generate_trace, the _bench_* calls and the device
 * front-ends (bn254s_g1_recover_from_x_batch, bn254s_g2_recover_from_x_batch, bn254s_g2_subgroup_check_batch,
 * bn254s_g2_clear_cofactor_batch, bn254s_map_to_g2_batch, bn254s_hash_to_g2_batch, bn254s_job_outputs_batch,
 * bn254s_hash_to_fq_batch, bn254s_map_to_g1_batch, bn254s_hash_to_g1_batch, bn254s_fq_sqrt_batch, bn254s_fq2_sqrt_batch,
 * bn254s_fq_inv_batch, bn254s_fq2_inv_batch, bn254s_job_check_batch, bn254s_scalar_mul_batch, bn254s_msm_multi_chain and the front-end halves of bn254s_g1_recover_from_x,
 * bn254s_g2_recover_from_x, bn254s_g2_subgroup_check, bn254s_g2_clear_cofactor, bn254s_job_outputs, bn254s_map_to_g1,
 * bn254s_fq_sqrt, bn254s_fq2_sqrt, bn254s_prove_batch_checked, bn254s_scalar_mul and bn254s_msm_multi, like those of bn254s_map_to_g2 and the msm chains) use the context's own stream and pooled buffers under keys of their own ("g2sub"
 * for the subgroup check, "g2cof" and "g2cof.link" for cofactor clearing, "m2g.batch" for the proof-free map, "jobout" for the
 * job outputs, "jobchk" for the job check, "smul" for the scalar multiplication without an offset, "msm.multi" for many MSMs in one chain, "m2g1", "h2f1.in" and "h2f1.out" for map_to_g1 and hash_to_fq, "fqsqrt", "fq2sqrt" and "fqinv" for the field
 * gadgets) and are independent of open batches.
 */
#ifndef BN254_STARK_H
#define BN254_STARK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN254S_ABI_VERSION 1

enum {
  BN254S_OK = 0,
  BN254S_E_INVALID_ARG = -1,
  BN254S_E_HIP = -2,            /* HIP runtime / launch failure, see bn254s_last_error */
  BN254S_E_OOM = -3,
  BN254S_E_INVALID_POINT = -4,  /* a + (-a) met during the double-and-add chain (generate_g1_add, add.rs:49-51) */
  BN254S_E_UNSUPPORTED = -5,    /* shape not implemented by this build */
  BN254S_E_TRANSCRIPT = -6,     /* opening point inside the subgroup (starky "Opening point is in the subgroup") */
  BN254S_E_INTERNAL = -7,       /* a device-side self check failed (the reference's assert!s in modulus_zero.rs:82,99-103) */
  BN254S_E_VERIFY = -8          /* bn254s_verify: the proof was rejected; bn254s_last_error holds the reference's error text */
};

typedef struct bn254s_ctx bn254s_ctx;
typedef struct bn254s_proof bn254s_proof;

/* StarkConfig::standard_fast_config() + min_rows (stark_proof.rs:152-154). POD, versioned by struct_size. */
typedef struct bn254s_params {
  uint32_t struct_size;
  uint32_t security_bits;   /* 100 */
  uint32_t num_challenges;  /* 2 */
  uint32_t rate_bits;       /* 1 */
  uint32_t cap_height;      /* 4 */
  uint32_t pow_bits;        /* 16 */
  uint32_t arity_bits;      /* 4  (ConstantArityBits(4, 5)) */
  uint32_t final_poly_bits; /* 5 */
  uint32_t num_queries;     /* 84 */
  uint32_t min_rows_log2;   /* 16 */
} bn254s_params;

void bn254s_params_default(bn254s_params* p);
int bn254s_abi_version(void);

/* One context per GPU: owns the HIP stream(s), twiddle tables and the pooled device workspace.
 * SURVEY.md section 8(b) sketched `bn254s_ctx_create(device_ids, n)` and `device_mask` / `batch_mode` fields in
 * bn254s_params; this ABI keeps the parameters a pure restatement of StarkConfig and expresses both ideas as calls instead:
 * one context per device (this function, any number of times) + bn254s_prove_batch_multi(ctxs, n_ctx, ...) for "these
 * devices", and bn254s_prove_g1 (one proof for all jobs, what Bn254Hook::constrain needs) vs bn254s_prove_batch (independent
 * per_proof-sized proofs) for the batch mode. */
int bn254s_ctx_create(int device_id, bn254s_ctx** out);
void bn254s_ctx_destroy(bn254s_ctx* ctx);
const char* bn254s_last_error(const bn254s_ctx* ctx);
/* Gives the device memory of every idle slot back to the driver (a slot = stream + workspace of one proof in flight; the
 * workspaces are grow-only otherwise: after a 2^23-row proof slot 0 keeps ~245 GB).  Slots that are proving right now are left
 * alone.  The next proof on a trimmed slot allocates its workspace again (a few ms). */
int bn254s_ctx_trim(bn254s_ctx* ctx);

/* Prove n G1 scalar multiplications s_i * x_i + offset_i in ONE STARK (timestamps 0..n-1), like
 * G1ScalarMulStark::generate_trace + prove (scalar_mul_stark.rs:55-69, common/prover.rs:18-72).
 * rows = max(2^min_rows_log2, 512 n) rounded up to a power of two; 2^16 .. 2^23 rows (n <= 16384) are supported
 * (a G1 proof of 2^22 rows keeps about 200 GB resident, one of 2^23 rows about 245 GB: its workspace is laid out to fit;
 * a G2 proof of 2^23 rows, whose two LDEs alone would be 296 GB, runs in a streaming workspace that keeps only coefficients
 * resident and recomputes LDE rows where they are needed: 8.0 s, ~250 GB),
 * i.e. one proof can cover all calls of a circuit exactly as Bn254Hook::constrain batches them (hook.rs:63-71). */
int bn254s_prove_g1(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars /* n x 4 */,
                    const uint64_t* x /* n x 8 */, const uint64_t* offset /* n x 8 */, size_t n, bn254s_proof** out);

/* Throughput entry point: n_total jobs are cut into ceil(n_total / per_proof) independent proofs
 * (per_proof = 128 gives the reference test shape, 2^16 rows) that are pipelined on the GPU.
 * proofs_out must have room for that many pointers. */
int bn254s_prove_g1_batch(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                          const uint64_t* offset, size_t n_total, size_t per_proof, bn254s_proof** proofs_out);

/* Generic form of the above: kind 0 = G1, 1 = G2 (points 16 words), 2 = Fq exp (x 4 words, offset NULL). */
int bn254s_prove_batch(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                       const uint64_t* offset, size_t n_total, size_t per_proof, bn254s_proof** proofs_out);

/* The same call in two halves, for a caller that keeps the GPU fed: _begin queues the proofs of the batch on the context's
 * worker threads and returns; _end waits for them and returns what bn254s_prove_batch would have (on an error every proof of
 * the batch is freed and its slot in proofs_out is NULL).  Batches are served in the order of their _begin calls, up to twelve
 * proofs in flight in total, so the first proofs of the next batch run while the last ones of the current batch finish (the
 * reference's callers do the same with rayon over independent circuits).  scalars / x / offset / proofs_out must stay valid
 * until _end; every handle must be passed to _end exactly once, before bn254s_ctx_destroy.  bn254s_prove_batch is
 * _begin followed by _end, and the single-proof entry points are a batch of one proof: all of them may be called while
 * handles are open (see "Threading" at the top). */
typedef struct bn254s_batch bn254s_batch;
int bn254s_prove_batch_begin(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                             const uint64_t* offset, size_t n_total, size_t per_proof, bn254s_proof** proofs_out,
                             bn254s_batch** handle);
int bn254s_prove_batch_end(bn254s_batch* handle);

/* Several GPUs from one process: proof i is proven by ctxs[i mod n_ctx] (one context per GPU); no inter-GPU traffic.
 * Same arguments and results as bn254s_prove_batch otherwise. */
int bn254s_prove_batch_multi(bn254s_ctx** ctxs, size_t n_ctx, int kind, const bn254s_params* params, const uint64_t* scalars,
                             const uint64_t* x, const uint64_t* offset, size_t n_total, size_t per_proof, bn254s_proof** proofs);

/* Same for G2 (points n x 16 words: x.c0, x.c1, y.c0, y.c1): src/generators/g2/stark_proof.rs:136-179. */
int bn254s_prove_g2(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                    const uint64_t* offset, size_t n, bn254s_proof** out);
/* Fq exponentiation x_i ^ s_i (FqExpInput { s, x }, src/starks/fields/exp_stark.rs:36-39): no offset. */
int bn254s_prove_fq_exp(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars /* n x 4 */,
                        const uint64_t* x /* n x 4 */, size_t n, bn254s_proof** out);

/* Proof accessors.  Pointers stay valid until bn254s_proof_free. */
int bn254s_proof_words(const bn254s_proof* p, const uint64_t** data, size_t* len);
/* Per-field accessor: the words of one field of StarkProofWithMetadata (reference common/prover.rs:66-71), i.e. what
 * set_stark_proof_target (generators/g1/stark_proof.rs:173) walks field by field.  Extension elements are two words
 * (c0, c1), digests four, a cap 16 digests; BN254S_SEC_QUERY_ROUNDS is the 84 query rounds back to back in the layout
 * documented at the top of this file (per round: three initial-tree openings, then one opening per FRI layer). */
enum {
  BN254S_SEC_TRACE_CAP = 0,
  BN254S_SEC_AUX_CAP = 1,
  BN254S_SEC_QUOTIENT_CAP = 2,
  BN254S_SEC_LOCAL_VALUES = 3,
  BN254S_SEC_NEXT_VALUES = 4,
  BN254S_SEC_AUX_POLYS = 5,
  BN254S_SEC_AUX_POLYS_NEXT = 6,
  BN254S_SEC_CTL_ZS_FIRST = 7,
  BN254S_SEC_QUOTIENT_POLYS = 8,
  BN254S_SEC_FRI_CAPS = 9,
  BN254S_SEC_QUERY_ROUNDS = 10,
  BN254S_SEC_FINAL_POLY = 11,
  BN254S_SEC_POW_WITNESS = 12,
  BN254S_SEC_INIT_CHALLENGER_STATE = 13,
  BN254S_SEC_COUNT = 14
};
int bn254s_proof_section(const bn254s_proof* p, int id, const uint64_t** data, size_t* len);
int bn254s_proof_degree_bits(const bn254s_proof* p);
/* n x (8 | 16 | 4) words: the outputs s*x+offset (what run_once writes with set_witness at :147-149). */
int bn254s_proof_outputs(const bn254s_proof* p, const uint64_t** data, size_t* len);
/* Per-stage GPU milliseconds of the call that produced the proof (names via bn254s_stage_name). */
int bn254s_proof_stage_ms(const bn254s_proof* p, const float** ms, size_t* n_stages);
const char* bn254s_stage_name(size_t stage);
size_t bn254s_proof_serialize(const bn254s_proof* p, uint8_t* buf, size_t cap); /* LE bytes of the word layout */
void bn254s_proof_free(bn254s_proof* p);

/* Native verification of a proof in the word layout above: the reference's `verify` (src/starks/common/verifier.rs:32-98:
 * challenges, starky's verify_stark_proof_with_challenges, plonky2's verify_fri_proof) plus the cross-table-lookup check
 * against the claimed inputs and outputs (common/ctl_values.rs:28-47 with the rows of scalar_mul_ctl.rs:57-80 /
 * g2 twin / exp_ctl.rs:54-75; timestamps are 0..n-1).  kind 0 = G1, 1 = G2, 2 = Fq exp (offset NULL); outputs = the
 * n x (8 | 16 | 4) words of bn254s_proof_outputs.  Returns BN254S_OK, or BN254S_E_VERIFY with the reason in
 * bn254s_last_error.  With a context the constraint sum at zeta is evaluated by the quotient kernels (csrc/verify.hip); see
 * bn254s_verify_host for the GPU-free form. */
int bn254s_verify(bn254s_ctx* ctx, int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words,
                  size_t n_words, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, const uint64_t* outputs,
                  size_t n);
/* The same verifier without a context and without a GPU: the constraint sum at zeta comes from an independent host statement
 * of the three AIRs over the quadratic extension (csrc/verify_air_host.h, written from the reference's eval_packed_generic
 * functions, not from the quotient kernels), everything else (transcript, FRI, Merkle paths, CTL sums) is host code in both.
 * A few milliseconds per proof on one core.  On rejection the reference verifier's error text is copied to err_buf
 * (may be NULL). */
int bn254s_verify_host(int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words, size_t n_words,
                       const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, const uint64_t* outputs, size_t n,
                       char* err_buf, size_t err_cap);

/* The same verifier for n_proofs proofs of ONE kind, parameter set and height (callers group their proofs): words[i] points to
 * the n_words words of proof i; the job arrays (scalars, x, offset, outputs) hold the jobs of all proofs one after the other in
 * proof order, n_jobs[i] of them for proof i.  Same argument rules as bn254s_verify (num_challenges = 2, rate_bits = 1,
 * degree_bits 7..30).
 *
 * Per proof, in this order: the front (shape, transcript, the AIR at zeta on the host as in bn254s_verify_host, proof of work);
 * the FRI query rounds; the cross-table-lookup check.  The fronts and the CTL checks of different proofs run on min(16, n_proofs)
 * host threads.  With a context the query rounds of every proof that passed its front run on the device (csrc/verify_batch.hip:
 * Merkle paths one lane per (proof, query, tree), FRI arithmetic one lane per (proof, query); proof words go up in chunks of at
 * most 256 MiB, device memory is allocated and freed by the call, all work goes on the context's stream, and the call may run
 * while a batch of bn254s_prove_batch_begin is open).  ctx = NULL: the query rounds run on the host threads too, no GPU.
 *
 * status[i] (and err + i * err_stride, NUL-terminated, at most err_stride bytes; err may be NULL) are what bn254s_verify_host
 * returns for proof i alone: BN254S_OK and "", or BN254S_E_VERIFY and the reference verifier's text.
 * Returns BN254S_OK: every proof accepted.  BN254S_E_VERIFY: at least one proof rejected, status and err filled for every proof
 * and bn254s_last_error reads "proof i: text" for the lowest rejected i.  Any other code: the call itself failed
 * (BN254S_E_INVALID_ARG: a NULL array or words[i], n_proofs = 0, some n_jobs[i] = 0, err given with err_stride = 0, a kind outside
 * 0..2, a params->struct_size mismatch; BN254S_E_HIP / BN254S_E_OOM from the device: status holds that code for every proof). */
int bn254s_verify_batch(bn254s_ctx* ctx, int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* const* words,
                        size_t n_words, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, const uint64_t* outputs,
                        const size_t* n_jobs, size_t n_proofs, int32_t* status, char* err, size_t err_stride);

/* The extra looking values of the two cross-table lookups (reference g1_generate_ctl_values, scalar_mul_ctl.rs:57-80; G2 twin;
 * fq_generate_ctl_values, exp_ctl.rs:54-75), i.e. what run_once hands to set_ctl_values_target (stark_proof.rs:174-178):
 * per instance one input row  [x limbs | offset limbs (not for Fq) | 16 scalar limbs | timestamp]  of 81 / 145 / 33 words and
 * one output row [output limbs | timestamp] of 33 / 65 / 17 words, all 16-bit little-endian limbs.  Host only, no context. */
int bn254s_ctl_values(int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset, const uint64_t* outputs,
                      size_t n, uint64_t* in_rows, uint64_t* out_rows);

/* map_to_g2 of n Fq2 elements u (8 words: c0, c1) - reference src/utils/hash_to_g2.rs:113-148 and its circuit :150-207, the
 * pipeline of BASELINE config 5: the Shallue-van de Woestijne candidates and the signed square root are computed on the device,
 * the two Legendre symbols per input are proven as Fq exponentiations ((p-1)/2, norm(g(x_i))), the cofactor is cleared by a
 * proven G2 scalar multiplication cofactor * (x, y) + offset, and output - offset is returned.
 * offsets: n non-infinity G2 points (what set_random_g2 supplies), 16 words each.  out_points: n x 16 words.
 * fq_jobs (may be NULL): 2n x 8 words (scalar | x) of the Legendre jobs; g2_jobs (may be NULL): n x 20 words (scalar | point)
 * of the cofactor-clearing jobs - the claimed inputs bn254s_verify needs.  fq_proofs: ceil(2n / 128) proofs, g2_proofs:
 * ceil(n / 128) proofs, each to be released with bn254s_proof_free.
 * Errors: BN254S_E_INVALID_ARG (a NULL pointer other than the job arrays, n == 0) before anything is touched.  On any other
 * error - BN254S_E_INVALID_POINT with "output equals +-offset" among them: the caller draws another offset - no proof is left
 * to the caller and every slot of fq_proofs and g2_proofs is NULL, as after the other proven calls. */
int bn254s_map_to_g2(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* u, const uint64_t* offsets, size_t n,
                     uint64_t* out_points, uint64_t* fq_jobs, uint64_t* g2_jobs, bn254s_proof** fq_proofs,
                     bn254s_proof** g2_proofs);

/* hash_to_fq2 (src/utils/hash_to_g2.rs:76-87): Poseidon challenger over `len` Goldilocks elements -> u in Fq2 (8 words), the
 * input of bn254s_map_to_g2; together they are the reference's hash_to_g2.  Host only, no context. */
int bn254s_hash_to_fq2(const uint64_t* input, size_t len, uint64_t* out /* 8 */);
/* n inputs of `len` elements each at once, on the device (inputs[n][len] -> out[n][8]); same values as n calls of the above. */
int bn254s_hash_to_fq2_batch(bn254s_ctx* ctx, const uint64_t* inputs, size_t n, size_t len, uint64_t* out);

/* g1_msm (src/utils/g1_msm.rs:22-36): the reference folds offset_0 = R (a random non-infinity point, set_random_g1),
 * offset_{i+1} = s_i x_i + offset_i with one G1 scalar-mul job per link, proves the n jobs (s_i, x_i, offset_i) in one G1
 * STARK (hook.rs:63-71) and returns msm = offset_n - R (G1Target::add: never infinity, a doubling is allowed).
 * bn254s_g1_msm_chain computes the witness chain on the device as a parallel prefix sum (products s_i x_i, a scan of the points,
 * one batched inversion; csrc/msm.hip): offsets_out[0..n] = R, R + s_0 x_0, ..., R + sum s_j x_j ((n + 1) x 8 words) and
 * result = offsets_out[n] - R (8 words).  Device front-end only, no proof.  BN254S_E_INVALID_POINT if some offset_i (i >= 1) is
 * the point at infinity (bn254s_last_error names the first such i) or if offset_n == R (the result would be infinity). */
int bn254s_g1_msm_chain(bn254s_ctx* ctx, const uint64_t* scalars /* n x 4 */, const uint64_t* x /* n x 8 */,
                        const uint64_t* offset /* R, 8 words */, size_t n, uint64_t* offsets_out, uint64_t* result /* 8 */);
/* The chain plus the proofs of its n jobs (s_i, x_i, offset_i), cut into ceil(n / per_proof) G1 proofs exactly as
 * bn254s_prove_batch cuts them (per_proof = n <= 16384: one proof, the hook's shape).  offsets_out may be NULL.  The outputs of
 * the proofs (computed by the trace generator on its own) are checked word for word against offsets_out[1..n]: a mismatch is
 * BN254S_E_INTERNAL.  On any error every proof of the call is freed and its slot in proofs is NULL.  per_proof > 16384:
 * BN254S_E_UNSUPPORTED before any device work. */
int bn254s_g1_msm(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                  const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                  bn254s_proof** proofs);
/* g2_msm: the G2 twin of g1_msm.  The reference has no g2_msm; this is the circuit of g1_msm.rs:22-36 written with its G2 gadgets
 * (set_random_g2 for R, g2_scalar_mul per link, G2Target::neg / add, curves/g2.rs:93-150): offset_0 = R (non-infinity),
 * offset_{i+1} = s_i x_i + offset_i, msm = offset_n - R.  Points are 16 words (x.c0, x.c1, y.c0, y.c1).  Scalars are used as
 * the full 256-bit values, as the G2 trace computes them: for x_i outside the r-torsion subgroup s x_i != (s mod r) x_i.
 * bn254s_g2_msm_chain (csrc/msm.hip): offsets_out[0..n] ((n + 1) x 16 words) and result = offsets_out[n] - R (16 words) on the
 * device, no proof.  BN254S_E_INVALID_POINT if some offset_i (i >= 1) is the point at infinity (bn254s_last_error names the
 * first such i) or if offset_n == R; offset_n == -R doubles. */
int bn254s_g2_msm_chain(bn254s_ctx* ctx, const uint64_t* scalars /* n x 4 */, const uint64_t* x /* n x 16 */,
                        const uint64_t* offset /* R, 16 words */, size_t n, uint64_t* offsets_out /* (n + 1) x 16 */,
                        uint64_t* result /* 16 */);
/* The chain plus the G2 proofs of its n jobs (bn254s_prove_batch, kind 1), with the same arguments, checks, linkage check and
 * error handling as bn254s_g1_msm.  per_proof > 16384 (the 2^23-row proof): BN254S_E_UNSUPPORTED before any device work. */
int bn254s_g2_msm(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                  const uint64_t* offset, size_t n, size_t per_proof, uint64_t* result, uint64_t* offsets_out,
                  bn254s_proof** proofs);

/* G1 point recovery from x: the witness side of G1Target::is_recoverable_from_x / recover_from_x (src/curves/g1.rs:76-95; native
 * form src/fields/recover.rs; is_square src/fields/fq.rs:283-295, sqrt_with_sgn src/fields/fq.rs:266-281).  For every x_i
 * (4 words, canonical: some x_i >= p is BN254S_E_INVALID_ARG, found on the host before any device work, and bn254s_last_error
 * names the first such i) the device computes g_i = x_i^3 + 3 and one exponentiation c = g_i^((p+1)/4) (csrc/root_front.hip):
 *   flags_out[i]  = 1 iff g_i is a square in Fq (g_i is never zero: -3 is not a cube modulo p);
 *   points_out[i] = (x_i, y_i) with y_i^2 = g_i, y_i < p and y_i even ("sgn false") where the flag is 1, (x_i, 0) where it is 0;
 *   fq_jobs[i]    = (p-1)/2 | g_i (8 words; may be NULL): the Fq-exp job whose output is the Legendre symbol of g_i.
 * bn254s_g1_recover_from_x_batch: device front-end only, no proof. */
int bn254s_g1_recover_from_x_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 4, canonical < p */, size_t n,
                                   uint64_t* points_out /* n x 8 */, uint8_t* flags_out /* n */,
                                   uint64_t* fq_jobs /* may be NULL: n x 8 = scalar (p-1)/2 | g */);
/* The front-end plus the Fq-exp proofs of the n Legendre jobs, cut into ceil(n / per_proof) proofs exactly as
 * bn254s_prove_batch (kind 2) cuts them.  The outputs of the proofs are checked word for word against the flags: job i must
 * give 1 where flags_out[i] is 1 and p - 1 where it is 0; a mismatch is BN254S_E_INTERNAL.  On any error every proof of the call
 * is freed and its slot in fq_proofs is NULL, and points_out, flags_out and fq_jobs are written on success only.
 * per_proof > 16384: BN254S_E_UNSUPPORTED before any device work (invalid arguments are reported first). */
int bn254s_g1_recover_from_x(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* xs, size_t n, size_t per_proof,
                             uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs /* may be NULL */,
                             bn254s_proof** fq_proofs);
/* G2 point recovery from x: the witness side of G2Target::g_circuit (src/curves/g2.rs:42-54), Fq2Target::is_square
 * (src/fields/fq2.rs:228-241) and Fq2Target::sqrt_with_sgn (fq2.rs:209-226; sign rule src/fields/sgn.rs:20-27).  For every x_i
 * (8 words: x.c0, x.c1, each canonical) and wanted sign sgns[i] (0 or 1; sgns == NULL: all 0) the device computes
 * g_i = x_i^3 + b' in Fq2 (b' = 3/(9+u), the twist coefficient), its norm N_i = g_i.c0^2 + g_i.c1^2 and the root by two
 * exponentiations with (p+1)/4 and one inversion (csrc/root_front.hip):
 *   flags_out[i]  = 1 iff g_i is a square in Fq2, that is iff N_i is a square in Fq: x_i is the x of a point ON THE TWIST CURVE.
 *                   Membership in the r-torsion subgroup is NOT checked (the reference's gadgets do not check it either):
 *                   bn254s_g2_subgroup_check does that.
 *                   g_i and N_i are never zero: the twist has odd order, so no point has y = 0;
 *   points_out[i] = (x_i, y_i) (16 words) with y_i^2 = g_i, both coordinates of y_i below p and sgn(y_i) == sgns[i] (the parity
 *                   of y.c0, or of y.c1 when y.c0 is zero) where the flag is 1, (x_i, 0) where it is 0;
 *   fq_jobs[i]    = (p-1)/2 | N_i (8 words; may be NULL): the Fq-exp job whose output is the Legendre symbol of N_i.
 * A coordinate >= p or an sgns[i] above 1 is BN254S_E_INVALID_ARG, found on the host before any device work and before any
 * output is written; bn254s_last_error names the first such i.
 * bn254s_g2_recover_from_x_batch: device front-end only, no proof. */
int bn254s_g2_recover_from_x_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 8: x.c0, x.c1, each < p */,
                                   const uint8_t* sgns /* n bytes, 0 or 1; NULL = all 0 */, size_t n,
                                   uint64_t* points_out /* n x 16 */, uint8_t* flags_out /* n */,
                                   uint64_t* fq_jobs /* may be NULL: n x 8 = (p-1)/2 | norm(g) */);
/* The front-end plus the Fq-exp proofs of the n Legendre jobs, cut into ceil(n / per_proof) proofs exactly as
 * bn254s_prove_batch (kind 2) cuts them.  The outputs of the proofs are checked word for word against the flags: job i must
 * give 1 where flags_out[i] is 1 and p - 1 where it is 0; a mismatch is BN254S_E_INTERNAL.  On any error every proof of the call
 * is freed and its slot in fq_proofs is NULL, and points_out, flags_out and fq_jobs are written on success only.
 * per_proof > 16384: BN254S_E_UNSUPPORTED before any device work (invalid arguments are reported first).  points_out is the
 * `x` argument of bn254s_g2_msm as it stands. */
int bn254s_g2_recover_from_x(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n,
                             size_t per_proof, uint64_t* points_out, uint8_t* flags_out, uint64_t* fq_jobs /* may be NULL */,
                             bn254s_proof** fq_proofs);
/* The field gadgets on their own: the witness side of FqTarget::is_square (src/fields/fq.rs:283-295), FqTarget::sqrt_with_sgn
 * (fq.rs:266-281, generator :357-365), Fq2Target::is_square (src/fields/fq2.rs:228-241), Fq2Target::sqrt_with_sgn (fq2.rs:209-226,
 * generator :305-313; sign rule src/fields/sgn.rs) and the two inv gadgets (fq.rs:241-255, fq2.rs:190-204; native inv.rs), for a
 * value that is not the g(x) of a curve (csrc/root_front.hip, the inversions csrc/field_gadgets.hip; the recovery and map calls above fuse the same arithmetic behind
 * their equations).  For every x_i (Fq: 4 words; Fq2: 8 words c0, c1; each coordinate canonical) and wanted sign sgns[i] (0 or 1;
 * sgns == NULL: all 0), exactly and with canonical outputs:
 *   square_out[i]  = the is_square gadget: 1 iff b^((p-1)/2) == 1 for b = x_i (Fq) or b = norm(x_i) = c0^2 + c1^2 (Fq2).  0 for
 *                    x_i = 0: the Legendre symbol of 0 is 0 (the norm is zero only for x_i = 0, as p = 3 mod 4);
 *   root_ok_out[i] = 1 iff a y exists with y^2 = x_i and sgn(y) == sgns[i].  For x_i != 0 that is square_out[i] (y and -y have
 *                    opposite signs, in Fq and under the Fq2 rule); for x_i = 0 it is sgns[i] == 0: the only root is 0, and a
 *                    circuit that asks for the odd root of zero has no witness;
 *   roots_out[i]   = that y where root_ok_out[i] is 1, zero words where it is 0 (the reference's generator panics there).
 *                    Fq sign: the parity of the canonical value; Fq2 sign: the parity of c0, or of c1 when c0 is zero;
 *   fq_jobs[i]     = (p-1)/2 | b (8 words; may be NULL): the Fq-exp job whose output is the Legendre symbol, as in
 *                    bn254s_g1_recover_from_x.
 * Errors, all before any device work and before anything is written: BN254S_E_INVALID_ARG for a NULL required pointer, n == 0 or
 * n >= 2^32, an sgns[i] above 1, or a coordinate >= p (bn254s_last_error names "x_<i>", for Fq2 with the coordinate c0 | c1; the
 * first such i, the coordinates before the sign).  BN254S_E_INTERNAL: a device self-check (the ladder's result squares to neither
 * x nor -x, or the root does not square back).
 * bn254s_fq_sqrt_batch, bn254s_fq2_sqrt_batch: device front-end only, no proof. */
int bn254s_fq_sqrt_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 4, canonical < p */,
                         const uint8_t* sgns /* n bytes, 0 or 1; NULL = all 0 */, size_t n, uint64_t* roots_out /* n x 4 */,
                         uint8_t* square_out /* n */, uint8_t* root_ok_out /* n */,
                         uint64_t* fq_jobs /* may be NULL: n x 8 = (p-1)/2 | x */);
int bn254s_fq2_sqrt_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 8: c0, c1, each < p */,
                          const uint8_t* sgns /* n bytes, 0 or 1; NULL = all 0 */, size_t n, uint64_t* roots_out /* n x 8 */,
                          uint8_t* square_out /* n */, uint8_t* root_ok_out /* n */,
                          uint64_t* fq_jobs /* may be NULL: n x 8 = (p-1)/2 | norm(x) */);
/* The front-end plus the Fq-exp proofs of the n Legendre jobs, cut into ceil(n / per_proof) proofs exactly as
 * bn254s_prove_batch (kind 2) cuts them.  The outputs of the proofs are checked word for word against the flags, three-valued:
 * job i must give 1 where square_out[i] is 1, p - 1 where it is 0 and the job's base is non-zero, and 0 where the base is zero; a
 * mismatch is BN254S_E_INTERNAL naming i.  On any error every proof of the call is freed, its slot in fq_proofs is NULL and no
 * output is written.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device work (invalid arguments are reported first). */
int bn254s_fq_sqrt(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n, size_t per_proof,
                   uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs /* may be NULL */,
                   bn254s_proof** fq_proofs /* ceil(n / per_proof) */);
int bn254s_fq2_sqrt(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* xs, const uint8_t* sgns, size_t n, size_t per_proof,
                    uint64_t* roots_out, uint8_t* square_out, uint8_t* root_ok_out, uint64_t* fq_jobs /* may be NULL */,
                    bn254s_proof** fq_proofs /* ceil(n / per_proof) */);
/* out[i] = x_i^-1, zero words for x_i = 0 (the gadgets' inv(0) = 0); for Fq2 the inverse is (c0, -c1) / norm(x_i).  Device only,
 * no proof (the gadgets constrain x * inv == 1 in the circuit).  Errors as above: NULL, n == 0 or n >= 2^32, a coordinate >= p. */
int bn254s_fq_inv_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 4, canonical < p */, size_t n, uint64_t* out /* n x 4 */);
int bn254s_fq2_inv_batch(bn254s_ctx* ctx, const uint64_t* xs /* n x 8: c0, c1, each < p */, size_t n, uint64_t* out /* n x 8 */);
/* G2 subgroup check: is P_i, a point of the twist curve E'(Fq2), in the r-torsion subgroup, [r] P_i = O?  The twist has the
 * cofactor 2p - r = 10069 * 5864401 * 1875725156269 * (a 178-bit prime), so bn254s_g2_recover_from_x hands out points that are
 * no group elements of G2; this is the link between it and bn254s_g2_msm.  The reference has no such gadget: it is the circuit
 * one writes with G2Target::new_checked, set_random_g2, g2_scalar_mul with the constant scalar r and connect.  Points are
 * 16 words (x.c0, x.c1, y.c0, y.c1).  The device decides [r] P_i = O with the endomorphism psi = twist^-1 o Frobenius o twist,
 * [x0 + 1]P + psi([x0]P) + psi^2([x0]P) == psi^3([2 x0]P) for the 63-bit BN parameter x0 (csrc/g2_subgroup.hip; why this holds
 * for exactly the members, on the whole of E'(Fq2): DESIGN.md "G2 subgroup check"):
 *   flags_out[i] = 1 iff [r] P_i is the point at infinity.
 * A coordinate >= p is BN254S_E_INVALID_ARG, found on the host before any device work and before any output is written;
 * bn254s_last_error names the first such i.  A point that is not on the twist curve (y^2 != x^3 + b') is BN254S_E_INVALID_ARG
 * too: it is found on the device, reported before any output is copied to the caller, bn254s_last_error names the smallest
 * such i, and no proof job is made of it (it is no valid G2Target; the trace generator never sees it).
 * bn254s_g2_subgroup_check_batch: device front-end only, no proof. */
int bn254s_g2_subgroup_check_batch(bn254s_ctx* ctx, const uint64_t* points /* n x 16, each coordinate < p */, size_t n,
                                   uint8_t* flags_out /* n */);
/* The front-end plus the G2 proofs of the n jobs (scalar r, x = P_i, offset = R_i = offsets[i]), cut into ceil(n / per_proof)
 * proofs exactly as bn254s_prove_batch (kind 1) cuts them.  The G2 trace walks all 256 bits of the scalar and starts its running
 * sum at the offset, so output i is R_i + [r] P_i: R_i exactly when P_i is a member.  The outputs of the proofs (computed bit by
 * bit by the trace generator on its own) are checked against the flags of the endomorphism front-end: output i must equal
 * offsets[i] word for word where flags_out[i] is 1 and differ from it where it is 0; a mismatch is BN254S_E_INTERNAL.
 * offsets: n x 16 words, random subgroup points as set_random_g2 draws them, every coordinate below p (else
 * BN254S_E_INVALID_ARG, as for the points).  If the running sum of a job meets the point at infinity (R_i unluckily equal to
 * -m P_i for a partial scalar m) the error is BN254S_E_INVALID_POINT, exactly as bn254s_prove_g2 reports it: draw another offset.
 * g2_jobs[i] = r | P_i (20 words; may be NULL).  flags_out and g2_jobs are written on success only.  On any error every proof
 * of the call is freed and its slot in g2_proofs is NULL.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device work
 * (invalid arguments are reported first; the context is checked last). */
int bn254s_g2_subgroup_check(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* points /* n x 16 */,
                             const uint64_t* offsets /* n x 16 */, size_t n, size_t per_proof, uint8_t* flags_out /* n */,
                             uint64_t* g2_jobs /* may be NULL: n x 20 = r | P_i */, bn254s_proof** g2_proofs);
/* G2 cofactor clearing: P_i -> [h] P_i for points of the twist curve E'(Fq2), h = 2p - r the cofactor of the r-torsion subgroup
 * (mul_by_cofactor at the end of the reference's map_to_g2, src/utils/hash_to_g2.rs:113-148; in its circuit g2_scalar_mul with the
 * constant scalar h).  It turns what bn254s_g2_recover_from_x hands out into points that bn254s_g2_subgroup_check accepts and
 * bn254s_g2_msm can fold.  Points are 16 words (x.c0, x.c1, y.c0, y.c1).  The device does not walk the 254 bits of h: with
 * psi = twist^-1 o Frobenius o twist and T = [6 x0^2] P (two chained ladders by the BN parameter, 63 and 65 bits),
 * [h] P = T + psi(T + P) - psi^2(P), exactly, on the whole of E'(Fq2) (csrc/g2_cofactor.hip; DESIGN.md "G2 cofactor clearing"):
 *   finite_out[i] = 1 iff [h] P_i is a finite point, 0 iff it is the point at infinity (the order of P_i divides h);
 *   images_out[i] = [h] P_i, affine, every coordinate below p, where finite_out[i] is 1; 16 zero words where it is 0.
 * A coordinate >= p is BN254S_E_INVALID_ARG, found on the host before any device work and before any output is written;
 * bn254s_last_error names the first such i.  A point that is not on the twist curve (y^2 != x^3 + b') is BN254S_E_INVALID_ARG
 * too: it is found on the device, reported before any output is copied to the caller, bn254s_last_error names the smallest
 * such i, and no proof job is made of it.
 * bn254s_g2_clear_cofactor_batch: device front-end only, no proof (one MI355X, copies included: 3.0 ms for 128 points,
 * 3.2 ms for 16 384, 67 ms for 2^20; profiles/g2_cofactor_times.txt). */
int bn254s_g2_clear_cofactor_batch(bn254s_ctx* ctx, const uint64_t* points /* n x 16, each coordinate < p */, size_t n,
                                   uint64_t* images_out /* n x 16 */, uint8_t* finite_out /* n */);
/* The front-end plus the G2 proofs of the n jobs (scalar h, x = P_i, offset = R_i = offsets[i]), cut into ceil(n / per_proof)
 * proofs exactly as bn254s_prove_batch (kind 1) cuts them.  Output i of the proofs is R_i + [h] P_i, computed bit by bit by the
 * trace generator on its own, and is checked against the front-end: it must equal offsets[i] word for word where finite_out[i] is
 * 0, and output i - R_i (the subtraction bn254s_map_to_g2 ends with) must equal images_out[i] word for word where it is 1; a
 * mismatch is BN254S_E_INTERNAL and bn254s_last_error names i.  Output i == +-R_i beside a finite image is
 * BN254S_E_INVALID_POINT, as bn254s_map_to_g2 reports it.  offsets: n x 16 words, random subgroup points as set_random_g2 draws
 * them, every coordinate below p (else BN254S_E_INVALID_ARG, as for the points).  If the running sum of a job meets the point at
 * infinity the error is BN254S_E_INVALID_POINT, exactly as bn254s_prove_g2 reports it: draw another offset.
 * g2_jobs[i] = h | P_i (20 words; may be NULL).  images_out, finite_out and g2_jobs are written on success only.  On any error
 * every proof of the call is freed and its slot in g2_proofs is NULL.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device
 * work (invalid arguments are reported first; the context is checked last). */
int bn254s_g2_clear_cofactor(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* points /* n x 16 */,
                             const uint64_t* offsets /* n x 16 */, size_t n, size_t per_proof, uint64_t* images_out /* n x 16 */,
                             uint8_t* finite_out /* n */, uint64_t* g2_jobs /* may be NULL: n x 20 = h | P_i */,
                             bn254s_proof** g2_proofs);
/* The reference's native map_to_g2 (src/utils/hash_to_g2.rs:113-148) for n inputs u (8 words: c0, c1, each below p) on the
 * device, no proof: the candidates of bn254s_map_to_g2, "g(x1) is a square" and "g(x2) is a square" decided from the norm's
 * exponentiation as bn254s_g2_recover_from_x decides its flag, the choice of x, y = sqrt(g(x)) with sgn(y) = sgn(u), and the
 * cofactor-clearing kernel on (x, y).  out_points (n x 16 words) are the out_points bn254s_map_to_g2 returns for the same u
 * (they do not depend on its offsets), without its 2 Fq-exp jobs and 1 G2 job per input (one MI355X: 3.9 ms against 1030 ms
 * for 4096 inputs; profiles/g2_cofactor_times.txt).
 * A coordinate of u >= p: BN254S_E_INVALID_ARG, found on the host, bn254s_last_error names the first such i.  g(x) of the chosen
 * x not a square (a device self-check): BN254S_E_INTERNAL.  An infinite image (a mapped point whose order divides h; never seen
 * in practice): BN254S_E_INVALID_POINT, bn254s_last_error names the smallest such i.  Nothing is written on an error. */
int bn254s_map_to_g2_batch(bn254s_ctx* ctx, const uint64_t* u /* n x 8, each coordinate < p */, size_t n,
                           uint64_t* out_points /* n x 16 */);
/* hash_to_g2 (src/utils/hash_to_g2.rs:40-43) for n inputs of `len` Goldilocks elements each: bn254s_hash_to_fq2_batch and then
 * bn254s_map_to_g2_batch, u staying on the device.  Errors as bn254s_map_to_g2_batch (u is below p by construction). */
int bn254s_hash_to_g2_batch(bn254s_ctx* ctx, const uint64_t* inputs /* n x len */, size_t n, size_t len,
                            uint64_t* out_points /* n x 16 */);
/* hash_to_fq: the first coordinate of hash_to_fq2 (src/utils/hash_to_g2.rs:76-87) - the same Poseidon challenger over `len`
 * Goldilocks elements, stopped after 16 challenges, whose low 32 bits are the little-endian limbs of a 512-bit integer that is
 * reduced modulo p.  out = words 0..3 of bn254s_hash_to_fq2 for every input: u in Fq (4 words), the input of bn254s_map_to_g1.
 * Host only, no context. */
int bn254s_hash_to_fq(const uint64_t* input, size_t len, uint64_t* out /* 4 */);
/* n inputs of `len` elements each at once, on the device (inputs[n][len] -> out[n][4]); same values as n calls of the above. */
int bn254s_hash_to_fq_batch(bn254s_ctx* ctx, const uint64_t* inputs, size_t n, size_t len, uint64_t* out /* n x 4 */);
/* map_to_g1: u in Fq -> a point of G1, total and of one shape for every u.  The reference has no such gadget: it is its map_to_g2
 * (src/utils/hash_to_g2.rs:113-148: Shallue-van de Woestijne, Z = 1) read over Fq on y^2 = x^3 + 3, the circuit one writes with
 * FqTarget::is_square (src/fields/fq.rs:283-295), sqrt_with_sgn (fq.rs:266-281), inv (src/fields/inv.rs: inv(0) = 0), sgn
 * (src/fields/sgn.rs:9-18: the parity of the canonical value) and G1Target::g_circuit (src/curves/g1.rs:43-51).  With
 * g(x) = x^3 + 3, nz2 = -1/2, tv4 = sqrt(-12) = (p - 12)^((p+1)/4) (ark-ff's root for p = 3 mod 4; it is even) and tv6 = -16/3:
 *   tv1 = 4 u^2;  tv2 = 1 + tv1;  tv1 = 1 - tv1;  tv3 = inv(tv1 tv2)
 *   tv5 = u tv1 tv3 tv4;  x1 = nz2 - tv5;  x2 = nz2 + tv5;  t = tv2^2 tv3;  x3 = 1 + tv6 t^2
 *   x = x1 if g(x1) is a square, else x2 if g(x2) is a square, else x3;  y = sqrt(g(x)) with the parity of u
 * G1 has the cofactor 1: nothing is cleared and no offset is needed.  For every u_i (4 words, canonical: some u_i >= p is
 * BN254S_E_INVALID_ARG, found on the host before any device work and before anything is written, and bn254s_last_error names the
 * first such i as "u_<i>") the device computes the candidates with one inversion and g(x_j)^((p+1)/4) for all three
 * (csrc/map_to_g1.hip):
 *   out_points[i]    = (x, y), 8 words, both below p, on the curve, y of the parity of u_i (y is never zero: -3 is no cube);
 *   sq_flags[2i + j] = 1 iff g(x_{j+1}) is a square in Fq, j = 0, 1 (2n bytes; may be NULL);
 *   fq_jobs[2i + j]  = (p-1)/2 | g(x_{j+1}) (8 words; may be NULL): the Fq-exp job whose output is that Legendre symbol, in the
 *                      order of bn254s_map_to_g2's fq_jobs.
 * A root that squares to neither g nor -g, or no candidate with a square g (device self-checks): BN254S_E_INTERNAL.  Nothing is
 * written on an error.  bn254s_map_to_g1_batch: device front-end only, no proof. */
int bn254s_map_to_g1_batch(bn254s_ctx* ctx, const uint64_t* u /* n x 4, canonical < p */, size_t n,
                           uint64_t* out_points /* n x 8 */, uint8_t* sq_flags /* may be NULL: 2n bytes */,
                           uint64_t* fq_jobs /* may be NULL: 2n x 8 = scalar (p-1)/2 | g(x_j) */);
/* hash_to_g1 for n inputs of `len` Goldilocks elements each: bn254s_hash_to_fq_batch and then bn254s_map_to_g1_batch, u staying
 * on the device.  Errors as bn254s_map_to_g1_batch (u is below p by construction). */
int bn254s_hash_to_g1_batch(bn254s_ctx* ctx, const uint64_t* inputs /* n x len */, size_t n, size_t len,
                            uint64_t* out_points /* n x 8 */);
/* The front-end plus the Fq-exp proofs of the 2n Legendre jobs, cut into ceil(2n / per_proof) proofs exactly as
 * bn254s_prove_batch (kind 2) cuts them.  The outputs of the proofs are checked word for word against the flags: job k must give
 * 1 where sq_flags[k] is 1 and p - 1 where it is 0; a mismatch is BN254S_E_INTERNAL.  out_points, sq_flags and fq_jobs are written
 * on success only.  On any error every proof of the call is freed and its slot in fq_proofs is NULL.  n >= 2^31 (2n must stay
 * below 2^32) is BN254S_E_INVALID_ARG; per_proof > 16384: BN254S_E_UNSUPPORTED before any device work (invalid arguments are
 * reported first; the context is checked last). */
int bn254s_map_to_g1(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* u /* n x 4 */, size_t n, size_t per_proof,
                     uint64_t* out_points /* n x 8 */, uint8_t* sq_flags /* may be NULL: 2n */,
                     uint64_t* fq_jobs /* may be NULL: 2n x 8 */, bn254s_proof** fq_proofs /* ceil(2n / per_proof) */);
/* Job outputs without a proof: what the reference's G1SingleGenerator / G2SingleGenerator / FqSingleGenerator compute with
 * arkworks, one call after the other on one host thread (src/generators/{g1,g2,fq}/single.rs:48-52), so that the rest of the
 * circuit can go on before the STARK of the same jobs is proven.  kind as in bn254s_prove_batch: 0 = G1, 1 = G2, 2 = Fq exp;
 * scalars n x 4 words, x and offset n x 8 (G1) / n x 16 (G2) words, x n x 4 words for Fq exp, whose offset is not read and may be
 * NULL (bn254s_prove_batch ignores it too).  For n independent jobs, each with its own scalar, the device computes
 *   outputs_out[i] = s_i x_i + offset_i (kinds 0, 1: affine, every coordinate below p) or x_i^s_i (kind 2; 0^0 = 1, as the trace has it);
 *   finite_out[i]  = 1, or 0 where s_i x_i + offset_i is the point at infinity: outputs_out[i] is zero words then.  Always 1 for kind 2.
 * by a fixed-window ladder over the lane's own scalar, one lane per job (csrc/job_outputs.hip; DESIGN.md "Job outputs").  The
 * scalar is used as the full 256-bit value, never reduced modulo r: on the twist s x != (s mod r) x for x outside the r-torsion
 * subgroup, and the G2 trace walks all 256 bits.  Every exceptional case of the group law is answered: s = 0 or a multiple of the
 * order of x (the output is the offset), an accumulator that meets a table entry or its negative, offset = +-[s]x.
 * BN254S_E_INVALID_ARG: a NULL argument (offset only for kinds 0, 1), n == 0, n >= UINT_MAX, a kind outside 0..2; a coordinate
 * >= p, found on the host before any device work; a point x_i or offset_i that is not on its curve, found on the device.  The last
 * two name the argument and the smallest such i in bn254s_last_error ("x_<i>", "offset_<i>") and happen before anything is written
 * to outputs_out or finite_out.
 * bn254s_job_outputs_batch: device front-end only, no proof. */
int bn254s_job_outputs_batch(bn254s_ctx* ctx, int kind, const uint64_t* scalars /* n x 4 */, const uint64_t* x,
                             const uint64_t* offset, size_t n, uint64_t* outputs_out /* n x (8 | 16 | 4) */,
                             uint8_t* finite_out /* n */);
/* The front-end followed by bn254s_prove_batch of the same jobs, cut into ceil(n / per_proof) proofs.  The outputs of the proofs
 * (bn254s_proof_outputs, computed bit by bit by the trace generator on its own), concatenated, must equal the front-end's word
 * for word: a mismatch is BN254S_E_INTERNAL and bn254s_last_error names the job.  A job whose output is the point at infinity
 * cannot be proven (the reference's targets cannot hold it): BN254S_E_INVALID_POINT naming the first such i, before any proof is
 * started.  Errors of the proofs themselves pass through unchanged - BN254S_E_INVALID_POINT where a running sum of the trace meets
 * a + (-a), which can happen for a job whose output is finite (bn254s_job_check_batch names such jobs).  outputs_out is written on success only; on any error every proof
 * of the call is freed and its slot in proofs_out is NULL.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device work
 * (invalid arguments are reported first; the context is checked last). */
int bn254s_job_outputs(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                       const uint64_t* offset, size_t n, size_t per_proof, uint64_t* outputs_out, bn254s_proof** proofs_out);
/* Job check: which curve jobs can be proven at all.  The scalar-multiplication traces add sum + double in every adding row,
 * whether or not the bit of the scalar is set, and the addition gadget cannot take opposite points: a job whose running sum meets
 * minus its doubling makes every proving entry point fail with BN254S_E_INVALID_POINT for the whole proof, without an index.
 * For a job (s, x, offset) of kind 0 (G1) or 1 (G2, on the twist), s the full 256-bit value, never reduced: dbl_0 = x,
 * sum_0 = offset, and for k = 0 .. 255
 *   step k hits iff sum_k == -dbl_k; otherwise sum_{k+1} = sum_k + dbl_k if bit k of s is set (equal points double, which can be
 *   proven), else sum_k; dbl_{k+1} = 2 dbl_k.
 * Equivalently step k hits iff offset == -[2^k + (s mod 2^k)] x.  A job is provable iff no step hits (DESIGN.md "Job check"): a
 * finite output (bn254s_job_outputs_batch) is necessary for that and not sufficient - offset = -x with s = 2 has the output x.
 *   provable_out[i] = 1 or 0;
 *   step_out[i]     = the first hitting k, which lies in row 2k of the job's 512-row frame, or BN254S_JOB_STEP_NONE.  May be NULL.
 * Unprovable jobs are a result, not an error: the call returns BN254S_OK.  Kind 2 (Fq exp) has no exceptional case: its
 * coordinates are validated, every job is provable and nothing is launched; offset is not read and may be NULL.
 * Arguments and errors are those of bn254s_job_outputs_batch with the prefix "job_check:": BN254S_E_INVALID_ARG for a NULL
 * argument (offset only for kinds 0, 1; step_out never), n == 0, n >= UINT_MAX, a kind outside 0..2; a coordinate >= p, found on
 * the host before any device work; a point x_i or offset_i that is not on its curve, found on the device, the smallest such i, x
 * before offset.  Nothing is written on an error.
 * bn254s_job_check_batch: device front-end only, no proof (csrc/job_check.hip). */
#define BN254S_JOB_STEP_NONE 0xFFFFu
int bn254s_job_check_batch(bn254s_ctx* ctx, int kind, const uint64_t* scalars /* n x 4 */, const uint64_t* x, const uint64_t* offset,
                           size_t n, uint8_t* provable_out /* n */, uint16_t* step_out /* n; may be NULL */);
/* The check followed by bn254s_prove_batch of the same jobs: if every job is provable the proofs are those of bn254s_prove_batch,
 * byte for byte.  If any job is not, BN254S_E_INVALID_POINT before any proof is started; bn254s_last_error names the smallest such
 * job and its step ("prove_batch_checked: job 77 cannot be proven: sum == -double at step 64 (row 128 of its frame)") and every
 * slot of proofs_out is NULL.  Unlike the other proven calls this one fills provable_out and step_out (n_total entries each, either
 * may be NULL) in that case as well as on success: they are the answer the caller came for.  Errors of the check (a coordinate
 * >= p, a point off its curve) leave them untouched.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device work (invalid
 * arguments are reported first; the context is checked last). */
int bn254s_prove_batch_checked(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars,
                               const uint64_t* x, const uint64_t* offset, size_t n_total, size_t per_proof,
                               uint8_t* provable_out /* may be NULL */, uint16_t* step_out /* may be NULL */,
                               bn254s_proof** proofs_out);
/* Scalar multiplication without an offset argument: products_out[i] = s_i x_i.  Every proving entry point above proves the
 * reference's statement s x + offset and leaves it to the caller to find offsets "as set_random_g1 / set_random_g2 draw them" and
 * to subtract them again (src/utils/g1_msm.rs:22-36, src/utils/hash_to_g2.rs:184-201).  This call draws the offsets, checks them
 * against the jobs, redraws the few that cannot be proven, and subtracts, all on the device (csrc/scalar_mul.hip; DESIGN.md
 * "Scalar multiplication without an offset").  kind 0 = G1, 1 = G2 (on the twist); PW = 8 | 16 words per point; scalars are the
 * full 256-bit values, never reduced.
 *   offset of job i at attempt a = 0, 1, ...: bn254s_hash_to_g1_batch | bn254s_hash_to_g2_batch of the eight Goldilocks elements
 *       seed[0], seed[1], seed[2], seed[3], i mod 2^32, i >> 32, a, 0x62736D00 + kind
 *     - a function of seed, i, a and kind alone, not of n, of the other jobs or of how the call is cut into proofs;
 *   attempts_out[i] = the smallest a < max_attempts for which (s_i, x_i, offset_i^(a)) is provable in the sense of
 *     bn254s_job_check_batch; offsets_out[i] = that offset.  If job i has no such a: BN254S_E_INVALID_POINT, and bn254s_last_error
 *     names the smallest such i with the step and row of its last attempt ("scalar_mul: job 77 cannot be proven: sum == -double at
 *     step 64 (row 128 of its frame) with the offset of attempt 3, the last of 4");
 *   outputs_out[i]  = s_i x_i + offsets_out[i]: what bn254s_proof_outputs of the proof holds; always finite;
 *   products_out[i] = outputs_out[i] - offsets_out[i] = s_i x_i, affine, every coordinate below p;
 *   finite_out[i]   = 1, or 0 with zero words in products_out[i] where s_i x_i is the point at infinity (s = 0, a multiple of the
 *     order of x, on the twist a point whose order divides s): a result, not an error.
 * The seed may be public: an x that is made to hit the offset of attempt 0 is answered with attempt 1, whose offset the same x
 * cannot also hit unless its maker solves a discrete logarithm between two hashed points.
 * BN254S_E_INVALID_ARG before any device work, nothing written: a NULL pointer (outputs_out and attempts_out may be NULL), n == 0,
 * n >= UINT_MAX, a kind outside 0..1 (Fq exp has no offset), max_attempts outside 1..8, a seed word that is not a canonical
 * Goldilocks element, a coordinate of x that is p or more (bn254s_last_error names "x_<i>", the first such i).  A point x_i off its
 * curve is found on the device before anything is written: BN254S_E_INVALID_ARG naming the smallest i.  A failed device self-check
 * (a drawn point or a product off its curve) is BN254S_E_INTERNAL.
 * bn254s_scalar_mul_batch: device front-end only, no proof. */
int bn254s_scalar_mul_batch(bn254s_ctx* ctx, int kind, const uint64_t* scalars /* n x 4 */, const uint64_t* x /* n x 8 | 16 */,
                            size_t n, const uint64_t seed[4], int max_attempts, uint64_t* products_out /* n x PW */,
                            uint8_t* finite_out /* n */, uint64_t* offsets_out /* n x PW */,
                            uint64_t* outputs_out /* may be NULL: n x PW */, uint8_t* attempts_out /* may be NULL: n */);
/* The front-end followed by bn254s_prove_batch(kind, ..., offsets_out, n, per_proof).  The concatenated outputs of the proofs must
 * equal the front-end's word for word: a mismatch is BN254S_E_INTERNAL and bn254s_last_error names the job.  scalars, x,
 * offsets_out, outputs_out and the proofs are exactly the arguments of bn254s_verify / bn254s_verify_batch.  Every output is
 * written on success only; on any error every proof of the call is freed and its slot in proofs_out is NULL.  per_proof > 16384:
 * BN254S_E_UNSUPPORTED before any device work (invalid arguments are reported first; the context is checked last). */
int bn254s_scalar_mul(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x, size_t n,
                      size_t per_proof, const uint64_t seed[4], int max_attempts, uint64_t* products_out, uint8_t* finite_out,
                      uint64_t* offsets_out, uint64_t* outputs_out, uint8_t* attempts_out,
                      bn254s_proof** proofs_out /* ceil(n / per_proof) */);
/* Many multi-scalar multiplications as one segmented chain: m MSMs, MSM j with seg_len[j] >= 1 inputs stored one after the other,
 * n = sum seg_len[j] inputs in all (csrc/msm.hip; DESIGN.md "Many MSMs in one chain").  The reference puts the links of every
 * g1_msm of a circuit into one STARK (src/hook.rs:63-71); bn254s_g1_msm / bn254s_g2_msm take one MSM per call, bring one random
 * point R per call and fail as a whole where a partial sum is infinity.  kind 0 = G1, 1 = G2 (on the twist); PW = 8 | 16 words
 * per point; scalars are the full 256-bit values, never reduced.  For input i, the t-th of MSM j, with T_{j,t} the sum of s x over
 * the first t inputs of MSM j (without R; it may be the point at infinity):
 *   offsets_out[i] = R_j + T_{j,t}      (R_j itself for t = 0)
 *   outputs_out[i] = R_j + T_{j,t+1}    (the offset of the next link)
 *   results_out[j] = T_{j,seg_len[j]}, affine, taken from the scan and not from outputs - R: it does not depend on R_j and is
 *     returned for every MSM, provable or not;
 *   finite_out[j]  = 1, or 0 with zero words in results_out[j] where the MSM is the point at infinity: a result, not an error.
 * MSM j is provable under R_j iff every link (s_i, x_i, offsets_out[i]) is provable in the sense of bn254s_job_check_batch (an
 * infinite output implies that its link hits at the top set bit of s_i, so the first bad link is always a hit on a finite offset):
 *   bad_link_out[j] = the smallest local t whose link hits, or BN254S_MSM_LINK_NONE; bad_step_out[j] = its step, or
 *     BN254S_JOB_STEP_NONE.  The rows of a bad MSM in offsets_out and outputs_out are zero words.
 * Where R comes from:
 *   R != NULL: m caller-supplied points, one attempt; seed and max_attempts are not read, attempts_out[j] = 0;
 *   R == NULL: R_j at attempt a = bn254s_hash_to_g1_batch | bn254s_hash_to_g2_batch of the eight Goldilocks elements
 *       seed[0], seed[1], seed[2], seed[3], j mod 2^32, j >> 32, a, 0x626D6D00 + kind
 *     - a function of seed, j, a and kind alone; attempts_out[j] = the smallest a < max_attempts (1..8) under which MSM j is
 *     provable, R_out[j] = that point.  An MSM with no such attempt keeps the bad_link / bad_step (and the point in R_out) of its
 *     last attempt, and attempts_out[j] = max_attempts.  On G2 a drawn point whose cleared image is infinity counts as a failed
 *     attempt (link 0, no step).
 * bn254s_msm_multi_chain: device front-end only, no proof.  Unprovable MSMs are a result: it returns BN254S_OK.
 * BN254S_E_INVALID_ARG before any device work, nothing written: a NULL pointer (R_out, attempts_out and bad_step_out may be NULL;
 * R or seed, not both), m == 0, some seg_len[j] == 0, sum seg_len != n, n >= UINT_MAX, a kind outside 0..1, drawn offsets with
 * max_attempts outside 1..8 or a seed word that is not a canonical Goldilocks element, a coordinate of x or R that is p or more
 * (bn254s_last_error names "x_<i>" / "R_<j>").  A point x_i or R_j off its curve is found on the device before anything is
 * written: BN254S_E_INVALID_ARG naming the smallest index, x before R.  A failed device self-check is BN254S_E_INTERNAL. */
#define BN254S_MSM_LINK_NONE 0xFFFFFFFFu
int bn254s_msm_multi_chain(bn254s_ctx* ctx, int kind, const uint64_t* scalars /* n x 4 */, const uint64_t* x /* n x PW */,
                           const size_t* seg_len /* m */, size_t m, size_t n, const uint64_t* R /* m x PW or NULL */,
                           const uint64_t* seed /* 4, read when R == NULL */, int max_attempts, uint64_t* results_out /* m x PW */,
                           uint8_t* finite_out /* m */, uint64_t* offsets_out /* n x PW */, uint64_t* outputs_out /* n x PW */,
                           uint64_t* R_out /* may be NULL: m x PW */, uint8_t* attempts_out /* may be NULL: m */,
                           uint32_t* bad_link_out /* m */, uint16_t* bad_step_out /* may be NULL: m */);
/* The front-end followed by bn254s_prove_batch(kind, scalars, x, offsets_out, n, per_proof): the n links are cut by per_proof
 * regardless of MSM boundaries, as the hook does.  The concatenated outputs of the proofs must equal outputs_out word for word: a
 * mismatch is BN254S_E_INTERNAL and bn254s_last_error names the job.  If any MSM is unprovable: BN254S_E_INVALID_POINT before any
 * proof, naming the smallest such MSM ("msm_multi: msm 3 cannot be proven: link 17, sum == -double at step 64 (row 128 of its
 * frame) with the offset of attempt 3, the last of 4"; "... with the supplied offset" for R != NULL).  Every output is written on
 * success only; on any error every slot in proofs_out is NULL.  per_proof > 16384: BN254S_E_UNSUPPORTED before any device work
 * (invalid arguments are reported first; the context is checked last). */
int bn254s_msm_multi(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* scalars, const uint64_t* x,
                     const size_t* seg_len, size_t m, size_t n, const uint64_t* R, const uint64_t* seed, int max_attempts,
                     size_t per_proof, uint64_t* results_out, uint8_t* finite_out, uint64_t* offsets_out, uint64_t* outputs_out,
                     uint64_t* R_out, uint8_t* attempts_out, uint32_t* bad_link_out, uint16_t* bad_step_out,
                     bn254s_proof** proofs_out /* ceil(n / per_proof) */);
/* Statement verifiers (csrc/point_sum.hip; DESIGN.md "Statement verifiers").  The proofs of bn254s_scalar_mul and bn254s_msm_multi
 * carry the reference's statement output_i = s_i x_i + offset_i.  What their caller wants to know, products[i] == s_i x_i or
 * results[j] == the sum of s x over MSM j, follows from the proofs only together with the linkage between the arrays:
 * product + offset == output, the offset chain inside an MSM, result + R == the last output.  The linkage is curve arithmetic and
 * is checked on the device; the proofs go through bn254s_verify_batch.
 *
 * bn254s_point_sum_check_batch: for each of n relations, is c_i == a_i + b_i?  kind 0 = G1, 1 = G2 (on the twist); PW = 8 | 16
 * words per point.  a_i may be the point at infinity (a_finite[i] == 0 and zero words); b_i and c_i are affine points.
 * code_out[i] is the first of these that applies: */
enum {
  BN254S_SUM_OK = 0,           /* the relation holds */
  BN254S_SUM_A_NOT_ZERO = 1,   /* a_finite[i] == 0 but a word of a_i is non-zero */
  BN254S_SUM_A_OFF_CURVE = 2,  /* a_finite[i] != 0 and a_i is not on its curve */
  BN254S_SUM_B_OFF_CURVE = 3,  /* b_i is not on its curve */
  BN254S_SUM_C_OFF_CURVE = 4,  /* c_i is not on its curve */
  BN254S_SUM_INFINITE = 5,     /* a_i == -b_i: the sum is O, which an affine c_i cannot state */
  BN254S_SUM_X = 6,            /* the x coordinate of a_i + b_i is not that of c_i */
  BN254S_SUM_Y = 7,            /* x agrees and y does not, i.e. c_i == -(a_i + b_i) */
  /* link codes of the two verifiers below only */
  BN254S_SUM_X_OFF_CURVE = 8,  /* an input point x of the job / of the MSM is not on its curve */
  BN254S_SUM_HEAD = 9,         /* msm_multi: the offset of the first link of the MSM is not R_j, word for word */
  BN254S_SUM_CHAIN = 10        /* msm_multi: offsets[i + 1] != outputs[i] inside the MSM, word for word */
};
/* The kernel takes no inversion: with d = x_b - x_a, e = y_b - y_a (d = 2 y_a, e = 3 x_a^2 where a_i == b_i) the relation holds
 * exactly when x_c d^2 == e^2 - (x_a + x_b) d^2 and (y_c + y_a) d == e (x_a - x_c); where a_i is O it is c_i == b_i, x compared
 * first.  A failing relation is a result, not an error: the call returns BN254S_OK.
 * BN254S_E_INVALID_ARG, nothing written: a NULL pointer, n == 0, n >= UINT_MAX, a kind outside 0..1; a coordinate of a_i (rows
 * with a_finite[i] != 0 only: the others are code 1 unless all zero), b_i or c_i that is p or more, found on the host before any
 * device work - bn254s_last_error names "a_<i>" / "b_<i>" / "c_<i>".  All work runs on the context's stream. */
int bn254s_point_sum_check_batch(bn254s_ctx* ctx, int kind /* 0 = G1, 1 = G2 on the twist */, const uint64_t* a /* n x PW */,
                                 const uint8_t* a_finite /* n */, const uint64_t* b /* n x PW */, const uint64_t* c /* n x PW */,
                                 size_t n, uint8_t* code_out /* n */);
/* bn254s_verify_scalar_mul: the statement products[i] == s_i x_i of a bn254s_scalar_mul call, from the arrays it returned and
 * the words of its proofs.  Proof k holds jobs k per_proof .. min(n, (k + 1) per_proof) - 1, as bn254s_prove_batch cuts them;
 * words[k], n_words[k] and degree_bits[k] are per proof (the last proof of a call can be lower than the others), and
 * bn254s_verify_batch is called once per run of consecutive proofs of equal (degree_bits, n_words).  Accepted iff
 *   every x_i is on its curve                                                   (link_out[i] = BN254S_SUM_X_OFF_CURVE otherwise),
 *   products[i] (with finite[i]) + offsets[i] == outputs[i] for every job       (link_out[i] = the code 1..7 of the relation),
 *   every proof is accepted for its jobs (s_i, x_i, offsets[i], outputs[i])     (proof_status[k] as bn254s_verify_batch gives it).
 * bn254s_verify_msm_multi: the statement results[j] == the sum of s x over MSM j of a bn254s_msm_multi call.  Per MSM j with
 * first input f_j and last input l_j, link_out[j] is the first failing check in this order:
 *   every x of the MSM is on its curve                                          (BN254S_SUM_X_OFF_CURVE),
 *   offsets[f_j] == R_j word for word                                           (BN254S_SUM_HEAD),
 *   offsets[i + 1] == outputs[i] word for word for f_j <= i < l_j               (BN254S_SUM_CHAIN),
 *   results[j] (with finite[j]) + R_j == outputs[l_j]                           (the code 1..7 of the relation),
 * and every proof must be accepted for its jobs (s_i, x_i, offsets[i], outputs[i]).
 * Where the offsets or the R come from (seed, attempts) is deliberately NOT checked: that s x + offset == output is proven for
 * the offset at hand, and subtracting that same offset gives s x whatever point it is.  Drawing the offsets again would double the
 * device work and verify nothing about the statement.
 * Returns BN254S_OK: everything above holds.  BN254S_E_VERIFY: something does not; link_out and proof_status (either may be
 * NULL) are filled for every entry - the linkage and the proofs are both always evaluated, a failing link does not stop the
 * proofs - and bn254s_last_error names the first linkage failure with its index ("verify_scalar_mul: job 64: products + offsets
 * != outputs (x)", "verify_msm_multi: msm 3: offsets[40] != outputs[39] (link 7 -> 8)") or, where the linkage is whole,
 * "proof k: <text of bn254s_verify_batch>" for the lowest rejected proof k of the call.  BN254S_E_INVALID_ARG before any device work, nothing written:
 * a NULL pointer other than the two optional outputs, n == 0, m == 0, per_proof == 0, n_proofs != ceil(n / per_proof), some
 * seg_len[j] == 0, sum seg_len != n, a kind outside 0..1, a params->struct_size mismatch, a coordinate of any point array that
 * is p or more (rows of products / results with finite == 0 excepted), naming the array and the index; no context (checked
 * last).  BN254S_E_HIP / BN254S_E_OOM pass through.  Anything other than BN254S_OK is not an acceptance. */
int bn254s_verify_scalar_mul(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* const* words,
                             const size_t* n_words, const uint32_t* degree_bits, size_t n_proofs, size_t per_proof,
                             const uint64_t* scalars, const uint64_t* x, size_t n, const uint64_t* products, const uint8_t* finite,
                             const uint64_t* offsets, const uint64_t* outputs, uint8_t* link_out /* n, may be NULL */,
                             int32_t* proof_status /* n_proofs, may be NULL */);
int bn254s_verify_msm_multi(bn254s_ctx* ctx, int kind, const bn254s_params* params, const uint64_t* const* words,
                            const size_t* n_words, const uint32_t* degree_bits, size_t n_proofs, size_t per_proof,
                            const uint64_t* scalars, const uint64_t* x, const size_t* seg_len, size_t m, size_t n, const uint64_t* R,
                            const uint64_t* results, const uint8_t* finite, const uint64_t* offsets, const uint64_t* outputs,
                            uint8_t* link_out /* m, may be NULL */, int32_t* proof_status /* n_proofs, may be NULL */);
/* Root statement verifiers (csrc/root_links.hip; DESIGN.md "Root statement verifiers").  The Fq-exp proofs of
 * bn254s_g1_recover_from_x, bn254s_g2_recover_from_x, bn254s_fq_sqrt, bn254s_fq2_sqrt and bn254s_map_to_g1 say
 * base^((p-1)/2) == output and nothing else.  What their caller wants to know - flags[i] says whether g(x_i) is a square and
 * points[i] is the root with the wanted sign; points[i] is the map_to_g1 image of u_i - follows from the proofs only with the
 * linkage: the base of job i is what the front-end says it is, the proven symbol matches the flag, the root squares back and has
 * the right sign, the flags select the point's x.  The field part is checked on the device; the proofs go through
 * bn254s_verify_batch against jobs that the verifier computes itself.
 *
 * bn254s_root_links_check_batch: `what` names the front-end whose arrays are checked:
 *   what  input `in`        `out`                base of the job(s)                    radicand
 *   0     x_i, 4 words      points, n x 8        g = x^3 + 3                           g             (G1 recover; the root is even)
 *   1     x_i, 8 words      points, n x 16       norm(g), g = x^3 + b' in Fq2          g             (G2 recover; sgns)
 *   2     x_i, 4 words      roots, n x 4         x_i                                   x_i           (Fq sqrt; sgns, root_ok)
 *   3     x_i, 8 words      roots, n x 8         norm(x_i)                             x_i           (Fq2 sqrt; sgns, root_ok)
 *   4     u_i, 4 words      points, n x 8        g(x1), g(x2) of the SvdW candidates:  g of the candidate that the two flags
 *                                                jobs and flags 2i, 2i + 1             select: x1 if sq_flags[2i], else x2 if
 *                                                                                      sq_flags[2i + 1], else x3; sign = parity of u_i
 * code_out[i] is the first of these that applies: */
enum {
  BN254S_ROOT_OK = 0,          /* every check below passes */
  BN254S_ROOT_JOB_SCALAR = 1,  /* fq_jobs given and the scalar words of a job of input i are not (p-1)/2 (what 4: of job 2i or 2i + 1) */
  BN254S_ROOT_JOB_BASE = 2,    /* fq_jobs given and the base words of a job of input i are not the base computed here, word for word */
  BN254S_ROOT_FLAG = 3,        /* a flag byte (flags, root_ok) or sgns[i] above 1; what 2, 3: square[i] set on a zero base, or
                                  root_ok[i] != (base != 0 ? square[i] : sgns[i] == 0) */
  BN254S_ROOT_CARRY = 4,       /* what 0, 1: the x words of points[i] are not x_i; what 4: not the candidate that the flags select */
  BN254S_ROOT_NOT_ZERO = 5,    /* no root is claimed (what 0, 1: flag clear; 2, 3: root_ok clear) and the y / root words are not
                                  all zero; never for what 4 */
  BN254S_ROOT_SQUARE = 6,      /* a root is claimed and y^2 != radicand (in Fq2 for what 1, 3); for what 4 this is also "both flags
                                  clear and g(x3) has no such root" */
  BN254S_ROOT_SIGN = 7         /* y squares back but has the other sign: Fq the parity of the canonical value, Fq2 the parity of
                                  c0, or of c1 when c0 is zero */
};
/* The kernel has no ladder and no exponentiation: a root is checked, never computed; what 4 takes the one inversion of the map.
 * bases_out (may be NULL) receives the canonical base words, n x 4 (2n x 4 for what 4), whatever the codes are.  fq_jobs (may be
 * NULL: codes 1 and 2 do not occur) is n x 8 (2n x 8): scalar | base.  sgns NULL = all 0; not read for what 0, 4.  root_ok is
 * read for what 2, 3 only.  flags is n bytes, 2n for what 4.  A failing relation is a result, not an error: the call returns
 * BN254S_OK.  BN254S_E_INVALID_ARG, nothing written, before any device work: a NULL required pointer, n == 0, n >= UINT_MAX
 * (n >= 2^31 for what 4), a what outside 0..4, a coordinate of `in` that is p or more, a coordinate that is p or more in the y /
 * root of a row whose root is claimed (what 0, 1: flags[i] != 0; 2, 3: root_ok[i] != 0; 4: every row) - bn254s_last_error names
 * it, "root_links_check: x_<i> is not below p" / "... x_<i> has c1 not below p", "... points_<i> has y.c0 not below p"; no
 * context (checked last).  Rows that are never read as a field element - the y of a clear flag, the root of a clear root_ok, the x of a point -
 * are compared only and not range-checked. */
int bn254s_root_links_check_batch(bn254s_ctx* ctx, int what, const uint64_t* in, const uint8_t* sgns /* NULL = all 0 */, size_t n,
                                  const uint64_t* out /* points or roots */, const uint8_t* flags /* n; 2n for what 4 */,
                                  const uint8_t* root_ok /* what 2, 3 only */, const uint64_t* fq_jobs /* may be NULL */,
                                  uint8_t* code_out /* n */, uint64_t* bases_out /* may be NULL */);
/* The five verifiers: the statement of a call of the front-end of the same name, from the arrays it returned and the words of
 * its Fq-exp proofs; words, n_words, degree_bits, n_proofs, per_proof as for bn254s_verify_scalar_mul, with n jobs (2n for
 * map_to_g1: n_proofs == ceil(2n / per_proof)).  Each runs the link check once and hands bn254s_verify_batch (kind 2, once per
 * run of consecutive proofs of equal (degree_bits, n_words)) jobs of its own making: the scalar (p-1)/2, the base from the device
 * and the output that the flag demands - 0 for a zero base (what 2, 3 only; a set flag there is code 3), else 1 where the flag
 * is set and p - 1 where it is clear.  So an accepted proof proves the flag; fq_jobs is only compared, may be NULL, and the
 * outputs of the proofs are not an argument.  Accepted iff every link_out[i] is BN254S_ROOT_OK and every proof is accepted.
 * Returns BN254S_OK, or BN254S_E_VERIFY with link_out and proof_status (either may be NULL) filled for every entry - both are
 * always evaluated - and bn254s_last_error naming the smallest failing input ("verify_g1_recover: input 7: y of the point does
 * not square to x^3 + 3"; a job code names the job, for map_to_g1 with its candidate) or, where the linkage is whole,
 * "proof k: <text of bn254s_verify_batch>" for the lowest rejected proof k.  BN254S_E_INVALID_ARG as for
 * bn254s_root_links_check_batch and bn254s_verify_scalar_mul (per_proof == 0, a wrong n_proofs, a NULL words[k], a
 * params->struct_size mismatch), the text with the verifier's name as its tag; the context is checked last.  Other codes of the
 * device pass through.  Anything other than BN254S_OK is not an acceptance. */
int bn254s_verify_g1_recover(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                             const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs, size_t n,
                             const uint64_t* points, const uint8_t* flags, const uint64_t* fq_jobs /* may be NULL */,
                             uint8_t* link_out /* n, may be NULL */, int32_t* proof_status /* n_proofs, may be NULL */);
int bn254s_verify_g2_recover(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                             const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                             const uint8_t* sgns /* NULL = all 0 */, size_t n, const uint64_t* points, const uint8_t* flags,
                             const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status);
int bn254s_verify_fq_sqrt(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                          const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                          const uint8_t* sgns /* NULL = all 0 */, size_t n, const uint64_t* roots, const uint8_t* square,
                          const uint8_t* root_ok, const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status);
int bn254s_verify_fq2_sqrt(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                           const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* xs,
                           const uint8_t* sgns /* NULL = all 0 */, size_t n, const uint64_t* roots, const uint8_t* square,
                           const uint8_t* root_ok, const uint64_t* fq_jobs, uint8_t* link_out, int32_t* proof_status);
int bn254s_verify_map_to_g1(bn254s_ctx* ctx, const bn254s_params* params, const uint64_t* const* words, const size_t* n_words,
                            const uint32_t* degree_bits, size_t n_proofs, size_t per_proof, const uint64_t* u, size_t n,
                            const uint64_t* points, const uint8_t* sq_flags /* 2n */, const uint64_t* fq_jobs /* 2n x 8, may be NULL */,
                            uint8_t* link_out /* n */, int32_t* proof_status);
/* ---- kernel-level entry points (parity tests and bench.py's roofline leg) ------------------------------ */
/* PolynomialBatch::from_values on host column-major values[C][2^16]: outputs (any may be NULL)
 * coeffs[C][N], lde[C][2N] in Merkle-leaf (bit-reversed) order, cap[16*4]. */
int bn254s_commit_values(bn254s_ctx* ctx, const uint64_t* values, size_t ncols, uint64_t* coeffs, uint64_t* lde,
                         uint64_t* cap);
/* Times `iters` runs of the NTT/LDE stage (iNTT + both coset NTTs) on ncols resident columns of 2^16
 * synthetic values; returns average milliseconds per run through *ms (HIP events on the kernels' stream). */
int bn254s_bench_ntt(bn254s_ctx* ctx, size_t ncols, int iters, float* ms);
/* The same, and the shader clock (MHz) the GPU held while the stage ran: mean over the timed iterations and the slowest ~10 us
 * interval (one extra wave samples the core-clock counter against the constant 100 MHz counter). */
int bn254s_bench_ntt_clock(bn254s_ctx* ctx, size_t ncols, int iters, float* ms, float* mhz, float* mhz_min);
/* Issue cost of the half-rate vector instruction class (64-bit adds / shifts / compares, v_mad_u64_u32, carry instructions) with
 * eight waves per SIMD: nanoseconds per wave-instruction and SIMD, and the shader clock held during the measurement. */
int bn254s_bench_issue(bn254s_ctx* ctx, float* ns_per_issue, float* mhz);
/* PMC calibration: `iters` plain copies of `words` u64 with 8-byte-per-lane loads/stores (known traffic). */
int bn254s_bench_copy(bn254s_ctx* ctx, size_t words, int iters);
/* Times the Merkle leaf-hash kernel alone: ncols columns x 2^log_leaves rows of synthetic data, ms per run. */
int bn254s_bench_leafhash(bn254s_ctx* ctx, size_t ncols, int log_leaves, int iters, float* ms);
/* Poseidon permutation of `n` 12-word states in place (host buffer). */
int bn254s_poseidon_permute(bn254s_ctx* ctx, uint64_t* states, size_t n);
/* debug: the hand-written Goldilocks sequences of the NTT kernels (csrc/gl_asm.h) on n operand pairs; out[n][17] =
 * a+b, a-b, b-a, a*b, a*2^{12,24,32,36,48,60,64,1,31}, a*2^-{12,24,1,31} (all mod p) */
int bn254s_selftest_field(bn254s_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* Debug: one implementation of the Poseidon permutation on `n` 12-word states in place (host buffer).  variant 0: the
 * hand-scheduled statement (the kernel of bn254s_poseidon_permute), 1: the compiler's code (poseidon_permute_plain), 2: the
 * cooperative code, 16 lanes per state (poseidon_permute_coop).  Other variants: BN254S_E_INVALID_ARG. */
int bn254s_selftest_poseidon(bn254s_ctx* ctx, int variant, uint64_t* states, size_t n);
/* Debug: the leaf-hash kernels on caller data.  data: column-major [ncols][2^log_leaves] (host), digests: 2^log_leaves x 4 words
 * (host).  kernel 0: what merkle_leaves picks in latency mode (any ncols >= 1: leaves of <= 4 elements are copied); 1: k_leaf_hash
 * (ncols > 4, at least 256 leaves); 2: k_leaf_hash_coop (ncols > 4, 2^log_leaves * ceil(ncols / 8) <= 65536, the shapes the
 * latency mode gives it); 3: k_leaf_absorb, fed chunk_cols columns per call (a positive multiple of 8; ncols > 4) with the sponge
 * states carried between calls as the streaming prover does.  chunk_cols is ignored by kernels 0..2.  Shapes a kernel never sees
 * in the prover are not launched: BN254S_E_INVALID_ARG. */
int bn254s_selftest_leaf_hash(bn254s_ctx* ctx, const uint64_t* data, size_t ncols, int log_leaves, int kernel, int chunk_cols,
                              uint64_t* digests);
/* Debug: BN254 Fq inversion as trace generation uses it (ark-ff `inverse()` at add.rs:66,80): x[n][4] canonical little-endian
 * words -> out[n][8] = x^-1 mod p twice, by the divstep inversion of the product path and by Fermat's little theorem. */
int bn254s_selftest_fq_inv(bn254s_ctx* ctx, const uint64_t* x, size_t n, uint64_t* out);
/* Debug: the BN254 Fq / Fq2 device arithmetic (csrc/fq_dev.h) and the cooperative pieces of the doubling chains
 * (csrc/chain_coop.h) on RAW register contents, one GPU lane per row.  An operand is four little-endian words of an integer below
 * p that is loaded as it is (the registers hold Montgomery residues x 2^260 mod p: no conversion is made, the caller chooses the
 * limbs the multiplier sees); a result is the raw residue, four words, canonical if the code is right.  With Ri = 2^-260 mod p a
 * product form returns formula * Ri mod p and a linear form formula mod p.  in[n][W_in], out[n][W_out] words by group:
 *  0 (16 -> 68)  a b c d -> a+b, a-b, -a, 2a, ab, a^2, ab+cd, fq_from_canonical(a) = a 2^260, fq_to_canonical(a) = a Ri, then the
 *                loose forms (a+b)^2, (3a)^2, (3a)b, (a+b)(c-d+2p), (a+b+c+d)(a+b-c-d+4p), (3a+3b)(3a-3b+6p), (3a)b+(3c)(2p-d),
 *                (3a)(3b)+(3c)(6p-3d)
 *  1 (16 -> 60)  x = (a, b) != 0, y = (c, d) -> fq2_mul(x, y), fq2_mul(3x loose, y), fq2_sqr<2>(x), fq2_sqr<4>(x + y lazy),
 *                fq2_sqr<6>(3x lazy) (two results each), fq2_norm(x), fq2_neg(x) (two), fq2_inv(x) (two)
 *  2 (32 -> 92)  e0 .. e7, stored in LDS slots -> g1coop::product(e0, e1; e2, e3) at the five (fa, ga, fb, gb) of the G1 chain
 *                (1,0,1,0) (2,0,1,0) (1,1,1,1) (3,0,3,0) (3,0,1,0); g2coop::product of the Fq2 slots (e0,e1) (e2,e3); (e4,e5) (e6,e7)
 *                at the same five tuples, each as c = 0, c = 1 and plain; chain_coop::combine of e0 .. e3 with the coefficient
 *                sets (1,4,4,-4; 4 p), (-1,-6,-6,6; 13 p) and (1,-8,0,0; 8 p)
 *  3 (72 -> 74)  Jacobian G1 P, Q (X Y Z each) and G2 P, Q (X.c0 X.c1 Y.c0 Y.c1 Z.c0 Z.c1 each) -> g1_double(P), g1_add(P, Q),
 *                g2_double(P), g2_add(P, Q) as raw X Y Z, then the return codes of g1_add and g2_add (one word each)
 * BN254S_E_INVALID_ARG: a NULL argument, an unknown group, an operand of p or more, x = 0 in group 1, a Z = 0 in group 3
 * (the curve code has no point at infinity); nothing is launched then. */
int bn254s_selftest_fq(bn254s_ctx* ctx, int group, const uint64_t* in, size_t n, uint64_t* out);
/* Debug: the LogUp range-check columns (csrc/aux.hip) of a caller's trace, through the same code the provers run.  trace:
 * column-major [ncols][rows] canonical words (host), rows a power of two in 64 .. 2^20; the n_rc columns from rc_begin on are the
 * range-checked ones, table_col / freq_col the table and its multiplicities; betas: the two challenges (canonical).  With
 * m = ceil(n_rc / 2), out[2 (m + 1)][rows] = per challenge the helper columns h_k = 1/(beta + f_2k) + 1/(beta + f_2k+1) (the
 * last of an odd n_rc has one term) and then Z: Z_0 = 0, Z_{i+1} = Z_i + sum_k h_k(i) - freq(i) / (beta + table(i)).
 * BN254S_E_INVALID_ARG: a NULL argument, a shape outside the above, a word of p or more (nothing is launched then).
 * BN254S_E_INTERNAL: a range-checked or table value above 65535 (found on the device; `out` is not meaningful then). */
int bn254s_selftest_logup(bn254s_ctx* ctx, const uint64_t* trace, size_t rows, int ncols, int rc_begin, int n_rc, int table_col,
                          int freq_col, const uint64_t betas[2], uint64_t* out);
/* Debug: the openings / FRI kernels (csrc/fri.hip) and the un-reduced accumulators of csrc/quotient_common.h on caller data,
 * through the launchers the provers run (csrc/fri_selftest.hip).  All buffers are host memory; every field word must be canonical
 * (below p = 2^64 - 2^32 + 1) and an extension element is two words (c0, c1).  BN254S_E_INVALID_ARG: a NULL argument, a size
 * outside what is stated below, a word of p or more; nothing is launched then.
 *
 * bn254s_selftest_acc: values[rows][T], weights[T] -> out[rows][2] = sum_t values[r][t] weights[t] mod p by Acc (acc_mad / acc_red)
 *   and by Acc3 (acc3_mad on the 22-bit limbs / acc3_red), one accumulator of each kind and one GPU lane per row.
 *   1 <= T <= 2^17 (the documented capacity of Acc3), 1 <= rows <= 4096.
 * bn254s_selftest_openings: coeffs[npolys][N], N = 2^(16 + log_r) in the transposed layout of the provers (coefficient
 *   k1 + R k2 at position k1 2^16 + k2, R = 2^log_r), 0 <= log_r <= 2, 1 <= npolys <= 64 -> out[npolys][R][5] = the partial
 *   evaluations {S_k1(zeta^R).c0, .c1, S_k1(zeta_next^R).c0, .c1, sum of the block's coefficients} as the device writes them
 *   (fri_opening_tables, fri_openings); P(z) = sum_k1 z^k1 S_k1(z^R).
 * bn254s_selftest_fri_combine, for a synthetic shape of trace width W (1 .. 4096), n_rc range-checked columns (1 .. W) and n_ctl
 *   cross-table lookups (0 or 2), i.e. A = 2 (ceil(n_rc / 2) + 1) + 2 n_ctl auxiliary columns of which the last 2 n_ctl are the Z's:
 *   mode 0 (fri_combine_coeffs): cols[W + A + 4][n] = trace | auxiliary | quotient columns, 1 <= n <= 2^16 (any n: stride and
 *     bound), aux_in = W + A + 4 weights as extension elements, points unused (may be NULL) -> out = comb[6][n]: rows 0,1 =
 *     sum over trace and auxiliary columns, rows 2,3 = sum over the quotient columns, rows 4,5 = sum over the Z columns with the
 *     FIRST 2 n_ctl weights (components c0 / c1 each).
 *   mode 1 (fri_combine_final): cols = cl[6][n], 1 <= n <= 2^20, aux_in = xs[n], points[12] = zeta, zeta_next, r0, r1, r2, alpha
 *     -> out[n][2] = alpha^(W + A + 2 n_ctl) (f0 - r0) / (x - zeta) + alpha^(2 n_ctl) (f1 - r1) / (x - zeta_next) + (f2 - r2) / (x - 1)
 *     with f1 = (cl0, cl1), f0 = f1 + (cl2, cl3), f2 = (cl4, cl5) and 1 / 0 := 0.
 * bn254s_selftest_fri_fold: in[2^log_m][2] extension values in bit-reversed order on shift <w_(2^log_m)>, 5 <= log_m <= 20, shift
 *   != 0 -> out[2^(log_m - 4)][2], the arity-16 fold at beta (fri_fold with inv16 = 1 / 16).
 * bn254s_selftest_fri_rows: lde[ncols][2^(log_n + 1)] (leaf order: coset h at h 2^log_n + bitrev(k)), 1 <= log_n <= 20, 1 <= ncols <=
 *   4096 -> window[ncols][rows] = rows k0 .. k0 + rows - 1 (mod 2^log_n) of coset h in {0, 1} (fri_extract_window; k0 < 2^log_n,
 *   1 <= rows <= 2^20) and gathered[ncols][nq] = lde[c][indices[q]] (fri_gather_rows; 1 <= nq <= 4096, indices < 2^(log_n + 1)). */
int bn254s_selftest_acc(bn254s_ctx* ctx, const uint64_t* values, const uint64_t* weights, size_t T, size_t rows, uint64_t* out);
int bn254s_selftest_openings(bn254s_ctx* ctx, const uint64_t* coeffs, int npolys, int log_r, const uint64_t zeta[2],
                             const uint64_t zeta_next[2], uint64_t* out);
int bn254s_selftest_fri_combine(bn254s_ctx* ctx, int mode, int W, int n_rc, int n_ctl, size_t n, const uint64_t* cols,
                                const uint64_t* aux_in, const uint64_t* points, uint64_t* out);
int bn254s_selftest_fri_fold(bn254s_ctx* ctx, const uint64_t* in, int log_m, uint64_t shift, const uint64_t beta[2], uint64_t* out);
int bn254s_selftest_fri_rows(bn254s_ctx* ctx, const uint64_t* lde, int ncols, int log_n, int h, size_t k0, size_t rows,
                             const uint32_t* indices, int nq, uint64_t* window, uint64_t* gathered);
/* Debug: the quotient (AIR constraint) kernels and the auxiliary columns of one STARK kind on caller data, through what the provers
 * and bn254s_verify run (csrc/quotient_selftest.hip).  kind: 0 = G1, 1 = G2, 2 = Fq exp, with that kind's real shape: trace width
 * W = 781 / 1295 / 427, A = 456 / 906 / 134 auxiliary columns (per challenge the LogUp helpers and Z, then the four CTL Z's),
 * K = 1573 / 2605 / 910 constraints in emission order (AIR, lookups, CTLs).  All buffers are host memory; every field word must be
 * canonical.  BN254S_E_INVALID_ARG: a NULL argument, a size or combination outside what is stated below, a word of p or more;
 * nothing is launched then.
 *
 * bn254s_selftest_quotient builds the alpha tables (quotient_host_tables), fills the kernel arguments (quotient_fill_args, and
 *   quotient_window_args in window mode) and calls the kind's quotient_launch: the part kernels, then k_quotient_finish.
 *   N = 2^log_n.  flags: BN254S_QS_WINDOW, BN254S_QS_RAW (or 0).
 *   Whole domain (no BN254S_QS_WINDOW; 3 <= log_n <= 12; h, k0, count, stride ignored: count = stride = 2 N): trace[W][2 N] and
 *     aux[A][2 N] in leaf order (point g w_2N^(2 k + h) at h N + bitrev(k)); the next row of a point is row k + 1 (mod N) of its coset.
 *   Window (3 <= log_n <= 20): trace[W][stride], aux[A][stride] hold the rows k0 .. k0 + count of coset h in {0, 1} in natural
 *     order (count + 1 rows: the last serves the transition constraints of the one before); 1 <= count, k0 + count <= N,
 *     count + 1 <= stride <= 8192.  The points evaluated are the first `count`.
 *   x / lfirst / llast: all NULL = the library's tables (quotient_point_tables / quotient_point_tables_window); otherwise three
 *     arrays of `count` words each (whole domain: 2 N, leaf order): x_j, L_first(x_j), L_last(x_j) as the kernels are to see them.
 *   BN254S_QS_RAW: zh_inv = {1, 1} and w_inv = 0 as bn254s_verify sets them: no division by Z_H, and the transition selector
 *     z_last is the table value x_j itself.  Otherwise z_last = x_j - w_N^-1 and the sums are multiplied by 1 / Z_H of the coset.
 *   out[2 alphas][2 cosets][N] (natural order on each coset) and part[7][2 alphas][stride] (the partial sums of part kernel p at
 *     [p][alpha][j], j as in trace; G1 writes parts 0..5, G2 0..6, Fq 0..1) are IN/OUT: they are uploaded as the caller filled
 *     them, so a word that no lane writes comes back unchanged.
 * bn254s_selftest_point_tables: out[3][n] = x, L_first, L_last as quotient_point_tables (window = 0: n = 2 N, leaf order; h, k0,
 *   count ignored) or quotient_point_tables_window (window = 1: n = count rows from k0 (mod N) of coset h; k0 < N, 1 <= count <= N)
 *   write them; 3 <= log_n <= 20.
 * bn254s_selftest_aux: trace[W][rows] (rows a power of two in 64 .. 2^16) -> out[A][rows], all auxiliary columns through aux_build
 *   with the kind's shape: per challenge the helpers and Z, then the CTL Z's in (ctl, challenge) order.  Returns the device error
 *   word: BN254S_E_INTERNAL for a range-checked or table value above 65535 or a CTL filter value other than 0 and 1 (`out` is not
 *   meaningful then). */
#define BN254S_QS_WINDOW 1
#define BN254S_QS_RAW 2
#define BN254S_QS_MAX_PARTS 7
int bn254s_selftest_quotient(bn254s_ctx* ctx, int kind, int log_n, int flags, int h, size_t k0, size_t count, size_t stride,
                             const uint64_t* trace, const uint64_t* aux, const uint64_t alphas[2], const uint64_t betas[2],
                             const uint64_t gammas[2], const uint64_t* x, const uint64_t* lfirst, const uint64_t* llast, uint64_t* out,
                             uint64_t* part);
int bn254s_selftest_point_tables(bn254s_ctx* ctx, int log_n, int window, int h, size_t k0, size_t count, uint64_t* out);
int bn254s_selftest_aux(bn254s_ctx* ctx, int kind, const uint64_t* trace, size_t rows, const uint64_t betas[2], const uint64_t gammas[2],
                        uint64_t* out);
/* Debug: the NTT / LDE stage at every supported height on caller data (csrc/ntt_selftest.hip).  All buffers are host memory and
 * every word must be canonical.  BN254S_E_INVALID_ARG: a NULL argument, a size or combination outside what is stated below, a word
 * of p or more; nothing is launched then.
 *
 * bn254s_selftest_transforms runs the transform dispatch of the provers (csrc/transforms.h) with the plan of a proof of 2^log_n
 *   rows, 16 <= log_n <= 23, on ncols columns (1 .. 64).  flags: bit 0 = the radix-2 split level above the tall transforms
 *   (18 <= log_n <= 23; log_n = 23 exists only with it), bit 1 = the compact workspace (column chunks of 16; log_n >= 17).
 *   N = 2^log_n.  Coefficients are in the STORED layout of that plan: natural order at 2^16 rows; tall (R = N / 2^16 > 1):
 *   coefficient k1 + R k2 at position k1 2^16 + k2; split: a column is [Pe | Po], the even and the odd coefficients, each in the
 *   tall layout of N / 2 words.  An LDE column is 2 N words in leaf order: coset h (shift g w_2N^h) at h N + bitrev(k).
 *     op 0  commit_ntt: in = values[ncols][N] -> out0 = coeffs[ncols][N], out1 = lde[ncols][2 N]
 *     op 1  lde: in = coeffs[ncols][N] -> out0 = lde[ncols][2 N] (out1 unused, as for ops 2 and 3); with the compact flag and
 *           without the split level ncols <= 16: lde does not work in chunks there and the plan's scratch holds one chunk
 *     op 2  lde_chunk of the streaming workspace (log_n >= 17, ncols <= 16): as op 1 for the cosets of coset_mask (1, 2 or 3: bit h =
 *           coset h); the output is filled with the word 2^64 - 1 first, a half that the mask leaves out keeps it
 *     op 3  quotient_coset_inverse (ncols = 4): in = qv[2][2][N], values of polynomial a on coset h in natural order at [a][h]
 *           -> out0 = ab[2][2][N], their interpolants' coefficients
 *   coset_mask is ignored by the other ops.  The transforms run on the context's stream WITHOUT the section that keeps the NTT
 *   stages of proofs in flight apart, and in scratch of the context: do not call it while proofs run on the same context.
 * bn254s_selftest_mul_2exp: x[n], 1 <= n <= 2^20 -> out[n][64], out[i][e] = x[i] 2^(3 e) mod p by the shift table of the outer
 *   passes (mul_2exp3, every e a compile-time constant as in the R-point DFT).
 * bn254s_selftest_outer_dft: in[n][R], R = 2^log_r, 1 <= log_r <= 6, 1 <= n <= 2^16, inverse in {0, 1} -> out[n][R] = the registers
 *   of dft_small<log_r, inverse> on each row in register order: register r holds X[bitrev(r)], X[k] = sum_i x[i] w^(i k) with
 *   w = 2^(192 / R) (inverse: its inverse; no factor 1 / R). */
int bn254s_selftest_transforms(bn254s_ctx* ctx, int op, int log_n, int flags, int ncols, int coset_mask, const uint64_t* in,
                               uint64_t* out0, uint64_t* out1);
int bn254s_selftest_mul_2exp(bn254s_ctx* ctx, const uint64_t* x, size_t n, uint64_t* out);
int bn254s_selftest_outer_dft(bn254s_ctx* ctx, int log_r, int inverse, const uint64_t* in, size_t n, uint64_t* out);
/* Debug: the parts of bn254s_verify_batch on caller data (csrc/verify_batch.hip, csrc/verify_query.h).
 * The FRONT RECORD of a proof is BN254S_VERIFY_RECORD_HEAD + num_queries words: fri_alpha (2 words: c0, c1), reduced[3] (6),
 * alpha_len[3] (6), zeta (2), g zeta (2), fri_betas[8] (16, zero past the last layer), then the query indices.
 * The CODE of a query is the first failing check in the verifier's order (L = FRI layers): 0 pass; 1, 2, 3 Merkle path of the
 * trace / auxiliary / quotient tree; 4 + 2l consistency at layer l; 5 + 2l Merkle path of layer l; 4 + 2L final polynomial.
 * bn254s_selftest_verify_front: host only.  Runs the front of one proof, writes its record (record_cap words available; too few:
 *   BN254S_E_INVALID_ARG) and returns the front's status (BN254S_OK, BN254S_E_VERIFY, ...); the record is complete only on BN254S_OK.
 * bn254s_selftest_query_round: the query rounds of n_proofs proofs on the caller's records (records[n_proofs][record words]) ->
 *   codes_out[n_proofs][num_queries], every code and not only the first.  ctx = NULL: on the host.  chunk_proofs: proofs per upload
 *   (0 = by size, 256 MiB).  BN254S_E_INVALID_ARG: a NULL argument, n_words that is not the size of such a proof, a record word of
 *   p or more, a query index of 2^(degree_bits + rate_bits) or more; nothing is launched then.
 * bn254s_selftest_query_text: the reference verifier's error text of a code for a proof of n_layers FRI layers ("" for 0; NULL for
 *   a code or a layer count that does not exist): the text bn254s_verify_batch reports for a proof whose first failing query has it.
 * bn254s_selftest_verify_batch_ms: the times of the context's latest bn254s_verify_batch in ms: front (wall), upload, k_vb_merkle,
 *   k_vb_fri (device events), CTL (wall). */
#define BN254S_VERIFY_RECORD_HEAD 34
int bn254s_selftest_verify_front(int kind, const bn254s_params* params, uint32_t degree_bits, const uint64_t* words, size_t n_words,
                                 uint64_t* record_out, size_t record_cap);
int bn254s_selftest_query_round(bn254s_ctx* ctx, int kind, const bn254s_params* params, uint32_t degree_bits,
                                const uint64_t* const* words, size_t n_words, const uint64_t* records, size_t n_proofs,
                                size_t chunk_proofs, int32_t* codes_out);
const char* bn254s_selftest_query_text(int n_layers, int code);
int bn254s_selftest_verify_batch_ms(bn254s_ctx* ctx, float ms_out[5]);
/* Debug: the plan of one proof - what the prover decides before it touches memory, the workspace layout above all - for a proof of n
 * instances of `kind` on a device with dev_total_bytes of memory (0 = unknown: the streaming workspace is then never chosen on
 * account of the size).  Host arithmetic only: no context, no GPU.  force_split / force_lowmem / force_stream / stream_win_log stand
 * for BN254S_FORCE_SPLIT / _FORCE_LOWMEM / _FORCE_STREAM / BN254S_STREAM_WIN_LOG, which the provers read per call (0 = off;
 * stream_win_log < 0 = not set).  out[BN254S_PLAN_WORDS]:
 *   0 kind  1 n  2 W (trace width)  3 A (auxiliary width)  4 constraints  5 words per point  6 N (rows)  7 log_n
 *   8 log_s (1: a radix-2 level above the tall transforms)  9 log_r  10 R = 2^log_r  11 NH = N >> log_s  12 NSPL = 1 << log_s
 *   13 stream  14 lowmem (compact or streaming workspace)  15 log_bk  16 BK = 2^log_bk rows per quotient window  17 BK + 1
 *   18 L (FRI layers)  19..26 their arity bits (0 past L)  27 proof words per query  28 words of a commitment tree
 *   29 words of the FRI layer values  30 words of the FRI trees  31 words of the job arrays
 *   32..52 words of the named workspace buffers in, tvals, tcoef, hist, tmp, ldechunk, sponge, comb, tlde, trees, avals, acoef, alde,
 *          scratch, quot, tabs, open, fri, fritrees, qout, win (0: no buffer of that name - it aliases another one or is not needed)
 *   53 bytes of pinned host staging
 * BN254S_E_UNSUPPORTED with the provers' message in err (NUL-terminated, at most err_len bytes; may be NULL): an unsupported height
 * or StarkConfig.  BN254S_E_INVALID_ARG: kind outside 0..2, n = 0, NULL params / out or a params->struct_size mismatch. */
#define BN254S_PLAN_WORDS 54
int bn254s_selftest_proof_plan(int kind, size_t n, const bn254s_params* params, uint64_t dev_total_bytes, int force_split,
                               int force_lowmem, int force_stream, int stream_win_log, uint64_t* out, char* err, size_t err_len);
/* Trace generation only: column-major trace[W][rows] copied to the host buffer.
 * kind: 0 = G1 scalar mul (W 781), 1 = G2 scalar mul (W 1295), 2 = Fq exp (W 427; offset ignored). */
int bn254s_generate_trace(bn254s_ctx* ctx, int kind, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset,
                          size_t n, uint32_t min_rows_log2, uint64_t* trace_out, uint64_t* outputs);
int bn254s_g1_generate_trace(bn254s_ctx* ctx, const uint64_t* scalars, const uint64_t* x, const uint64_t* offset,
                             size_t n, uint32_t min_rows_log2, uint64_t* trace_out, uint64_t* outputs);

#ifdef __cplusplus
}
#endif
#endif /* BN254_STARK_H */
