//! FFI declarations of `include/bn254_stark.h` (ABI version 1) - one `extern "C"` item per C function, same order.
//! Source only: never compiled in this repository (rust/README.md).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int};

/// `bn254s_params`: StarkConfig::standard_fast_config() + min_rows (reference stark_proof.rs:152-154).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct Bn254sParams {
    pub struct_size: u32,
    pub security_bits: u32,
    pub num_challenges: u32,
    pub rate_bits: u32,
    pub cap_height: u32,
    pub pow_bits: u32,
    pub arity_bits: u32,
    pub final_poly_bits: u32,
    pub num_queries: u32,
    pub min_rows_log2: u32,
}
#[repr(C)]
pub struct Bn254sCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct Bn254sProof {
    _p: [u8; 0],
}
#[repr(C)]
pub struct Bn254sBatch {
    _p: [u8; 0],
}

pub const BN254S_OK: c_int = 0;
pub const BN254S_E_INVALID_POINT: c_int = -4;
pub const BN254S_E_VERIFY: c_int = -8;
/// `kind` argument of the generic entry points.
pub const KIND_G1: c_int = 0;
pub const KIND_G2: c_int = 1;
pub const KIND_FQ_EXP: c_int = 2;
/// `id` argument of `bn254s_proof_section`.
pub const SEC_TRACE_CAP: c_int = 0;
pub const SEC_AUX_CAP: c_int = 1;
pub const SEC_QUOTIENT_CAP: c_int = 2;
pub const SEC_LOCAL_VALUES: c_int = 3;
pub const SEC_NEXT_VALUES: c_int = 4;
pub const SEC_AUX_POLYS: c_int = 5;
pub const SEC_AUX_POLYS_NEXT: c_int = 6;
pub const SEC_CTL_ZS_FIRST: c_int = 7;
pub const SEC_QUOTIENT_POLYS: c_int = 8;
pub const SEC_FRI_CAPS: c_int = 9;
pub const SEC_QUERY_ROUNDS: c_int = 10;
pub const SEC_FINAL_POLY: c_int = 11;
pub const SEC_POW_WITNESS: c_int = 12;
pub const SEC_INIT_CHALLENGER_STATE: c_int = 13;

extern "C" {
    pub fn bn254s_params_default(p: *mut Bn254sParams);
    pub fn bn254s_abi_version() -> c_int;
    pub fn bn254s_ctx_create(device_id: c_int, out: *mut *mut Bn254sCtx) -> c_int;
    pub fn bn254s_ctx_destroy(ctx: *mut Bn254sCtx);
    pub fn bn254s_last_error(ctx: *const Bn254sCtx) -> *const c_char;
    pub fn bn254s_prove_g1(ctx: *mut Bn254sCtx, params: *const Bn254sParams, scalars: *const u64, x: *const u64,
                           offset: *const u64, n: usize, out: *mut *mut Bn254sProof) -> c_int;
    pub fn bn254s_prove_g2(ctx: *mut Bn254sCtx, params: *const Bn254sParams, scalars: *const u64, x: *const u64,
                           offset: *const u64, n: usize, out: *mut *mut Bn254sProof) -> c_int;
    pub fn bn254s_prove_fq_exp(ctx: *mut Bn254sCtx, params: *const Bn254sParams, scalars: *const u64, x: *const u64,
                               n: usize, out: *mut *mut Bn254sProof) -> c_int;
    /// idle slots give their (grow-only) device workspaces back to the driver
    pub fn bn254s_ctx_trim(ctx: *mut Bn254sCtx) -> c_int;
    /// hash_to_fq2 of n messages of `len` Goldilocks elements each, on the device: out[n][8]
    pub fn bn254s_hash_to_fq2_batch(ctx: *mut Bn254sCtx, inputs: *const u64, n: usize, len: usize, out: *mut u64) -> c_int;
    pub fn bn254s_prove_batch(ctx: *mut Bn254sCtx, kind: c_int, params: *const Bn254sParams, scalars: *const u64,
                              x: *const u64, offset: *const u64, n_total: usize, per_proof: usize,
                              proofs: *mut *mut Bn254sProof) -> c_int;
    /// queues the batch on the context's worker pool and returns; `bn254s_prove_batch_end` waits for it.  Inputs and
    /// `proofs_out` must outlive the handle.  Other proving calls made meanwhile queue behind it (never share a slot).
    pub fn bn254s_prove_batch_begin(ctx: *mut Bn254sCtx, kind: c_int, params: *const Bn254sParams, scalars: *const u64,
                                    x: *const u64, offset: *const u64, n_total: usize, per_proof: usize,
                                    proofs_out: *mut *mut Bn254sProof, handle: *mut *mut Bn254sBatch) -> c_int;
    pub fn bn254s_prove_batch_end(handle: *mut Bn254sBatch) -> c_int;
    /// one context per GPU, proof i on context i mod n_ctx
    pub fn bn254s_prove_batch_multi(ctxs: *mut *mut Bn254sCtx, n_ctx: usize, kind: c_int, params: *const Bn254sParams,
                                    scalars: *const u64, x: *const u64, offset: *const u64, n_total: usize,
                                    per_proof: usize, proofs: *mut *mut Bn254sProof) -> c_int;
    pub fn bn254s_proof_words(p: *const Bn254sProof, data: *mut *const u64, len: *mut usize) -> c_int;
    pub fn bn254s_proof_section(p: *const Bn254sProof, id: c_int, data: *mut *const u64, len: *mut usize) -> c_int;
    pub fn bn254s_proof_degree_bits(p: *const Bn254sProof) -> c_int;
    pub fn bn254s_proof_outputs(p: *const Bn254sProof, data: *mut *const u64, len: *mut usize) -> c_int;
    pub fn bn254s_proof_serialize(p: *const Bn254sProof, buf: *mut u8, cap: usize) -> usize;
    pub fn bn254s_proof_free(p: *mut Bn254sProof);
    /// what set_ctl_values_target consumes (scalar_mul_ctl.rs:57-80 and twins)
    pub fn bn254s_ctl_values(kind: c_int, scalars: *const u64, x: *const u64, offset: *const u64, outputs: *const u64,
                             n: usize, in_rows: *mut u64, out_rows: *mut u64) -> c_int;
    /// 0, or BN254S_E_VERIFY with the reference verifier's error text in bn254s_last_error
    pub fn bn254s_verify(ctx: *mut Bn254sCtx, kind: c_int, params: *const Bn254sParams, degree_bits: u32,
                         words: *const u64, n_words: usize, scalars: *const u64, x: *const u64, offset: *const u64,
                         outputs: *const u64, n: usize) -> c_int;
    pub fn bn254s_map_to_g2(ctx: *mut Bn254sCtx, params: *const Bn254sParams, u: *const u64, offsets: *const u64, n: usize,
                            out_points: *mut u64, fq_jobs: *mut u64, g2_jobs: *mut u64, fq_proofs: *mut *mut Bn254sProof,
                            g2_proofs: *mut *mut Bn254sProof) -> c_int;
    /// g1_msm (src/utils/g1_msm.rs:22-36): offsets_out[0..=n] = R, R + s_0 x_0, ..., ((n + 1) x 8 words), result = offsets_out[n] - R
    pub fn bn254s_g1_msm_chain(ctx: *mut Bn254sCtx, scalars: *const u64, x: *const u64, offset: *const u64, n: usize,
                               offsets_out: *mut u64, result: *mut u64) -> c_int;
    /// the chain plus ceil(n / per_proof) G1 proofs of its jobs (s_i, x_i, offset_i); offsets_out may be null
    pub fn bn254s_g1_msm(ctx: *mut Bn254sCtx, params: *const Bn254sParams, scalars: *const u64, x: *const u64, offset: *const u64,
                         n: usize, per_proof: usize, result: *mut u64, offsets_out: *mut u64, proofs: *mut *mut Bn254sProof) -> c_int;
    /// g2_msm (the g1_msm circuit with the G2 gadgets): offsets_out[0..=n] = R, R + s_0 x_0, ... ((n + 1) x 16 words, unreduced
    /// 256-bit scalars), result = offsets_out[n] - R
    pub fn bn254s_g2_msm_chain(ctx: *mut Bn254sCtx, scalars: *const u64, x: *const u64, offset: *const u64, n: usize,
                               offsets_out: *mut u64, result: *mut u64) -> c_int;
    /// the chain plus ceil(n / per_proof) G2 proofs of its jobs (s_i, x_i, offset_i); offsets_out may be null
    pub fn bn254s_g2_msm(ctx: *mut Bn254sCtx, params: *const Bn254sParams, scalars: *const u64, x: *const u64, offset: *const u64,
                         n: usize, per_proof: usize, result: *mut u64, offsets_out: *mut u64, proofs: *mut *mut Bn254sProof) -> c_int;
    pub fn bn254s_hash_to_fq2(input: *const u64, len: usize, out: *mut u64) -> c_int;
    /// hash_to_fq: the first coordinate of hash_to_fq2 (out: 4 words); host only
    pub fn bn254s_hash_to_fq(input: *const u64, len: usize, out: *mut u64) -> c_int;
    /// map_to_g1 of n inputs u (4 words each, below p) on the device, no proof: out_points n x 8 words; sq_flags (2n bytes) and
    /// fq_jobs (2n x 8 words: (p-1)/2 | g(x_j)) may be null
    pub fn bn254s_map_to_g1_batch(ctx: *mut Bn254sCtx, u: *const u64, n: usize, out_points: *mut u64, sq_flags: *mut u8,
                                  fq_jobs: *mut u64) -> c_int;
    /// the front-end plus ceil(2n / per_proof) Fq-exp proofs of the Legendre jobs, their outputs checked against the flags
    pub fn bn254s_map_to_g1(ctx: *mut Bn254sCtx, params: *const Bn254sParams, u: *const u64, n: usize, per_proof: usize,
                            out_points: *mut u64, sq_flags: *mut u8, fq_jobs: *mut u64, fq_proofs: *mut *mut Bn254sProof) -> c_int;
    /// the outputs s_i x_i + offset_i (kind 0 = G1, 1 = G2) or x_i^s_i (kind 2, offset unused) of n jobs on the device, no proof:
    /// what the SingleGenerators compute (src/generators/{g1,g2,fq}/single.rs:48-52).  outputs_out: n x (8 | 16 | 4) words, zeros
    /// where finite_out[i] is 0 (the output is the point at infinity)
    pub fn bn254s_job_outputs_batch(ctx: *mut Bn254sCtx, kind: c_int, scalars: *const u64, x: *const u64, offset: *const u64,
                                    n: usize, outputs_out: *mut u64, finite_out: *mut u8) -> c_int;
    /// the front-end plus ceil(n / per_proof) proofs of the same jobs (bn254s_prove_batch), their outputs checked word for word
    pub fn bn254s_job_outputs(ctx: *mut Bn254sCtx, kind: c_int, params: *const Bn254sParams, scalars: *const u64, x: *const u64,
                              offset: *const u64, n: usize, per_proof: usize, outputs_out: *mut u64,
                              proofs_out: *mut *mut Bn254sProof) -> c_int;
    /// which of n curve jobs (kind 0 = G1, 1 = G2) can be proven, on the device, no proof: provable_out[i] = 0 where the running
    /// sum of the trace meets minus its doubling, step_out[i] (may be null) the first such step k (row 2k of the job's frame) or
    /// BN254S_JOB_STEP_NONE = 0xFFFF.  Unprovable jobs are a result, not an error.  Every job of kind 2 is provable
    pub fn bn254s_job_check_batch(ctx: *mut Bn254sCtx, kind: c_int, scalars: *const u64, x: *const u64, offset: *const u64,
                                  n: usize, provable_out: *mut u8, step_out: *mut u16) -> c_int;
    /// the check, then bn254s_prove_batch of the same jobs if every one is provable; otherwise BN254S_E_INVALID_POINT before any
    /// proof, with provable_out and step_out (either may be null) filled all the same
    pub fn bn254s_prove_batch_checked(ctx: *mut Bn254sCtx, kind: c_int, params: *const Bn254sParams, scalars: *const u64,
                                      x: *const u64, offset: *const u64, n_total: usize, per_proof: usize, provable_out: *mut u8,
                                      step_out: *mut u16, proofs_out: *mut *mut Bn254sProof) -> c_int;
    /// is_square and sqrt_with_sgn of n Fq elements (4 words each, below p; sgns: n bytes 0 | 1, null = all 0) on the device, no
    /// proof: square_out[i] = 1 iff x_i^((p-1)/2) == 1 (0 for x_i = 0), root_ok_out[i] = 1 iff a root with the wanted parity exists,
    /// roots_out[i] that root or zeros; fq_jobs (n x 8 words: (p-1)/2 | x_i) may be null
    pub fn bn254s_fq_sqrt_batch(ctx: *mut Bn254sCtx, xs: *const u64, sgns: *const u8, n: usize, roots_out: *mut u64,
                                square_out: *mut u8, root_ok_out: *mut u8, fq_jobs: *mut u64) -> c_int;
    /// the same for Fq2 (8 words: c0, c1): the Legendre symbol of norm(x_i) (fq_jobs: (p-1)/2 | norm(x_i)); sign: the parity of c0,
    /// or of c1 when c0 is zero
    pub fn bn254s_fq2_sqrt_batch(ctx: *mut Bn254sCtx, xs: *const u64, sgns: *const u8, n: usize, roots_out: *mut u64,
                                 square_out: *mut u8, root_ok_out: *mut u8, fq_jobs: *mut u64) -> c_int;
    /// the front-end plus ceil(n / per_proof) Fq-exp proofs of the Legendre jobs, their outputs checked against the flags: 1 for a
    /// square, p - 1 for a non-square, 0 for a zero base
    pub fn bn254s_fq_sqrt(ctx: *mut Bn254sCtx, params: *const Bn254sParams, xs: *const u64, sgns: *const u8, n: usize,
                          per_proof: usize, roots_out: *mut u64, square_out: *mut u8, root_ok_out: *mut u8, fq_jobs: *mut u64,
                          fq_proofs: *mut *mut Bn254sProof) -> c_int;
    pub fn bn254s_fq2_sqrt(ctx: *mut Bn254sCtx, params: *const Bn254sParams, xs: *const u64, sgns: *const u8, n: usize,
                           per_proof: usize, roots_out: *mut u64, square_out: *mut u8, root_ok_out: *mut u8, fq_jobs: *mut u64,
                           fq_proofs: *mut *mut Bn254sProof) -> c_int;
    /// x_i^-1 of n Fq (4 words) or Fq2 (8 words) elements on the device, zeros for x_i = 0
    pub fn bn254s_fq_inv_batch(ctx: *mut Bn254sCtx, xs: *const u64, n: usize, out: *mut u64) -> c_int;
    pub fn bn254s_fq2_inv_batch(ctx: *mut Bn254sCtx, xs: *const u64, n: usize, out: *mut u64) -> c_int;
}
