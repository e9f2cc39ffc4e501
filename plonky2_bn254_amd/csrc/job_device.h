// The device halves of the proof-free front-ends for callers whose jobs are on the device already (scalar_mul.hip, msm.hip and the
// rounds they share, offset_draw.h), as
// g2_cofactor.h does it for cofactor clearing: each launches its kernels on the context's stream and returns without waiting.
// All counts are below UINT_MAX; every pointer is device memory.
#pragma once
#include "ctx.h"

// k_job_check<G1 | G2> (job_check.hip), kind 0 | 1: d_step n half-words, the first hitting step or BN254S_JOB_STEP_NONE; a job
// whose x (offset) is off its curve writes no step and lowers d_bad[0] (d_bad[1]), preset to UINT_MAX, to its index.
int bn254s_job_check_device(bn254s_ctx* c, int kind, const u64* d_scalars, const u64* d_x, const u64* d_offset, size_t n,
                            unsigned short* d_step, unsigned* d_bad);

// k_job_outputs<G1 | G2 | FqExp> (job_outputs.hip): d_out n x PW canonical words (zeros where the output is O), d_finite n bytes;
// d_bad as above, and such a job writes nothing.
int bn254s_job_outputs_device(bn254s_ctx* c, int kind, const u64* d_scalars, const u64* d_x, const u64* d_offset, size_t n, u64* d_out,
                              unsigned char* d_finite, unsigned* d_bad);

// hash_to_g1 (map_to_g1.hip: k_hash_to_fq, k_m2g1_point) and hash_to_g2 (map_to_g2.hip: k_hash_to_fq2, k_m2g_point,
// k_g2_clear_cofactor) of n inputs of len Goldilocks elements each, d_in n x len, in a workspace of bn254s_hash_to_g{1,2}_device_words(n)
// words.  Where the results lie in the workspace comes back in `at`; the self-check words are cleared by the call itself.
struct HashedPoints {
  const u64* points;            // n x 8 | 16 canonical words
  const int* err;               // non-zero: a root did not square back, or no candidate had a square g(x) (BN254S_E_INTERNAL)
  const unsigned* bad;          // G2 only (else nullptr): below UINT_MAX where a mapped point is off the twist curve
  const unsigned char* finite;  // G2 only (else nullptr): n bytes, 0 where the cleared image is the point at infinity
};
size_t bn254s_hash_to_g1_device_words(size_t n);
size_t bn254s_hash_to_g2_device_words(size_t n);
int bn254s_hash_to_g1_device(bn254s_ctx* c, const u64* d_in, size_t n, size_t len, u64* d_work, HashedPoints* at);
int bn254s_hash_to_g2_device(bn254s_ctx* c, const u64* d_in, size_t n, size_t len, u64* d_work, HashedPoints* at);
