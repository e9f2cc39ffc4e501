// The draw-and-repair rounds of the front-ends that draw their own offsets (scalar_mul.hip: one per job; msm.hip: one per MSM):
//   item i at attempt a draws  hash_to_g1 | hash_to_g2 (seed[0..3], i mod 2^32, i >> 32, a, domain + kind)
// Rounds, one per attempt, over a list of items (round 0: all of them; later: the items just rejected, a handful at most):
//   k_draw_inputs    the eight hash inputs of every listed item
//   [hash_to_g1 / hash_to_g2 of the inputs: map_to_g1.hip, map_to_g2.hip through job_device.h]
//   body             the caller's kernels: they mark every item that cannot keep its point in rejected[] and count them
//   -> the 32 control words go to the host; the rounds end when nothing was rejected or no attempt is left, otherwise
//   k_draw_compact   the list of the marked items, their attempt raised by one
// What happens to items that are still rejected after the last attempt is the caller's business.
#pragma once
#include <climits>
#include <string>
#include "ctx.h"
#include "gl_dev.h"  // GL_P
#include "job_device.h"

namespace {

constexpr int DRAW_MAX_ATTEMPTS = 8;

// The control words: 32 u32, cleared before round 0 but for the four bad words, which start at UINT_MAX (draw_ctl_clear).
enum { CTL_COUNT = 0 /* [8]: items rejected in round r */, CTL_ERR = 8, CTL_BAD = 10 /* [2]: x, offset off the curve */,
       CTL_CHK_BAD = 12 /* [2]: msm.hip: what k_job_check says of x and of the offsets */,
       CTL_LIST = 16 /* [8]: length of the list built after round r */, CTL_WORDS = 32 };
enum { CTL_ERR_DRAW = 1 /* self-check of the hash-to-curve kernels; a caller's own codes follow */ };

struct DrawSeed {
  u64 w[4];
};

// four Goldilocks elements in canonical form
inline bool seed_canonical(const uint64_t* seed) {
  for (int w = 0; w < 4; w++)
    if (seed[w] >= GL_P) return false;
  return true;
}

// in: cnt x 8 Goldilocks elements; list: the cnt listed items, or nullptr for items 0 .. cnt - 1
__global__ __launch_bounds__(256) void k_draw_inputs(DrawSeed seed, u64 domain, const unsigned* __restrict__ list,
                                                     const unsigned char* __restrict__ attempts, size_t cnt, u64* __restrict__ in) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= cnt) return;
  const u64 i = list ? list[k] : k;
  u64* o = in + 8 * k;
#pragma unroll
  for (int w = 0; w < 4; w++) o[w] = seed.w[w];
  o[4] = i & 0xFFFFFFFFu;
  o[5] = i >> 32;
  o[6] = attempts[i];
  o[7] = domain;
}

// list: the marked items (in no particular order: everything an item gets depends on its own index alone), *len their number
__global__ __launch_bounds__(256) void k_draw_compact(const unsigned char* __restrict__ rejected, size_t cnt,
                                                      unsigned char* __restrict__ attempts, unsigned* __restrict__ list,
                                                      unsigned* __restrict__ len) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt || !rejected[i]) return;
  attempts[i]++;
  list[atomicAdd(len, 1u)] = (unsigned)i;
}

// what the hash-to-curve kernels say of themselves, for the one lane of a caller's kernel that reads it
__device__ __forceinline__ void draw_self_check(const HashedPoints& at, unsigned* ctl) {
  if (*at.err != 0 || (at.bad && *at.bad != UINT_MAX)) atomicCAS(ctl + CTL_ERR, 0u, (unsigned)CTL_ERR_DRAW);
}

inline size_t draw_device_words(int kind, size_t n) {
  return kind == 0 ? bn254s_hash_to_g1_device_words(n) : bn254s_hash_to_g2_device_words(n);
}
inline int draw_points(bn254s_ctx* c, int kind, const u64* d_in, size_t n, u64* d_work, HashedPoints* at) {
  return kind == 0 ? bn254s_hash_to_g1_device(c, d_in, n, 8, d_work, at) : bn254s_hash_to_g2_device(c, d_in, n, 8, d_work, at);
}

inline int draw_ctl_clear(bn254s_ctx* c, unsigned* d_ctl) {
  HIP_TRY(c, hipMemsetAsync(d_ctl, 0, CTL_WORDS * 4, c->stream));
  HIP_TRY(c, hipMemsetAsync(d_ctl + CTL_BAD, 0xFF, 16, c->stream));  // bad and chk_bad
  return BN254S_OK;
}

// the caller's device memory: in n x 8 words, hash draw_device_words(kind, n) words, attempts and rejected n bytes (cleared),
// list n words, ctl CTL_WORDS words (draw_ctl_clear)
struct DrawBuffers {
  u64 *in, *hash;
  unsigned char *attempts, *rejected;
  unsigned *list, *ctl;
};

// The rounds over n items.  who: the prefix of the error texts; noun: what the items are called in them.  seed == nullptr: the
// points are the caller's own, nothing is drawn and there is one round.
//   body(round, list, listed, at) -> rc   the caller's kernels for the `listed` items of `list` (nullptr: all n, in order) and
//                                         the points `at` drawn for them, which count the rejected in ctl[CTL_COUNT + round]
//   check(h_ctl) -> rc                    the caller's own errors among the control words of the round
// On BN254S_OK *still_rejected (where it is asked for) is the count of the round that ended the loop; it is not zero only after
// the last attempt, round max_attempts - 1.
template <class Body, class Check>
int draw_rounds(bn254s_ctx* c, const std::string& who, const char* noun, int kind, u64 domain, const uint64_t* seed, int max_attempts,
                size_t n, const DrawBuffers& b, Body body, Check check, unsigned* still_rejected = nullptr) {
  hipStream_t st = c->stream;
  const DrawSeed sd = seed ? DrawSeed{{seed[0], seed[1], seed[2], seed[3]}} : DrawSeed{{0, 0, 0, 0}};
  if (!seed) max_attempts = 1;
  unsigned h_ctl[CTL_WORDS];
  size_t listed = n;  // items of the round
  for (int round = 0;; round++) {
    const unsigned* list = round ? b.list : nullptr;
    HashedPoints at = {};
    if (seed) {
      k_draw_inputs<<<(unsigned)((listed + 255) / 256), 256, 0, st>>>(sd, domain + (u64)kind, list, b.attempts, listed, b.in);
      HIP_TRY(c, hipGetLastError());
      const int rc = draw_points(c, kind, b.in, listed, b.hash, &at);
      if (rc != BN254S_OK) return rc;
    }
    int rc = body(round, list, listed, at);
    if (rc != BN254S_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(h_ctl, b.ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    rc = check(h_ctl);
    if (rc != BN254S_OK) return rc;
    const unsigned count = h_ctl[CTL_COUNT + round];
    if (count == 0 || round + 1 == max_attempts) {
      if (still_rejected) *still_rejected = count;
      return BN254S_OK;
    }
    k_draw_compact<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(b.rejected, n, b.attempts, b.list, b.ctl + CTL_LIST + round);
    HIP_TRY(c, hipGetLastError());
    unsigned len = 0;  // (this path is the rare one: a second small copy costs nothing that matters)
    HIP_TRY(c, hipMemcpyAsync(&len, b.ctl + CTL_LIST + round, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (len != count) {  // the next round would read list entries nobody wrote
      c->set_err(who + "the list built after round " + std::to_string(round) + " has " + std::to_string(len) + " " + noun + ", " +
                 std::to_string(count) + " were rejected (device self-check)");
      return BN254S_E_INTERNAL;
    }
    listed = count;
  }
}

}  // namespace
