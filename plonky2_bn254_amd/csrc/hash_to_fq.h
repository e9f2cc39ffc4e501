// hash_to_fq / hash_to_fq2 (reference src/utils/hash_to_g2.rs:76-87) for the two hash-to-curve front-ends (map_to_g2.hip,
// map_to_g1.hip): Challenger::observe_elements(input), then per coordinate the low 32 bits of 16 challenges as the little-endian
// limbs of a 512-bit integer, reduced modulo p (f_slice_to_biguint, :226-240, then `.into()`).  hash_to_fq is the first coordinate
// of hash_to_fq2: the same challenger, stopped after 16 challenges.
#pragma once
#include <cstring>
#include "fq_dev.h"
#include "transcript.h"

namespace {

// host: ncoord (1 or 2) coordinates of four canonical words each
inline void hash_to_fq_host(const uint64_t* input, size_t len, int ncoord, uint64_t* out) {
  static const u64 PW[4] = {0x3c208c16d87cfd47ULL, 0x97816a916871ca8dULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  Challenger ch;
  ch.observe_n(input, len);
  for (int coord = 0; coord < ncoord; coord++) {
    u32 limbs[16];
    for (int i = 0; i < 16; i++) limbs[i] = (u32)ch.challenge();
    u64 r[4] = {0, 0, 0, 0};  // r = value mod p, one bit at a time from the top (r < p < 2^254: the doubling cannot overflow)
    for (int bit = 511; bit >= 0; bit--) {
      u64 carry = (limbs[bit >> 5] >> (bit & 31)) & 1;
      for (int w = 0; w < 4; w++) {
        u64 nc = r[w] >> 63;
        r[w] = (r[w] << 1) | carry;
        carry = nc;
      }
      bool ge = true;
      for (int w = 3; w >= 0; w--) {
        if (r[w] != PW[w]) {
          ge = r[w] > PW[w];
          break;
        }
      }
      if (ge) {
        u64 borrow = 0;
        for (int w = 0; w < 4; w++) {
          unsigned __int128 d = (unsigned __int128)r[w] - PW[w] - borrow;
          r[w] = (u64)d;
          borrow = (u64)(d >> 64) & 1;
        }
      }
    }
    memcpy(out + 4 * coord, r, 32);
  }
}

// One lane's input x of `len` Goldilocks elements -> NCOORD coordinates (four canonical words each) at out: the challenger absorbs
// the input in chunks of eight (overwrite mode; a last partial chunk, or an empty input, is permuted when the first challenge is
// asked for), then NCOORD x 16 challenges are popped - eight per permutation, lane 7 first - and their low 32 bits are the
// little-endian limbs of a 512-bit integer per coordinate, reduced modulo p: lo + hi 2^256 with both halves taken into Montgomery
// form.
__device__ static constexpr u32 H2F_TWO256_MONT[FQ_NL] = {0x3b5ae02, 0x3ab61e1, 0xaa4ba8, 0x3e9cdb2, 0x2f6ebb, 0x4553ac, 0x116483a, 0x468428, 0x236e920, 0x33056};  // 2^256 R mod p
template <int NCOORD>
__device__ __forceinline__ void hash_to_fq_lane(const u64* __restrict__ x, size_t len, u64* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  u64 st[12];
#pragma unroll
  for (int i = 0; i < 12; i++) st[i] = 0;
  size_t pos = 0;
  bool have_out = false;
  for (; len - pos >= 8; pos += 8) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = x[pos + i];
    poseidon_permute(st);
    have_out = true;
  }
  const int rem = (int)(len - pos);
  if (rem > 0 || !have_out) {
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (i < rem) st[i] = x[pos + i];
    poseidon_permute(st);
  }
  fq r2, c256;
#pragma unroll
  for (int i = 0; i < FQ_NL; i++) {
    r2.l[i] = FQ_R2[i];
    c256.l[i] = H2F_TWO256_MONT[i];
  }
#pragma unroll 1
  for (int coord = 0; coord < NCOORD; coord++) {
    u64 w[8];  // the 512-bit integer as eight 64-bit words: limb 2j | limb 2j+1 << 32
#pragma unroll
    for (int half = 0; half < 2; half++) {
      if (coord + half > 0) poseidon_permute(st);  // output buffer used up (8 challenges per permutation)
#pragma unroll
      for (int j = 0; j < 4; j++) w[4 * half + j] = (u64)(u32)st[7 - 2 * j] | ((u64)(u32)st[6 - 2 * j] << 32);
    }
    const fq lo = fq_mul(fq_unpack(w), r2), hi = fq_mul(fq_unpack(w + 4), r2);  // (values below 2^256 < 6 p: loose operands)
    const fqw c = fq_to_canonical(fq_add(lo, fq_mul(hi, c256)));
#pragma unroll
    for (int i = 0; i < 4; i++) out[4 * coord + i] = c.l[i];
  }
#endif
}

}  // namespace
