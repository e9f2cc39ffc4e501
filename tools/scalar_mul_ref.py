"""Reference for the scalar multiplication without an offset argument (csrc/scalar_mul.hip, bn254s_scalar_mul_batch): s x on G1
and on the twist curve, with the offset of the statement s x + offset drawn from a seed and redrawn where the job cannot be proven.

    offset_i^(a) = hash_to_g1 | hash_to_g2 (seed[0..3], i mod 2^32, i >> 32, a, 0x62736D00 + kind)         a = 0, 1, ...
    job i takes the smallest a < max_attempts for which (s_i, x_i, offset_i^(a)) is provable (tools/job_check_ref.py)
    output_i = s_i x_i + offset_i^(a),  product_i = output_i - offset_i^(a) = s_i x_i

  hash_inputs(kind, seed, i, a)          the eight Goldilocks elements
  offset(kind, seed, i, a)               the drawn point (map_to_g1_ref / map_to_g2_ref on the hash of the inputs)
  scalar_mul_one(kind, s, x, seed, i)    (product, offset, output, attempt) of one job; Exhausted if no attempt is accepted
  scalar_mul(kind, scalars, x, seed)     the same over ABI words, as bn254s_scalar_mul_batch returns it
  crafted_x(kind, seed, i, s, k)         the x that makes job i hit step k with the offset of attempt 0
  opposite_x(kind, seed, i, s)           the x whose output is minus the offset of attempt 0 (the subtraction doubles)

kind as in bn254s_prove_batch: 0 = G1, 1 = G2 (on the twist).  Points and words as in tools/job_outputs_ref.py."""
from __future__ import annotations

import functools

import numpy as np

from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import map_to_g1_ref as m2g1
from tools import map_to_g2_ref as m2g2
from tools import synth

P, R = synth.P, synth.R_ORDER
DOMAIN = 0x62736D00
MAX_ATTEMPTS = 8


class Exhausted(ValueError):
    """No attempt below max_attempts gives job `i` an offset it can be proven with; `step` is the hit of the last attempt."""

    def __init__(self, i, step, attempt):
        super().__init__(f"job {i} cannot be proven: sum == -double at step {step} (row {2 * step} of its frame) with the offset of "
                         f"attempt {attempt}")
        self.i, self.step, self.attempt = i, step, attempt


def hash_inputs(kind, seed, i: int, a: int):
    assert len(seed) == 4 and all(0 <= int(v) < m2g2.GL_P for v in seed) and 0 <= a < MAX_ATTEMPTS
    return [int(v) for v in seed] + [i & 0xFFFFFFFF, i >> 32, a, DOMAIN + kind]


@functools.lru_cache(maxsize=None)
def _offset(kind, seed, i, a):
    ins = hash_inputs(kind, seed, i, a)
    if kind == 0:
        return m2g1.map_to_g1(m2g1.hash_to_fq(ins))
    return m2g2.map_to_g2(m2g2.hash_to_fq2(ins))


def offset(kind, seed, i: int, a: int):
    """offset_i^(a): a point of G1, or of the order-r subgroup of the twist (map_to_g2 clears the cofactor)."""
    return _offset(kind, tuple(int(v) for v in seed), i, a)


def scalar_mul_one(kind, s: int, x, seed, i: int, max_attempts: int = 4):
    """(product, offset, output, attempt): product is None where s x is the point at infinity."""
    add, neg = jr._law(kind)
    step = jc.STEP_NONE
    for a in range(max_attempts):
        off = offset(kind, seed, i, a)
        provable, step = jc.check_one(kind, s, x, off)
        if provable:
            out = jr.output_one(kind, s, x, off)
            assert out is not None  # the last sum of a walk without a hit
            return add(out, neg(off)), off, out, a
    raise Exhausted(i, step, max_attempts - 1)


def scalar_mul(kind, scalars, x, seed, max_attempts: int = 4, first: int = 0):
    """(products, finite, offsets, outputs, attempts) for jobs in ABI words, job j of the arrays being job first + j of its call."""
    n, pw = len(scalars), jr.POINT_WORDS[kind]
    res = [scalar_mul_one(kind, synth.words_to_int(scalars[j]), jr.from_words(kind, x[j]), seed, first + j, max_attempts) for j in range(n)]
    words = lambda col: np.array([jr.to_words(kind, r[col]) for r in res], dtype=np.uint64).reshape(n, pw)
    return (words(0), np.array([r[0] is not None for r in res], dtype=np.uint8), words(1), words(2),
            np.array([r[3] for r in res], dtype=np.uint8))


def _scaled(kind, k: int, pt):
    """[k mod r] pt for a point of order r."""
    return jr.g1_mul_complete(k, pt) if kind == 0 else synth.g2_mul_unreduced(k % R, pt)


def crafted_x(kind, seed, i: int, s: int, k: int):
    """x = [-(m^-1 mod r)] R0 with R0 = offset_i^(0) and m = 2^k + (s mod 2^k): offset == -[m] x, so job i hits step k at attempt 0
    (and no earlier step unless another m_j is congruent to m modulo r).  None where m is a multiple of r.  On G2 this works
    because R0, and with it x, lies in the order-r subgroup."""
    m = jc.multiplier(s, k) % R
    if m == 0:
        return None
    return _scaled(kind, -pow(m, -1, R), offset(kind, seed, i, 0))


def opposite_x(kind, seed, i: int, s: int):
    """x = [-(2 s^-1) mod r] R0: s x = -2 R0, the output is -R0 and output - offset doubles it.  None where s is a multiple of r."""
    if s % R == 0:
        return None
    return _scaled(kind, -2 * pow(s, -1, R), offset(kind, seed, i, 0))
