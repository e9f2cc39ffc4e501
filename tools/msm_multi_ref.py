"""Reference for many MSMs as one segmented chain (csrc/msm.hip, bn254s_msm_multi_chain), in big integers.

m MSMs stored one after the other, MSM j with seg_len[j] inputs.  For input i, the t-th of MSM j, with T_{j,t} the sum of s x over
the first t inputs of MSM j (R is not in it; it may be the point at infinity):

    offsets[i] = R_j + T_{j,t}        outputs[i] = R_j + T_{j,t+1}        results[j] = T_{j,seg_len[j]}

MSM j is provable under R_j iff every link (s_i, x_i, offsets[i]) is provable (tools/job_check_ref.py); an infinite offset is
checked as R_j, which cannot matter: the link before it has hit already.  R_j is supplied, or drawn:

    R_j^(a) = hash_to_g1 | hash_to_g2 (seed[0..3], j mod 2^32, j >> 32, a, 0x626D6D00 + kind)            a = 0, 1, ...
    MSM j takes the smallest a < max_attempts under which it is provable; with none, it keeps what its last attempt gave

  hash_inputs(kind, seed, j, a)       the eight Goldilocks elements
  drawn(kind, seed, j, a)             the drawn point
  products(kind, scalars, x)          s_i x_i over ABI words, None for the point at infinity (on G2 the scalar is never reduced)
  naive_fold(kind, ss, xs, R)         the reference's sequential fold of one MSM, offset_{t+1} = s_t x_t + offset_t
  chain_one(kind, prods, R)           (offsets, outputs, result) of one MSM from its products
  first_bad_link(kind, ss, xs, offsets, R)   (t, step) of the first link that hits, or (LINK_NONE, STEP_NONE)
  msm_multi(kind, scalars, x, seg_len, R=None, seed=None, ...)   everything bn254s_msm_multi_chain returns, in ABI words
  crafted_x(kind, R, T, s, k)         the x that makes a link with offset R + T and scalar s hit at step k

kind as in bn254s_prove_batch: 0 = G1, 1 = G2 (on the twist).  Points and words as in tools/job_outputs_ref.py."""
from __future__ import annotations

import collections
import functools

import numpy as np

from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import map_to_g1_ref as m2g1
from tools import map_to_g2_ref as m2g2
from tools import synth

P, R_ORD = synth.P, synth.R_ORDER
DOMAIN = 0x626D6D00
MAX_ATTEMPTS = 8
LINK_NONE = 0xFFFFFFFF
STEP_NONE = jc.STEP_NONE

Result = collections.namedtuple("Result", "results finite offsets outputs R attempts bad_link bad_step")


def hash_inputs(kind, seed, j: int, a: int):
    assert len(seed) == 4 and all(0 <= int(v) < m2g2.GL_P for v in seed) and 0 <= a < MAX_ATTEMPTS
    return [int(v) for v in seed] + [j & 0xFFFFFFFF, j >> 32, a, DOMAIN + kind]


@functools.lru_cache(maxsize=None)
def _drawn(kind, seed, j, a):
    ins = hash_inputs(kind, seed, j, a)
    if kind == 0:
        return m2g1.map_to_g1(m2g1.hash_to_fq(ins))
    return m2g2.map_to_g2(m2g2.hash_to_fq2(ins))


def drawn(kind, seed, j: int, a: int):
    """R_j^(a): a point of G1, or of the order-r subgroup of the twist (map_to_g2 clears the cofactor)."""
    return _drawn(kind, tuple(int(v) for v in seed), j, a)


def _mul(kind):
    return jr.g1_mul_complete if kind == 0 else synth.g2_mul_unreduced


def products(kind, scalars, x):
    """[s_i x_i] for inputs in ABI words."""
    mul = _mul(kind)
    return [mul(synth.words_to_int(scalars[i]), jr.from_words(kind, x[i])) for i in range(len(scalars))]


def naive_fold(kind, ss, xs, R):
    """[offset_0 = R, offset_1, ..., offset_len] by one affine scalar multiplication with offset per link, as the reference's
    run_once computes it (synth.g1_scalar_mul_offset; on G2 its twin over the unreduced scalar).  For MSMs no partial sum of which
    is infinite: the affine laws raise there."""
    offs = [R]
    for s, x in zip(ss, xs):
        if kind == 0:
            offs.append(synth.g1_scalar_mul_offset(s, x, offs[-1]))
        else:
            prod = synth.g2_mul_unreduced(s, x)
            offs.append(offs[-1] if prod is None else synth.g2_add(prod, offs[-1]))
    return offs


def chain_one(kind, prods, R):
    """(offsets, outputs, result) of one MSM: its running sum T starts at infinity and never sees R."""
    add, _ = jr._law(kind)
    total, offsets, outputs = None, [], []
    for p in prods:
        offsets.append(add(R, total))
        total = add(total, p)
        outputs.append(add(R, total))
    return offsets, outputs, total


def first_bad_link(kind, ss, xs, offsets, R):
    """(t, step) of the first link of one MSM that hits, by the walk of job_check_ref."""
    for t, (s, x, off) in enumerate(zip(ss, xs, offsets)):
        provable, step = jc.check_one(kind, s, x, R if off is None else off)
        if not provable:
            return t, step
    return LINK_NONE, STEP_NONE


def msm_multi(kind, scalars, x, seg_len, R=None, seed=None, max_attempts: int = 4, prods=None, check=None):
    """Result of arrays as bn254s_msm_multi_chain writes them.  R: [m, PW] words, or None for points drawn from `seed`.
    prods: products(kind, scalars, x) where the caller has them already.  check: the MSMs whose links are walked (default: all of
    them); the others are taken as provable - for callers who establish that otherwise, the walk being 256 affine steps per link."""
    n, m, pw = len(scalars), len(seg_len), jr.POINT_WORDS[kind]
    assert sum(int(v) for v in seg_len) == n and all(int(v) >= 1 for v in seg_len) and (R is not None or seed is not None)
    prods = products(kind, scalars, x) if prods is None else prods
    res = Result(np.zeros((m, pw), np.uint64), np.zeros(m, np.uint8), np.zeros((n, pw), np.uint64), np.zeros((n, pw), np.uint64),
                 np.zeros((m, pw), np.uint64), np.zeros(m, np.uint8), np.full(m, LINK_NONE, np.uint32), np.full(m, STEP_NONE, np.uint16))
    first = 0
    for j, ln in enumerate(int(v) for v in seg_len):
        lo, hi = first, first + ln
        first = hi
        ss = [synth.words_to_int(scalars[i]) for i in range(lo, hi)]
        xs = [jr.from_words(kind, x[i]) for i in range(lo, hi)]
        for a in range(1 if R is not None else max_attempts):
            Rj = jr.from_words(kind, R[j]) if R is not None else drawn(kind, seed, j, a)
            if Rj is None:  # a drawn point whose cleared image is infinity: a failed attempt, link 0 without a step
                Rj, bad, offs, outs = xs[0], (0, STEP_NONE), [None] * ln, [None] * ln
                total = chain_one(kind, prods[lo:hi], Rj)[2]
            else:
                offs, outs, total = chain_one(kind, prods[lo:hi], Rj)
                bad = first_bad_link(kind, ss, xs, offs, Rj) if check is None or j in check else (LINK_NONE, STEP_NONE)
            if bad[0] == LINK_NONE:
                break
        res.results[j] = jr.to_words(kind, total)
        res.finite[j] = total is not None
        res.R[j] = jr.to_words(kind, Rj)
        res.bad_link[j], res.bad_step[j] = bad
        if bad[0] == LINK_NONE:
            res.attempts[j] = a
            res.offsets[lo:hi] = np.array([jr.to_words(kind, v) for v in offs], np.uint64).reshape(ln, pw)
            res.outputs[lo:hi] = np.array([jr.to_words(kind, v) for v in outs], np.uint64).reshape(ln, pw)
        else:
            res.attempts[j] = 0 if R is not None else max_attempts
    return res


def crafted_x(kind, R, T, s: int, k: int):
    """x = [-(c^-1 mod r)] (R + T) with c = 2^k + (s mod 2^k): the offset R + T is -[c] x, so the link hits at step k (and at no
    earlier step unless another c_j is congruent to c modulo r).  None where c is a multiple of r or R + T is infinite.  On G2,
    R + T must lie in the order-r subgroup."""
    add, _ = jr._law(kind)
    c, off = jc.multiplier(s, k) % R_ORD, add(R, T)
    if c == 0 or off is None:
        return None
    e = -pow(c, -1, R_ORD) % R_ORD
    return jr.g1_mul_complete(e, off) if kind == 0 else synth.g2_mul_unreduced(e, off)
