"""Reference for the point-sum check (csrc/point_sum.hip, bn254s_point_sum_check_batch): is c == a + b for affine points b, c and a
point a that may be the point at infinity, on G1 (kind 0) and on the twist curve (kind 1).

  code_one(kind, a, a_finite, b, c)   the definition in Python integers, ABI words in: a + b by the complete law of
                                      tools/job_outputs_ref.py, then compared with c - not the cross-multiplied equations of
                                      the kernel, which this file is there to check
  codes(kind, a, a_finite, b, c)      the same for arrays, as the entry point returns them
  cases(kind)                         the crafted relations, accepted and rejected, with the code each was made for

The code of a relation is the first that applies of
  1 a_finite == 0 with a non-zero word of a     2, 3, 4 a (where finite), b, c off the curve
  5 a == -b: the sum is the point at infinity   6 the x of a + b is not that of c        7 x agrees, y does not: c == -(a + b)
and 0 where the relation holds."""
from __future__ import annotations

import numpy as np

from tools import job_outputs_ref as jr
from tools import synth

P = synth.P
(OK, A_NOT_ZERO, A_OFF_CURVE, B_OFF_CURVE, C_OFF_CURVE, INFINITE, SUM_X, SUM_Y) = range(8)


def on_curve(kind, pt) -> bool:
    if kind == 0:
        return (pt[1] * pt[1] - pt[0] * pt[0] * pt[0] - 3) % P == 0
    return synth.g2_on_curve(pt)


def code_one(kind, a, a_finite, b, c) -> int:
    """a, b, c: the PW words of the three points."""
    add, _ = jr._law(kind)
    if not a_finite:
        if any(int(w) for w in a):
            return A_NOT_ZERO
        pa = None
    else:
        pa = jr.from_words(kind, a)
        if not on_curve(kind, pa):
            return A_OFF_CURVE
    pb, pc = jr.from_words(kind, b), jr.from_words(kind, c)
    if not on_curve(kind, pb):
        return B_OFF_CURVE
    if not on_curve(kind, pc):
        return C_OFF_CURVE
    total = add(pa, pb)
    if total is None:
        return INFINITE
    if total[0] != pc[0]:
        return SUM_X
    return OK if total[1] == pc[1] else SUM_Y


def codes(kind, a, a_finite, b, c):
    return np.array([code_one(kind, a[i], a_finite[i], b[i], c[i]) for i in range(len(a))], dtype=np.uint8)


def _bump(kind, pt, coord):
    """The words of pt with the lowest word of one coordinate changed in its lowest bit: below p still, and off the curve."""
    w = jr.to_words(kind, pt)
    w[4 * coord] ^= 1
    assert synth.words_to_int(w[4 * coord:4 * coord + 4]) < P and not on_curve(kind, jr.from_words(kind, w))
    return w


def cases(kind, seed=0x70736D):
    """(a [k,PW], a_finite [k], b [k,PW], c [k,PW], want [k] uint8, names [k]): every relation made for its code from seeded random
    points - on G2 points of the r-torsion subgroup but for the cases that say otherwise."""
    add, neg = jr._law(kind)
    pw = jr.POINT_WORDS[kind]
    _, xw, ow = jr.random_jobs(kind, 24, seed + kind)
    pts = [jr.from_words(kind, w) for w in xw] + [jr.from_words(kind, w) for w in ow]
    it = iter(pts)
    words = lambda pt: jr.to_words(kind, pt)
    zero = [0] * pw
    rows = []  # (name, a words, finite, b words, c words, code)

    def put(name, a, fin, b, c, code):
        rows.append((name, a, fin, b, c, code))

    a, b = next(it), next(it)
    put("general", words(a), 1, words(b), words(add(a, b)), OK)
    b = next(it)
    put("a = O", zero, 0, words(b), words(b), OK)
    a = next(it)
    put("a == b", words(a), 1, words(a), words(add(a, a)), OK)
    if kind == 1:
        rng = synth.Xoshiro256ss(seed + 7)
        a, b = synth._g2_random_twist_point(rng), synth._g2_random_twist_point(rng)
        assert not synth.g2_in_subgroup(a) and not synth.g2_in_subgroup(b)
        put("twist points outside the subgroup", words(a), 1, words(b), words(add(a, b)), OK)
        put("a == b outside the subgroup", words(a), 1, words(a), words(add(a, a)), OK)
        put("outside the subgroup, c = -(a + b)", words(a), 1, words(b), words(neg(add(a, b))), SUM_Y)
    a, b = next(it), next(it)
    put("c = -(a + b)", words(a), 1, words(b), words(neg(add(a, b))), SUM_Y)
    a = next(it)
    put("a == b, c = -(2a)", words(a), 1, words(a), words(neg(add(a, a))), SUM_Y)
    a, c = next(it), next(it)
    put("a = -b", words(a), 1, words(neg(a)), words(c), INFINITE)
    a = next(it)
    put("a = -b, c = a", words(a), 1, words(neg(a)), words(a), INFINITE)
    b = next(it)
    put("a = O, c = -b", zero, 0, words(b), words(neg(b)), SUM_Y)
    b, c = next(it), next(it)
    put("a = O, c another point", zero, 0, words(b), words(c), SUM_X)
    a, b, c = next(it), next(it), next(it)
    put("c another point", words(a), 1, words(b), words(c), SUM_X)
    a, b = next(it), next(it)
    put("a == b, c = a", words(a), 1, words(a), words(a), SUM_X)
    a, b = next(it), next(it)
    put("finite = 0, the words of a point", words(a), 0, words(b), words(add(a, b)), A_NOT_ZERO)
    b = next(it)
    put("finite = 0, one word", zero[:-1] + [1], 0, words(b), words(b), A_NOT_ZERO)
    b = next(it)
    put("finite = 0, words not below p", [synth.MASK64] * pw, 0, words(b), words(b), A_NOT_ZERO)
    for coord in range(pw // 4):  # every coordinate once: x, y (x.c0, x.c1, y.c0, y.c1)
        a, b = next(it), next(it)
        s = add(a, b)
        put(f"a off its curve ({coord})", _bump(kind, a, coord), 1, words(b), words(s), A_OFF_CURVE)
        put(f"b off its curve ({coord})", words(a), 1, _bump(kind, b, coord), words(s), B_OFF_CURVE)
        put(f"c off its curve ({coord})", words(a), 1, words(b), _bump(kind, s, coord), C_OFF_CURVE)
    a, b = next(it), next(it)
    put("a and c off their curves", _bump(kind, a, 0), 1, words(b), _bump(kind, add(a, b), 0), A_OFF_CURVE)  # the first applies
    arr = lambda k: np.array([r[k] for r in rows], dtype=np.uint64).reshape(len(rows), pw)
    return (arr(1), np.array([r[2] for r in rows], dtype=np.uint8), arr(3), arr(4), np.array([r[5] for r in rows], dtype=np.uint8),
            [r[0] for r in rows])
