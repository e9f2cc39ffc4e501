"""Reference for the job check (csrc/job_check.hip, bn254s_job_check_batch): which curve jobs (s, x, offset) the
scalar-multiplication traces can prove.  The trace adds sum + double in every adding row, whether or not the bit of the scalar
is set, and its addition cannot take opposite points: with dbl_0 = x, sum_0 = offset, for k = 0 .. 255

    step k hits iff sum_k == -dbl_k; otherwise sum_{k+1} = sum_k + dbl_k if bit k of s is set (equal points double), else sum_k;
    dbl_{k+1} = 2 dbl_k

and a job is provable iff no step hits.  s is the full 256-bit value, never reduced.

  walk(kind, s, x, offset)          the steps one by one with the complete laws: (k, "add" | "double" | "hit")
  check_one(kind, s, x, offset)     (provable, step) by that walk: step is the first hitting k, or STEP_NONE
  closed_form(kind, s, x, offset)   the hitting steps by offset == -[2^k + (s mod 2^k)] x, one scalar multiplication per k
  check(kind, scalars, x, offset)   check_one over ABI words, as bn254s_job_check_batch returns it
  edge_jobs(kind)                   64 jobs: the crafted ones of every class below beside seeded random ones, shuffled

kind as in bn254s_prove_batch: 0 = G1, 1 = G2 (on the twist).  Points and words as in tools/job_outputs_ref.py."""
from __future__ import annotations

import numpy as np

from tools import job_outputs_ref as jr
from tools import synth

P, R = synth.P, synth.R_ORDER
STEP_NONE = 0xFFFF
SMALL = jr.SMALL
BOUNDARIES = (1, 63, 64, 127, 128, 191, 192, 255)  # around the words of the scalar


def _mul(kind):
    """k -> [k]pt for the integer k as it is (G1 has the prime order r, so reducing there changes nothing)."""
    return jr.g1_mul_complete if kind == 0 else synth.g2_mul_unreduced


def multiplier(s: int, k: int) -> int:
    """m_k = 2^k + (s mod 2^k): step k hits iff offset == -[m_k] x."""
    return (1 << k) + (s & ((1 << k) - 1))


def walk(kind, s: int, x, offset):
    """Yields (k, case) for k = 0, 1, ...: "hit" where sum_k == -dbl_k, which ends the walk; "double" where sum_k == dbl_k;
    "add" otherwise."""
    add, neg = jr._law(kind)
    total, dbl = offset, x
    for k in range(256):
        if total == neg(dbl):
            yield k, "hit"
            return
        yield k, "double" if total == dbl else "add"
        if (s >> k) & 1:
            total = add(total, dbl)
        dbl = add(dbl, dbl)


def check_one(kind, s: int, x, offset):
    """(provable, step) of one job; every Fq-exp job (kind 2) is provable."""
    if kind != 2:
        for k, case in walk(kind, s, x, offset):
            if case == "hit":
                return 0, k
    return 1, STEP_NONE


def closed_form(kind, s: int, x, offset, ks=range(256)):
    """The steps k of ks with offset == -[m_k] x, each by a scalar multiplication of its own (on G2 over every bit of m_k).  The
    smallest hitting k of all 256 is check_one's step.  One job costs 256 multiplications: pass the steps that matter as ks."""
    mul, (_, neg) = _mul(kind), jr._law(kind)
    return [k for k in ks if neg(mul(multiplier(s, k), x)) == offset]


def check(kind, scalars, x, offset=None):
    """(provable [n] uint8, step [n] uint16) for jobs in ABI words."""
    n = len(scalars)
    res = [check_one(kind, synth.words_to_int(scalars[i]), jr.from_words(kind, x[i]),
                     None if kind == 2 else jr.from_words(kind, offset[i])) for i in range(n)]
    return np.array([r[0] for r in res], dtype=np.uint8), np.array([r[1] for r in res], dtype=np.uint16)


def edge_jobs(kind, seed=0x63686B):
    """(scalars [64,4], x [64,PW], offset [64,PW], classes [64], expected [64]) for kind 0 or 1: the crafted jobs of the classes
    below, filled up with seeded random jobs (class "random") to exactly 64 and shuffled, so that special lanes run beside
    ordinary ones in one wave.  expected[i] = (provable, step) as the construction of the job has it, not as check_one finds it."""
    assert kind in (0, 1)
    top = (1 << 256) - 1
    add, neg = jr._law(kind)
    mul = _mul(kind)
    rs, rx, ro = jr.random_jobs(kind, 64, seed)
    pool_x = [jr.from_words(kind, v) for v in rx]
    pool_o = [jr.from_words(kind, v) for v in ro]
    rnd = synth.Xoshiro256ss(seed + 1)
    jobs = []  # (class, s, x, offset, expected)

    def put(cls, s, off, x=None, step=None):
        """off: a function of x, or None for the random offset of the pool; step: the expected hit."""
        px = pool_x[len(jobs)] if x is None else x
        po = pool_o[len(jobs)] if off is None else off(px)
        assert po is not None
        jobs.append((cls, s, px, po, (1, STEP_NONE) if step is None else (0, step)))

    def hit(s, k):  # the offset that makes step k of the scalar s hit
        return lambda px: neg(mul(multiplier(s, k), px))

    def double(s, k):  # the offset with sum_k == dbl_k: offset + [s mod 2^k]x = [2^k]x
        return lambda px: mul((1 << k) - (s & ((1 << k) - 1)), px)

    put("offset = -x, s odd", rnd.next_u256() | 1, neg, step=0)
    put("offset = -x, s = 2", 2, neg, step=0)
    put("offset = x, s = 1", 1, lambda px: px)
    for k in BOUNDARIES:
        s = rnd.next_u256()
        put(f"hit at step {k}", s, hit(s, k), step=k)
        s = rnd.next_u256() | (1 << k)  # bit k is set: the doubled sum is kept
        put(f"doubling at step {k}", s, double(s, k))
    put("s = 0, offset = -[2^7]x", 0, hit(0, 7), step=7)
    put("s = 2^256 - 1", top, None)
    put("s = 2^256 - 1, hit at step 255", top, hit(top, 255), step=255)
    if kind == 0:
        for name, s in (("r - 1", R - 1), ("r", R), ("r + 1", R + 1)):
            put(f"s = {name}", s, None)
            put(f"s = {name}, hit at step 252", s, hit(s, 252), step=252)  # (m_253 of s = r is r itself: no finite offset)
    else:
        pts, _, cls = synth.g2_subgroup_inputs(6, seed=seed + 2, with_classes=True)
        assert cls[1][0] == 1 and cls[3] == (3, SMALL) and cls[0][0] == 0
        off_subgroup, small, member = (synth.g2_from_words(pts[i]) for i in (1, 3, 0))
        assert not synth.g2_in_subgroup(off_subgroup)
        for k in (255, 254, 130):  # the unreduced multiple: m_k >= 2^254 > r, and [m]x != [m mod r]x off the subgroup
            s = rnd.next_u256() | (1 << 255)
            m = multiplier(s, k)
            assert m < R or mul(m, off_subgroup) != mul(m % R, off_subgroup)
            put(f"off the subgroup, s >= 2^255, hit at step {k}", s, hit(s, k), x=off_subgroup, step=k)
        s = rnd.next_u256()
        while any((multiplier(s, j) - multiplier(s, 20)) % SMALL == 0 for j in range(20)):  # no earlier step of the small group
            s = rnd.next_u256()
        put("order 10069, hit at step 20", s, hit(s, 20), x=small, step=20)
        put("order 10069, subgroup offset", rnd.next_u256(), lambda px: member, x=small)
    assert len(jobs) <= 64
    while len(jobs) < 64:
        i = len(jobs)
        jobs.append(("random", synth.words_to_int(rs[i]), pool_x[i], pool_o[i], (1, STEP_NONE)))
    order = list(range(64))
    for i in range(63, 0, -1):  # Fisher-Yates with the seeded generator
        j = rnd.next_u64() % (i + 1)
        order[i], order[j] = order[j], order[i]
    jobs = [jobs[i] for i in order]
    pw = jr.POINT_WORDS[kind]
    scalars = np.array([synth._to_words(j[1]) for j in jobs], dtype=np.uint64).reshape(64, 4)
    x = np.array([jr.to_words(kind, j[2]) for j in jobs], dtype=np.uint64).reshape(64, pw)
    offset = np.array([jr.to_words(kind, j[3]) for j in jobs], dtype=np.uint64).reshape(64, pw)
    return scalars, x, offset, [j[0] for j in jobs], [j[4] for j in jobs]
