"""Reference for the proof-free job outputs (csrc/job_outputs.hip, bn254s_job_outputs_batch): s x + offset on G1 and on the twist
curve, x^s in Fq, for jobs that each bring their own 256-bit scalar.

  outputs(kind, scalars, x, offset)   the definition in Python integers (tools/synth.py), ABI words in and out
  ladder(kind, s, x, offset, w)       a limb-free model of the kernel's fixed-window ladder that also reports which of its
                                      additions met a case the ordinary addition law cannot take
  edge_jobs(kind)                     64 jobs: the crafted ones of every class below beside seeded random ones, shuffled

kind as in bn254s_prove_batch: 0 = G1, 1 = G2, 2 = Fq exp.  A point is an affine pair (G2: of Fq2 pairs) or None for the point
at infinity.  The G2 scalar is the full 256-bit value (g2_mul_unreduced): off the r-torsion subgroup s x != (s mod r) x.  On G1,
of prime order r, the scalar is reduced first.  Fq: pow(x, s, p), with 0^0 = 1 - which is also what the Fq-exp trace puts out (its
product column starts at 1 and no bit of s = 0 multiplies it), so Python and the oracle agree there and nothing is overridden."""
from __future__ import annotations

import numpy as np

from tools import synth

P, R = synth.P, synth.R_ORDER
WINDOW = {0: 3, 1: 2, 2: 4}          # the windows of the three kernels (csrc/job_outputs.hip)
POINT_WORDS = {0: 8, 1: 16, 2: 4}
SMALL = 10069                        # the smallest prime of the twist's cofactor
# classes of edge_jobs whose output is the point at infinity, and classes whose output is finite although a bit-by-bit walk from
# the offset may meet a + (-a) (twist points of order 10069 whose offset lies in the same small group)
INFINITE = ("offset = -x, s = 1", "offset = -[2]x, s = 2", "offset = x, s = r - 1")
SMALL_ORDER = ("order 10069, s = 10069", "order 10069, s = 10069 * 2^w + 1", "order 10069, accumulator equals an entry",
               "order 10069, accumulator is minus an entry")


# ---- the group laws with None as the point at infinity ---------------------------------------------------------------------
def g1_neg(a):
    return None if a is None else (a[0], (-a[1]) % P)


def g1_add_complete(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0] and (a[1] + b[1]) % P == 0:
        return None
    return synth.g1_add(a, b)


def g1_mul_complete(k: int, pt):
    k %= R
    return synth.g1_mul(k, pt) if k else None


def _law(kind):
    """(add, neg) of the curve of `kind`."""
    return (g1_add_complete, g1_neg) if kind == 0 else (synth.g2_add_complete, synth.g2_neg)


def output_one(kind, s: int, x, offset=None):
    """s x + offset (None for infinity), or x^s for kind 2."""
    if kind == 2:
        return pow(x, s, P)
    if kind == 0:
        return g1_add_complete(g1_mul_complete(s, x), offset)
    return synth.g2_add_complete(synth.g2_mul_unreduced(s, x), offset)


# ---- ABI words <-> Python values -----------------------------------------------------------------------------------------
def from_words(kind, w):
    if kind == 2:
        return synth.words_to_int(w)
    if kind == 0:
        return (synth.words_to_int(w[:4]), synth.words_to_int(w[4:]))
    return synth.g2_from_words(w)


def to_words(kind, v):
    """The output words of one job: zeros for the point at infinity."""
    if v is None:
        return [0] * POINT_WORDS[kind]
    if kind == 2:
        return synth._to_words(v)
    if kind == 0:
        return synth._to_words(v[0]) + synth._to_words(v[1])
    return [int(t) for t in synth.g2_points_to_words([v])[0]]


def outputs(kind, scalars, x, offset=None):
    """(outputs [n, 8 | 16 | 4] uint64, finite [n] uint8) for jobs in ABI words, as bn254s_job_outputs_batch returns them: zero
    words and finite = 0 where s x + offset is the point at infinity; finite = 1 for every Fq-exp job."""
    n = len(scalars)
    vals = [output_one(kind, synth.words_to_int(scalars[i]), from_words(kind, x[i]),
                       None if kind == 2 else from_words(kind, offset[i])) for i in range(n)]
    words = np.array([to_words(kind, v) for v in vals], dtype=np.uint64).reshape(n, POINT_WORDS[kind])
    return words, np.array([v is not None for v in vals], dtype=np.uint8)


# ---- the ladder of csrc/window_ladder.h, without limbs ---------------------------------------------------------------------
def digits(s: int, w: int):
    """The digits of the 256-bit s, highest first: the first one holds the 256 mod w bits the others leave over (w where w
    divides 256), every other one w bits."""
    nwin = (256 + w - 1) // w
    return [(s >> (w * i)) & ((1 << w) - 1) for i in range(nwin - 1, -1, -1)]


def ladder(kind, s: int, x, offset=None, w=None):
    """(output, events): the output as output_one gives it, computed like the kernel - the table [1]x .. [2^w - 1]x, the first
    digit's entry, then per digit w doublings and one addition, and + offset at the end.  events lists (where, case) for every
    addition whose operands are not distinct, non-opposite and finite: where is "table", "ladder" or "offset", case is "O"
    (an operand is the point at infinity; a zero digit counts), "equal" or "opposite".  Fq-exp has no such case."""
    w = WINDOW[kind] if w is None else w
    ds = digits(s, w)
    if kind == 2:
        tab = [1]
        for _ in range((1 << w) - 1):
            tab.append(tab[-1] * x % P)
        acc = tab[ds[0]]
        for d in ds[1:]:
            for _ in range(w):
                acc = acc * acc % P
            acc = acc * tab[d] % P
        return acc, []
    add, neg = _law(kind)
    events = []

    def note(where, a, b):
        if a is None or b is None:
            events.append((where, "O"))
        elif a == b:
            events.append((where, "equal"))
        elif a == neg(b):
            events.append((where, "opposite"))
        return add(a, b)

    tab = [None, x, add(x, x)]
    for _ in range(3, 1 << w):
        tab.append(note("table", tab[-1], x))
    acc = tab[ds[0]]
    for d in ds[1:]:
        for _ in range(w):
            acc = add(acc, acc)
        acc = note("ladder", acc, tab[d])
    return note("offset", acc, offset), events


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def random_jobs(kind, n, seed):
    """(scalars, x, offset) in ABI words as synth makes them (offset None for kind 2)."""
    if kind == 0:
        return synth.g1_inputs(n, seed)
    if kind == 1:
        return synth.g2_inputs(n, seed)
    return synth.fq_inputs(n, seed) + (None,)


def provable_jobs(kind, n, seed):
    """random_jobs whose proofs the G2 trace can make, and on G2 with every other x replaced by a random point of the twist (outside
    the r-torsion subgroup) and its scalar raised to 2^255 or more, above r: jobs whose output depends on the unreduced scalar."""
    s, x, o = random_jobs(kind, n, seed)
    if kind == 1:
        rng = synth.Xoshiro256ss(seed + 1)
        for i in range(1, n, 2):
            x[i] = synth.g2_points_to_words([synth._g2_random_twist_point(rng)])[0]
            s[i, 3] |= np.uint64(1 << 63)
    return s, x, o


def alternating(w: int, low: bool):
    """Digits alternately all ones and zero, the lowest one all ones if `low`."""
    v = 0
    for i in range(0 if low else 1, (256 + w - 1) // w, 2):
        v |= ((1 << w) - 1) << (w * i)
    return v & ((1 << 256) - 1)


def edge_jobs(kind, seed=0x6A6F62):
    """(scalars [64,4], x [64,PW], offset [64,PW] or None, classes [64]): the crafted jobs of the classes named below, filled up with
    seeded random jobs (class "random") to exactly 64 and shuffled, so that special lanes run beside ordinary ones in one wave."""
    w = WINDOW[kind]
    top = (1 << 256) - 1
    rs, rx, ro = random_jobs(kind, 64, seed)
    pool_x = [from_words(kind, v) for v in rx]
    pool_o = [from_words(kind, v) for v in ro] if kind != 2 else [None] * 64
    rnd = synth.Xoshiro256ss(seed + 1)
    jobs = []  # (class, s, x, offset)

    def take():
        i = len(jobs)
        return pool_x[i], pool_o[i]

    def put(cls, s, x=None, off=None):
        px, po = take()
        jobs.append((cls, s, px if x is None else x, po if off is None else off))

    if kind == 2:
        for xn, xv in (("0", 0), ("1", 1), ("2", 2), ("p - 1", P - 1)):
            for sn, sv in (("0", 0), ("1", 1), ("p - 1", P - 1), ("p", P), ("2^256 - 1", top)):
                jobs.append((f"x = {xn}, s = {sn}", sv, xv, None))
        named = [("s = 2^w - 1", (1 << w) - 1), ("s = 2^w", 1 << w), ("s = 2^255", 1 << 255), ("alternating digits", alternating(w, True)),
                 ("alternating digits", alternating(w, False))]
        for cls, sv in named:
            put(cls, sv)
    else:
        add, neg = _law(kind)
        mul = g1_mul_complete if kind == 0 else synth.g2_mul_unreduced
        for sv in (0, 1, 2):
            put(f"s = {sv}", sv)
        for ww in (2, 3, 4):  # the windows the ladder model is run with; w of the kernel among them
            put("s = 2^w - 1", (1 << ww) - 1)
            put("s = 2^w", 1 << ww)
        put("s = 2^255", 1 << 255)
        put("s = 2^256 - 1", top)
        put("alternating digits", alternating(w, True))
        put("alternating digits", alternating(w, False))
        put("s = r - 1", R - 1)
        put("s = r", R)
        put("s = r + 1", R + 1)
        put("s = largest multiple of r", top // R * R)
        px, _ = take()
        put("offset = x, s = 1", 1, px, px)
        px, _ = take()
        put("offset = -x, s = 1", 1, px, neg(px))
        px, _ = take()
        put("offset = -[2]x, s = 2", 2, px, neg(add(px, px)))
        px, _ = take()
        sv = rnd.next_u256()
        put("offset = [s]x", sv, px, mul(sv, px))
        if kind == 0:
            px, _ = take()
            put("offset = x, s = r - 1", R - 1, px, px)
            for ww in (2, 3, 4):  # s = r + 2d with 2^w | r + d: the prefix m = (r + d) / 2^w gives [2^w m]x = [d]x, then the digit d
                d = -R % (1 << ww)
                put("accumulator equals an entry, s = r + 2d", R + 2 * d)
        else:
            pts, _, cls = synth.g2_subgroup_inputs(9, seed=seed + 2, with_classes=True)
            for i in (1, 5, 8):  # two random twist points and a member plus a point of order 10069: none in the subgroup
                assert cls[i][0] in (1, 5)
                put("off the subgroup, s >= r", rnd.next_u256() | (1 << 255), synth.g2_from_words(pts[i]))
            small = synth.g2_from_words(pts[3])
            assert cls[3] == (3, SMALL)
            inv = pow(1 << w, -1, SMALL)
            put("order 10069, s = 10069", SMALL, small)
            for ww in (2, 3, 4):
                put("order 10069, s = 10069 * 2^w + 1", SMALL * (1 << ww) + 1, small)
            # [2^w m]x = [1]x: the accumulator is the entry that is added; [2^w m]x = -[1]x: its negative
            put("order 10069, accumulator equals an entry", (inv << w) + 1, small)
            put("order 10069, accumulator is minus an entry", ((SMALL - inv) << w) + 1, small)
    assert len(jobs) <= 64
    while len(jobs) < 64:
        i = len(jobs)
        jobs.append(("random", synth.words_to_int(rs[i]), pool_x[i], pool_o[i]))
    order = list(range(64))
    for i in range(63, 0, -1):  # Fisher-Yates with the seeded generator
        j = rnd.next_u64() % (i + 1)
        order[i], order[j] = order[j], order[i]
    jobs = [jobs[i] for i in order]
    pw = POINT_WORDS[kind]
    scalars = np.array([synth._to_words(j[1]) for j in jobs], dtype=np.uint64).reshape(64, 4)
    x = np.array([to_words(kind, j[2]) for j in jobs], dtype=np.uint64).reshape(64, pw)
    offset = None if kind == 2 else np.array([to_words(kind, j[3]) for j in jobs], dtype=np.uint64).reshape(64, pw)
    return scalars, x, offset, [j[0] for j in jobs]
