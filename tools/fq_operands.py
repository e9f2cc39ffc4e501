"""Operand table and big-integer expectations for bn254s_selftest_fq (the BN254 Fq / Fq2 device arithmetic on RAW residues).

The registers of csrc/fq_dev.h hold Montgomery residues x 2^260 mod p in ten 26-bit limbs.  The table below chooses those
register contents directly (integers below p whose LIMBS are extreme), so the multiplier really sees p - 1, all-ones limbs and
so on.  Expected raw results: a product form is formula * 2^-260 mod p, a linear form is formula mod p.

Shared by tests/test_gpu_fq_arith.py (the compiled gfx950 code) and tests/test_fq_limb_model_cpu.py (tools/fq_limb_model.py)."""
from __future__ import annotations

import numpy as np

from tools import synth

P = synth.P
LB, NL = 26, 10
LMASK = (1 << LB) - 1
R = pow(2, 260, P)
RI = pow(R, -1, P)
R2 = R * R % P
P_TOP = P >> (LB * (NL - 1))          # 0xc1913

IN_WORDS = (16, 16, 32, 72)            # u64 words per row, by group (csrc/fq_selftest.h)
OUT_WORDS = (68, 60, 92, 74)

# (fa, ga, fb, gb) of g1coop::product / g2coop::product in the two doubling chains: levels 1, 1, 2, 2, 3
PRODUCT_TUPLES = ((1, 0, 1, 0), (2, 0, 1, 0), (1, 1, 1, 1), (3, 0, 3, 0), (3, 0, 1, 0))
# (k0, k1, k2, k3, off) of chain_coop::combine in the chains: X', w, Y'
COMBINE_SETS = ((1, 4, 4, -4, 4), (-1, -6, -6, 6, 13), (1, -8, 0, 0, 8))


def limbs(v: int):
    return [(v >> (LB * j)) & LMASK for j in range(NL)]


def from_limbs(l) -> int:
    return sum(int(x) << (LB * j) for j, x in enumerate(l))


ALL_ONES_LOW = from_limbs([LMASK] * 9 + [0])             # every low limb all-ones, top limb 0
ALL_ONES_TOP = from_limbs([LMASK] * 9 + [P_TOP - 1])     # every low limb all-ones under the largest top limb that stays below p


def extreme_values():
    """Integers below p that are extreme AS REGISTER CONTENTS, most important first."""
    v = [P - 1, 0, ALL_ONES_TOP, ALL_ONES_LOW, 1, 2, P - 2, (P - 1) // 2, (P + 1) // 2, R, R2]
    v += [from_limbs([LMASK if j % 2 == 0 else 0 for j in range(NL - 1)] + [0]),
          from_limbs([LMASK if j % 2 == 1 else 0 for j in range(NL - 1)] + [P_TOP - 1])]
    v += [LMASK << (LB * j) for j in range(NL - 1)] + [(P_TOP - 1) << (LB * (NL - 1))]   # one limb at its maximum
    v += [1 << (LB * j) for j in range(1, NL)] + [(1 << (LB * j)) - 1 for j in range(1, NL)]
    out = []
    for x in v:
        assert 0 <= x < P
        if x not in out:
            out.append(x)
    return out


def _rng(seed):
    g = synth.Xoshiro256ss(seed)
    return lambda: g.next_u256() % P


def field_rows(n_random: int = 3000, seed: int = 0x46715F31):
    """Rows (a, b, c, d) for groups 0 and 1: every pairing of the extreme list for (a, b) with (c, d) cycling through the cross
    product of a short list (so the 3x / 6p forms meet p - 1, all-ones limbs and 0 on all four operands at once), the full
    four-fold cross product of that short list, and random rows."""
    ext = extreme_values()
    short = [P - 1, ALL_ONES_TOP, ALL_ONES_LOW, 0, 1]
    cd = [(c, d) for c in short for d in short]
    rows = [(a, b, c, d) for a in short for b in short for c, d in cd]
    k = 0
    for a in ext:
        for b in ext:
            rows.append((a, b) + cd[k % len(cd)])
            k += 1
    rnd = _rng(seed)
    for i in range(n_random):
        row = [rnd(), rnd(), rnd(), rnd()]
        if i % 4 == 1:                 # a random row with one extreme operand
            row[(i >> 2) % 4] = ext[(i >> 4) % len(ext)]
        rows.append(tuple(row))
    return rows


def fq2_rows():
    """Group 1 needs x = (a, b) != 0 (fq2_inv)."""
    return [r for r in field_rows(seed=0x46715F32) if r[0] or r[1]]


# ---- combine -------------------------------------------------------------------------------------------------------------------
def combine_value(cs, s):
    k0, k1, k2, k3, off = cs
    return k0 * s[0] + k1 * s[1] + k2 * s[2] + k3 * s[3] + off * P


def combine_range(cs):
    """Smallest and largest integer the set can produce on canonical slots."""
    lo = sum(k * (P - 1) for k in cs[:4] if k < 0) + cs[4] * P
    hi = sum(k * (P - 1) for k in cs[:4] if k > 0) + cs[4] * P
    return lo, hi


def combine_targets(cs):
    """Every (k, d), d in (-1, 0, 1), with k p + d in the set's range."""
    lo, hi = combine_range(cs)
    return [(k, d) for k in range(hi // P + 2) for d in (-1, 0, 1) if lo <= k * P + d <= hi]


def _solve_combine(cs, target, rnd, draw):
    """Slots (s0 .. s3) with combine_value == target: s1 .. s3 chosen, s0 (coefficient +-1) solved."""
    k0 = cs[0]
    assert k0 in (1, -1)
    for _ in range(20000):
        s = [0, draw(), draw(), draw()]
        s0 = (target - combine_value(cs, s)) * k0
        if 0 <= s0 < P:
            s[0] = s0
            return s
    raise AssertionError("no slots for target %d of %r" % (target, cs))


def combine_rows(per_target: int = 3, seed: int = 0x46715F33):
    """Rows of four slots and the (set, k, d) each was made for: the integer value of set `set` is exactly k p + d.  Also the
    smallest and largest value of every set."""
    rnd = _rng(seed)
    g = synth.Xoshiro256ss(seed + 1)

    def draw():
        m = g.next_u64() % 4
        return 0 if m == 0 else P - 1 if m == 1 else rnd()

    rows, tags = [], []
    for ci, cs in enumerate(COMBINE_SETS):
        for k, d in combine_targets(cs):
            for _ in range(per_target):
                rows.append(_solve_combine(cs, k * P + d, rnd, draw))
                tags.append((ci, k, d))
        lo, hi = combine_range(cs)
        for tgt in (lo, hi):
            s = [(P - 1) if (kk < 0) == (tgt == lo) and kk != 0 else 0 for kk in cs[:4]]
            assert combine_value(cs, s) == tgt
            rows.append(s)
            tags.append((ci, tgt // P, tgt - (tgt // P) * P))
    return rows, tags


def coop_rows(n_random: int = 2500):
    """Rows e0 .. e7 of group 2 and the combine tags (None for rows not made for combine)."""
    crow, ctag = combine_rows()
    rnd = _rng(0x46715F34)
    rows, tags = [], []
    for s, t in zip(crow, ctag):
        rows.append(tuple(s) + (rnd(), rnd(), rnd(), rnd()))
        tags.append(t)
    f = field_rows(n_random=n_random, seed=0x46715F35)
    short = [P - 1, ALL_ONES_TOP, ALL_ONES_LOW, 0, 1]
    for i, r in enumerate(f):          # e4 .. e7: extreme together with e0 .. e3 on the crafted rows, random otherwise
        if i < len(short) ** 4:
            tail = (r[2], r[3], r[0], r[1]) if i % 2 else (r[0], r[1], r[2], r[3])
        else:
            tail = (rnd(), rnd(), rnd(), rnd())
        rows.append(tuple(r) + tail)
        tags.append(None)
    for v in short:                    # all eight operands at the same extreme
        rows.append((v,) * 8)
        tags.append(None)
    return rows, tags


# ---- expectations (Python integers) ----------------------------------------------------------------------------------------------
def expect_fq(row):
    a, b, c, d = row
    m = lambda v: v * RI % P
    return [(a + b) % P, (a - b) % P, -a % P, 2 * a % P, m(a * b), m(a * a), m(a * b + c * d), m(a * R2), m(a),
            m((a + b) ** 2), m(9 * a * a), m(3 * a * b), m((a + b) * (c - d)), m((a + b + c + d) * (a + b - c - d)),
            m(9 * (a + b) * (a - b)), m(3 * a * b - 3 * c * d), m(9 * a * b - 9 * c * d)]


def expect_fq2(row):
    a, b, c, d = row
    m = lambda v: v * RI % P
    inv = synth.f2_inv((m(a), m(b)))   # on the field elements the residues stand for, then back to a residue
    return [m(a * c - b * d), m(a * d + b * c), m(3 * (a * c - b * d)), m(3 * (a * d + b * c)),
            m((a + b) * (a - b)), m(2 * a * b),
            m((a + c + b + d) * (a + c - b - d)), m(2 * (a + c) * (b + d)),
            m(9 * (a + b) * (a - b)), m(18 * a * b),
            m(a * a + b * b), -a % P, -b % P, inv[0] * R % P, inv[1] * R % P]


def expect_coop(row):
    e = row
    m = lambda v: v * RI % P
    out = []
    for fa, ga, fb, gb in PRODUCT_TUPLES:
        out.append(m((fa * e[0] + ga * e[1]) * (fb * e[2] + gb * e[3])))
    for fa, ga, fb, gb in PRODUCT_TUPLES:
        a0, a1 = fa * e[0] + ga * e[2], fa * e[1] + ga * e[3]
        b0, b1 = fb * e[4] + gb * e[6], fb * e[5] + gb * e[7]
        out += [m(a0 * b0 - a1 * b1), m(a0 * b1 + a1 * b0), m(a0 * b0 + a1 * b1)]
    for cs in COMBINE_SETS:
        s = (e[0], e[1], e[2], e[3]) if cs[2] else (e[0], e[1], e[1], e[1])
        out.append(combine_value(cs, s) % P)
    return out


# ---- curve rows ------------------------------------------------------------------------------------------------------------------
def _mont(v):
    return v * R % P


def _g1_jac(pt, z):
    """Affine point under Jacobian z, as raw residues (X, Y, Z)."""
    return [_mont(pt[0] * z * z % P), _mont(pt[1] * z * z * z % P), _mont(z)]


def _g2_jac(pt, z):
    z2 = synth.f2_mul(z, z)
    x, y = synth.f2_mul(pt[0], z2), synth.f2_mul(pt[1], synth.f2_mul(z2, z))
    return [_mont(x[0]), _mont(x[1]), _mont(y[0]), _mont(y[1]), _mont(z[0]), _mont(z[1])]


def curve_rows(n: int = 48, seed: int = 0x46715F36):
    """Rows of group 3 with what to expect: (row, kind) with kind 0 = distinct points (affine sum), 1 = the same point under two
    different Z (doubling), 2 = P and -P under different Z.  Z is random or a value whose RESIDUE is extreme (never 0 or the
    residue of 1).  `points` holds the affine (g1 P, g1 Q, g2 P, g2 Q) of each row."""
    rnd = _rng(seed)
    ext =[v * RI % P for v in (P - 1, ALL_ONES_TOP, ALL_ONES_LOW, 2, 1, (P - 1) // 2)]   # Z whose register content is extreme

    def z1(i, j):
        return ext[(i + 3 * j) % len(ext)] if (i + j) % 3 == 0 else rnd() or 1

    rows, kinds, points = [], [], []
    for i in range(n):
        kind = (0, 0, 0, 1, 0, 2)[i % 6]
        ks = [rnd() % 65535 + 2 for _ in range(4)]   # short scalars: the coordinates are full-size field elements all the same
        # (the scalars of P and Q differ and stay far below the group order: Q is neither P nor -P)
        p1, q1 = synth.g1_mul(ks[0], synth.G1_GEN), synth.g1_mul(ks[0] + 1 + ks[1], synth.G1_GEN)
        p2, q2 = synth.g2_mul(ks[2], synth.G2_GEN), synth.g2_mul(ks[2] + 1 + ks[3], synth.G2_GEN)
        if kind == 1:
            q1, q2 = p1, p2
        elif kind == 2:
            q1, q2 = (p1[0], -p1[1] % P), (p2[0], synth.f2_sub((0, 0), p2[1]))
        za, zb = z1(i, 0), z1(i, 1)
        if za == zb:
            zb = (zb + 1) % P or 1
        zc = (z1(i, 2), rnd() if i % 2 else 0)
        zd = (rnd() if i % 4 < 2 else 0, z1(i, 3))
        assert za and zb and zc != (0, 0) and zd != (0, 0) and zc != zd
        rows.append(_g1_jac(p1, za) + _g1_jac(q1, zb) + _g2_jac(p2, zc) + _g2_jac(q2, zd))
        kinds.append(kind)
        points.append((p1, q1, p2, q2))
    return rows, kinds, points


def g1_affine_from_raw(x, y, z):
    """Raw Jacobian residues -> affine integers."""
    x, y, z = x * RI % P, y * RI % P, z * RI % P
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def g2_affine_from_raw(w):
    x, y, z = [(w[2 * k] * RI % P, w[2 * k + 1] * RI % P) for k in range(3)]
    zi = synth.f2_inv(z)
    zi2 = synth.f2_mul(zi, zi)
    return (synth.f2_mul(x, zi2), synth.f2_mul(y, synth.f2_mul(zi2, zi)))


# ---- what the tables claim to hold ------------------------------------------------------------------------------------------------
def check_tables(frows, crows, ctags):
    """Asserts that the tables really contain their extremes, so that a change of the generators cannot thin them silently."""
    ones = lambda v: limbs(v)[:NL - 1] == [LMASK] * (NL - 1)
    ext = extreme_values()
    assert ones(ALL_ONES_TOP) and ones(ALL_ONES_LOW) and limbs(ALL_ONES_TOP)[NL - 1] == 0xc1912 and ALL_ONES_TOP < P
    assert any(all(ones(v) for v in r) for r in frows), "no row with all-ones low limbs on all four operands"
    assert (P - 1,) * 4 in set(frows) and (0,) * 4 in set(frows), "no row with p - 1 (or 0) on all four operands"
    ab = {(r[0], r[1]) for r in frows}
    assert all((a, b) in ab for a in ext for b in ext), "a pairing of the extreme values is missing"
    assert {P - 1, P - 2, 0, 1, 2, (P - 1) // 2, (P + 1) // 2, R, R2, ALL_ONES_TOP, ALL_ONES_LOW} <= set(ext)
    assert all((LMASK << (LB * j)) in ext and (1 << (LB * j)) in ext and (1 << (LB * j)) - 1 in ext for j in range(1, NL - 1))
    assert 4000 <= len(frows) <= 8000 and 4000 <= len(crows) <= 8000
    assert any(all(ones(v) for v in r) for r in crows) and (P - 1,) * 8 in set(crows)
    for ci, cs in enumerate(COMBINE_SETS):
        vals = {combine_value(cs, r[:4]) for r in crows}
        lo, hi = combine_range(cs)
        assert lo in vals and hi in vals and 0 < lo and hi < 32 * P, "combine set %d: minimum or maximum missing" % ci
        for k, d in combine_targets(cs):
            assert k * P + d in vals, "combine set %d: no row with value %d p %+d" % (ci, k, d)
        assert len({k for k, d in combine_targets(cs) if d == 0}) == hi // P, "combine set %d: a multiple of p is out of reach" % ci
    for r, t in zip(crows, ctags):
        if t is not None:
            assert combine_value(COMBINE_SETS[t[0]], r[:4]) == t[1] * P + t[2]
    assert combine_range(COMBINE_SETS[1]) == (13, 19 * P - 6)


# ---- words -----------------------------------------------------------------------------------------------------------------------
def rows_to_words(rows) -> np.ndarray:
    """[[int]] -> uint64[n][4 * len(row)], little-endian words."""
    out = np.zeros((len(rows), 4 * len(rows[0])), np.uint64)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            for k in range(4):
                out[i, 4 * j + k] = (v >> (64 * k)) & synth.MASK64
    return out


def words_to_rows(w: np.ndarray):
    """uint64[n][4 m] -> [[int] * m]"""
    n, m = w.shape[0], w.shape[1] // 4
    return [[sum(int(w[i, 4 * j + k]) << (64 * k) for k in range(4)) for j in range(m)] for i in range(n)]
