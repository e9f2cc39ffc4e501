"""Deterministic synthetic inputs for the BN254 scalar-mul STARKs (SURVEY.md §8(d) "Synthetic inputs").

Pure-Python big-integer BN254 arithmetic: independent of both the HIP build and the C++ oracle, so it
also serves as the generator of golden vectors for the BN254 layer (tools/gen_bn254_golden.py).
Mirrors the reference's test inputs (src/starks/curves/g1/scalar_mul_stark.rs:557-566): scalar = 32
uniformly random bytes (not reduced mod r), x and offset = random non-infinity G1 points.
"""
from __future__ import annotations

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617
G1_GEN = (1, 2)
MASK64 = (1 << 64) - 1


class Xoshiro256ss:
    """xoshiro256** seeded through splitmix64 (public-domain algorithm by Blackman & Vigna)."""

    def __init__(self, seed: int):
        s = seed & MASK64
        self.s = []
        for _ in range(4):
            s = (s + 0x9E3779B97F4A7C15) & MASK64
            z = s
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
            self.s.append(z ^ (z >> 31))

    @staticmethod
    def _rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & MASK64

    def next_u64(self) -> int:
        s = self.s
        result = (self._rotl((s[1] * 5) & MASK64, 7) * 9) & MASK64
        t = (s[1] << 17) & MASK64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = self._rotl(s[3], 45)
        return result

    def next_u256(self) -> int:
        return sum(self.next_u64() << (64 * i) for i in range(4))


# ---- G1 affine / Jacobian arithmetic over Python ints -------------------------------------------------
def g1_add(a, b):
    """Affine add of non-infinity points with b != -a (textbook short-Weierstrass formulas)."""
    (x1, y1), (x2, y2) = a, b
    if x1 != x2:
        lam = (y2 - y1) * pow(x2 - x1, -1, P) % P
    else:
        if (y1 + y2) % P == 0:
            raise ValueError("point at infinity")
        lam = 3 * x1 * x1 * pow(2 * y1, -1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    y3 = (lam * (x1 - x3) - y1) % P
    return (x3, y3)


def _jac_double(p):
    x, y, z = p
    if y == 0:
        return (1, 1, 0)
    a = x * x % P
    b = y * y % P
    c = b * b % P
    d = 2 * ((x + b) * (x + b) - a - c) % P
    e = 3 * a % P
    f = e * e % P
    x3 = (f - 2 * d) % P
    y3 = (e * (d - x3) - 8 * c) % P
    z3 = 2 * y * z % P
    return (x3, y3, z3)


def _jac_add_affine(p, q):
    x1, y1, z1 = p
    x2, y2 = q
    if z1 == 0:
        return (x2, y2, 1)
    z1z1 = z1 * z1 % P
    u2 = x2 * z1z1 % P
    s2 = y2 * z1 * z1z1 % P
    if u2 == x1:
        if s2 == y1:
            return _jac_double(p)
        return (1, 1, 0)
    h = (u2 - x1) % P
    hh = h * h % P
    i = 4 * hh % P
    j = h * i % P
    r = 2 * (s2 - y1) % P
    v = x1 * i % P
    x3 = (r * r - j - 2 * v) % P
    y3 = (r * (v - x3) - 2 * y1 * j) % P
    z3 = ((z1 + h) * (z1 + h) - z1z1 - hh) % P
    return (x3, y3, z3)


def g1_mul(k: int, pt):
    """k * pt for k >= 1 (returns affine; raises on infinity)."""
    acc = (1, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jac_double(acc)
        if bit == "1":
            acc = _jac_add_affine(acc, pt)
    x, y, z = acc
    if z == 0:
        raise ValueError("point at infinity")
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def g1_scalar_mul_offset(s: int, x, offset):
    """s*x + offset as the reference computes the expected output (scalar_mul_stark.rs:105-106)."""
    k = s % R_ORDER
    if k == 0:
        return offset
    return g1_add(g1_mul(k, x), offset)


def _to_words(v: int, n: int = 4):
    return [(v >> (64 * i)) & MASK64 for i in range(n)]


def g1_inputs(n: int, seed: int = 0x706C6F6E6B7932):
    """n synthetic G1 scalar-mul jobs in ABI wire form.

    Returns (scalars[n,4], x[n,8], offset[n,8]) as uint64 numpy arrays: little-endian 64-bit words,
    canonical (non-Montgomery) coordinates, x then y.
    """
    rng = Xoshiro256ss(seed)
    scalars = np.zeros((n, 4), dtype=np.uint64)
    xs = np.zeros((n, 8), dtype=np.uint64)
    offs = np.zeros((n, 8), dtype=np.uint64)
    for i in range(n):
        s = rng.next_u256()
        k1 = rng.next_u256() % (R_ORDER - 1) + 1
        k2 = rng.next_u256() % (R_ORDER - 1) + 1
        x = g1_mul(k1, G1_GEN)
        off = g1_mul(k2, G1_GEN)
        scalars[i] = _to_words(s)
        xs[i] = _to_words(x[0]) + _to_words(x[1])
        offs[i] = _to_words(off[0]) + _to_words(off[1])
    return scalars, xs, offs


def words_to_int(w) -> int:
    return sum(int(v) << (64 * i) for i, v in enumerate(w))


# ---- g1_msm (reference src/utils/g1_msm.rs:22-36) ----------------------------------------------------------------------
def g1_msm_chain(scalars, xs, R):
    """The reference's sequential fold offset_0 = R, offset_{i+1} = s_i x_i + offset_i, msm = offset_n - R, with a Jacobian
    accumulator so that infinite partial sums pass through.  scalars [n,4] / xs [n,8] / R [8] in ABI words (or int pairs for the
    points).  Returns (offsets: n + 1 affine (x, y) int pairs, None for infinity; msm: affine pair, None for infinity)."""
    def pt(p):
        return (words_to_int(p[:4]), words_to_int(p[4:])) if len(p) == 8 else (int(p[0]), int(p[1]))

    def affine(j):
        x, y, z = j
        if z == 0:
            return None
        zi = pow(z, -1, P)
        return (x * zi * zi % P, y * zi * zi * zi % P)

    r = pt(R)
    acc = (r[0], r[1], 1)
    offsets = [r]
    for s, x in zip(scalars, xs):
        k = (words_to_int(s) if not isinstance(s, int) else s) % R_ORDER
        if k:
            acc = _jac_add_affine(acc, g1_mul(k, pt(x)))
        offsets.append(affine(acc))
    msm = affine(_jac_add_affine(acc, (r[0], (-r[1]) % P)))
    return offsets, msm


def g1_points_to_words(pts):
    """Affine int pairs -> uint64 [len, 8] ABI words."""
    return np.array([_to_words(p[0]) + _to_words(p[1]) for p in pts], dtype=np.uint64).reshape(-1, 8)


# ---- Fq2 = Fq[u]/(u^2+1) and G2 (y^2 = x^3 + b2) over Python ints ---------------------------------------
G2_B = (19485874751759354771024239261021720505790618469301721065564631296452457478373,
        266929791119991161246907387137283842545076965332900288569378510910307636690)   # src/curves/g2.rs:29-36
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    n = pow((a[0] * a[0] + a[1] * a[1]) % P, -1, P)
    return (a[0] * n % P, (-a[1]) * n % P)


def g2_add(a, b):
    """Affine add on the twist (textbook formulas), b != -a."""
    (x1, y1), (x2, y2) = a, b
    if x1 != x2:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    else:
        if f2_add(y1, y2) == (0, 0):
            raise ValueError("point at infinity")
        lam = f2_mul(f2_mul((3, 0), f2_mul(x1, x1)), f2_inv(f2_mul((2, 0), y1)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), x1), x2)
    y3 = f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1)
    return (x3, y3)


def g2_mul(k: int, pt):
    """k * pt (k >= 1) by affine double-and-add; raises on infinity."""
    acc = None
    for bit in bin(k)[2:]:
        if acc is not None:
            acc = g2_add(acc, acc)
        if bit == "1":
            acc = pt if acc is None else g2_add(acc, pt)
    return acc


def g2_scalar_mul_offset(s: int, x, offset):
    k = s % R_ORDER
    if k == 0:
        return offset
    return g2_add(g2_mul(k, x), offset)


def g2_inputs(n: int, seed: int = 0x706C6F6E6B7932 + 3):
    """(scalars[n,4], x[n,16], offset[n,16]); point = x.c0, x.c1, y.c0, y.c1 (4 words each)."""
    rng = Xoshiro256ss(seed)
    scalars = np.zeros((n, 4), dtype=np.uint64)
    xs = np.zeros((n, 16), dtype=np.uint64)
    offs = np.zeros((n, 16), dtype=np.uint64)
    for i in range(n):
        s = rng.next_u256()
        k1 = rng.next_u256() % (R_ORDER - 1) + 1
        k2 = rng.next_u256() % (R_ORDER - 1) + 1
        x = g2_mul(k1, G2_GEN)
        off = g2_mul(k2, G2_GEN)
        scalars[i] = _to_words(s)
        xs[i] = _to_words(x[0][0]) + _to_words(x[0][1]) + _to_words(x[1][0]) + _to_words(x[1][1])
        offs[i] = _to_words(off[0][0]) + _to_words(off[0][1]) + _to_words(off[1][0]) + _to_words(off[1][1])
    return scalars, xs, offs


def g2_from_words(w):
    return ((words_to_int(w[0:4]), words_to_int(w[4:8])), (words_to_int(w[8:12]), words_to_int(w[12:16])))


# ---- g2_msm: the g1_msm circuit (src/utils/g1_msm.rs:22-36) with the G2 gadgets --------------------------------------------
def _f2j_double(p):
    """2 p in Jacobian coordinates over Fq2 (the formulas of _jac_double); (1, 1, 0) = infinity."""
    x, y, z = p
    if z == (0, 0) or y == (0, 0):
        return ((1, 0), (1, 0), (0, 0))
    a = f2_mul(x, x)
    b = f2_mul(y, y)
    c = f2_mul(b, b)
    xb = f2_add(x, b)
    d = f2_sub(f2_sub(f2_mul(xb, xb), a), c)
    d = f2_add(d, d)
    e = f2_add(f2_add(a, a), a)
    x3 = f2_sub(f2_mul(e, e), f2_add(d, d))
    c8 = ((8 * c[0]) % P, (8 * c[1]) % P)
    y3 = f2_sub(f2_mul(e, f2_sub(d, x3)), c8)
    z3 = f2_mul(f2_add(y, y), z)
    return (x3, y3, z3)


def _f2j_add_affine(p, q):
    """p (Jacobian over Fq2) + q (affine, not infinity), complete: doubles equal points, gives infinity for opposite ones."""
    x1, y1, z1 = p
    x2, y2 = q
    if z1 == (0, 0):
        return (x2, y2, (1, 0))
    z1z1 = f2_mul(z1, z1)
    u2 = f2_mul(x2, z1z1)
    s2 = f2_mul(y2, f2_mul(z1, z1z1))
    if u2 == x1:
        if s2 == y1:
            return _f2j_double(p)
        return ((1, 0), (1, 0), (0, 0))
    h = f2_sub(u2, x1)
    hh = f2_mul(h, h)
    hhh = f2_mul(h, hh)
    r = f2_sub(s2, y1)
    v = f2_mul(x1, hh)
    x3 = f2_sub(f2_sub(f2_mul(r, r), hhh), f2_add(v, v))
    y3 = f2_sub(f2_mul(r, f2_sub(v, x3)), f2_mul(y1, hhh))
    z3 = f2_mul(z1, h)
    return (x3, y3, z3)


def _f2j_affine(j):
    x, y, z = j
    if z == (0, 0):
        return None
    zi = f2_inv(z)
    zi2 = f2_mul(zi, zi)
    return (f2_mul(x, zi2), f2_mul(y, f2_mul(zi2, zi)))


def g2_mul_unreduced(k: int, pt):
    """k * pt by Jacobian double-and-add over every bit of k, NOT reduced mod r (pt may lie outside the r-torsion subgroup, where
    k pt != (k mod r) pt); affine result, None for infinity."""
    acc = ((1, 0), (1, 0), (0, 0))
    for bit in bin(k)[2:] if k else "":
        acc = _f2j_double(acc)
        if bit == "1":
            acc = _f2j_add_affine(acc, pt)
    return _f2j_affine(acc)


def g2_msm_chain(scalars, xs, R):
    """The g2_msm fold offset_0 = R, offset_{i+1} = s_i x_i + offset_i, msm = offset_n - R (the G2 twin of g1_msm_chain), with a
    Jacobian Fq2 accumulator so that infinite partial sums pass through and the products over the unreduced 256-bit s_i, as the
    G2 trace computes them.  scalars [n,4] (or ints) / xs [n,16] / R [16] in ABI words (or ((x0, x1), (y0, y1)) points).
    Returns (offsets: n + 1 affine points, None for infinity; msm: affine point, None for infinity)."""
    def pt(p):
        return g2_from_words(p) if len(p) == 16 else ((int(p[0][0]), int(p[0][1])), (int(p[1][0]), int(p[1][1])))

    r = pt(R)
    acc = (r[0], r[1], (1, 0))
    offsets = [r]
    for s, x in zip(scalars, xs):
        k = words_to_int(s) if not isinstance(s, int) else s
        prod = g2_mul_unreduced(k, pt(x))
        if prod is not None:
            acc = _f2j_add_affine(acc, prod)
        offsets.append(_f2j_affine(acc))
    msm = _f2j_affine(_f2j_add_affine(acc, (r[0], ((-r[1][0]) % P, (-r[1][1]) % P))))
    return offsets, msm


def g2_points_to_words(pts):
    """Affine ((x0, x1), (y0, y1)) points -> uint64 [len, 16] ABI words (x.c0, x.c1, y.c0, y.c1)."""
    return np.array([_to_words(p[0][0]) + _to_words(p[0][1]) + _to_words(p[1][0]) + _to_words(p[1][1]) for p in pts],
                    dtype=np.uint64).reshape(-1, 16)


def fq_inputs(n: int, seed: int = 0x706C6F6E6B7932 + 5):
    """(scalars[n,4], x[n,4]) for the Fq exponentiation STARK: x uniform in [0,p), s any 256-bit value."""
    rng = Xoshiro256ss(seed)
    scalars = np.zeros((n, 4), dtype=np.uint64)
    xs = np.zeros((n, 4), dtype=np.uint64)
    for i in range(n):
        scalars[i] = _to_words(rng.next_u256())
        xs[i] = _to_words(rng.next_u256() % P)
    return scalars, xs


# ---- G1 point recovery from x (reference src/fields/recover.rs, src/curves/g1.rs:76-95) ----------------------------------
def g1_recover_from_x(x: int):
    """(x, y) with y^2 = x^3 + 3 and y even ("sgn false", recover_from_x), or None when x^3 + 3 is not a square
    (is_recoverable_from_x).  p = 3 (mod 4): the root of a square g is g^((p+1)/4)."""
    g = (x * x * x + 3) % P
    y = pow(g, (P + 1) // 4, P)
    if y * y % P != g:
        return None
    return (x, P - y if y & 1 else y)


def g1_recover_inputs(n: int, seed: int):
    """xs[n,4] for G1 point recovery: the edge cases 0, 1, 2, 4, p - 1, p - 2 and the x of three g1_inputs points first, then
    uniform values below p."""
    _, pts, _ = g1_inputs(3, seed)
    vals = [0, 1, 2, 4, P - 1, P - 2] + [words_to_int(p[:4]) for p in pts]
    rng = Xoshiro256ss(seed)
    while len(vals) < n:
        vals.append(rng.next_u256() % P)
    return np.array([_to_words(v) for v in vals[:n]], dtype=np.uint64).reshape(-1, 4)


# ---- G2 point recovery from x (reference src/curves/g2.rs:42-54, src/fields/fq2.rs:209-241, src/fields/sgn.rs:20-27) -------
def g2_rhs(x):
    """x^3 + b' on the twist (G2Target::g_circuit)."""
    return f2_add(f2_mul(f2_mul(x, x), x), G2_B)


def f2_sgn(a) -> bool:
    """src/fields/sgn.rs:20-27: parity of c0, or of c1 when c0 = 0."""
    return bool(a[0] & 1) or (a[0] == 0 and bool(a[1] & 1))


def g2_recover_from_x(x, sgn):
    """(x, y) with y^2 = x^3 + b' in Fq2 and f2_sgn(y) == sgn (sqrt_with_sgn), or None when x^3 + b' is not a square
    (is_square: the Legendre symbol of its norm).  The root is ark-ff's QuadExtField::sqrt (complex method, in ark's order of
    cases: tools/map_to_g2_ref.py f2_sqrt), negated when its sign is not the wanted one."""
    from tools import map_to_g2_ref

    y = map_to_g2_ref.f2_sqrt(g2_rhs(x))
    if y is None:
        return None
    if f2_sgn(y) != bool(sgn):
        y = ((-y[0]) % P, (-y[1]) % P)
    return (x, y)


def _g2_recover_real_g(c: int):
    """x = (sqrt((c^3 - b'.c1)/(3c)), c): the imaginary part 3 x0^2 c - c^3 + b'.c1 of x^3 + b' vanishes."""
    s = (c ** 3 - G2_B[1]) * pow(3 * c, -1, P) % P
    x0 = pow(s, (P + 1) // 4, P)
    assert x0 * x0 % P == s, "no such x for this c"
    return (x0, c)


def g2_recover_inputs(n: int, seed: int):
    """(xs[n,8], sgns[n]) for G2 point recovery: the edge cases (0,0), (1,0), (0,1), (p-1,p-1) with sgn 0, the two x with a real
    x^3 + b' (c = 2: a square of Fq, root (t, 0); c = 7: a non-square, root (0, t)) with sgn 0 and 1, the x of three g2_inputs
    points with the sign of their y and again with the opposite sign, then uniform (x, sgn) pairs."""
    _, pts, _ = g2_inputs(3, seed)
    known = [g2_from_words(w) for w in pts]
    cases = [((0, 0), 0), ((1, 0), 0), ((0, 1), 0), ((P - 1, P - 1), 0), (_g2_recover_real_g(2), 0), (_g2_recover_real_g(7), 1)]
    cases += [(x, int(f2_sgn(y))) for x, y in known] + [(x, 1 - int(f2_sgn(y))) for x, y in known]
    rng = Xoshiro256ss(seed)
    while len(cases) < n:
        x = (rng.next_u256() % P, rng.next_u256() % P)
        cases.append((x, rng.next_u256() & 1))
    cases = cases[:n]
    xs = np.array([_to_words(x[0]) + _to_words(x[1]) for x, _ in cases], dtype=np.uint64).reshape(-1, 8)
    return xs, np.array([s for _, s in cases], dtype=np.uint8)


# ---- G2 subgroup membership: [r]P = O, and the untwist-Frobenius-twist endomorphism psi ------------------------------------
X0 = 4965661367192848881                     # the BN parameter: p = 36 x0^4 + 36 x0^3 + 24 x0^2 + 6 x0 + 1
G2_COFACTOR = 2 * P - R_ORDER                # #E'(Fq2) = r (2p - r)
G2_COFACTOR_PRIMES = (10069, 5864401, 1875725156269, 197620364512881247228717050342013327560683201906968909)
XI = (9, 1)                                  # the twist is y^2 = x^3 + 3/xi


def f2_conj(a):
    return (a[0], (-a[1]) % P)


def f2_pow(a, e: int):
    r = (1, 0)
    for bit in bin(e)[2:] if e else "":
        r = f2_mul(r, r)
        if bit == "1":
            r = f2_mul(r, a)
    return r


PSI_X = f2_pow(XI, (P - 1) // 3)             # psi(x, y) = (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))
PSI_Y = f2_pow(XI, (P - 1) // 2)


def g2_neg(pt):
    return None if pt is None else (pt[0], ((-pt[1][0]) % P, (-pt[1][1]) % P))


def g2_add_complete(a, b):
    """a + b for affine points of the twist with None as the point at infinity: equal points double, opposite ones give None."""
    if a is None:
        return b
    if b is None:
        return a
    return _f2j_affine(_f2j_add_affine((a[0], a[1], (1, 0)), b))


def g2_on_curve(pt) -> bool:
    return f2_mul(pt[1], pt[1]) == g2_rhs(pt[0])


def g2_in_subgroup(pt) -> bool:
    """The definition: [r] pt is the point at infinity (pt on the twist curve, any order)."""
    return g2_mul_unreduced(R_ORDER, pt) is None


def psi(pt):
    """The endomorphism twist^-1 o Frobenius_p o twist of E'; None (infinity) stays None.  It satisfies psi^2 - t psi + p = 0 with
    t = 6 x0^2 + 1, and acts on the r-torsion subgroup of E'(Fq2) as multiplication by p."""
    if pt is None:
        return None
    return (f2_mul(f2_conj(pt[0]), PSI_X), f2_mul(f2_conj(pt[1]), PSI_Y))


def g2_in_subgroup_psi(pt) -> bool:
    """The endomorphism criterion (El Housni, Guillevic, Piellard: "Co-factor clearing and subgroup membership testing on
    pairing-friendly curves"): [x0 + 1]P + psi([x0]P) + psi^2([x0]P) == psi^3([2 x0]P), one 63-bit scalar multiplication."""
    q = g2_mul_unreduced(X0, pt)
    lhs = g2_add_complete(g2_add_complete(g2_add_complete(q, pt), psi(q)), psi(psi(q)))
    return lhs == psi(psi(psi(g2_add_complete(q, q))))


def _g2_random_twist_point(rng):
    """A uniform-looking point of E'(Fq2) (almost never in the r-torsion subgroup): g2_recover_from_x of random x until one is
    the x of a point."""
    while True:
        x = (rng.next_u256() % P, rng.next_u256() % P)
        pt = g2_recover_from_x(x, rng.next_u64() & 1)
        if pt is not None:
            return pt


G2_SUBGROUP_CLASSES = ("generator multiple", "random twist point", "cofactor-cleared", "prime order f", "order 10069 * 5864401",
                       "member + order 10069", "negated member")


def g2_subgroup_inputs(n: int, seed: int, with_classes: bool = False):
    """(points[n,16], flags[n]) for the G2 subgroup check; input i is of class i % 7 of G2_SUBGROUP_CLASSES:
    k G2_GEN; a random twist point; [h]T; [r h / f]T of prime order f (the four primes of the cofactor h in turn); a point of
    order 10069 * 5864401; a member plus a point of order 10069; the negation of a member.  Prefix-stable in n.  With
    with_classes also the list of (class index, order of the cofactor part) per input."""
    rng = Xoshiro256ss(seed)
    h, primes = G2_COFACTOR, G2_COFACTOR_PRIMES

    def of_order(d):
        """A point of exact order d (a divisor of h made of distinct primes of h)."""
        while True:
            q = g2_mul_unreduced(R_ORDER * h // d, _g2_random_twist_point(rng))
            if q is not None and all(g2_mul_unreduced(d // f, q) is not None for f in primes if d % f == 0):
                return q

    def member():
        return g2_mul(rng.next_u256() % (R_ORDER - 1) + 1, G2_GEN)

    pts, flags, classes, turn = [], [], [], 0
    for i in range(n):
        c, d = i % 7, 1
        if c == 0:
            pt = member()
        elif c == 1:
            pt = _g2_random_twist_point(rng)
            d = 0  # (unknown)
        elif c == 2:
            pt = None
            while pt is None:
                pt = g2_mul_unreduced(h, _g2_random_twist_point(rng))
        elif c == 3:
            d = primes[turn % 4]
            turn += 1
            pt = of_order(d)
        elif c == 4:
            d = primes[0] * primes[1]
            pt = of_order(d)
        elif c == 5:
            d = primes[0]
            pt = g2_add(member(), of_order(d))
        else:
            pt = g2_neg(member())
        pts.append(pt)
        flags.append(1 if c in (0, 2, 6) else 0)
        classes.append((c, d))
    out = (g2_points_to_words(pts), np.array(flags, dtype=np.uint8))
    return out + (classes,) if with_classes else out


# ---- G2 cofactor clearing: P -> [h]P, h = 2p - r -------------------------------------------------------------------------
def g2_clear_cofactor(pt):
    """The definition: [h] pt over every bit of h = 2p - r (pt on the twist curve, any order); None for infinity."""
    return g2_mul_unreduced(G2_COFACTOR, pt)


def g2_clear_cofactor_psi(pt):
    """The form csrc/g2_cofactor.hip uses: h = p - 1 + t and [p] = [t] psi - psi^2 (psi^2 - t psi + p = 0, t = 6 x0^2 + 1) give
    [h]P = T + psi(T + P) - psi^2(P) with T = [6 x0^2]P = [6 x0]([x0]P): two short scalar multiplications, affine complete
    additions, no use of h."""
    t = g2_mul_unreduced(6 * X0, g2_mul_unreduced(X0, pt))
    s = g2_add_complete(t, psi(g2_add_complete(t, pt)))
    return g2_add_complete(s, g2_neg(psi(psi(pt))))
