"""map_to_g1 / hash_to_g1 on Python integers: the G1 twin of tools/map_to_g2_ref.py.

The reference has no map_to_g1; this is its `map_to_g2` (src/utils/hash_to_g2.rs:113-148: Shallue-van de Woestijne, Z = 1) read
over Fq on E: y^2 = x^3 + 3, the circuit one writes with FqTarget::is_square (src/fields/fq.rs:283-295), sqrt_with_sgn
(fq.rs:266-281), inv (src/fields/inv.rs), sgn (src/fields/sgn.rs:9-18) and G1Target::g_circuit (src/curves/g1.rs:43-51).  G1 has
cofactor 1: nothing is cleared, and the only STARK work is the two Legendre jobs per input, (p-1)/2 | g(x1) and (p-1)/2 | g(x2).

Constants for Z = 1: g(x) = x^3 + 3, gz = g(1) = 4, nz2 = -1/2, tv6 = -4 gz/3 = -16/3 and tv4 = sqrt(-3 gz) = sqrt(-12) as
ark-ff's Fq root for p = 3 (mod 4), (p - 12)^((p+1)/4).  That root is even, which is RFC 9380's sign condition on its c3: the map
is map_to_curve_svdw of RFC 9380 6.6.1 for BN254 G1 with Z = 1 (no published vectors are checked here).  The other root would
swap x1 and x2.
"""
from __future__ import annotations

import numpy as np

from tools import synth
from tools import map_to_g2_ref as m2g
from tools.synth import P

LEGENDRE_EXP = (P - 1) // 2
GZ = 4                                        # g(Z), Z = 1
NEG_Z_BY_2 = (P - 1) // 2                     # -1/2 (2 * (p-1)/2 = p - 1)
TV4 = pow(P - 3 * GZ, (P + 1) // 4, P)        # sqrt(-3 g(Z))
TV6 = (P - 4 * GZ) * pow(3, -1, P) % P        # -4 g(Z) / (3 Z^2)
assert TV4 * TV4 % P == P - 12 and TV4 % 2 == 0

CRAFTED = (0, 1, P - 1, 2, 3, (P + 1) // 2, (P - 1) // 2)  # 0, +-1, one input per later branch, +-1/2 (tv1 tv2 = 0)


def g(x: int) -> int:
    """Right-hand side of y^2 = x^3 + 3 (src/curves/g1.rs:43-51)."""
    return (x * x * x + 3) % P


def fq_inv(a: int) -> int:
    """src/fields/inv.rs: inv(0) = 0."""
    return pow(a, P - 2, P)


def is_square(a: int) -> bool:
    """The Legendre symbol is 1 (fq.rs:283-295).  g(x) is never zero, so the symbol is 1 or p - 1 wherever the map asks."""
    return pow(a, LEGENDRE_EXP, P) == 1


def candidates(u: int):
    """(x1, x2, x3) of hash_to_g2.rs:119-127 over Fq."""
    tv1 = u * u % P * GZ % P
    tv2 = (1 + tv1) % P
    tv1 = (1 - tv1) % P
    tv3 = fq_inv(tv1 * tv2 % P)
    tv5 = u * tv1 % P * tv3 % P * TV4 % P
    x1 = (NEG_Z_BY_2 - tv5) % P
    x2 = (NEG_Z_BY_2 + tv5) % P
    t = tv2 * tv2 % P * tv3 % P
    x3 = (1 + TV6 * (t * t % P)) % P
    return x1, x2, x3


def select_point(u: int, is_gx1_sq: bool, is_gx2_sq: bool):
    """(x, y) given the two Legendre results (hash_to_g2.rs:128-145): the first candidate with a square g, y = sqrt(g(x)) with
    the parity of u (sgn.rs:9-18)."""
    x1, x2, x3 = candidates(u)
    x = x1 if is_gx1_sq else x2 if is_gx2_sq else x3
    y = m2g.fq_sqrt(g(x))
    if y is None:
        raise ValueError("g(x) is not a square: inconsistent Legendre results")
    if (y & 1) != (u & 1):
        y = P - y  # y != 0: g is never zero
    return x, y


def map_to_g1(u: int):
    """The point of G1 for u in Fq."""
    x1, x2, _ = candidates(u)
    return select_point(u, is_square(g(x1)), is_square(g(x2)))


def branch(u: int) -> int:
    """0, 1 or 2: the candidate that map_to_g1 takes."""
    x1, x2, _ = candidates(u)
    return 0 if is_square(g(x1)) else 1 if is_square(g(x2)) else 2


def fq_exp_jobs(us):
    """The 2n Legendre jobs as an array [2n, 8] = (p-1)/2 | g(x_i); job 2k+i belongs to candidate x_{i+1} of input k."""
    jobs = np.zeros((2 * len(us), 8), np.uint64)
    for k, u in enumerate(us):
        x1, x2, _ = candidates(u)
        for i, xc in enumerate((x1, x2)):
            jobs[2 * k + i] = synth._to_words(LEGENDRE_EXP) + synth._to_words(g(xc))
    return jobs


def front_end(us):
    """(points [n,8], sq_flags [2n] uint8, fq_jobs [2n,8]) as bn254s_map_to_g1_batch returns them."""
    pts = np.zeros((len(us), 8), np.uint64)
    flags = np.zeros(2 * len(us), np.uint8)
    for k, u in enumerate(us):
        x1, x2, _ = candidates(u)
        flags[2 * k], flags[2 * k + 1] = is_square(g(x1)), is_square(g(x2))
        x, y = select_point(u, bool(flags[2 * k]), bool(flags[2 * k + 1]))
        pts[k] = synth._to_words(x) + synth._to_words(y)
    return pts, flags, fq_exp_jobs(us)


def hash_to_fq(inputs) -> int:
    """The first coordinate of hash_to_fq2 (hash_to_g2.rs:76-87): the same challenger, 16 challenges whose low 32 bits are the
    little-endian limbs of a 512-bit integer, reduced modulo p."""
    return m2g.hash_to_fq2(inputs)[0]


def inputs(n: int, seed: int = 0x706C6F6E6B7932 + 11):
    """n uniform inputs u below p."""
    rng = synth.Xoshiro256ss(seed)
    return [rng.next_u256() % P for _ in range(n)]


def to_words(us):
    return np.array([synth._to_words(u) for u in us], np.uint64).reshape(-1, 4)
