"""Big-integer definitions of the field gadgets (reference src/fields/: FqTarget / Fq2Target is_square, sqrt_with_sgn, inv; sign
rule sgn.rs), written independently of the device algorithm of csrc/root_front.hip and csrc/field_gadgets.hip: the Fq root is pow(x, (p+1)/4), the Fq2
root the "complex method" for p = 3 mod 4 in Fq2 arithmetic (Adj, Rodriguez-Henriquez, "Square root computation over even
extension fields", algorithm 9), with no norm ladder and no delta.  The root with a given sign is unique (y and -y have opposite
signs for y != 0), so any correct root normalised by sign is the expectation.

  square:  the is_square gadget, Legendre symbol == 1 (of x, or of norm(x) = c0^2 + c1^2 for Fq2); 0 for x = 0
  root_ok: a y exists with y^2 = x and sgn(y) == sgn: `square` for x != 0, sgn == 0 for x = 0
  root:    that y, or zero where root_ok is 0
  inv:     x^-1, 0 for x = 0
Also the crafted input sets of tests/test_gpu_field_gadgets.py and the conversion to the ABI's words."""
import random

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
LEGENDRE_EXP = (P - 1) // 2
assert P % 4 == 3


def to_words(v: int):
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]


def from_words(w) -> int:
    return sum(int(v) << (64 * i) for i, v in enumerate(w))


# ---- Fq ---------------------------------------------------------------------------------------------------------------------
def legendre(x: int) -> int:
    """x^((p-1)/2): 0, 1 or p - 1."""
    return pow(x, LEGENDRE_EXP, P)


def fq_is_square(x: int) -> bool:
    return legendre(x) == 1


def fq_sgn(y: int) -> int:
    return y & 1


def fq_sqrt(x: int, sgn: int):
    """-> (root, square, root_ok)"""
    square = fq_is_square(x)
    if x == 0:
        return 0, False, sgn == 0
    if not square:
        return 0, False, False
    y = pow(x, (P + 1) // 4, P)
    if fq_sgn(y) != sgn:
        y = P - y
    return y, True, True


def fq_inv(x: int) -> int:
    return pow(x, P - 2, P)  # 0 for 0


# ---- Fq2 = Fq[u]/(u^2 + 1) ----------------------------------------------------------------------------------------------------
class Fq2:
    __slots__ = ("c0", "c1")

    def __init__(self, c0, c1=0):
        self.c0, self.c1 = c0 % P, c1 % P

    def __eq__(self, o):
        return self.c0 == o.c0 and self.c1 == o.c1

    def __add__(self, o):
        return Fq2(self.c0 + o.c0, self.c1 + o.c1)

    def __neg__(self):
        return Fq2(-self.c0, -self.c1)

    def __mul__(self, o):
        return Fq2(self.c0 * o.c0 - self.c1 * o.c1, self.c0 * o.c1 + self.c1 * o.c0)

    def __pow__(self, e: int):
        r, b = Fq2(1), self
        while e:
            if e & 1:
                r = r * b
            b = b * b
            e >>= 1
        return r

    def conj(self):  # the Frobenius x -> x^p
        return Fq2(self.c0, -self.c1)

    def norm(self) -> int:
        return (self.c0 * self.c0 + self.c1 * self.c1) % P

    def is_zero(self) -> bool:
        return self.c0 == 0 and self.c1 == 0

    def pair(self):
        return (self.c0, self.c1)


def fq2_is_square(x) -> bool:
    return legendre(Fq2(*x).norm()) == 1


def fq2_sgn(y) -> int:
    """sgn.rs:20-27: the parity of c0, or of c1 when c0 is zero."""
    return (y[0] & 1) if y[0] != 0 else (y[1] & 1)


def _fq2_any_root(a: Fq2):
    """A root of a != 0 by the complex method, or None."""
    a1 = a ** ((P - 3) // 4)
    alpha = a1 * a1 * a
    if alpha.conj() * alpha == Fq2(-1):
        return None
    x0 = a1 * a
    if alpha == Fq2(-1):
        return Fq2(0, 1) * x0
    return (Fq2(1) + alpha) ** ((P - 1) // 2) * x0


def fq2_sqrt(x, sgn: int):
    """x = (c0, c1) -> ((r0, r1), square, root_ok)"""
    a = Fq2(*x)
    if a.is_zero():
        return (0, 0), False, sgn == 0
    y = _fq2_any_root(a)
    square = fq2_is_square(x)
    assert (y is not None) == square
    if y is None:
        return (0, 0), False, False
    assert y * y == a
    if fq2_sgn(y.pair()) != sgn:
        y = -y
    return y.pair(), True, True


def fq2_inv(x):
    a = Fq2(*x)
    ninv = fq_inv(a.norm())
    return (a.c0 * ninv % P, (P - a.c1) * ninv % P)


# ---- ABI words ----------------------------------------------------------------------------------------------------------------
def fq_words(vals) -> np.ndarray:
    return np.array([to_words(v) for v in vals], np.uint64).reshape(-1, 4)


def fq2_words(vals) -> np.ndarray:
    return np.array([to_words(a) + to_words(b) for a, b in vals], np.uint64).reshape(-1, 8)


def fq_sqrt_words(xs, sgns):
    """xs [n,4], sgns [n] -> (roots [n,4], square [n], root_ok [n], fq_jobs [n,8]) as bn254s_fq_sqrt_batch returns them."""
    roots, square, ok, jobs = [], [], [], []
    for w, s in zip(xs, sgns):
        x = from_words(w)
        r, sq, k = fq_sqrt(x, int(s))
        roots.append(to_words(r))
        square.append(sq)
        ok.append(k)
        jobs.append(to_words(LEGENDRE_EXP) + to_words(x))
    return np.array(roots, np.uint64), np.array(square, np.uint8), np.array(ok, np.uint8), np.array(jobs, np.uint64)


def fq2_sqrt_words(xs, sgns):
    """xs [n,8], sgns [n] -> (roots [n,8], square [n], root_ok [n], fq_jobs [n,8]) as bn254s_fq2_sqrt_batch returns them."""
    roots, square, ok, jobs = [], [], [], []
    for w, s in zip(xs, sgns):
        x = (from_words(w[:4]), from_words(w[4:]))
        r, sq, k = fq2_sqrt(x, int(s))
        roots.append(to_words(r[0]) + to_words(r[1]))
        square.append(sq)
        ok.append(k)
        jobs.append(to_words(LEGENDRE_EXP) + to_words(Fq2(*x).norm()))
    return np.array(roots, np.uint64), np.array(square, np.uint8), np.array(ok, np.uint8), np.array(jobs, np.uint64)


def fq_inv_words(xs) -> np.ndarray:
    return fq_words([fq_inv(from_words(w)) for w in xs])


def fq2_inv_words(xs) -> np.ndarray:
    return fq2_words([fq2_inv((from_words(w[:4]), from_words(w[4:]))) for w in xs])


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def random_fq(n: int, seed: int):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(n)]


def random_fq2(n: int, seed: int):
    rng = random.Random(seed)
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(n)]


def random_sgns(n: int, seed: int) -> np.ndarray:
    rng = random.Random(seed ^ 0x5A5A)
    return np.array([rng.randrange(2) for _ in range(n)], np.uint8)


def smallest_non_residue() -> int:
    n = 2
    while legendre(n) != P - 1:
        n += 1
    return n


def both_signs(vals):
    """Every value with the wanted sign 0 and then 1 -> (values, sgns)."""
    return [v for v in vals for _ in (0, 1)], np.array([s for _ in vals for s in (0, 1)], np.uint8)


def crafted_fq():
    """name -> x.  The last is the square of a y whose top 64-bit word and top 26-bit limb are those of p, the largest a canonical
    value has: p minus a 180-bit number."""
    rng = random.Random(0xF1E1D)
    top = P - rng.getrandbits(180) - 2
    assert top >> 192 == P >> 192 and top >> 234 == P >> 234
    half_lo, half_hi = (P - 1) // 2, (P + 1) // 2
    return {"0": 0, "1": 1, "p-1": P - 1, "4": 4, "p-4": P - 4, "smallest non-residue": smallest_non_residue(),
            "((p-1)/2)^2": half_lo * half_lo % P, "((p+1)/2)^2": half_hi * half_hi % P, "root with the top limb at its maximum": top * top % P}


def fq2_delta_is_residue(x):
    """For a square x of Fq2 with c1 != 0: is delta = (alpha + c0)/2 a residue, alpha the residue root of the norm?  The device
    algorithm's `plus`; here only to label crafted inputs."""
    n = Fq2(*x).norm()
    alpha = pow(n, (P + 1) // 4, P)
    assert alpha * alpha % P == n and x[1] != 0
    return legendre((alpha + x[0]) * fq_inv(2) % P) == 1


def crafted_fq2():
    """name -> (c0, c1): the zero, the c1 = 0 and c0 = 0 cases, non-residue norms and both branches on delta."""
    rng = random.Random(0xF2E2D2)
    nr = smallest_non_residue()
    a, t = rng.randrange(1, P), rng.randrange(1, P)
    out = {"(0,0)": (0, 0), "(a^2,0)": (a * a % P, 0), "(n,0), n a non-residue": (nr, 0), "(n',0), n' a random non-residue": None,
           "(p-1,0)": (P - 1, 0), "(1,0)": (1, 0), "(0,1)": (0, 1)}
    while out["(n',0), n' a random non-residue"] is None:
        v = rng.randrange(1, P)
        if legendre(v) == P - 1:
            out["(n',0), n' a random non-residue"] = (v, 0)
    # (0, c1): its norm c1^2 is always a square; the two kinds are c1 a residue or not (2 c1 decides which branch the root takes)
    want = {1: "(0,c1), c1 a residue", P - 1: "(0,c1), c1 a non-residue"}
    while want:
        v = rng.randrange(1, P)
        name = want.pop(legendre(v), None)
        if name:
            out[name] = (0, v)
    out["(t,0)^2"] = (Fq2(t, 0) * Fq2(t, 0)).pair()
    out["(0,t)^2"] = (Fq2(0, t) * Fq2(0, t)).pair()
    k = 0
    while k < 3:  # non-residue norms: no root
        v = (rng.randrange(P), rng.randrange(1, P))
        if legendre(Fq2(*v).norm()) == P - 1:
            out[f"non-residue norm {k}"] = v
            k += 1
    need = {True: 2, False: 2}
    while need[True] or need[False]:
        v = (rng.randrange(P), rng.randrange(1, P))
        if not fq2_is_square(v):
            continue
        kind = fq2_delta_is_residue(v)
        if need[kind]:
            need[kind] -= 1
            out[f"delta a {'residue' if kind else 'non-residue'} {need[kind]}"] = v
    return out


def crafted_inv_fq():
    return [0, 1, P - 1, 2, (P + 1) // 2]


def crafted_inv_fq2():
    rng = random.Random(0x1F2)
    c = rng.randrange(1, P)
    return [(0, 0), (c, 0), (0, c), (1, 0), (0, 1), (P - 1, P - 1)]
