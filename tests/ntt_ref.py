"""Reference of the NTT / LDE stage at any height, for tests/test_gpu_ntt_tall.py (checked without a GPU by
tests/test_ntt_ref_cpu.py).

The transforms are the oracle's orc_ntt (oracle/ntt.hpp: a plain radix-2 FFT, pinned against an O(N^2) DFT by
tests/test_oracle_golden.py), which knows nothing of the decomposition of csrc/ntt.hip: no 2^16-point blocks, no outer pass, no
split level.  What this file adds is bookkeeping only: the leaf order of an LDE, the stored layouts of the coefficients above
2^16 rows, the test columns, and two closed forms that go through no NTT at all (Python's pow at sampled positions).

g = GL_GEN is the coset shift of the LDE domain (plonky2's MULTIPLICATIVE_GROUP_GENERATOR); coset h of the 2N-point domain is
g w_2N^h <w_N>."""
from functools import lru_cache

import numpy as np

from tests import oracle_lib
from tools.fri_ref import GL_GEN, P, bitrev, inv, root_of_unity

M16 = 1 << 16
SPLIT, COMPACT = 1, 2   # flags of Context.selftest_transforms
NOT_A_WORD = np.uint64(2**64 - 1)
# the boundary values of test_commit_values_structured_columns
EDGE = np.array([0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, P - 2**32, 2**63, 2**48, 0xFFFFFFFE00000001,
                 0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFF0000FFFF0001], dtype=np.uint64)
CONSTANTS = (P - 1, P - 2, 2**32 - 1)


# ---- transforms ---------------------------------------------------------------------------------------------------------------
def orc_ntt(oracle, a, mode, shift=0):
    """A transformed copy of a: mode 1 = ifft, 2 = coset_fft, 3 = coset_ifft (natural order in and out)."""
    a = np.array(a, dtype=np.uint64)
    oracle.orc_ntt(oracle_lib.ptr(a), a.size, mode, shift)
    return a


def coset_shift(h, log_n):
    """Shift of coset h of the 2N-point LDE domain: g, g w_2N."""
    return GL_GEN * root_of_unity(log_n + 1) % P if h else GL_GEN


def bitrev_perm(bits):
    """perm[j] = bitrev(j, bits) for all j, by doubling: bitrev_b(j) = 2 bitrev_(b-1)(j mod 2^(b-1)) + (the top bit of j)."""
    perm = np.zeros(1, np.uint32)
    for _ in range(bits):
        perm = np.concatenate([2 * perm, 2 * perm + 1])
    return perm


def coefficients(oracle, values):
    """Natural-order coefficients of the interpolant of values on <w_N>."""
    return orc_ntt(oracle, values, 1)


def lde(oracle, coeffs):
    """coeffs[N] in natural order -> the 2N values on g <w_2N> in leaf order: out[j] = P(g w_2N^bitrev(j)); coset h is then the
    lower / upper half."""
    n = coeffs.size
    log_n = n.bit_length() - 1
    nat = orc_ntt(oracle, np.concatenate([coeffs, np.zeros(n, np.uint64)]), 2, GL_GEN)
    return nat[bitrev_perm(log_n + 1)]


def quotient_interpolant(oracle, values, h):
    """Values on coset h (natural order) -> natural-order coefficients of their interpolant."""
    return orc_ntt(oracle, values, 3, coset_shift(h, values.size.bit_length() - 1))


# ---- stored layouts -----------------------------------------------------------------------------------------------------------
def _tall_to_stored(nat):
    r = nat.size // M16
    return np.ascontiguousarray(nat.reshape(M16, r).T).reshape(-1)       # [k2][k1] -> [k1][k2]


def _tall_from_stored(stored):
    r = stored.size // M16
    return np.ascontiguousarray(stored.reshape(r, M16).T).reshape(-1)


def to_stored(nat, split=False):
    """Natural-order coefficients -> the layout the provers keep them in.  Tall (R = N / 2^16): coefficient k1 + R k2 at
    k1 2^16 + k2 (the identity for R = 1); split: [Pe | Po], the even and the odd coefficients, each tall over N / 2."""
    if split:
        return np.concatenate([_tall_to_stored(nat[0::2]), _tall_to_stored(nat[1::2])])
    return _tall_to_stored(nat)


def from_stored(stored, split=False):
    if split:
        h = stored.size // 2
        nat = np.empty_like(stored)
        nat[0::2] = _tall_from_stored(stored[:h])
        nat[1::2] = _tall_from_stored(stored[h:])
        return nat
    return _tall_from_stored(stored)


def stored_position(k, log_n, split=False):
    """Where coefficient k sits in the stored layout (plain integers: the second route to the layouts above)."""
    n = 1 << log_n
    if split:
        half = n // 2
        return (k & 1) * half + stored_position(k >> 1, log_n - 1)
    r = n // M16
    return (k % r) * M16 + k // r


# ---- columns ------------------------------------------------------------------------------------------------------------------
def rand_field(rng, n):
    return rng.integers(0, P, size=n, dtype=np.uint64)


def column(log_n, j):
    """Column j of the list (kind j mod 6; j >= 6 repeats the kinds with another seed / another rotation of the edge values):
    0 structured pairs (positions i and i + N/2 run through all pairings of edge values), 1 uniform random, 2 random with 30 % of
    the positions at p - 1, 3 block-periodic (the DFT across the 2^16-row blocks sees edge values only), 4 sparse (40 edge values,
    among them positions 0, 2^16 - 1, 2^16, N - 1), 5 constant."""
    n = 1 << log_n
    kind, variant = j % 6, j // 6
    rng = np.random.default_rng(1000 * log_n + j)
    edge = np.roll(EDGE, variant)
    if kind == 0:
        i = np.arange(n // 2)
        return np.concatenate([edge[i % 15], edge[(i // 15) % 15]])
    if kind == 1:
        return rand_field(rng, n)
    if kind == 2:
        v = rand_field(rng, n)
        v[rng.random(n) < 0.3] = np.uint64(P - 1)
        return v
    if kind == 3:
        i = np.arange(n)
        return edge[(7 * (i >> 16) + (i & (M16 - 1))) % 15]
    if kind == 4:
        v = np.zeros(n, np.uint64)
        pos = [p for p in (0, M16 - 1, M16, n - 1) if p < n]
        pos += rng.integers(0, n, size=40 - len(pos)).tolist()
        v[pos] = EDGE[1:][rng.integers(0, 14, size=len(pos))]
        return v
    return np.full(n, np.uint64(CONSTANTS[variant % len(CONSTANTS)]))


def columns(log_n, js):
    return np.stack([column(log_n, j) for j in js])


# ---- closed forms (no NTT) ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _domain(log_n):
    """(w_N, w_2N, 1 / N)"""
    return root_of_unity(log_n), root_of_unity(log_n + 1), inv(1 << log_n)


def impulse_coefficient(log_n, j0, k):
    """Coefficient k of the interpolant of the value impulse v[j0] = 1: N^-1 w_N^(-j0 k)."""
    w, _, n_inv = _domain(log_n)
    return n_inv * pow(w, (-j0 * k) % (1 << log_n), P) % P


def impulse_lde_value(log_n, j0, m):
    """The same interpolant at x = g w_2N^m: N^-1 sum_k (x w_N^-j0)^k = N^-1 (y^N - 1) / (y - 1), y = x w_N^-j0 (y != 1: g is in no
    subgroup of two-power order)."""
    n = 1 << log_n
    w, w2, n_inv = _domain(log_n)
    y = GL_GEN * pow(w2, m, P) * pow(w, (-j0) % n, P) % P
    return n_inv * (pow(y, n, P) - 1) * inv(y - 1) % P


def monomial_lde_value(log_n, k0, m):
    """x^k0 at x = g w_2N^m: natural-order LDE value m of the coefficient impulse c[k0] = 1."""
    return pow(GL_GEN * pow(_domain(log_n)[1], m, P) % P, k0, P)


def leaf_to_natural(j, log_n):
    """Leaf position j of an LDE column holds natural-order value bitrev(j, log_n + 1)."""
    return bitrev(j, log_n + 1)
