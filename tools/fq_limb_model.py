"""Limb-level model of csrc/fq_dev.h and csrc/chain_coop.h with explicit register widths, vectorised over rows with numpy.

A field element is a uint64 array [10][n] of 26-bit-limb REGISTER contents (u32 in the device code: every limb is asserted to
fit 32 bits).  Column sums are uint64 and every accumulation is checked for wrap-around; the signed carry chains of fq_add,
fq_sub, fq_cond_sub_p and chain_coop::combine are int64 here with every intermediate asserted to fit a signed 32-bit register.
A value that reaches the final conditional subtraction at 2p or more, or negative, is an error too.  Violations raise
ModelError: the model states what the code RELIES on, not what its comments say.

`faults` switches single bugs on (tests/test_fq_limb_model_cpu.py checks that the operand table catches each):
  subconst_short  FqSubConst<M> raises the low limbs by (M/2 - 1) 2^26 instead of (M/2) 2^26
  off_minus_one   combine adds (off - 1) p
  skip_cond_sub   no final conditional subtraction
  q_from_p9       combine's quotient constant is 2^40 / P9 instead of 2^40 / (P9 + 1)
  tpl_sub4        a 3x operand is fed to fq_sub_lazy<4> instead of <6>"""
from __future__ import annotations

import numpy as np

from tools.fq_operands import LB, NL, LMASK, P, limbs

U64 = np.uint64
NINV = 0x866389
P_L = limbs(P)
FAULTS = ("subconst_short", "off_minus_one", "skip_cond_sub", "q_from_p9", "tpl_sub4")


class ModelError(AssertionError):
    pass


def _check(cond, what):
    if not cond:
        raise ModelError(what)


def to_limbs(vals) -> np.ndarray:
    """[int below 2^260] -> uint64[10][n]"""
    out = np.zeros((NL, len(vals)), U64)
    for i, v in enumerate(vals):
        for j in range(NL):
            out[j, i] = (v >> (LB * j)) & LMASK
    return out


def to_ints(x: np.ndarray):
    cols = [x[j].tolist() for j in range(NL)]
    return [sum(cols[j][i] << (LB * j) for j in range(NL)) for i in range(x.shape[1])]


def sub_const(M: int, short: bool = False):
    """FqSubConst<M>::k"""
    k, c = [], 0
    for j in range(NL):
        v = M * P_L[j] + c
        k.append(v & LMASK)
        c = v >> LB
    k[NL - 1] += c << LB
    raise_by = M // 2 - 1 if short else M // 2
    for j in range(NL - 1):
        k[j] += raise_by << LB
        k[j + 1] -= raise_by
    assert sum(v << (LB * j) for j, v in enumerate(k)) == M * P
    return k


class Model:
    def __init__(self, faults=()):
        for f in faults:
            assert f in FAULTS, f
        self.faults = frozenset(faults)
        self.max_col = 0       # largest 64-bit column sum seen
        self.max_limb = 0      # largest limb of an operand handed to a product
        self.two_p = limbs(2 * P)

    # ---- register widths ----------------------------------------------------------------------------------------------------
    def _u32(self, x, what):
        _check(int(x.max()) < (1 << 32), "u32 overflow in " + what)
        return x

    def _operand(self, x):
        m = int(x.max())
        _check(m < (1 << 32), "operand limb does not fit 32 bits")
        self.max_limb = max(self.max_limb, m)

    def _acc(self, acc, add):
        s = acc + add
        _check(bool((s >= acc).all()), "64-bit column sum wrapped")
        self.max_col = max(self.max_col, int(s.max()))
        return s

    @staticmethod
    def _i32(v, what):
        _check(-(1 << 31) <= int(v.min()) and int(v.max()) < (1 << 31), "signed 32-bit overflow in " + what)
        return v

    # ---- canonical results -----------------------------------------------------------------------------------------------------
    def _below_2p(self, r):
        lt = np.zeros(r.shape[1], bool)
        eq = np.ones(r.shape[1], bool)
        for j in range(NL - 1, -1, -1):
            lt |= eq & (r[j] < U64(self.two_p[j]))
            eq &= r[j] == U64(self.two_p[j])
        return bool(lt.all())

    def cond_sub_p(self, r):
        """r: uint64[10][n], low limbs normalised, the top limb what is left"""
        _check(int(r[NL - 1].max()) < (1 << 31), "top limb does not fit (int)")
        _check(self._below_2p(r), "value of 2p or more before the conditional subtraction")
        if "skip_cond_sub" in self.faults:
            return r.copy()
        t = np.zeros(r.shape, np.int64)
        c = np.zeros(r.shape[1], np.int64)
        for j in range(NL):
            v = self._i32(r[j].astype(np.int64) - P_L[j] + c, "fq_cond_sub_p")
            t[j] = v & LMASK
            c = v >> LB
        keep = c < 0           # mask all ones: r < p
        _check(bool(((c == 0) | (c == -1)).all()), "fq_cond_sub_p: carry out is not a sign")
        return np.where(keep, r.astype(np.int64), t).astype(U64)

    def fix_negative(self, t, borrow):
        _check(bool(((borrow == 0) | (borrow == -1)).all()), "fq_fix_negative: borrow is not a sign")
        r = np.zeros(t.shape, U64)
        c = np.zeros(t.shape[1], np.int64)
        for j in range(NL):
            v = self._i32(t[j] + np.where(borrow < 0, P_L[j], 0) + c, "fq_fix_negative")
            r[j] = (v & LMASK).astype(U64)
            c = v >> LB
        return r

    def add(self, a, b):
        t = np.zeros(a.shape, np.int64)
        c = np.zeros(a.shape[1], np.int64)
        for j in range(NL):
            s = self._u32(a[j] + b[j], "fq_add").astype(np.int64)
            v = self._i32(self._i32(s, "fq_add") - P_L[j] + c, "fq_add")
            t[j] = v & LMASK
            c = v >> LB
        return self.fix_negative(t, c)

    def sub(self, a, b):
        t = np.zeros(a.shape, np.int64)
        c = np.zeros(a.shape[1], np.int64)
        for j in range(NL):
            v = self._i32(a[j].astype(np.int64) - b[j].astype(np.int64) + c, "fq_sub")
            t[j] = v & LMASK
            c = v >> LB
        return self.fix_negative(t, c)

    def neg(self, a):
        return self.sub(np.zeros_like(a), a)

    def dbl(self, a):
        return self.add(a, a)

    # ---- products ----------------------------------------------------------------------------------------------------------------
    def _mont(self, pairs):
        """fq_mul (one pair) / fq_mul2 (two pairs): operand scanning with the interleaved reduction"""
        n = pairs[0][0].shape[1]
        for x, y in pairs:
            self._operand(x)
            self._operand(y)
        acc = [np.zeros(n, U64) for _ in range(NL + 1)]
        for i in range(NL):
            for x, y in pairs:
                for j in range(NL):
                    acc[j] = self._acc(acc[j], x[j] * y[i])
            m = ((acc[0] & U64(0xFFFFFFFF)) * U64(NINV)) & U64(LMASK)
            for j in range(NL):
                acc[j] = self._acc(acc[j], m * U64(P_L[j]))
            _check(not (acc[0] & U64(LMASK)).any(), "reduction digit wrong")
            carry = acc[0] >> U64(LB)
            acc = acc[1:] + [np.zeros(n, U64)]
            acc[0] = self._acc(acc[0], carry)
        return self._finish(acc[:NL])

    def _finish(self, acc):
        r = np.zeros((NL, acc[0].shape[0]), U64)
        for j in range(NL - 1):
            acc[j + 1] = self._acc(acc[j + 1], acc[j] >> U64(LB))
            r[j] = acc[j] & U64(LMASK)
        _check(int(acc[NL - 1].max()) < (1 << 32), "top limb of a product does not fit 32 bits")
        r[NL - 1] = acc[NL - 1]
        return self.cond_sub_p(r)

    def mul(self, a, b):
        return self._mont([(a, b)])

    def mul2(self, a, b, c, d):
        return self._mont([(a, b), (c, d)])

    def sqr(self, a):
        self._operand(a)
        n = a.shape[1]
        c = [np.zeros(n, U64) for _ in range(2 * NL)]
        for i in range(NL):
            c[2 * i] = self._acc(c[2 * i], a[i] * a[i])
            d = self._u32(a[i] << U64(1), "fq_sqr doubling")
            for j in range(i + 1, NL):
                c[i + j] = self._acc(c[i + j], d * a[j])
        for i in range(NL):
            m = ((c[i] & U64(0xFFFFFFFF)) * U64(NINV)) & U64(LMASK)
            for j in range(NL):
                c[i + j] = self._acc(c[i + j], m * U64(P_L[j]))
            _check(not (c[i] & U64(LMASK)).any(), "reduction digit wrong")
            c[i + 1] = self._acc(c[i + 1], c[i] >> U64(LB))
        return self._finish(c[NL:])

    # ---- loose operands ----------------------------------------------------------------------------------------------------------
    def add_lazy(self, a, b):
        return self._u32(a + b, "fq_add_lazy")

    def dbl_lazy(self, a):
        return self.add_lazy(a, a)

    def tpl_lazy(self, a):
        return self._u32(a * U64(3), "fq_tpl_lazy")

    def sub_lazy(self, M, a, b, tripled=False):
        """tripled: b is a 3x operand (where the fault tpl_sub4 bites)"""
        if tripled:
            assert M == 6
            if "tpl_sub4" in self.faults:
                M = 4
        k = sub_const(M, "subconst_short" in self.faults)
        r = np.zeros(a.shape, U64)
        for j in range(NL):
            v = a[j].astype(np.int64) + k[j] - b[j].astype(np.int64)
            _check(int(v.min()) >= 0, "fq_sub_lazy<%d>: negative limb" % M)
            r[j] = self._u32(v.astype(U64), "fq_sub_lazy")
        return r

    # ---- Fq2 ---------------------------------------------------------------------------------------------------------------------
    def fq2_mul(self, a, b):
        nb1 = self.sub_lazy(2, np.zeros_like(b[1]), b[1])
        return self.mul2(a[0], b[0], a[1], nb1), self.mul2(a[0], b[1], a[1], b[0])

    def fq2_sqr(self, M, a, tripled=False):
        return (self.mul(self.add_lazy(a[0], a[1]), self.sub_lazy(M, a[0], a[1], tripled)), self.mul(self.dbl_lazy(a[0]), a[1]))

    def fq2_norm(self, a):
        return self.mul2(a[0], a[0], a[1], a[1])

    # ---- cooperative pieces ------------------------------------------------------------------------------------------------------
    def g1_product(self, u, v, x, y, fa, ga, fb, gb):
        A = self._u32(u * U64(fa) + v * U64(ga), "g1coop::product")
        B = self._u32(x * U64(fb) + y * U64(gb), "g1coop::product")
        return self.mul(A, B)

    def g2_product(self, c, plain, S1, S2, T1, T2, fa, ga, fb, gb):
        A0 = self._u32(S1[0] * U64(fa) + S2[0] * U64(ga), "g2coop::product")
        A1 = self._u32(S1[1] * U64(fa) + S2[1] * U64(ga), "g2coop::product")
        B0 = self._u32(T1[0] * U64(fb) + T2[0] * U64(gb), "g2coop::product")
        B1 = self._u32(T1[1] * U64(fb) + T2[1] * U64(gb), "g2coop::product")
        nB1 = self.sub_lazy(6, np.zeros_like(B1), B1, tripled=True)
        Pp = B1 if c else B0
        Q = B0 if c else (B1 if plain else nB1)
        return self.mul2(A0, Pp, A1, Q)

    def combine(self, s, ks, off):
        """Returns (canonical result, quotient estimate q, top limb before the estimate)."""
        if "off_minus_one" in self.faults:
            off -= 1
        n = s[0].shape[1]
        t = []
        for j in range(NL):
            acc = np.zeros(n, np.int64)
            for v, k in zip(s, ks):
                acc = self._i32(acc + self._i32(v[j].astype(np.int64) * k, "combine"), "combine")
            t.append(self._i32(acc + P_L[j] * off, "combine"))
        cy = np.zeros(n, np.int64)
        for j in range(NL - 1):
            v = self._i32(t[j] + cy, "combine")
            t[j] = v & LMASK
            cy = v >> LB
        t[NL - 1] = self._i32(t[NL - 1] + cy, "combine")
        _check(int(t[NL - 1].min()) >= 0, "combine: negative value")
        _check(int(t[NL - 1].max()) < (1 << 25), "combine: value of 32p or more")
        qc = (1 << 40) // (P_L[NL - 1] if "q_from_p9" in self.faults else P_L[NL - 1] + 1)
        q = (t[NL - 1] * qc) >> 40
        r = np.zeros((NL, n), U64)
        cy = np.zeros(n, np.int64)
        for j in range(NL):
            qp = q * P_L[j]
            _check(int(qp.max()) < (1 << 31), "combine: q p_j does not fit (int)")
            v = self._i32(t[j] - qp + cy, "combine")
            if j < NL - 1:
                r[j] = (v & LMASK).astype(U64)
                cy = v >> LB
            else:
                _check(int(v.min()) >= 0, "combine: quotient estimate too large")
                r[j] = v.astype(U64)
        return self.cond_sub_p(r), q, t[NL - 1]


# ---- the rows of bn254s_selftest_fq through the model (outputs in the order of the kernels, fq2_inv and group 3 left out) ------------
def _cols(rows, k):
    return [to_limbs([r[i] for r in rows]) for i in range(k)]


def _ints(outs):
    cols = [to_ints(o) for o in outs]
    return [list(r) for r in zip(*cols)]


def replay_fq(m: Model, rows):
    """Group 0 without fq_from_canonical / fq_to_canonical as such: they are fq_mul by R^2 and by 1 and are replayed as that."""
    from tools.fq_operands import R2
    a, b, c, d = _cols(rows, 4)
    n = len(rows)
    zero = np.zeros_like(a)
    a3, b3, c3, d3 = m.tpl_lazy(a), m.tpl_lazy(b), m.tpl_lazy(c), m.tpl_lazy(d)
    ab, cd = m.add_lazy(a, b), m.add_lazy(c, d)
    return _ints([
        m.add(a, b), m.sub(a, b), m.neg(a), m.dbl(a), m.mul(a, b), m.sqr(a), m.mul2(a, b, c, d),
        m.mul(a, to_limbs([R2] * n)), m.mul(a, to_limbs([1] * n)),
        m.sqr(ab), m.sqr(a3), m.mul(a3, b), m.mul(ab, m.sub_lazy(2, c, d)),
        m.mul(m.add_lazy(ab, cd), m.sub_lazy(4, ab, cd)),
        m.mul(m.add_lazy(a3, b3), m.sub_lazy(6, a3, b3, tripled=True)),
        m.mul2(a3, b, c3, m.sub_lazy(2, zero, d)),
        m.mul2(a3, b3, c3, m.sub_lazy(6, zero, d3, tripled=True))])


def replay_fq2(m: Model, rows):
    """Group 1 up to fq2_neg (13 of the 15 results; the inversion is not modelled)."""
    a, b, c, d = _cols(rows, 4)
    x, y = (a, b), (c, d)
    x3 = (m.tpl_lazy(a), m.tpl_lazy(b))
    xy = (m.add_lazy(a, c), m.add_lazy(b, d))
    outs = []
    outs += m.fq2_mul(x, y)
    outs += m.fq2_mul(x3, y)
    outs += m.fq2_sqr(2, x)
    outs += m.fq2_sqr(4, xy)
    outs += m.fq2_sqr(6, x3, tripled=True)
    outs += [m.fq2_norm(x), m.neg(a), m.neg(b)]
    return _ints(outs)


def replay_coop(m: Model, rows):
    """Group 2; also returns, per combine set, (quotient estimates, top limbs)."""
    from tools.fq_operands import COMBINE_SETS, PRODUCT_TUPLES
    e = _cols(rows, 8)
    outs = [m.g1_product(e[0], e[1], e[2], e[3], *t) for t in PRODUCT_TUPLES]
    S1, S2, T1, T2 = (e[0], e[1]), (e[2], e[3]), (e[4], e[5]), (e[6], e[7])
    for t in PRODUCT_TUPLES:
        outs += [m.g2_product(0, False, S1, S2, T1, T2, *t), m.g2_product(1, False, S1, S2, T1, T2, *t),
                 m.g2_product(0, True, S1, S2, T1, T2, *t)]
    qs = []
    for cs in COMBINE_SETS:
        s = (e[0], e[1], e[2], e[3]) if cs[2] else (e[0], e[1], e[1], e[1])
        r, q, top = m.combine(s, cs[:4], cs[4])
        outs.append(r)
        qs.append((q.tolist(), top.tolist()))
    return _ints(outs), qs
