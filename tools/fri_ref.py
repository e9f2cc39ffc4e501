"""Plain reference of the openings / FRI stage and of the un-reduced accumulators, on Python integers only.

Everything here is written from the DEFINITION of the operation (a sum of products mod p, a polynomial evaluated at a point, the
interpolant of a coset evaluated at beta), not from the way csrc/fri.hip and csrc/quotient_common.h decompose it: no 22-bit limbs,
no power tables per lane, no butterflies, no shared inversion.  tests/test_gpu_fri_kernels.py compares the kernels with it word
for word through the debug entry points of csrc/fri_selftest.hip; tests/test_fri_ref_cpu.py checks it by a second route without a
GPU.  The one exception is acc3_limb_model at the end: that IS the decomposition of Acc3, with explicit 64-bit columns, and exists
to pin the documented capacity of the accumulator.

Field: Goldilocks p = 2^64 - 2^32 + 1 and F2 = F_p[X] / (X^2 - 7); an extension element is a pair (c0, c1).
"""
from operator import mul

P = 2**64 - 2**32 + 1
GL_GEN = 0xc65c18b67785d900        # multiplicative generator = coset shift of the LDE domain
GL_POW2_GEN = 0x64fdd1a46201e246   # element of order 2^32
W = 7                              # X^2 = 7


def root_of_unity(k):
    """A primitive 2^k-th root of unity, the one the library uses (w_(2^k) = GL_POW2_GEN^(2^(32 - k)))."""
    assert 0 <= k <= 32
    return pow(GL_POW2_GEN, 1 << (32 - k), P)


def inv(a):
    """1 / a mod p with inv(0) := 0."""
    return pow(a, P - 2, P)


def bitrev(x, bits):
    r = 0
    for i in range(bits):
        r |= ((x >> i) & 1) << (bits - 1 - i)
    return r


# ---- F2 ---------------------------------------------------------------------------------------------------------------------
def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + W * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_scale(a, s):
    return (a[0] * s % P, a[1] * s % P)


def e_inv(a):
    """1 / a in F2 with e_inv(0) := (0, 0): conj(a) / (a conj(a))."""
    n = inv((a[0] * a[0] - W * a[1] * a[1]) % P)
    return (a[0] * n % P, (P - a[1]) * n % P)


def e_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e_mul(r, a)
        a = e_mul(a, a)
        e >>= 1
    return r


def e_powers(z, n):
    """(c0 list, c1 list) of z^0 .. z^(n-1), z^0 = 1 also for z = 0."""
    c0, c1 = [0] * n, [0] * n
    if z[1] == 0:   # a base-field point stays in the base field
        x, zz = 1, z[0]
        for k in range(n):
            c0[k] = x
            x = x * zz % P
        return c0, c1
    a0, a1, z0, z1 = 1, 0, z[0], z[1]
    for k in range(n):   # (e_mul written out: this loop builds tables of 2^18 powers)
        c0[k] = a0
        c1[k] = a1
        a0, a1 = (a0 * z0 + W * a1 * z1) % P, (a0 * z1 + a1 * z0) % P
    return c0, c1


def dot(a, b):
    """sum a_k b_k mod p of two equally long integer sequences.  A constant a (a polynomial with all coefficients equal) has its
    common factor taken out of the same sum."""
    assert len(a) == len(b)
    if len(a) > 1 and a.count(a[0]) == len(a):
        return a[0] * sum(b) % P
    return sum(map(mul, a, b)) % P


def e_dot(coeffs, pw):
    """sum_k coeffs[k] * pw[k] for base-field coeffs and extension pw = (c0 list, c1 list)."""
    return (dot(coeffs, pw[0]), dot(coeffs, pw[1]) if any(pw[1]) else 0)


# ---- operands ---------------------------------------------------------------------------------------------------------------
def extreme_words():
    """Canonical words with extreme limbs: 2^64 - 1 - 2^k, k = 32 .. 63 (every 22-bit limb full but for one bit), and the edges
    of the reductions."""
    ws = [2**64 - 1 - 2**k for k in range(32, 64)]
    ws += [P - 1, 0, 1, 2**32 + 1, 2**32 - 1, 2**32, P - 2**32, 2**44 - 1, 2**22 - 1, 2**44, 2**22]
    assert P - 2 == ws[0]   # (p - 2 is the first of them)
    assert all(0 <= w < P for w in ws) and len(set(ws)) == len(ws)
    return ws


WORST = 2**64 - 1 - 2**32   # the largest canonical word with all three limbs (nearly) full


def operand_words(rng, n, random_share=4):
    """n canonical words: the extreme words in an order drawn from rng, every `random_share`-th one random."""
    ext = extreme_words()
    pick = rng.integers(0, len(ext), size=n).tolist()
    rnd = rng.integers(0, P, size=n, dtype="uint64").tolist()
    return [rnd[k] if k % random_share == random_share - 1 else ext[pick[k]] for k in range(n)]


def pairing_words(n, stride):
    """Word k = extreme word (k // stride) mod count: with stride 1 for one factor and stride = count for the other, every pair
    of extreme words meets within count^2 terms."""
    ext = extreme_words()
    return [ext[(k // stride) % len(ext)] for k in range(n)]


# ---- accumulators -----------------------------------------------------------------------------------------------------------
def acc_sum(values, weights):
    """sum_t values[t] weights[t] mod p: what both Acc and Acc3 have to return."""
    return dot(values, weights)


# ---- openings ---------------------------------------------------------------------------------------------------------------
# A polynomial of N = R * M coefficients is stored transposed: coefficient k1 + R k2 (k1 < R, k2 < M) at position k1 M + k2.
# The library has M = 2^16; M is a parameter here so that the layout can be checked on short polynomials.
def stored_position(k, r, m):
    return (k % r) * m + k // r


def to_stored(nat, r, m):
    assert len(nat) == r * m
    out = [0] * (r * m)
    for k, c in enumerate(nat):
        out[stored_position(k, r, m)] = c
    return out


def eval_naive(nat, z):
    """P(z) = sum_k nat[k] z^k by the definition, term by term."""
    acc, zp = (0, 0), (1, 0)
    for c in nat:
        acc = e_add(acc, e_scale(zp, c))
        zp = e_mul(zp, z)
    return acc


def eval_naive_ext(coefs, z):
    """The same for extension coefficients."""
    acc, zp = (0, 0), (1, 0)
    for c in coefs:
        acc = e_add(acc, e_mul(zp, c))
        zp = e_mul(zp, z)
    return acc


def eval_stored(stored, r, m, pz):
    """P(z) = sum_k c_k z^k for a polynomial in the stored layout; pz = e_powers(z, r m).  Block k1 holds the coefficients
    k1, k1 + R, k1 + 2 R, ..., so it meets the powers pz[k1::R]."""
    acc = (0, 0)
    for k1 in range(r):
        blk = stored[k1 * m:(k1 + 1) * m]
        acc = e_add(acc, e_dot(blk, (pz[0][k1::r], pz[1][k1::r])))
    return acc


def opening_partials(stored, r, m, pz0, pz1):
    """The partial evaluations the device writes for one polynomial: per block k1 the five words {S(zeta^R).c0, .c1,
    S(zeta_next^R).c0, .c1, sum of the coefficients}, S_k1(y) = sum_k2 c_(k1 + R k2) y^k2.  pz0, pz1 = e_powers of zeta and of
    zeta_next over r m terms: (z^R)^k2 is entry R k2."""
    y0 = (pz0[0][0::r], pz0[1][0::r])
    y1 = (pz1[0][0::r], pz1[1][0::r])
    out = []
    for k1 in range(r):
        blk = stored[k1 * m:(k1 + 1) * m]
        s0, s1 = e_dot(blk, y0), e_dot(blk, y1)
        out.append([s0[0], s0[1], s1[0], s1[1], sum(blk) % P])
    return out


def recombine_openings(partials, r, zeta, zeta_next):
    """(P(zeta), P(zeta_next), P(1)) from the R partial records of one polynomial, as the prover's host code recombines them:
    P(z) = sum_k1 z^k1 S_k1(z^R), P(1) = the sum of the block sums."""
    v0, v1, s = (0, 0), (0, 0), 0
    for k1 in range(r):
        q = [int(x) for x in partials[k1]]
        v0 = e_add(v0, e_mul(e_pow(zeta, k1), (q[0], q[1])))
        v1 = e_add(v1, e_mul(e_pow(zeta_next, k1), (q[2], q[3])))
        s = (s + q[4]) % P
    return v0, v1, s


# ---- batched quotient -------------------------------------------------------------------------------------------------------
def shape_widths(w, n_rc, n_ctl):
    """(A, number of lookup columns) of the synthetic shape: per challenge ceil(n_rc / 2) helper columns and one Z, then two Z
    columns per cross-table lookup."""
    n_lookup = 2 * ((n_rc + 1) // 2 + 1)
    return n_lookup + 2 * n_ctl, n_lookup


def combine_coeffs(cols, w, n_rc, n_ctl, weights):
    """The three weighted sums of the batch, column by column.  cols: W + A + 4 lists of n words (trace | auxiliary | quotient),
    weights: W + A + 4 extension elements.  Returns comb[6][n]: f1 = sum over trace and auxiliary columns with weights 0 ..
    W + A - 1, the quotient part = sum over the four quotient columns with the weights after those, f2 = sum over the 2 n_ctl
    CTL Z columns (the last auxiliary ones) with weights 0 .. 2 n_ctl - 1; components c0, c1 each."""
    a, n_lookup = shape_widths(w, n_rc, n_ctl)
    assert len(cols) == len(weights) == w + a + 4
    n = len(cols[0])
    f1 = [[0] * n, [0] * n]
    fq = [[0] * n, [0] * n]
    f2 = [[0] * n, [0] * n]

    def add(dst, col, wt):
        for comp in range(2):
            if wt[comp]:
                s = wt[comp]
                d = dst[comp]
                for j in range(n):
                    d[j] += col[j] * s

    for c in range(w + a):
        add(f1, cols[c], weights[c])
    for c in range(4):
        add(fq, cols[w + a + c], weights[w + a + c])
    for i in range(2 * n_ctl):
        add(f2, cols[w + n_lookup + i], weights[i])
    return [[v % P for v in col] for col in (f1[0], f1[1], fq[0], fq[1], f2[0], f2[1])]


def combine_final(cl, xs, zeta, zeta_next, r0, r1, r2, alpha, w, n_rc, n_ctl):
    """out[j] = alpha^(n1 + n2) (f0 - r0) / (x - zeta) + alpha^n2 (f1 - r1) / (x - zeta_next) + (f2 - r2) / (x - 1) with
    n1 = W + A, n2 = 2 n_ctl, f1 = (cl0, cl1), f0 = f1 + (cl2, cl3), f2 = (cl4, cl5) at point j, and 1 / 0 := 0."""
    a, _ = shape_widths(w, n_rc, n_ctl)
    n1, n2 = w + a, 2 * n_ctl
    a2, a12 = e_pow(alpha, n2), e_pow(alpha, n1 + n2)
    out = []
    for j, x in enumerate(xs):
        f1 = (cl[0][j], cl[1][j])
        f0 = e_add(f1, (cl[2][j], cl[3][j]))
        f2 = (cl[4][j], cl[5][j])
        t0 = e_mul(e_sub(f0, r0), e_inv(e_sub((x, 0), zeta)))
        t1 = e_mul(e_sub(f1, r1), e_inv(e_sub((x, 0), zeta_next)))
        t2 = e_scale(e_sub(f2, r2), inv((x - 1) % P))
        out.append(e_add(e_add(e_mul(t0, a12), e_mul(t1, a2)), t2))
    return out


# ---- arity-16 fold ----------------------------------------------------------------------------------------------------------
# vals: M = 2^log_m extension values in bit-reversed order on shift * <w_M>.  Position 16 c + t holds the value at
# x0 * w_16^br4(t), x0 = shift * w_M^bitrev(c, log_m - 4): the 16 points of one coset of <w_16>.  The fold takes the unique
# polynomial of degree < 16 through those values and evaluates it at beta:
#   R(beta) = (1 / 16) sum_m (beta / x0)^m  sum_i v_i w_16^(-i m)
def fold_coset_sums(vals, log_m):
    """Per coset c the 16 inner sums D_m = sum_i v_i w_16^(-i m), m = 0 .. 15, by the direct sum (they depend on the values only)."""
    m_out = 1 << (log_m - 4)
    assert len(vals) == 16 << (log_m - 4)
    w16i = inv(root_of_unity(4))
    wp = [pow(w16i, k, P) for k in range(16)]
    out = []
    for c in range(m_out):
        v = [None] * 16
        for t in range(16):
            v[bitrev(t, 4)] = vals[16 * c + t]
        out.append([(sum(v[i][0] * wp[(i * m) % 16] for i in range(16)) % P,
                     sum(v[i][1] * wp[(i * m) % 16] for i in range(16)) % P) for m in range(16)])
    return out


def fold_from_sums(sums, log_m, shift, beta):
    m_out = 1 << (log_m - 4)
    wm = root_of_unity(log_m)
    i16 = inv(16)
    out = []
    for c in range(m_out):
        x0 = shift * pow(wm, bitrev(c, log_m - 4), P) % P
        y = e_scale(beta, inv(x0))
        acc, yp = (0, 0), (1, 0)
        for m in range(16):
            acc = e_add(acc, e_mul(yp, sums[c][m]))
            yp = e_mul(yp, y)
        out.append(e_scale(acc, i16))
    return out


def fold(vals, log_m, shift, beta):
    """2^(log_m - 4) extension values: the fold of vals at beta, in bit-reversed order on shift^16 * <w_(M / 16)>."""
    return fold_from_sums(fold_coset_sums(vals, log_m), log_m, shift, beta)


def coset_evaluations_bitrev(coefs, log_m, shift):
    """An extension polynomial (coefficient list, degree < 2^log_m) on shift * <w_M> in bit-reversed order, term by term."""
    m = 1 << log_m
    wm = root_of_unity(log_m)
    out = []
    for j in range(m):
        x = shift * pow(wm, bitrev(j, log_m), P) % P
        s0 = s1 = 0
        xp = 1
        for c in coefs:
            s0 += c[0] * xp
            s1 += c[1] * xp
            xp = xp * x % P
        out.append((s0 % P, s1 % P))
    return out


def fold_by_polynomial(coefs, log_m, shift, beta):
    """The second route to the fold: with P = sum_j X^j P_j(X^16), the folded polynomial is sum_j beta^j P_j(Y), evaluated on
    Y = x^16, i.e. on shift^16 * <w_(M / 16)> in bit-reversed order."""
    lo = log_m - 4
    assert len(coefs) <= 1 << log_m
    folded = [(0, 0)] * (1 << lo)
    for k, c in enumerate(coefs):   # coefficient k = j + 16 q goes to Y^q with the factor beta^j
        j, q = k % 16, k // 16
        folded[q] = e_add(folded[q], e_mul(e_pow(beta, j), c))
    return coset_evaluations_bitrev(folded, lo, pow(shift, 16, P))


# ---- rows -------------------------------------------------------------------------------------------------------------------
def extract_window(lde, log_n, h, k0, rows):
    """Rows k0 .. k0 + rows - 1 (mod N) of coset h of columns in leaf order (row k of coset h at h N + bitrev(k))."""
    n = 1 << log_n
    return [[col[h * n + bitrev((k0 + t) % n, log_n)] for t in range(rows)] for col in lde]


def gather_rows(lde, indices):
    return [[col[i] for i in indices] for col in lde]


# ---- the limb model of Acc3 (csrc/quotient_common.h) ------------------------------------------------------------------------------
M22 = (1 << 22) - 1


def limbs22(x):
    return (x & M22, (x >> 22) & M22, x >> 44)


def acc3_term(v, w):
    """What one term adds to the five columns: the nine limb products of value and weight by the sum of their limb indices."""
    v0, v1, v2 = limbs22(v)
    w0, w1, w2 = limbs22(w)
    return (v0 * w0, v0 * w1 + v1 * w0, v0 * w2 + v1 * w1 + v2 * w0, v1 * w2 + v2 * w1, v2 * w2)


def acc3_limb_model(values, weights, start=None):
    """(result, wrapped, largest column) of Acc3 over the terms: five columns that wrap at 2^64 as the device registers do, then
    the fold of acc3_red (columns 0..2 as one 128-bit integer, columns 3 and 4 through 2^66 and 2^88).  wrapped: a column passed
    2^64 on the way, and then the result is not the sum any more.  start: the columns to begin with (all zero by default)."""
    c = list(start) if start else [0] * 5
    assert len(c) == 5 and all(0 <= x < 2**64 for x in c)
    wrapped, largest = False, 0
    for v, w in zip(values, weights):
        t = acc3_term(v, w)
        for k in range(5):
            s = c[k] + t[k]
            if s >> 64:
                wrapped = True
            largest = max(largest, s)
            c[k] = s & (2**64 - 1)
    t = c[0] + (c[1] << 22) + (c[2] << 44)
    assert t < 2**128   # (true for any 64-bit columns: c2 2^44 < 2^108)
    r = (t + (c[3] % P) * 2**66 + (c[4] % P) * 2**88) % P
    return r, wrapped, largest


def acc3_first_wrap(v, w):
    """The smallest number of terms v * w (the same operands every time) after which a column has passed 2^64; None if no
    column grows."""
    t = max(acc3_term(v, w))
    return None if t == 0 else -(-(2**64) // t)
