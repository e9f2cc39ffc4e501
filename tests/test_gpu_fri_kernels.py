"""The openings / FRI kernels of csrc/fri.hip and the un-reduced accumulators of csrc/quotient_common.h at their operand bounds.

A proof only ever feeds these kernels pseudo-random words, so the rare carry and borrow branches of gl_reduce128 behind a
product and of gl_add (a result in [p, 2^64): about 2^-32 per operation), the full limbs of Acc3, the zero denominators of
k_fri_combine_final, opening points of small order and the wrap of k_extract_window never run in the whole-proof tests.  Here the debug entry points of csrc/fri_selftest.hip run the
provers' own launchers on crafted data: canonical words with extreme limbs (tools/fri_ref.extreme_words) as values and as
weights, the documented 2^17 terms of an accumulator, opening points 0, 1, p - 1, X, w_256, w_65536, points x equal to zeta.
Every output word is compared with tools/fri_ref.py (Python integers, written from the definitions and checked by a second
route in tests/test_fri_ref_cpu.py); there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from tools import fri_ref as F

pytestmark = pytest.mark.gpu
P = F.P
WORST = F.WORST
E_ARG = -1


def u64(a):
    return np.array(a, dtype=np.uint64)


def rand_word(rng):
    return int(rng.integers(0, P, dtype=np.uint64))


def rand_ext(rng):
    return (rand_word(rng), rand_word(rng))


def assert_words_equal(got, want, what):
    got, want = np.asarray(got, dtype=np.uint64), u64(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if bad.size:
        lines = ["%s: got %#x%s, expected %#x" % (tuple(i), int(got[tuple(i)]), " (not below p)" if int(got[tuple(i)]) >= P else "",
                                                  int(want[tuple(i)])) for i in bad[:8].tolist()]
        raise AssertionError("%s: %d of %d words differ\n" % (what, len(bad), got.size) + "\n".join(lines))


# ---- accumulators -----------------------------------------------------------------------------------------------------------
ACC_T = (1, 9, 31, 1 << 17)
ACC_ROWS = ("all 2^64-1-2^32", "all p-1", "0 / 2^64-1-2^32 alternating", "2^64-1-2^32 / 0 alternating", "extreme words by blocks",
            "extreme and random words", "random", "random")
ACC_WEIGHTS = ("all 2^64-1-2^32", "all p-1", "extreme words in turn", "random")


@pytest.fixture(scope="module")
def acc_cases():
    """T -> (values[8][T], {weight set: weights[T]}, {weight set: [sum per row]}); the sums are sum(v w) mod p on integers."""
    out = {}
    n_ext = len(F.extreme_words())
    for t in ACC_T:
        rng = np.random.default_rng(1000 + t)
        rows = [[WORST] * t, [P - 1] * t, [0 if k % 2 == 0 else WORST for k in range(t)],
                [WORST if k % 2 == 0 else 0 for k in range(t)], F.pairing_words(t, n_ext), F.operand_words(rng, t),
                rng.integers(0, P, size=t, dtype=np.uint64).tolist(), rng.integers(0, P, size=t, dtype=np.uint64).tolist()]
        weights = {"all 2^64-1-2^32": [WORST] * t, "all p-1": [P - 1] * t, "extreme words in turn": F.pairing_words(t, 1),
                   "random": rng.integers(0, P, size=t, dtype=np.uint64).tolist()}
        assert tuple(weights) == ACC_WEIGHTS and len(rows) == len(ACC_ROWS)
        want = {k: [F.acc_sum(r, w) for r in rows] for k, w in weights.items()}
        out[t] = (u64(rows), {k: u64(w) for k, w in weights.items()}, want)
    return out


@pytest.mark.parametrize("t", ACC_T)
def test_accumulators_equal_the_integer_sum(gpu_ctx, acc_cases, t):
    """Acc (128 + 32 bits) and Acc3 (five carry-free columns of 22-bit limb products) over T terms in ONE accumulator each, up to
    the documented capacity of 2^17 terms with every limb of value and weight full: both equal sum(v w) mod p."""
    values, weights, want = acc_cases[t]
    for name in ACC_WEIGHTS:
        got = gpu_ctx.selftest_acc(values, weights[name])
        for k, kind in enumerate(("Acc", "Acc3")):
            assert_words_equal(got[:, k], want[name], "%s, T = %d, weights %s (rows: %s)" % (kind, t, name, "; ".join(ACC_ROWS)))


# ---- openings ---------------------------------------------------------------------------------------------------------------
M16 = 1 << 16
MAX_LOG_R = 2


@pytest.fixture(scope="module")
def opening_powers():
    """point -> its powers over the longest polynomial, shared by the three heights (the points that do not depend on g)."""
    cache = {}
    yield cache
    cache.clear()


def opening_points(log_r):
    """The pairs (zeta, zeta_next); g = w_N as in a proof.  The points of the first seven pairs are the same at every height."""
    rng = np.random.default_rng(77)
    g = F.root_of_unity(16 + log_r)
    a, b, c = rand_ext(rng), rand_ext(rng), rand_ext(rng)
    base = rand_word(rng)
    w256, w65536 = F.root_of_unity(8), F.root_of_unity(16)
    mm, x, zero, one = (P - 1, P - 1), (0, 1), (0, 0), (1, 0)
    return [("random pair", a, b), ("0, 0", zero, zero), ("1, 0", one, zero), ("(p-1, p-1) twice", mm, mm), ("X twice", x, x),
            ("0, 1", zero, one), ("p-1 in the base field twice", (P - 1, 0), (P - 1, 0)),
            ("base field, g zeta", (base, 0), (base * g % P, 0)),
            ("w_256 (the table of (z^256)^q is all ones), g zeta", (w256, 0), (w256 * g % P, 0)),
            ("w_65536 (periodic table), g zeta", (w65536, 0), (w65536 * g % P, 0)),
            ("extension zeta, g zeta", c, F.e_scale(c, g))]


@pytest.fixture(scope="module", params=[0, 1, 2])
def opening_case(request, opening_powers):
    """Per log_r: the dense and the sparse polynomials (stored layout) and, per point pair, the expected partial records and the
    values P(zeta), P(zeta_next), P(1) by the naive sum over all coefficients.  The powers of a point are formed once and every
    polynomial is a dot product with them."""
    log_r = request.param
    r, n = 1 << log_r, M16 << log_r
    points = opening_points(log_r)
    same_everywhere = {z for _, z0, z1 in points[:7] for z in (z0, z1)} | {z0 for _, z0, _ in points[7:]}

    def powers_of(z):
        if z not in same_everywhere:
            return F.e_powers(z, n)
        if z not in opening_powers:
            opening_powers[z] = F.e_powers(z, M16 << MAX_LOG_R)
        c0, c1 = opening_powers[z]
        return c0[:n], c1[:n]

    rng = np.random.default_rng(500 + log_r)
    dense = [[P - 1] * n, [WORST] * n, rng.integers(0, P, size=n, dtype=np.uint64).tolist()]
    # stored position -> word: an impulse at coefficient 0, one at coefficient N - 1 (k1 = R - 1, k2 = 2^16 - 1: the last stored
    # word too), and a single word in lane 255 of the last block (its first round, q = 0)
    assert F.stored_position(n - 1, r, M16) == n - 1 and F.stored_position(0, r, M16) == 0
    sparse = [{0: WORST}, {n - 1: P - 1}, {(r - 1) * M16 + 255: rand_word(rng)}]
    sparse_arr = np.zeros((3, n), np.uint64)
    for i, s in enumerate(sparse):
        for pos, v in s.items():
            sparse_arr[i, pos] = v
    blocks = [[p[k1 * M16:(k1 + 1) * M16] for k1 in range(r)] for p in dense]
    sums = [[sum(b) % P for b in blocks[p]] for p in range(3)]
    per_z = {}

    def at(z):
        """([poly][k1] -> S_k1(z^R), [poly] -> P(z)) for the dense and the sparse polynomials."""
        if z not in per_z:
            pz = powers_of(z)
            strided = [(pz[0][k1::r], pz[1][k1::r]) for k1 in range(r)]
            y = strided[0]   # the powers of z^R
            d_part = [[F.e_dot(b, y) for b in blocks[p]] for p in range(3)]
            # P(z) = the sum over ALL coefficients c_k z^k: block k1 holds the coefficients k1 + R k2 and meets the powers
            # pz[k1::R] (F.eval_stored); for block 0 those are the powers of z^R, the dot product just formed
            d_val = []
            for p in range(3):
                v = d_part[p][0]
                for k1 in range(1, r):
                    v = F.e_add(v, F.e_dot(blocks[p][k1], strided[k1]))
                d_val.append(v)
            s_part, s_val = [], []
            for s in sparse:
                part, val = [(0, 0)] * r, (0, 0)
                for pos, v in s.items():
                    k1, k2 = pos // M16, pos % M16
                    part[k1] = F.e_add(part[k1], (v * pz[0][r * k2] % P, v * pz[1][r * k2] % P))
                    k = k1 + r * k2   # the coefficient's index
                    val = F.e_add(val, (v * pz[0][k] % P, v * pz[1][k] % P))
                s_part.append(part)
                s_val.append(val)
            per_z[z] = (d_part, d_val, s_part, s_val)
        return per_z[z]

    cases = []
    for name, z0, z1 in points:
        e0, e1 = at(z0), at(z1)
        want_dense = [[[e0[0][p][k1][0], e0[0][p][k1][1], e1[0][p][k1][0], e1[0][p][k1][1], sums[p][k1]] for k1 in range(r)]
                      for p in range(3)]
        want_sparse = [[[e0[2][p][k1][0], e0[2][p][k1][1], e1[2][p][k1][0], e1[2][p][k1][1],
                         sum(v for pos, v in sparse[p].items() if pos // M16 == k1) % P] for k1 in range(r)] for p in range(3)]
        vals_dense = [(e0[1][p], e1[1][p], sum(dense[p]) % P) for p in range(3)]
        vals_sparse = [(e0[3][p], e1[3][p], sum(sparse[p].values()) % P) for p in range(3)]
        cases.append((name, z0, z1, want_dense, want_sparse, vals_dense, vals_sparse))
    return log_r, u64(dense), sparse_arr, cases


def test_openings_partials_and_recombined_values(gpu_ctx, opening_case):
    """All five words of every partial record, and P(zeta), P(g zeta), P(1) recombined from the DEVICE's records as the prover's
    host code does, against the sum over all coefficients."""
    log_r, dense, sparse, cases = opening_case
    r = 1 << log_r
    for name, z0, z1, want_dense, want_sparse, vals_dense, vals_sparse in cases:
        for kind, coeffs, want, vals in (("dense", dense, want_dense, vals_dense), ("sparse", sparse, want_sparse, vals_sparse)):
            got = gpu_ctx.selftest_openings(coeffs, log_r, z0, z1)
            what = "log_r = %d, point pair %s, %s polynomials" % (log_r, name, kind)
            assert_words_equal(got, want, what + " [poly][block][S0.c0 S0.c1 S1.c0 S1.c1 sum]")
            for p in range(3):
                assert F.recombine_openings(got[p], r, z0, z1) == vals[p], (what, p)


# ---- batched quotient, coefficient part -------------------------------------------------------------------------------------------
COMBINE_SHAPES = ((1, 1, 0), (8, 6, 2), (9, 7, 2), (781, 7, 2))
COMBINE_N = (1, 255, 300)


@pytest.fixture(scope="module")
def combine_cases():
    """Per shape: cols[W + A + 4][300] from the operand list and two weight sets (extreme words; the true powers of a random
    alpha) with comb[6][300] of each.  Column j of the sums depends on column j of the inputs only, so n = 1 and n = 255 are the
    first columns of the same reference."""
    out = {}
    for w, n_rc, n_ctl in COMBINE_SHAPES:
        rng = np.random.default_rng(w)
        a, _ = F.shape_widths(w, n_rc, n_ctl)
        n_polys = w + a + 4
        cols = [F.operand_words(rng, 300) for _ in range(n_polys)]
        cols[0][:6] = [WORST, P - 1, 0, WORST, P - 1, 1]
        ext_w = list(zip(F.operand_words(rng, n_polys, 7), F.operand_words(rng, n_polys, 5)))
        head = [(WORST, WORST), (P - 1, P - 1), (0, 0), (1, 0), (0, 1)]
        ext_w[:len(head)] = head[:n_polys]
        alpha = rand_ext(rng)
        pw = [F.e_pow(alpha, k) for k in range(n_polys)]
        sets = {"extreme": ext_w, "powers of alpha": pw}
        out[(w, n_rc, n_ctl)] = (u64(cols), {k: (u64(v), F.combine_coeffs(cols, w, n_rc, n_ctl, v)) for k, v in sets.items()})
    return out


@pytest.mark.parametrize("shape", COMBINE_SHAPES, ids=lambda s: "W%d_rc%d_ctl%d" % s)
def test_combine_coeffs_all_six_columns(gpu_ctx, combine_cases, shape):
    """k_fri_combine_coeffs: the remainders of the `unroll 8` loops (W = 1, 8, 9, 781; 4, 8 and 10 lookup columns), the empty and
    the non-empty Z loop, n = 1, 255 and 300 (a last partial block; n is stride and bound only)."""
    w, n_rc, n_ctl = shape
    cols, sets = combine_cases[shape]
    for name, (weights, want) in sets.items():
        for n in COMBINE_N:
            got = gpu_ctx.selftest_fri_combine_coeffs(np.ascontiguousarray(cols[:, :n]), w, n_rc, n_ctl, weights)
            assert_words_equal(got, [c[:n] for c in want], "comb[6][n], shape %r, n = %d, weights: %s" % (shape, n, name))


# ---- batched quotient, point-wise part --------------------------------------------------------------------------------------------
FINAL_M = 300


def _final_case(name, rng, shape, zeta, zeta_next, x_one, r_at):
    """xs: zeta.c0, zeta_next.c0, 1 (or 2 where no denominator may vanish), 0, p - 1 at the start, around the block boundary and
    at the end, random elsewhere; cl from the operand list; r_b = f_b at the points r_at (a zero numerator)."""
    m = FINAL_M
    special = [zeta[0], zeta_next[0], x_one, 0, P - 1]
    xs = rng.integers(0, P, size=m, dtype=np.uint64).tolist()
    xs[0:5] = special
    xs[253:258] = special
    xs[m - 1] = zeta[0]
    cl = [F.operand_words(rng, m) for _ in range(6)]
    f1 = lambda j: (cl[0][j], cl[1][j])
    f0 = lambda j: F.e_add(f1(j), (cl[2][j], cl[3][j]))
    f2 = lambda j: (cl[4][j], cl[5][j])
    r0, r1, r2 = f0(r_at[0]), f1(r_at[1]), f2(r_at[2])
    alpha = rand_ext(rng)
    want = F.combine_final(cl, xs, zeta, zeta_next, r0, r1, r2, alpha, *shape)
    return name, u64(cl), u64(xs), shape, (zeta, zeta_next, r0, r1, r2, alpha), want


@pytest.fixture(scope="module")
def final_cases():
    rng = np.random.default_rng(41)
    z0, z1 = rand_word(rng), rand_word(rng)
    ze, zf = rand_ext(rng), rand_ext(rng)
    return [
        # base-field points that occur among the xs: each denominator vanishes somewhere, one at a time; numerators vanish elsewhere
        _final_case("base-field zeta and zeta_next among the points", rng, (9, 7, 2), (z0, 0), (z1, 0), 1, (7, 8, 9)),
        # all three denominators vanish at the same point x = 1
        _final_case("zeta = zeta_next = 1", rng, (9, 7, 2), (1, 0), (1, 0), 1, (7, 8, 9)),
        # zeta = zeta_next: two vanish together; the numerators vanish at the very points where the denominators do
        _final_case("zeta = zeta_next in the base field, r_b = f_b there", rng, (8, 6, 2), (z0, 0), (z0, 0), 1, (0, 1, 2)),
        # a proper extension zeta: x - zeta has c1 != 0 and x = 1 is not among the points, so nothing vanishes
        _final_case("proper extension points, no zero denominator", rng, (781, 7, 2), ze, zf, 2, (7, 8, 9)),
        # n_ctl = 0: alpha^(2 n_ctl) = 1; extreme opening points
        _final_case("zeta = (p-1, p-1), zeta_next = (p-1, 0), no CTL", rng, (1, 1, 0), (P - 1, P - 1), (P - 1, 0), 1, (3, 4, 2)),
    ]


def test_combine_final_with_vanishing_denominators(gpu_ctx, final_cases):
    """k_fri_combine_final, m = 300 (a last partial block): where x = zeta, x = zeta_next or x = 1 that term is 0 and the other
    two are exact (one shared inversion behind all three); a zero numerator; a case where nothing vanishes."""
    for name, cl, xs, shape, pts, want in final_cases:
        zeta, zeta_next = pts[0], pts[1]
        xl = xs.tolist()
        n_zero = sum((zeta[1] == 0 and x == zeta[0]) + (zeta_next[1] == 0 and x == zeta_next[0]) + (x == 1) for x in xl)
        assert (n_zero == 0) == ("no zero denominator" in name), (name, n_zero)
        got = gpu_ctx.selftest_fri_combine_final(cl, xs, *shape, *pts)
        assert_words_equal(got, want, "out[m][2], case: " + name)


# ---- fold -------------------------------------------------------------------------------------------------------------------
FOLD_LOG_M = (5, 9, 13)
FOLD_SHIFTS = (F.GL_GEN, pow(F.GL_GEN, 16, P), 1)


def fold_betas():
    return [(0, 0), (1, 0), (P - 1, P - 1), (0, 1), rand_ext(np.random.default_rng(5))]


@pytest.fixture(scope="module", params=FOLD_LOG_M)
def fold_case(request):
    """Per log_m the four inputs and, per (shift, beta), the expected fold of each: the inner sums over a coset depend on the
    values only and are formed once."""
    log_m = request.param
    m = 1 << log_m
    rng = np.random.default_rng(600 + log_m)
    one_per_coset = [(0, 0)] * m
    for c in range(m >> 4):   # one nonzero value per coset, at position c mod 16: each of the 16 positions
        one_per_coset[16 * c + c % 16] = (WORST, P - 1) if c % 3 else rand_ext(rng)
    inputs = {"all p-1": [(P - 1, P - 1)] * m, "all 2^64-1-2^32": [(WORST, WORST)] * m, "one nonzero value per coset": one_per_coset,
              "random": [rand_ext(rng) for _ in range(m)]}
    sums = {k: F.fold_coset_sums(v, log_m) for k, v in inputs.items()}
    want = {(k, s, b): F.fold_from_sums(sums[k], log_m, s, b) for k in inputs for s in FOLD_SHIFTS for b in fold_betas()}
    return log_m, {k: u64(v) for k, v in inputs.items()}, want


def test_fold_equals_interpolation_at_beta(gpu_ctx, fold_case):
    """k_fri_fold: the shift-only inverse DFT (gl_mul_2exp) on values whose sums and differences carry and borrow, beta = 0, 1,
    (p-1, p-1), X and random, the three shifts of the first layers and of a plain subgroup; one, two and 512 cosets."""
    log_m, inputs, want = fold_case
    for (k, s, b), w in want.items():
        got = gpu_ctx.selftest_fri_fold(inputs[k], s, b)
        assert_words_equal(got, w, "fold, log_m = %d, input %s, shift %#x, beta %r" % (log_m, k, s, b))


@pytest.fixture(scope="module")
def fold_polynomial():
    rng = np.random.default_rng(19)
    coefs = [rand_ext(rng) for _ in range(512)]
    beta = rand_ext(rng)
    return [(s, u64(F.coset_evaluations_bitrev(coefs, 9, s)), beta, F.fold_by_polynomial(coefs, 9, s, beta)) for s in FOLD_SHIFTS]


def test_fold_of_a_polynomial_is_the_folded_polynomial(gpu_ctx, fold_polynomial):
    """log_m = 9: a random extension polynomial of degree < 512 on shift <w_512>, folded on the device, equals
    sum_j beta^j P_j(Y) on Y = x^16 (no interpolation in the reference at all)."""
    for s, vals, beta, want in fold_polynomial:
        assert_words_equal(gpu_ctx.selftest_fri_fold(vals, s, beta), want, "folded polynomial, shift %#x" % s)


# ---- rows -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows_lde():
    rng = np.random.default_rng(23)
    return [F.operand_words(rng, 512) for _ in range(3)]


@pytest.mark.parametrize("rows", [1, 257])
def test_window_wraps_and_rows_gather(gpu_ctx, rows_lde, rows):
    """log_n = 8, three columns, both cosets: a window that starts at the last row (and, 257 rows long, goes round the whole
    coset once: two blocks of the grid) and queries at index 0, at 2 N - 1 and repeated, one and 84 of them."""
    log_n, n = 8, 256
    rng = np.random.default_rng(rows)
    idx84 = [0, 2 * n - 1, 0, 2 * n - 1, 255, 256, 255] + rng.integers(0, 2 * n, size=77).tolist()
    for h in (0, 1):
        for k0 in (n - 1, 200, 0):
            for idx in ([0], [2 * n - 1], idx84):
                win, gat = gpu_ctx.selftest_fri_rows(u64(rows_lde), h, k0, rows, idx)
                what = "coset %d, k0 = %d, rows = %d, nq = %d" % (h, k0, rows, len(idx))
                assert_words_equal(win, F.extract_window(rows_lde, log_n, h, k0, rows), "window, " + what)
                assert_words_equal(gat, F.gather_rows(rows_lde, idx), "gathered rows, " + what)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host_and_the_context_lives_on(gpu_ctx):
    """A word equal to p, a NULL pointer or a size out of range: BN254S_E_INVALID_ARG from every entry point before any launch
    (the output buffer is untouched), and the context then passes a small positive case of each."""
    import plonky2_bn254_amd as pk
    lib, h = pk.load_library(), gpu_ctx._h
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    out = np.full(1 << 12, 7, np.uint64)

    def refused(rc):
        assert rc == E_ARG and (out == 7).all(), rc

    def with_p(a, pos):
        b = a.copy()
        b.reshape(-1)[pos] = P
        return b

    # accumulators: T = 2^17 + 1 is past the documented capacity
    t_big = (1 << 17) + 1
    v, w = np.ones((2, 9), np.uint64), np.ones(9, np.uint64)
    big_v, big_w = np.ones((1, t_big), np.uint64), np.ones(t_big, np.uint64)
    refused(lib.bn254s_selftest_acc(h, ptr(big_v), ptr(big_w), t_big, 1, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, ptr(v), ptr(w), 0, 2, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, ptr(v), ptr(w), 9, 0, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, ptr(v), ptr(w), 9, 4097, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, None, ptr(w), 9, 2, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, ptr(v), None, 9, 2, ptr(out)))
    assert lib.bn254s_selftest_acc(h, ptr(v), ptr(w), 9, 2, None) == E_ARG
    refused(lib.bn254s_selftest_acc(h, ptr(with_p(v, 17)), ptr(w), 9, 2, ptr(out)))
    refused(lib.bn254s_selftest_acc(h, ptr(v), ptr(with_p(w, 8)), 9, 2, ptr(out)))
    assert gpu_ctx.selftest_acc(v, w).tolist() == [[9, 9], [9, 9]]

    # openings
    co = np.ones((1, M16), np.uint64)
    z = u64([3, 4])
    refused(lib.bn254s_selftest_openings(h, ptr(with_p(co, M16 - 1)), 1, 0, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, 0, ptr(u64([P, 0])), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, 0, ptr(z), ptr(u64([0, P])), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 0, 0, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 65, 0, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, -1, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, 3, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, None, 1, 0, ptr(z), ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, 0, None, ptr(z), ptr(out)))
    refused(lib.bn254s_selftest_openings(h, ptr(co), 1, 0, ptr(z), None, ptr(out)))
    assert lib.bn254s_selftest_openings(h, ptr(co), 1, 0, ptr(z), ptr(z), None) == E_ARG
    got = gpu_ctx.selftest_openings(co, 0, (1, 0), (0, 0))
    assert got.tolist() == [[[M16, 0, 1, 0, M16]]]

    # batched quotient, both modes: shape (1, 1, 0) has 1 + 4 + 4 polynomials
    cols, wts = np.ones((9, 3), np.uint64), np.ones((9, 2), np.uint64)
    cl, xs, pts = np.ones((6, 3), np.uint64), u64([5, 6, 7]), np.ones(12, np.uint64)
    for args in ((2, 1, 1, 0, 3), (-1, 1, 1, 0, 3), (0, 0, 1, 0, 3), (0, 4097, 1, 0, 3), (0, 1, 0, 0, 3), (0, 1, 2, 0, 3), (0, 1, 1, 1, 3),
                 (0, 1, 1, 3, 3), (0, 1, 1, 0, 0), (0, 1, 1, 0, (1 << 16) + 1)):
        refused(lib.bn254s_selftest_fri_combine(h, *args, ptr(cols), ptr(wts), None, ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 0, 1, 1, 0, 3, None, ptr(wts), None, ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 0, 1, 1, 0, 3, ptr(cols), None, None, ptr(out)))
    assert lib.bn254s_selftest_fri_combine(h, 0, 1, 1, 0, 3, ptr(cols), ptr(wts), None, None) == E_ARG
    refused(lib.bn254s_selftest_fri_combine(h, 0, 1, 1, 0, 3, ptr(with_p(cols, 26)), ptr(wts), None, ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 0, 1, 1, 0, 3, ptr(cols), ptr(with_p(wts, 17)), None, ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, 3, ptr(cl), ptr(xs), None, ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, 0, ptr(cl), ptr(xs), ptr(pts), ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, (1 << 20) + 1, ptr(cl), ptr(xs), ptr(pts), ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, 3, ptr(with_p(cl, 17)), ptr(xs), ptr(pts), ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, 3, ptr(cl), ptr(with_p(xs, 2)), ptr(pts), ptr(out)))
    refused(lib.bn254s_selftest_fri_combine(h, 1, 1, 1, 0, 3, ptr(cl), ptr(xs), ptr(with_p(pts, 11)), ptr(out)))
    got = gpu_ctx.selftest_fri_combine_coeffs(cols, 1, 1, 0, wts)
    assert got.tolist() == [[5] * 3, [5] * 3, [4] * 3, [4] * 3, [0] * 3, [0] * 3]
    got = gpu_ctx.selftest_fri_combine_final(cl, xs, 1, 1, 0, *[(1, 1)] * 6)
    assert_words_equal(got, F.combine_final(cl.tolist(), xs.tolist(), *[(1, 1)] * 6, 1, 1, 0), "small positive case")

    # fold: log_m = 4 is refused (the kernel would reverse the bits of an index over 0 bits: a shift by 32)
    vals, beta = np.ones((32, 2), np.uint64), u64([2, 3])
    for log_m in (4, 0, -1, 21):
        refused(lib.bn254s_selftest_fri_fold(h, ptr(vals), log_m, 1, ptr(beta), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, ptr(vals), 5, 0, ptr(beta), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, ptr(vals), 5, P, ptr(beta), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, ptr(with_p(vals, 63)), 5, 1, ptr(beta), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, ptr(vals), 5, 1, ptr(u64([2, P])), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, None, 5, 1, ptr(beta), ptr(out)))
    refused(lib.bn254s_selftest_fri_fold(h, ptr(vals), 5, 1, None, ptr(out)))
    assert lib.bn254s_selftest_fri_fold(h, ptr(vals), 5, 1, ptr(beta), None) == E_ARG
    # the constant 1 + X interpolates to itself on every coset
    assert gpu_ctx.selftest_fri_fold(vals, F.GL_GEN, (2, 3)).tolist() == [[1, 1], [1, 1]]

    # rows
    lde = np.arange(2 * 8, dtype=np.uint64).reshape(2, 8)
    idx = np.array([0, 7, 3], np.uint32)
    iptr = idx.ctypes.data_as(C.c_void_p)
    o2 = np.full(64, 7, np.uint64)
    for a in ((0, 2, 0, 0, 2), (4097, 2, 0, 0, 2), (2, 0, 0, 0, 2), (2, 21, 0, 0, 2), (2, 2, 2, 0, 2), (2, 2, -1, 0, 2), (2, 2, 0, 4, 2),
              (2, 2, 0, 0, 0), (2, 2, 0, 0, (1 << 20) + 1)):
        refused(lib.bn254s_selftest_fri_rows(h, ptr(lde), *a, iptr, 3, ptr(out), ptr(o2)))
        assert (o2 == 7).all()
    for nq in (0, 4097, -1):
        refused(lib.bn254s_selftest_fri_rows(h, ptr(lde), 2, 2, 0, 0, 2, iptr, nq, ptr(out), ptr(o2)))
    bad_idx = np.array([0, 8, 3], np.uint32)
    refused(lib.bn254s_selftest_fri_rows(h, ptr(lde), 2, 2, 0, 0, 2, bad_idx.ctypes.data_as(C.c_void_p), 3, ptr(out), ptr(o2)))
    refused(lib.bn254s_selftest_fri_rows(h, ptr(with_p(lde, 15)), 2, 2, 0, 0, 2, iptr, 3, ptr(out), ptr(o2)))
    refused(lib.bn254s_selftest_fri_rows(h, None, 2, 2, 0, 0, 2, iptr, 3, ptr(out), ptr(o2)))
    refused(lib.bn254s_selftest_fri_rows(h, ptr(lde), 2, 2, 0, 0, 2, None, 3, ptr(out), ptr(o2)))
    assert lib.bn254s_selftest_fri_rows(h, ptr(lde), 2, 2, 0, 0, 2, iptr, 3, None, ptr(o2)) == E_ARG
    assert lib.bn254s_selftest_fri_rows(h, ptr(lde), 2, 2, 0, 0, 2, iptr, 3, ptr(out), None) == E_ARG
    assert (o2 == 7).all()
    win, gat = gpu_ctx.selftest_fri_rows(lde, 1, 3, 3, idx)   # rows 3, 0, 1 of coset 1: positions 4 + bitrev2 = 7, 4, 6
    assert win.tolist() == [[7, 4, 6], [15, 12, 14]] and gat.tolist() == [[0, 7, 3], [8, 15, 11]]
