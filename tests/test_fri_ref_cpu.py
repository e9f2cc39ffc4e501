"""No GPU: the plain reference of the openings / FRI stage (tools/fri_ref.py) checked by a second route, so that the bit-exact
comparisons of tests/test_gpu_fri_kernels.py rest on something that was itself tested.  The fold (interpolate each 16-point coset,
evaluate at beta) must equal the folded POLYNOMIAL sum_j beta^j P_j(Y) on Y = x^16; the transposed coefficient layout and the
recombination of the partial evaluations must equal the naive evaluation; and the limb model of Acc3 (five columns that wrap at
2^64) must hold its documented 2^17 terms on the worst canonical operands without a wrap."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import fri_ref as F

P = F.P


def _ext(rng):
    return (int(rng.integers(0, P, dtype=np.uint64)), int(rng.integers(0, P, dtype=np.uint64)))


def test_field_constants():
    assert pow(F.GL_POW2_GEN, 1 << 31, P) == P - 1                      # order exactly 2^32
    assert pow(F.GL_GEN, (P - 1) // 2, P) == P - 1                      # a non-residue: the coset shift is outside every <w>
    assert F.root_of_unity(4) == pow(2, 12, P) and pow(7, (P - 1) // 2, P) == P - 1   # w_16 = 2^12; X^2 - 7 is irreducible
    a = (123456789, P - 5)
    assert F.e_mul(a, F.e_inv(a)) == (1, 0) and F.e_inv((0, 0)) == (0, 0) and F.inv(0) == 0
    assert all(w < P for w in F.extreme_words()) and F.WORST in F.extreme_words()
    for k in range(32, 64):   # every 22-bit limb full except for one bit
        l0, l1, l2 = F.limbs22(2**64 - 1 - 2**k)
        assert sorted([F.M22 - l0, F.M22 - l1, (1 << 20) - 1 - l2])[:2] == [0, 0]


@pytest.mark.parametrize("shift", [F.GL_GEN, pow(F.GL_GEN, 16, P), 1])
def test_fold_equals_the_folded_polynomial(shift):
    """A random extension polynomial of degree < 2^8 on shift * <w_256>, bit-reversed, folded at beta = sum_j beta^j P_j(x^16)."""
    rng = np.random.default_rng(8)
    coefs = [_ext(rng) for _ in range(256)]
    vals = F.coset_evaluations_bitrev(coefs, 8, shift)
    for beta in ((0, 0), (1, 0), (P - 1, P - 1), (0, 1), _ext(rng)):
        assert F.fold(vals, 8, shift, beta) == F.fold_by_polynomial(coefs, 8, shift, beta), beta


def test_fold_of_a_low_degree_polynomial_keeps_it():
    """Degree < 16: every coset interpolates to the polynomial itself, so each folded value is P(beta) whatever the coset."""
    rng = np.random.default_rng(9)
    coefs = [_ext(rng) for _ in range(16)]
    beta = _ext(rng)
    vals = F.coset_evaluations_bitrev(coefs, 6, F.GL_GEN)
    want = F.eval_naive_ext(coefs, beta)
    assert F.fold(vals, 6, F.GL_GEN, beta) == [want] * 4


@pytest.mark.parametrize("r", [1, 2, 4])
def test_transposed_layout_and_recombination_equal_the_naive_evaluation(r):
    """Block length 2^4 in place of 2^16: coefficient k1 + R k2 at k1 M + k2; P(z) = sum_k1 z^k1 S_k1(z^R); P(1) = sum of sums."""
    m = 16
    rng = np.random.default_rng(100 + r)
    nat = [int(v) for v in rng.integers(0, P, size=r * m, dtype=np.uint64)]
    nat[3], nat[-1] = P - 1, F.WORST
    stored = F.to_stored(nat, r, m)
    assert sorted(stored) == sorted(nat) and all(stored[(k % r) * m + k // r] == nat[k] for k in range(r * m))
    if r == 1:
        assert stored == nat
    g = F.root_of_unity((r * m).bit_length() - 1)
    for zeta in (_ext(rng), (0, 0), (1, 0), (P - 1, P - 1), (0, 1), (int(rng.integers(0, P, dtype=np.uint64)), 0)):
        zn = F.e_scale(zeta, g)
        pz0, pz1 = F.e_powers(zeta, r * m), F.e_powers(zn, r * m)
        parts = F.opening_partials(stored, r, m, pz0, pz1)
        assert len(parts) == r and all(len(q) == 5 for q in parts)
        v0, v1, s = F.recombine_openings(parts, r, zeta, zn)
        assert v0 == F.eval_naive(nat, zeta) == F.eval_stored(stored, r, m, pz0), zeta
        assert v1 == F.eval_naive(nat, zn) == F.eval_stored(stored, r, m, pz1), zeta
        assert s == sum(nat) % P == F.eval_naive(nat, (1, 0))[0]


def test_combine_final_is_the_batched_quotient_of_consistent_openings():
    """With f_b(x) = q_b(x) (x - z_b) + r_b at every point, the point-wise formula returns the alpha-weighted sum of the q_b; at
    x = z_b the term is dropped (1 / 0 := 0)."""
    rng = np.random.default_rng(12)
    w, n_rc, n_ctl = 5, 3, 2
    a, _ = F.shape_widths(w, n_rc, n_ctl)
    assert a == 2 * 3 + 4
    zeta, zn, alpha = (17, 0), _ext(rng), _ext(rng)
    r0, r1, r2 = _ext(rng), _ext(rng), _ext(rng)
    xs = [17, 1, 0, P - 1] + [int(v) for v in rng.integers(0, P, size=12, dtype=np.uint64)]
    q = [[_ext(rng) for _ in xs] for _ in range(3)]
    f0 = [F.e_add(F.e_mul(q[0][j], F.e_sub((x, 0), zeta)), r0) for j, x in enumerate(xs)]
    f1 = [F.e_add(F.e_mul(q[1][j], F.e_sub((x, 0), zn)), r1) for j, x in enumerate(xs)]
    f2 = [F.e_add(F.e_scale(q[2][j], (x - 1) % P), r2) for j, x in enumerate(xs)]
    fq = [F.e_sub(f0[j], f1[j]) for j in range(len(xs))]
    cl = [[v[0] for v in f1], [v[1] for v in f1], [v[0] for v in fq], [v[1] for v in fq], [v[0] for v in f2], [v[1] for v in f2]]
    got = F.combine_final(cl, xs, zeta, zn, r0, r1, r2, alpha, w, n_rc, n_ctl)
    a2, a12 = F.e_pow(alpha, 4), F.e_pow(alpha, w + a + 4)
    for j, x in enumerate(xs):
        want = F.e_add(F.e_add(F.e_mul(q[0][j] if x != 17 else (0, 0), a12), F.e_mul(q[1][j], a2)), q[2][j] if x != 1 else (0, 0))
        assert got[j] == want, j


def test_acc3_limb_model_holds_its_documented_capacity():
    """Acc3 (csrc/quotient_common.h: "up to 2^17 terms", "columns stay below 2^62"): at T = 2^17 on the worst canonical operands
    no column wraps, the fold of acc3_red returns the big-integer sum, and the first term count at which a column would wrap is
    reported; it must not be below the documented 2^17."""
    t = 1 << 17
    ext = F.extreme_words()
    first = min((F.acc3_first_wrap(v, w), v, w) for v in ext for w in ext if F.acc3_first_wrap(v, w))
    print("Acc3: a column first wraps at T = %d (%.4f * 2^19) terms, operands %#x * %#x" % (first[0], first[0] / 2.0**19, first[1], first[2]))
    assert first[0] == 524289 and first[0] >= t          # 2^19 + 1: column 1 = two products of (2^22 - 1)^2 per term
    for v, w in ((F.WORST, F.WORST), (first[1], first[2]), (P - 1, P - 1)):
        r, wrapped, largest = F.acc3_limb_model([v] * t, [w] * t)
        assert not wrapped and largest < 1 << 62 and r == v * w * t % P, (hex(v), hex(w))
    # one term short of the first wrap the model is still exact; at the wrap it is not, and says so
    v, w = first[1], first[2]
    col = F.acc3_term(v, w)
    assert (first[0] - 1) * max(col) < 2**64 <= first[0] * max(col)
    rng = np.random.default_rng(3)
    vals = [int(x) for x in rng.integers(0, P, size=999, dtype=np.uint64)]
    wts = F.operand_words(rng, 999)
    r, wrapped, _ = F.acc3_limb_model(vals, wts)
    assert not wrapped and r == F.acc_sum(vals, wts)


def test_acc3_limb_model_reports_a_wrap():
    """The reported term count is the model's own: started from the columns after n - 2 equal terms, one more term is still
    exact; started from those after n - 1, the n-th term wraps a column and the result is not the sum any more."""
    v = w = 2**64 - 1 - 2**63   # limbs (2^22 - 1, 2^22 - 1, 2^19 - 1): the largest column 1 a canonical pair can give
    n = F.acc3_first_wrap(v, w)
    col = F.acc3_term(v, w)
    assert n == 524289 and col[1] == 2 * (2**22 - 1)**2 == max(col)
    r, wrapped, _ = F.acc3_limb_model([v], [w], start=[(n - 2) * x for x in col])
    assert not wrapped and r == (n - 1) * v * w % P
    r, wrapped, _ = F.acc3_limb_model([v], [w], start=[(n - 1) * x for x in col])
    assert wrapped and r != n * v * w % P


def test_entry_points_refuse_a_null_context():
    lib = pk.load_library()
    buf = np.ones(64, np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.bn254s_selftest_acc(None, p, p, 4, 2, p) == -1
    assert lib.bn254s_selftest_openings(None, p, 1, 0, p, p, p) == -1
    assert lib.bn254s_selftest_fri_combine(None, 0, 1, 1, 0, 1, p, p, p, p) == -1
    assert lib.bn254s_selftest_fri_fold(None, p, 5, 1, p, p) == -1
    assert lib.bn254s_selftest_fri_rows(None, p, 1, 2, 0, 0, 1, p, 1, p, p) == -1
