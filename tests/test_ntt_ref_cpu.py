"""tests/ntt_ref.py, the reference of tests/test_gpu_ntt_tall.py, by second routes and without a GPU: against the oracle's
from_values at 2^16 rows, the stored layouts against plain index arithmetic and as a round trip, the two closed forms against the
oracle's NTT at every position of 2^17 (the LDE of the value impulse at sampled ones), and coset_ifft against coset_fft."""
import numpy as np
import pytest

from tests import ntt_ref as R
from tests import oracle_lib
from tools.fri_ref import P, bitrev, inv, root_of_unity


def test_helper_equals_from_values_at_2pow16(oracle):
    """Coefficients, leaf order and stored layout (the identity at R = 1) of the helper equal oracle_lib.commit_values."""
    vals = R.columns(16, range(6))
    c_ref, l_ref, _ = oracle_lib.commit_values(oracle, vals)
    for j in range(vals.shape[0]):
        c = R.coefficients(oracle, vals[j])
        assert np.array_equal(R.to_stored(c), c_ref[j]), j
        assert np.array_equal(R.lde(oracle, c), l_ref[j]), j


def test_bitrev_perm_and_cosets_of_the_leaf_order(oracle):
    assert R.bitrev_perm(0).tolist() == [0]
    for bits in (1, 5, 12):
        assert R.bitrev_perm(bits).tolist() == [bitrev(j, bits) for j in range(1 << bits)]
    # coset h of the leaf order is the N-point coset FFT with shift g w_2N^h, in bit-reversed order
    log_n = 10
    c = R.rand_field(np.random.default_rng(3), 1 << log_n)
    leaf = R.lde(oracle, c)
    br = R.bitrev_perm(log_n)
    for h in range(2):
        want = R.orc_ntt(oracle, c, 2, R.coset_shift(h, log_n))[br]
        assert np.array_equal(leaf[h << log_n:(h + 1) << log_n], want), h


@pytest.mark.parametrize("log_n,split", [(17, False), (19, False), (22, False), (18, True), (23, True)])
def test_stored_layouts_round_trip(log_n, split):
    """Stored -> natural -> stored is the identity (tall R = 2, 8, 64; split over R = 2 and 64), and the reshapes put coefficient k
    where the index arithmetic says: k1 + R k2 at k1 2^16 + k2, under the split level [Pe | Po]."""
    n = 1 << log_n
    stored = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    nat = R.from_stored(stored, split)
    assert np.array_equal(R.to_stored(nat, split), stored)
    assert np.array_equal(R.from_stored(R.to_stored(stored, split), split), stored)
    rng = np.random.default_rng(log_n)
    for k in [0, 1, 2, 3, n // 2, n - 2, n - 1, R.M16 - 1, R.M16, R.M16 + 1] + rng.integers(0, n, size=200).tolist():
        pos = R.stored_position(k, log_n, split)
        assert nat[k] == stored[pos], (k, pos)
    if not split:
        r = n >> 16
        k1, k2 = 1, 3
        assert R.stored_position(k1 + r * k2, log_n) == k1 * R.M16 + k2
    else:
        assert R.stored_position(0, log_n, True) == 0 and R.stored_position(1, log_n, True) == n // 2


def test_closed_forms_equal_the_oracle_at_every_position_of_2pow17(oracle):
    """The two closed forms of the GPU test, impulse_coefficient and monomial_lde_value, at every position; impulse_lde_value (the
    LDE of the value impulse, one modular inversion per position) at every 257th position and the last."""
    log_n = 17
    n = 1 << log_n
    for j0 in (R.M16 + 1, n - 1):
        imp = np.zeros(n, np.uint64)
        imp[j0] = 1
        c = R.coefficients(oracle, imp)
        want = [R.impulse_coefficient(log_n, j0, k) for k in range(n)]
        assert c.tolist() == want, j0
        leaf = R.lde(oracle, c)
        nat = np.empty_like(leaf)
        nat[R.bitrev_perm(log_n + 1)] = leaf
        for m in list(range(0, 2 * n, 257)) + [2 * n - 1]:
            assert int(nat[m]) == R.impulse_lde_value(log_n, j0, m), (j0, m)
            assert R.leaf_to_natural(bitrev(m, log_n + 1), log_n) == m
    for k0 in (n - 1, R.M16 + 3):
        c = np.zeros(n, np.uint64)
        c[k0] = 1
        leaf = R.lde(oracle, c)
        perm = R.bitrev_perm(log_n + 1)
        want = np.array([R.monomial_lde_value(log_n, k0, int(m)) for m in perm], dtype=np.uint64)
        assert np.array_equal(leaf, want), k0


def test_coset_ifft_inverts_coset_fft_for_both_shifts(oracle):
    log_n = 17
    vals = R.columns(log_n, [0, 1])
    for h in range(2):
        s = R.coset_shift(h, log_n)
        for v in vals:
            q = R.quotient_interpolant(oracle, v, h)
            assert np.array_equal(R.orc_ntt(oracle, q, 2, s), v), h
    ratio = R.coset_shift(1, log_n) * inv(R.coset_shift(0, log_n)) % P       # w_2N: its square is w_N, its N-th power -1
    assert ratio * ratio % P == root_of_unity(log_n) and pow(ratio, 1 << log_n, P) == P - 1


def test_columns_are_canonical_and_as_described():
    for log_n in (16, 17):
        n = 1 << log_n
        cols = R.columns(log_n, range(12))
        assert cols.shape == (12, n) and int(cols.max()) < P
        a = cols[0]
        pairs = {(int(a[i]), int(a[i + n // 2])) for i in range(225)}
        assert len(pairs) == len(set(R.EDGE.tolist())) ** 2        # every pairing of two edge values at (i, i + N/2)
        assert np.count_nonzero(cols[4]) <= 40 and cols[4][0] and cols[4][R.M16 - 1] and cols[4][n - 1]
        assert log_n == 16 or cols[4][R.M16]
        assert (cols[5] == np.uint64(P - 1)).all() and not np.array_equal(cols[0], cols[6])
        share = np.count_nonzero(cols[2] == np.uint64(P - 1)) / n
        assert 0.28 < share < 0.32
