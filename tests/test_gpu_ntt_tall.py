"""The tall and split NTT / LDE paths of csrc/ntt.hip, element by element, at every height from 2^16 to 2^23 rows.

Whole proofs reach these paths on honest traces only (mostly 16-bit limbs), compare them with the oracle up to 2^18 rows, and
above that a verifier opens about a hundred of 2^21 .. 2^24 LDE positions.  Here bn254s_selftest_transforms drives the provers' own
transform dispatch (csrc/transforms.h: commit_ntt, lde, lde_chunk, quotient_coset_inverse under the plan of each height, with
and without the split level and the compact workspace) on columns of boundary values, and EVERY word of its output is compared
with the oracle's plain radix-2 NTT (tests/ntt_ref.py, checked on the CPU by tests/test_ntt_ref_cpu.py): LOGR = 1 .. 6 of the outer
passes, the split level at 2^18 and at 2^23 (every split_pow table entry), both coset masks of the streaming path, the 2^16
ntt_lde and ntt_coset_inverse.  The shift table (mul_2exp3, all 64 shifts) and the R-point DFT (dft_small, all twelve
instantiations) are compared with Python integers at their operand bounds.  Impulses are also checked against closed forms that
use no NTT.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import ntt_ref as R
from tools.fri_ref import P, bitrev

pytestmark = pytest.mark.gpu
E_ARG = -1
SPLIT, COMPACT = R.SPLIT, R.COMPACT
CACHED_UP_TO = 19   # heights whose reference columns several tests share


def assert_columns_equal(got, want, what):
    """Exact, with the first differing (column, position) pairs."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    lines = ["(col %d, pos %d): got %#x%s, expected %#x" % (c, i, int(got[c, i]), " (not below p)" if int(got[c, i]) >= P else "",
                                                             int(want[c, i])) for c, i in bad[:10].tolist()]
    raise AssertionError("%s: %d of %d words differ; first (column, position) pairs:\n" % (what, len(bad), got.size) + "\n".join(lines))


@pytest.fixture(scope="module")
def ref_columns(oracle):
    """(log_n, j) -> (values, natural-order coefficients, LDE in leaf order) of column j of the list, by the oracle; computed once
    per column up to 2^19 rows, where several tests use the same columns."""
    cache = {}

    def get(log_n, js):
        out = []
        for j in js:
            if (log_n, j) in cache:
                out.append(cache[log_n, j])
                continue
            v = R.column(log_n, j)
            c = R.coefficients(oracle, v)
            item = (v, c, R.lde(oracle, c))
            for a in item:
                a.setflags(write=False)
            if log_n <= CACHED_UP_TO:
                cache[log_n, j] = item
            out.append(item)
        return tuple(np.stack([item[k] for item in out]) for k in range(3))

    yield get
    cache.clear()


def stored(coeffs, flags):
    return np.stack([R.to_stored(c, bool(flags & SPLIT)) for c in coeffs])


def check_commit(gpu_ctx, ref_columns, log_n, flags, js):
    vals, coef, lde = ref_columns(log_n, js)
    got_c, got_l = gpu_ctx.selftest_transforms(0, log_n, flags, vals)
    what = "2^%d rows, flags %d" % (log_n, flags)
    assert_columns_equal(got_c, stored(coef, flags), "coefficients, " + what)
    assert_columns_equal(got_l, lde, "LDE, " + what)
    return got_c, got_l


# ---- from_values at every height ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,ncols", [(16, 6), (17, 6), (18, 6), (19, 6), (20, 4), (21, 3), (22, 2)])
def test_commit_every_height(gpu_ctx, ref_columns, log_n, ncols):
    """commit_ntt under the plain plan: the fused 2^16 path and LOGR = 1 .. 6 of k_ntt_outer_inv / k_ntt_outer_fwd."""
    check_commit(gpu_ctx, ref_columns, log_n, 0, range(ncols))
    if log_n >= 22:
        gpu_ctx.trim()


@pytest.mark.parametrize("log_n,ncols", [(18, 17), (23, 1)])
def test_split_level(gpu_ctx, ref_columns, log_n, ncols):
    """The radix-2 level above the tall transforms: two chunks of the 16-column loop at 2^18 (the second of one column), and the real
    height, LOGR = 6 under the g^2 base shift with every entry of the split_pow tables."""
    check_commit(gpu_ctx, ref_columns, log_n, SPLIT, range(ncols))
    if log_n >= 22:
        gpu_ctx.trim()


def test_compact_chunks(gpu_ctx, ref_columns):
    """The chunk loop of the compact workspace: word for word what the plain plan gives, and the reference."""
    js = range(17)
    got_c, got_l = check_commit(gpu_ctx, ref_columns, 17, COMPACT, js)
    plain_c, plain_l = gpu_ctx.selftest_transforms(0, 17, 0, ref_columns(17, js)[0])
    assert_columns_equal(got_c, plain_c, "coefficients, compact against plain")
    assert_columns_equal(got_l, plain_l, "LDE, compact against plain")


@pytest.mark.parametrize("log_n,flags", [(16, 0), (19, 0), (18, SPLIT), (17, COMPACT)])
def test_lde_from_coefficients(gpu_ctx, ref_columns, log_n, flags):
    """lde on the reference's stored coefficients (2^16 rows: ntt_lde; compact: the scratch of one chunk)."""
    _, coef, lde = ref_columns(log_n, range(3))
    got = gpu_ctx.selftest_transforms(1, log_n, flags, stored(coef, flags))
    assert_columns_equal(got, lde, "LDE from coefficients, 2^%d rows, flags %d" % (log_n, flags))


@pytest.mark.parametrize("log_n,flags", [(17, 0), (18, SPLIT)])
def test_lde_chunk_coset_masks(gpu_ctx, ref_columns, log_n, flags):
    """lde_chunk of the streaming workspace: the cosets of the mask equal the reference, the other half is untouched."""
    n = 1 << log_n
    _, coef, lde = ref_columns(log_n, range(3))
    st = stored(coef, flags)
    for mask in (1, 2, 3):
        got = gpu_ctx.selftest_transforms(2, log_n, flags, st, coset_mask=mask)
        want = lde.copy()
        for h in range(2):
            if not (mask >> h) & 1:
                want[:, h * n:(h + 1) * n] = R.NOT_A_WORD
        assert_columns_equal(got, want, "chunk LDE, 2^%d rows, flags %d, coset mask %d" % (log_n, flags, mask))


@pytest.mark.parametrize("log_n,flags", [(16, 0), (17, 0), (19, 0), (22, 0), (18, SPLIT), (23, SPLIT)])
def test_quotient_coset_inverse(gpu_ctx, oracle, log_n, flags):
    """quotient_coset_inverse (2^16 rows: ntt_coset_inverse; k_coset_unscale, k_coset_unscale_half): each of the four inputs
    against coset_ifft on its own shift, in the stored layout."""
    qv = R.columns(log_n, [0, 1, 2, 4])   # [alpha][coset]
    got = gpu_ctx.selftest_transforms(3, log_n, flags, qv)
    want = np.stack([R.to_stored(R.quotient_interpolant(oracle, qv[k], k & 1), bool(flags & SPLIT)) for k in range(4)])
    assert_columns_equal(got, want, "coset interpolants, 2^%d rows, flags %d" % (log_n, flags))
    if log_n >= 22:
        gpu_ctx.trim()


@pytest.mark.parametrize("log_n,flags", [(19, 0), (22, 0), (23, SPLIT)])
def test_closed_forms(gpu_ctx, log_n, flags):
    """Impulses against closed forms by Python's pow (no NTT anywhere): a value impulse at j0 has the coefficients N^-1 w_N^(-j0 k)
    (and the LDE values of that geometric sum), a coefficient impulse at k0 the LDE values (g w_2N^m)^k0; 4096 sampled positions
    plus the first and the last of each output."""
    n = 1 << log_n
    split = bool(flags & SPLIT)
    rng = np.random.default_rng(log_n)
    ks = [0, n - 1] + rng.integers(0, n, size=4096).tolist()
    leaves = [0, 2 * n - 1] + rng.integers(0, 2 * n, size=4096).tolist()
    j0s, k0s = (R.M16 + 1, n - 1), (n - 1, R.M16 + 3)
    vals = np.zeros((2, n), np.uint64)
    for c, j0 in enumerate(j0s):
        vals[c, j0] = 1
    got_c, got_l = gpu_ctx.selftest_transforms(0, log_n, flags, vals)
    for c, j0 in enumerate(j0s):
        bad = [(k, hex(int(got_c[c, R.stored_position(k, log_n, split)]))) for k in ks
               if int(got_c[c, R.stored_position(k, log_n, split)]) != R.impulse_coefficient(log_n, j0, k)]
        assert not bad, "value impulse at %d, coefficients (k, got): %s" % (j0, bad[:10])
        bad = [(j, hex(int(got_l[c, j]))) for j in leaves
               if int(got_l[c, j]) != R.impulse_lde_value(log_n, j0, R.leaf_to_natural(j, log_n))]
        assert not bad, "value impulse at %d, LDE (leaf, got): %s" % (j0, bad[:10])
    coef = np.zeros((2, n), np.uint64)
    for c, k0 in enumerate(k0s):
        coef[c, R.stored_position(k0, log_n, split)] = 1
    got = gpu_ctx.selftest_transforms(1, log_n, flags, coef)
    for c, k0 in enumerate(k0s):
        bad = [(j, hex(int(got[c, j]))) for j in leaves if int(got[c, j]) != R.monomial_lde_value(log_n, k0, R.leaf_to_natural(j, log_n))]
        assert not bad, "coefficient impulse at %d, LDE (leaf, got): %s" % (k0, bad[:10])
    if log_n >= 22:
        gpu_ctx.trim()


# ---- the building blocks of the outer passes ------------------------------------------------------------------------------------
FIELD_EDGE = [0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, 2**63 - 1, P - 2**32, P - 2**32 - 1, P - 2**32 + 1,
              2**64 - 2**33, 0xFFFFFFFF00000000, 0xFFFFFFFE00000001, 0xFFFFFFFEFFFFFFFF, 0x00000000FFFFFFFE, 0x0000000100000000,
              0x8000000000000000, 0x7FFFFFFF80000000, 2**48, 2**48 - 1, 2**16, 0xFFFF0000FFFF0001, 0x0000FFFF00000000,
              0x00000001FFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE, 0x1000, 0xFFF, 0xFFFFFFFF00000000 - 1]   # of test_field_asm_edge_cases


def test_mul_2exp_all_shifts(gpu_ctx):
    """mul_2exp3(x, e) = x 2^(3 e) for all e in 0 .. 63 (every branch of gl_mul_2exp: S < 64, 64 <= S < 96, S >= 96 with its
    negation) on boundary operands, random operands and operands of one to three bits and p minus those."""
    rng = np.random.default_rng(6)
    xs = sorted({e % P for e in FIELD_EDGE}) + [int(v) for v in R.rand_field(rng, 20000)]
    for _ in range(10000):
        s = sum(1 << int(k) for k in rng.integers(0, 64, size=rng.integers(1, 4))) % P
        xs += [s, (P - s) % P]
    out = gpu_ctx.selftest_mul_2exp(np.array(xs, dtype=np.uint64))
    tw = [pow(2, 3 * e, P) for e in range(64)]
    want = np.array([[x * t % P for t in tw] for x in xs], dtype=np.uint64)
    if not np.array_equal(out, want):
        bad = np.argwhere(out != want)
        raise AssertionError("%d products differ; first (x, e, got, expected): %s" % (
            len(bad), [(hex(xs[i]), e, hex(int(out[i, e])), hex(int(want[i, e]))) for i, e in bad[:10].tolist()]))


def dft_rows(log_r):
    """Rows of R words: all pairs (a, b, a, b, ...) of edge values, every edge value repeated, random mixtures of edge values,
    random rows; 340 rows at R = 64, more below."""
    r = 1 << log_r
    rng = np.random.default_rng(40 + log_r)
    n_mix = 50 * (64 // r)
    rows = [np.tile(np.array([a, b], dtype=np.uint64), r // 2) for a in R.EDGE for b in R.EDGE]
    rows += [np.full(r, a, dtype=np.uint64) for a in R.EDGE]
    rows += [R.EDGE[rng.integers(0, R.EDGE.size, size=r)] for _ in range(n_mix)]
    rows += [R.rand_field(rng, r) for _ in range(n_mix)]
    return np.stack(rows)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_r", [1, 2, 3, 4, 5, 6])
def test_outer_dft_rows(gpu_ctx, log_r, inverse):
    """dft_small<LOGR, INV> against the O(R^2) sum X[k] = sum_i x[i] w^(i k) on Python integers, w = 2^(192 / R) (inverse: w^-1, no
    factor 1 / R); register r holds X[bitrev(r)], as k_ntt_outer_inv reads it."""
    r = 1 << log_r
    rows = dft_rows(log_r)
    assert rows.shape[0] >= 300
    got = gpu_ctx.selftest_outer_dft(log_r, inverse, rows)
    w = pow(2, 192 // r, P)
    if inverse:
        w = pow(w, P - 2, P)
    mat = np.array([[pow(w, i * k % r, P) for k in range(r)] for i in range(r)], dtype=object)
    x = rows.astype(object).dot(mat) % P                    # x[row][k] on Python integers
    want = np.array([[x[i, bitrev(reg, log_r)] for reg in range(r)] for i in range(rows.shape[0])], dtype=np.uint64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("R = %d, %s: %d registers differ; first (row, register, got, expected): %s" % (
            r, "inverse" if inverse else "forward", len(bad),
            [(i, reg, hex(int(got[i, reg])), hex(int(want[i, reg]))) for i, reg in bad[:10].tolist()]))


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse(gpu_ctx, ref_columns):
    """Every bad argument is BN254S_E_INVALID_ARG before anything is launched, and the context works afterwards."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    n = 1 << 17

    def transforms(op, log_n, flags, ncols, mask, data, out0, out1):
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return lib.bn254s_selftest_transforms(h, op, log_n, flags, ncols, mask, ptr(data), ptr(out0), ptr(out1))

    data = np.zeros((17, n), np.uint64)
    big = np.zeros((4, n), np.uint64)
    o0, o1 = np.zeros((17, 2 * n), np.uint64), np.zeros((17, 2 * n), np.uint64)
    assert transforms(0, 17, 0, 1, 3, None, o0, o1) == E_ARG
    assert transforms(0, 17, 0, 1, 3, data, None, o1) == E_ARG
    assert transforms(0, 17, 0, 1, 3, data, o0, None) == E_ARG
    assert lib.bn254s_selftest_transforms(None, 0, 17, 0, 1, 3, data.ctypes.data_as(C.c_void_p), o0.ctypes.data_as(C.c_void_p),
                                          o1.ctypes.data_as(C.c_void_p)) == E_ARG
    data[0, 5] = np.uint64(P)
    assert transforms(0, 17, 0, 1, 3, data, o0, o1) == E_ARG            # a word equal to p
    data[0, 5] = 0
    assert transforms(0, 24, 0, 1, 3, data, o0, o1) == E_ARG            # (rejected before anything is read)
    assert transforms(0, 15, 0, 1, 3, data, o0, o1) == E_ARG
    assert transforms(0, 17, SPLIT, 1, 3, data, o0, o1) == E_ARG        # the split level starts at 2^18 rows
    assert transforms(0, 23, 0, 1, 3, data, o0, o1) == E_ARG            # 2^23 rows exist only with it
    assert transforms(0, 16, COMPACT, 1, 3, data, o0, o1) == E_ARG
    assert transforms(0, 17, 0, 0, 3, data, o0, o1) == E_ARG
    assert transforms(0, 17, 0, 65, 3, data, o0, o1) == E_ARG
    assert transforms(4, 17, 0, 1, 3, data, o0, o1) == E_ARG
    assert transforms(0, 17, 4, 1, 3, data, o0, o1) == E_ARG
    assert transforms(2, 17, 0, 17, 3, data, o0, None) == E_ARG         # a chunk has at most 16 columns
    assert transforms(1, 17, COMPACT, 17, 3, data, o0, None) == E_ARG   # lde is not chunked: the compact plan's scratch holds 16
    assert transforms(2, 17, 0, 3, 0, data, o0, None) == E_ARG
    assert transforms(2, 17, 0, 3, 4, data, o0, None) == E_ARG
    assert transforms(2, 16, 0, 3, 3, data, o0, None) == E_ARG          # no streaming workspace at 2^16 rows
    assert transforms(3, 17, 0, 3, 3, big, o0, None) == E_ARG           # the quotient is 2 x 2 columns
    x, out = np.zeros(8, np.uint64), np.zeros((8, 64), np.uint64)
    xp, outp = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert lib.bn254s_selftest_mul_2exp(h, None, 8, outp) == E_ARG and lib.bn254s_selftest_mul_2exp(h, xp, 8, None) == E_ARG
    assert lib.bn254s_selftest_mul_2exp(h, xp, 0, outp) == E_ARG
    x[3] = np.uint64(P)
    assert lib.bn254s_selftest_mul_2exp(h, xp, 8, outp) == E_ARG
    assert lib.bn254s_selftest_outer_dft(h, 3, 0, xp, 1, outp) == E_ARG  # (the row holds p)
    x[3] = 0
    for log_r, inverse, rows in ((0, 0, 1), (7, 0, 1), (3, 2, 1), (3, 0, 0)):
        assert lib.bn254s_selftest_outer_dft(h, log_r, inverse, xp, rows, outp) == E_ARG
    assert lib.bn254s_selftest_outer_dft(h, 3, 0, None, 1, outp) == E_ARG and lib.bn254s_selftest_outer_dft(h, 3, 0, xp, 1, None) == E_ARG
    check_commit(gpu_ctx, ref_columns, 17, 0, [0])
