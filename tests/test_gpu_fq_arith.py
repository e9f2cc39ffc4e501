"""The BN254 Fq / Fq2 device arithmetic (csrc/fq_dev.h, csrc/chain_coop.h) at its operand bounds: bn254s_selftest_fq runs the
prover's own inline functions on RAW register contents, so the multiplier really sees p - 1, all-ones limbs, 3x operands on both
sides and values of combine that are exact multiples of p.  Reference: Python integers (tools/fq_operands.py), compared word for
word.  The same table goes through the limb model on the CPU in tests/test_fq_limb_model_cpu.py."""
import numpy as np
import pytest

from tools import fq_operands as T
from tools import synth

pytestmark = pytest.mark.gpu
P = T.P

FQ_NAMES = ("fq_add", "fq_sub", "fq_neg", "fq_dbl", "fq_mul", "fq_sqr", "fq_mul2", "fq_from_canonical", "fq_to_canonical",
            "(a+b)^2", "(3a)^2", "(3a)b", "(a+b)(c-d+2p)", "(a+b+c+d)(a+b-c-d+4p)", "(3a+3b)(3a-3b+6p)", "mul2(3a,b,3c,2p-d)",
            "mul2(3a,3b,3c,6p-3d)")
FQ2_NAMES = ("fq2_mul.c0", "fq2_mul.c1", "fq2_mul(3x).c0", "fq2_mul(3x).c1", "fq2_sqr<2>.c0", "fq2_sqr<2>.c1", "fq2_sqr<4>.c0",
             "fq2_sqr<4>.c1", "fq2_sqr<6>.c0", "fq2_sqr<6>.c1", "fq2_norm", "fq2_neg.c0", "fq2_neg.c1", "fq2_inv.c0", "fq2_inv.c1")
COOP_NAMES = tuple("g1coop::product%r" % (t,) for t in T.PRODUCT_TUPLES) + \
    tuple("g2coop::product%r %s" % (t, w) for t in T.PRODUCT_TUPLES for w in ("c=0", "c=1", "plain")) + \
    tuple("combine%r" % (cs,) for cs in T.COMBINE_SETS)


@pytest.fixture(scope="module")
def tables():
    """The operand tables, built once; they are checked for the extremes they claim before anything runs on them."""
    frows, f2rows = T.field_rows(), T.fq2_rows()
    crows, ctags = T.coop_rows()
    T.check_tables(frows, crows, ctags)
    T.check_tables(f2rows + [(0,) * 4], crows, ctags)   # (the Fq2 table is the same construction without x = 0)
    return {"fq": frows, "fq2": f2rows, "coop": crows}


def assert_exact(rows, got, expected, names):
    """got: uint64[n][4 k] from the GPU, expected: [[int] * k] raw residues; word for word, every output below p."""
    assert all(0 <= v < P for e in expected for v in e)
    exp = T.rows_to_words(expected)
    assert got.shape == exp.shape
    bad = np.argwhere((got != exp).reshape(len(rows), len(names), 4).any(axis=2))
    if bad.size:
        lines = []
        for i, k in bad[:8].tolist():
            g = synth.words_to_int(got[i, 4 * k:4 * k + 4])
            lines.append("row %d %s: got %#x%s, expected %#x, operands %s" % (
                i, names[k], g, " (not below p)" if g >= P else "", expected[i][k], [hex(v) for v in rows[i]]))
        raise AssertionError("%d of %d results differ:\n" % (len(bad), len(rows) * len(names)) + "\n".join(lines))


def test_fq_forms_on_extreme_residues(gpu_ctx, tables):
    rows = tables["fq"]
    got = gpu_ctx.selftest_fq(0, T.rows_to_words(rows))
    assert_exact(rows, got, [T.expect_fq(r) for r in rows], FQ_NAMES)


def test_fq2_forms_on_extreme_residues(gpu_ctx, tables):
    rows = tables["fq2"]
    got = gpu_ctx.selftest_fq(1, T.rows_to_words(rows))
    assert_exact(rows, got, [T.expect_fq2(r) for r in rows], FQ2_NAMES)


def test_cooperative_products_and_combine(gpu_ctx, tables):
    """g1coop::product, g2coop::product and chain_coop::combine read from LDS slots as in the doubling chains; the combine rows
    hold every k p, k p - 1 and k p + 1 each coefficient set can reach, its minimum and its maximum (19 p - 6 for the w set)."""
    rows = tables["coop"]
    got = gpu_ctx.selftest_fq(2, T.rows_to_words(rows))
    assert_exact(rows, got, [T.expect_coop(r) for r in rows], COOP_NAMES)


def test_curve_arithmetic_under_rescaled_z(gpu_ctx):
    """g1_double / g1_add / g2_double / g2_add on Jacobian points with random and extreme Z: the affine result is the affine sum,
    the same point under two Z doubles (code 1), opposite points under two Z report code 2."""
    rows, kinds, points = T.curve_rows()
    assert set(kinds) == {0, 1, 2}
    got = gpu_ctx.selftest_fq(3, T.rows_to_words(rows))
    vals = T.words_to_rows(got[:, :72])
    for i, (kind, (p1, q1, p2, q2)) in enumerate(zip(kinds, points)):
        v = vals[i]
        assert all(x < P for x in v), (i, "a coordinate is not canonical")
        assert (int(got[i, 72]), int(got[i, 73])) == (kind, kind), (i, kind)
        d1, s1, d2, s2 = v[0:3], v[3:6], v[6:12], v[12:18]
        assert T.g1_affine_from_raw(*d1) == synth.g1_add(p1, p1), (i, "g1_double")
        assert T.g2_affine_from_raw(d2) == synth.g2_add(p2, p2), (i, "g2_double")
        if kind == 0:
            assert T.g1_affine_from_raw(*s1) == synth.g1_add(p1, q1), (i, "g1_add")
            assert T.g2_affine_from_raw(s2) == synth.g2_add(p2, q2), (i, "g2_add")
        elif kind == 1:
            assert s1 == d1 and s2 == d2, (i, "an addition of equal points is the doubling of the first")
        else:
            assert s1 == rows[i][0:3] and s2 == rows[i][6:12], (i, "opposite points: the first operand comes back")


def test_selftest_fq_rejects_what_the_kernels_cannot_take(gpu_ctx):
    """With a live context: an unknown group, an operand of p or more, x = 0 for fq2_inv and Z = 0 are refused before any launch."""
    import ctypes as C
    import plonky2_bn254_amd as pk
    lib, E_ARG = pk.load_library(), -1
    h = gpu_ctx._h

    def call(group, rows):
        w = T.rows_to_words(rows)
        out = np.full((w.shape[0], T.OUT_WORDS[group % 4]), 7, np.uint64)
        rc = lib.bn254s_selftest_fq(h, group, w.ctypes.data_as(C.c_void_p), w.shape[0], out.ctypes.data_as(C.c_void_p))
        assert rc == 0 or (out == 7).all()
        return rc

    ok = [(1, 2, 3, 4), (P - 1, 0, P - 1, 0)]
    assert call(0, ok) == 0 and call(1, ok) == 0
    assert call(4, ok) == E_ARG and call(-1, ok) == E_ARG
    for bad in (P, P + 1, (1 << 256) - 1, 1 << 255):
        for pos in range(4):
            row = [1, 2, 3, 4]
            row[pos] = bad
            assert call(0, ok + [tuple(row)]) == E_ARG and call(1, [tuple(row)] + ok) == E_ARG
    assert call(2, [(1,) * 7 + (P,)]) == E_ARG and call(2, [(P - 1,) * 8]) == 0
    assert call(1, ok + [(0, 0, 5, 6)]) == E_ARG and call(0, [(0, 0, 5, 6)]) == 0 and call(1, [(0, 1, 0, 0)]) == 0
    rows, _, _ = T.curve_rows(n=2)
    assert call(3, rows) == 0
    for zpos in ((2,), (5,), (10, 11), (16, 17)):   # Z of G1 P, G1 Q, G2 P, G2 Q
        r = list(rows[0])
        for k in zpos:
            r[k] = 0
        assert call(3, [rows[1], r]) == E_ARG
    r = list(rows[0])
    r[10] = 0                                        # one component of an Fq2 Z may vanish
    r[11] = r[11] or 1
    assert call(3, [r]) == 0
    with pytest.raises(ValueError):
        gpu_ctx.selftest_fq(4, T.rows_to_words(ok))
