"""No GPU: the limb-level model of csrc/fq_dev.h and csrc/chain_coop.h (tools/fq_limb_model.py: u64 column sums, u32 limbs, the
signed 32-bit carry chains) on the operand table of tests/test_gpu_fq_arith.py.  The model must agree with big integers without
any overflow and without a value of 2p or more before a conditional subtraction; its largest column sum and limb are the
figures quoted in fq_dev.h.  Then single faults are switched on in the model: the table has to catch each of them, which is how
it earns trust without a mutated GPU build.  Also the argument checks of bn254s_selftest_fq that need no context."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import fq_limb_model as M
from tools import fq_operands as T

P = T.P


@pytest.fixture(scope="module")
def tables():
    frows, f2rows = T.field_rows(), T.fq2_rows()
    crows, ctags = T.coop_rows()
    T.check_tables(frows, crows, ctags)
    return {"fq": frows, "fq2": f2rows, "coop": crows,
            "fq_exp": [T.expect_fq(r) for r in frows], "fq2_exp": [T.expect_fq2(r)[:13] for r in f2rows],
            "coop_exp": [T.expect_coop(r) for r in crows]}


def test_model_agrees_with_big_integers_within_the_register_widths(tables):
    m = M.Model()
    assert M.replay_fq(m, tables["fq"]) == tables["fq_exp"]
    assert M.replay_fq2(m, tables["fq2"]) == tables["fq2_exp"]
    got, _ = M.replay_coop(m, tables["coop"])
    assert got == tables["coop_exp"]
    col, limb = m.max_col.bit_length(), m.max_limb.bit_length()
    print("largest column sum %d bits (%.3f * 2^60), largest operand limb %d bits (%.3f * 2^26)"
          % (col, m.max_col / 2.0 ** 60, limb, m.max_limb / 2.0 ** 26))
    # the figures in the loose-operand comment of fq_dev.h; the limb is that of fq_sub_lazy<6> of a 3x operand, just below 7 * 2^26
    assert (col, limb) == (60, 29)
    assert 6 << 26 < m.max_limb < 7 << 26


def test_combine_quotient_estimate_is_exact_or_one_short(tables):
    """q from the top limb is never above floor(value / p) and at most one below it, at every k p, k p - 1 and k p + 1; both cases
    occur, and the value stays below 32 p (top limb below 2^25)."""
    _, qs = M.replay_coop(M.Model(), tables["coop"])
    for cs, (q, top) in zip(T.COMBINE_SETS, qs):
        short = set()
        for r, qi, ti in zip(tables["coop"], q, top):
            v = T.combine_value(cs, r[:4])
            assert ti == v >> 234 and 0 <= v // P - qi <= 1, (cs, hex(v), qi)
            short.add(v // P - qi)
        assert short == {0, 1}, cs
        lo, hi = T.combine_range(cs)
        reached = {T.combine_value(cs, r[:4]) for r in tables["coop"]}
        assert {lo, hi} <= reached and all(k * P + d in reached for k, d in T.combine_targets(cs))


def _caught(replay, expected):
    try:
        return replay() != expected
    except M.ModelError:
        return True


def _combine_only(m, rows, ci):
    cs = T.COMBINE_SETS[ci]
    s = [M.to_limbs([r[i] for r in rows]) for i in range(4)]
    return M.to_ints(m.combine(s, cs[:4], cs[4])[0])


@pytest.mark.parametrize("fault", M.FAULTS)
def test_the_table_catches_a_faulty_model(tables, fault):
    m = M.Model(faults=(fault,))
    if fault in ("off_minus_one", "q_from_p9"):      # combine: each coefficient set on its own
        rows = tables["coop"]
        for ci, cs in enumerate(T.COMBINE_SETS):
            exp = [T.combine_value(cs, r[:4]) % P for r in rows]
            assert _combine_only(M.Model(), rows, ci) == exp
            assert _caught(lambda: _combine_only(m, rows, ci), exp), (fault, cs)
    else:
        assert _caught(lambda: M.replay_fq(m, tables["fq"]), tables["fq_exp"]), fault
        if fault != "skip_cond_sub":                 # (the lazy subtractions of the Fq2 forms and of g2coop::product too)
            assert _caught(lambda: M.replay_fq2(m, tables["fq2"]), tables["fq2_exp"]), fault


def test_a_skipped_conditional_subtraction_shows_in_the_results(tables):
    """That fault leaves every register in range, so nothing in the model can assert: the RESULTS must differ from big integers
    on a good part of the table (results are all the GPU test sees)."""
    got = M.replay_fq(M.Model(faults=("skip_cond_sub",)), tables["fq"])
    assert sum(g != e for g, e in zip(got, tables["fq_exp"])) > len(got) // 4


def test_selftest_fq_without_a_context():
    """bn254s_selftest_fq(NULL, ...) is BN254S_E_INVALID_ARG whatever else is passed and writes nothing (the cases that need a
    context - an unknown group, an operand of p or more, x = 0 for fq2_inv, Z = 0 - are in tests/test_gpu_fq_arith.py)."""
    lib, E_ARG = pk.load_library(), -1
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    good = T.rows_to_words([(1, 2, 3, 4), (P - 1, P - 2, 0, 1)])
    for group, rows in ((0, good), (1, good), (7, good), (-1, good), (0, T.rows_to_words([(P, 0, 0, 0)])),
                        (1, T.rows_to_words([(0, 0, 1, 1)]))):
        out = np.full((rows.shape[0], 92), 7, np.uint64)
        assert lib.bn254s_selftest_fq(None, group, vp(rows), rows.shape[0], vp(out)) == E_ARG
        assert lib.bn254s_selftest_fq(None, group, vp(rows), 0, vp(out)) == E_ARG
        assert (out == 7).all()
    assert lib.bn254s_selftest_fq(None, 0, None, 2, None) == E_ARG
    assert pk.Context.SELFTEST_FQ_WORDS == tuple(zip(T.IN_WORDS, T.OUT_WORDS))
