"""The LogUp columns from the per-proof inverse table (csrc/aux.hip: k_logup_inv_table, k_logup_helpers, k_logup_terms, k_scan)
through bn254s_selftest_logup, which runs the provers' aux_build on a caller's trace: every helper and every running-sum element
against Python big integers.

Shapes: 2^9 and 2^10 rows (one and four blocks of the helper kernel, a scan block of fewer than and of exactly 1024 threads),
6 and 7 range-checked columns (even count / single-column last helper).  The columns hold 0, 1, 65534, 65535, one value repeated
down a whole column and random 16-bit values.  The second challenge is p - 30000: beta + v wraps past p for every v >= 30000 (the
canonical-add edge of the table fill), and beta + 30000 = 0, the one denominator without an inverse, whose table entry is 0 as
pow(0, p - 2, p) is.  A value of 65536 never indexes past the table (the index is masked in logup_inv_at): it comes back as
BN254S_E_INTERNAL (-7), and the context goes on working."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0xFFFFFFFF00000001
BETAS = (0x9E3779B97F4A7C15 % P, P - 30000)
RC_BEGIN = 1   # one unrelated column in front


def make_trace(rows, n_rc, seed):
    """[junk | n_rc range-checked | table | freq] x rows."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n_rc + 3, rows), np.uint64)
    t[0] = rng.integers(0, P, size=rows, dtype=np.uint64)
    rc = rng.integers(0, 65536, size=(n_rc, rows), dtype=np.uint64)
    rc[0, :8] = [0, 1, 65534, 65535, 65535, 0, 30000, 29999]
    rc[1, :8] = [65535, 65534, 1, 0, 65535, 0, 30001, 30000]
    rc[2, :] = 65535                      # one value down a whole column
    rc[3, :] = 0
    rc[n_rc - 1, -4:] = [65535, 0, 1, 65534]   # (the single column of the odd last helper when n_rc is odd)
    t[RC_BEGIN:RC_BEGIN + n_rc] = rc
    table = rng.integers(0, 65536, size=rows, dtype=np.uint64)
    table[:4] = [0, 65535, 30000, 1]
    t[RC_BEGIN + n_rc] = table
    freq = rng.integers(0, P, size=rows, dtype=np.uint64)
    freq[:3] = [0, P - 1, 1]
    t[RC_BEGIN + n_rc + 1] = freq
    return t


def expected(trace, n_rc):
    rows = trace.shape[1]
    m = (n_rc + 1) // 2
    tr = [[int(v) for v in col] for col in trace]
    out = np.zeros((2 * (m + 1), rows), np.uint64)
    for ch, beta in enumerate(BETAS):
        inv = {}

        def iv(v):
            if v not in inv:
                inv[v] = pow((beta + v) % P, P - 2, P)
            return inv[v]

        z = 0
        for i in range(rows):
            out[ch * (m + 1) + m, i] = z
            tot = 0
            for k in range(m):
                h = iv(tr[RC_BEGIN + 2 * k][i])
                if 2 * k + 1 < n_rc:
                    h = (h + iv(tr[RC_BEGIN + 2 * k + 1][i])) % P
                out[ch * (m + 1) + k, i] = h
                tot += h
            z = (z + tot - tr[RC_BEGIN + n_rc + 1][i] * iv(tr[RC_BEGIN + n_rc][i])) % P
    return out


CASES = [(9, 6), (9, 7), (10, 6), (10, 7)]


@pytest.fixture(scope="module")
def references():
    ref = {}
    for log_rows, n_rc in CASES:
        t = make_trace(1 << log_rows, n_rc, seed=100 * log_rows + n_rc)
        ref[log_rows, n_rc] = (t, expected(t, n_rc))
    return ref


@pytest.mark.parametrize("log_rows,n_rc", CASES)
def test_logup_columns_match_big_integers(gpu_ctx, references, log_rows, n_rc):
    trace, want = references[log_rows, n_rc]
    got = gpu_ctx.selftest_logup(trace, RC_BEGIN, n_rc, RC_BEGIN + n_rc, RC_BEGIN + n_rc + 1, BETAS)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{bad.shape[0]} elements differ, first at (column, row) {tuple(bad[0])}"


def test_value_above_16_bits_is_an_error_code_and_the_context_survives(gpu_ctx, references):
    trace, want = references[9, 7]
    args = (RC_BEGIN, 7, RC_BEGIN + 7, RC_BEGIN + 8, BETAS)
    for col, row in ((RC_BEGIN + 4, 77), (RC_BEGIN + 6, 511), (RC_BEGIN + 7, 5)):   # a pair column, the single last one, the table
        bad = trace.copy()
        bad[col, row] = 65536
        with pytest.raises(RuntimeError, match="-7"):
            gpu_ctx.selftest_logup(bad, *args)
    assert np.array_equal(gpu_ctx.selftest_logup(trace, *args), want)


def test_argument_errors(gpu_ctx, references):
    trace, _ = references[9, 6]
    notcanon = trace.copy()
    notcanon[0, 3] = P
    for t, a in ((notcanon, (RC_BEGIN, 6, 7, 8, BETAS)), (trace, (RC_BEGIN, 9, 7, 8, BETAS)), (trace, (RC_BEGIN, 6, 9, 8, BETAS)),
                 (trace, (RC_BEGIN, 6, 7, 8, (P, 1))), (trace[:, :48], (RC_BEGIN, 6, 7, 8, BETAS))):
        with pytest.raises(RuntimeError, match="-1"):
            gpu_ctx.selftest_logup(t, *a)
