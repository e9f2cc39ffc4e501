"""All auxiliary columns of the three STARK kinds through bn254s_selftest_aux (the provers' aux_build with the kind's real shape):
the LogUp helpers and running sums, and the CTL Z columns, which bn254s_selftest_logup leaves out - k_ctl_terms and the suffix mode
of k_scan - word for word against the oracle's lookup_helper_columns and ctl_z_column (orc_aux_columns).

Rows: 64 (a scan block of 64 threads), 1024 (one element per scan thread), 4096 (four per thread: the inner loops of k_scan in
both modes).  Filter patterns per CTL: all 0, all 1, first row only, last row only, alternating, random.  Range-checked cells:
random 16-bit values, all 0, all 65535; multiplicities up to p - 1.  The betas keep beta + v != 0 for every v <= 65535 (asserted),
so every denominator has an inverse on both sides.  A filter value of 2 is BN254S_E_INTERNAL (-7), "Non-binary filter?" in the
oracle, and the context goes on working."""
import numpy as np
import pytest

from tests import oracle_lib
from tools import quotient_ref as qr

pytestmark = pytest.mark.gpu

P = qr.P
KINDS = (0, 1, 2)
BETAS = (0x9E3779B97F4A7C15 % P, P - 65536)   # the second: beta + 65535 = p - 1, the largest sum that does not wrap
GAMMAS = (0x243F6A8885A308D3 % P, P - 1)
for _b in BETAS:
    assert 1 <= _b <= P - 65536   # beta + v = 0 (mod p) for no v in 0 .. 65535


def pattern(name, rows, rng):
    f = np.zeros(rows, np.uint64)
    if name == "ones":
        f[:] = 1
    elif name == "first":
        f[0] = 1
    elif name == "last":
        f[-1] = 1
    elif name == "alternating":
        f[1::2] = 1
    elif name == "random":
        f[:] = rng.integers(0, 2, size=rows, dtype=np.uint64)
    else:
        assert name == "zeros"
    return f


def make_trace(kind, rows, f0, f1, rc, seed):
    lay = qr.LAYOUTS[kind]
    rng = np.random.default_rng(seed)
    t = qr.rand_field(rng, (lay.W, rows))
    n_rc = lay.RC_END - lay.RC_BEGIN
    if rc == "random":
        t[lay.RC_BEGIN:lay.RC_END] = rng.integers(0, 65536, size=(n_rc, rows), dtype=np.uint64)
        t[lay.RC_BEGIN, :4] = [0, 65535, 1, 65534]
    else:
        t[lay.RC_BEGIN:lay.RC_END] = int(rc)
    t[lay.RANGE] = rng.integers(0, 65536, size=rows, dtype=np.uint64)
    t[lay.RANGE, :2] = [0, 65535]
    t[lay.FREQ, :3] = [P - 1, 0, 1]
    t[lay.ctl_filter[0]] = pattern(f0, rows, rng)
    t[lay.ctl_filter[1]] = pattern(f1, rows, rng)
    return t


# (rows, filter of CTL 0, filter of CTL 1, range-checked cells)
CASES = [(64, "zeros", "ones", "random"), (64, "random", "first", "65535"),
         (1024, "first", "last", "0"), (1024, "alternating", "random", "random"),
         (4096, "random", "alternating", "random"), (4096, "last", "zeros", "65535"), (4096, "ones", "random", "0")]


@pytest.mark.parametrize("rows,f0,f1,rc", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_aux_columns_match_the_oracle(gpu_ctx, oracle, kind, rows, f0, f1, rc):
    lay = qr.LAYOUTS[kind]
    trace = make_trace(kind, rows, f0, f1, rc, seed=rows + kind)
    want = oracle_lib.aux_columns(oracle, kind, trace, BETAS, GAMMAS)
    got = gpu_ctx.selftest_aux(kind, trace, BETAS, GAMMAS)
    assert got.shape == want.shape == (lay.n_aux, rows)
    bad = np.argwhere(got != want)
    names = {lay.m: "LogUp Z 0", 2 * lay.m + 1: "LogUp Z 1"}
    names.update({2 * (lay.m + 1) + i: f"CTL {i // 2} Z of challenge {i % 2}" for i in range(4)})
    assert bad.size == 0, (f"{bad.shape[0]} words differ, first at (column, row) {tuple(int(v) for v in bad[0])} "
                           f"({names.get(int(bad[0][0]), 'helper')})")
    # the Z columns mean what the constraints say: LogUp Z starts at 0; a CTL Z with an empty filter is 0 throughout
    assert not got[lay.m, 0] and not got[2 * lay.m + 1, 0]
    for ctl, f in enumerate((f0, f1)):
        if f == "zeros":
            assert not got[2 * (lay.m + 1) + 2 * ctl: 2 * (lay.m + 1) + 2 * ctl + 2].any()


@pytest.mark.parametrize("kind", KINDS)
def test_non_binary_filter_is_an_error_and_the_context_survives(gpu_ctx, oracle, kind):
    lay = qr.LAYOUTS[kind]
    trace = make_trace(kind, 1024, "random", "random", "random", seed=7)
    want = oracle_lib.aux_columns(oracle, kind, trace, BETAS, GAMMAS)
    for ctl, row in ((0, 0), (1, 1023), (1, 300)):
        bad = trace.copy()
        bad[lay.ctl_filter[ctl], row] = 2
        with pytest.raises(RuntimeError, match="failed with -7"):
            gpu_ctx.selftest_aux(kind, bad, BETAS, GAMMAS)
        with pytest.raises(RuntimeError, match="Non-binary filter"):
            oracle_lib.aux_columns(oracle, kind, bad, BETAS, GAMMAS)
    assert np.array_equal(gpu_ctx.selftest_aux(kind, trace, BETAS, GAMMAS), want)


def test_argument_errors(gpu_ctx):
    trace = make_trace(2, 64, "ones", "ones", "random", seed=1)
    for t, b, g in ((trace[:, :32], BETAS, GAMMAS), (trace[:, :48], BETAS, GAMMAS), (trace, (P, 1), GAMMAS), (trace, BETAS, (0, P))):
        with pytest.raises(RuntimeError, match="failed with -1"):
            gpu_ctx.selftest_aux(2, np.ascontiguousarray(t), b, g)
    bad = trace.copy()
    bad[100, 5] = P
    with pytest.raises(RuntimeError, match="failed with -1"):
        gpu_ctx.selftest_aux(2, bad, BETAS, GAMMAS)
    # a range-checked value above 65535 is found on the device, as in bn254s_selftest_logup
    bad = trace.copy()
    bad[qr.LAYOUTS[2].RC_BEGIN + 1, 9] = 65536
    with pytest.raises(RuntimeError, match="failed with -7"):
        gpu_ctx.selftest_aux(2, bad, BETAS, GAMMAS)
    assert gpu_ctx.selftest_aux(2, trace, BETAS, GAMMAS).shape == (134, 64)
