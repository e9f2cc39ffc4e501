"""The quotient (AIR constraint) kernels point by point: csrc/quotient_g1.hip, quotient_g2fq.hip, quotient_sched.h and
lookup_and_ctl_constraints of quotient_common.h, through bn254s_selftest_quotient, which runs the provers' quotient_host_tables,
quotient_fill_args / quotient_window_args and quotient_launch on caller columns.

For every point the oracle gives the K constraint values in emission order (orc_eval_vanishing_values; established in
tests/test_vanishing_ref_cpu.py); Python integers weight them with alpha^(K-1-e) (tools/quotient_ref.py).  Checked, exactly:
  * each part kernel's two partial sums against the weighted sum over the constraint range the part owns (quotient_ref.PARTS);
  * out - sum(parts) against the lookup + CTL range (raw mode), out against the whole sum times 1 / Z_H of the coset (prover mode);
  * part slots and output words that no lane owns keep the sentinel they were filled with.
Modes: the library's point tables with z_last = x - w^-1 and the division by Z_H (what the provers run), and caller tables with
zh_inv = 1, w_inv = 0 (what bn254s_verify runs).  Shapes: 128 points (fewer than a workgroup: the j >= count guard), 256 (one
workgroup, the verifier's shape), 512 (two workgroups); windows of 300 rows (ragged, two workgroups) of a 2^10 domain at the
start, inside and at the end of each coset.  A failure names the kind, the part, its constraint range and the first point."""
import functools

import numpy as np
import pytest

from tests import oracle_lib
from tools import quotient_ref as qr
from tools import synth

pytestmark = pytest.mark.gpu

P = qr.P
KINDS = (0, 1, 2)
SENT = 0xDEADBEEF12345678   # canonical, and no sum of anything here
assert SENT < P


@functools.lru_cache(maxsize=None)
def leaf_tables(log_n):
    return qr.tables_leaf(log_n)


@functools.lru_cache(maxsize=None)
def leaf_maps(log_n):
    m = 2 << log_n
    hk = [qr.leaf_point(log_n, j) for j in range(m)]
    return (np.array([h for h, _ in hk]), np.array([k for _, k in hk]), np.array([qr.next_leaf(log_n, j) for j in range(m)], np.uint64))


def random_tables(n, seed):
    return qr.rand_field(np.random.default_rng(seed), (3, n))


def compare(kind, tag, values, alphas, got_out, got_part, zh_inv, raw):
    """values[n][K] (object) of n points; got_out[2][n], got_part[7][2][n]: the device's words for the same points;
    zh_inv[n] (object): what the sum of a point is multiplied with."""
    lay = qr.LAYOUTS[kind]
    parts = qr.PARTS[kind]
    for p in range(len(parts), got_part.shape[0]):
        assert (got_part[p] == np.uint64(SENT)).all(), f"{tag}: part slot {p} is no part of kind {kind} and was written"
    for a in range(2):
        w = qr.weights(int(alphas[a]), lay.K)
        total = np.zeros(values.shape[0], dtype=object)
        dev_sum = np.zeros(values.shape[0], dtype=object)
        for p, (lo, hi) in sorted(parts.items()):
            want = qr.weighted(values, w, lo, hi)
            got = qr.to_object(got_part[p][a])
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (f"{tag}: part {p} (constraints {lo}..{hi - 1}), alpha {a}: {bad.size} of {got.size} points differ, "
                                   f"first at point {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")
            total = total + want
            dev_sum = dev_sum + got
        look = qr.weighted(values, w, lay.n_constraints, lay.K)
        out = qr.to_object(got_out[a])
        if raw:
            rest = (out - dev_sum) % P
            bad = np.nonzero(rest != look)[0]
            assert bad.size == 0, (f"{tag}: lookups + CTLs (constraints {lay.n_constraints}..{lay.K - 1}), alpha {a}: {bad.size} points "
                                   f"differ, first at point {bad[0]}")
        want = (total + look) % P * zh_inv % P
        bad = np.nonzero(out != want)[0]
        assert bad.size == 0, f"{tag}: output, alpha {a}: {bad.size} points differ, first at point {bad[0]}"


def run_whole(ctx, oracle, kind, log_n, trace, aux, ch, raw, tables, tag):
    """One whole-domain launch against the oracle; returns the device's (out, part)."""
    alphas, betas, gammas = ch
    n = 1 << log_n
    hs, ks, nxt = leaf_maps(log_n)
    tab = leaf_tables(log_n) if tables is None else tables
    w_inv = 0 if raw else qr.w_inv(log_n)
    z_last = np.array([(int(x) - w_inv) % P for x in tab[0]], dtype=np.uint64)
    idx = np.arange(2 * n, dtype=np.uint64)
    values = qr.to_object(oracle_lib.vanishing_values_at(oracle, kind, trace, aux, idx, nxt, betas, gammas, z_last, tab[1], tab[2]))
    assert values.shape == (2 * n, qr.LAYOUTS[kind].K)
    out, part = ctx.selftest_quotient(kind, log_n, trace, aux, alphas, betas, gammas, raw=raw, tables=tables, fill=SENT)
    zi = [1, 1] if raw else [qr.zh_inv(log_n, 0), qr.zh_inv(log_n, 1)]
    zh = np.array([zi[h] for h in hs], dtype=object)
    compare(kind, f"kind {kind}, 2^{log_n} rows, {tag}", values, alphas, out[:, hs, ks], part, zh, raw)
    return out, part


def both_modes(ctx, oracle, kind, log_n, trace, aux, ch, tag, seed):
    run_whole(ctx, oracle, kind, log_n, trace, aux, ch, False, None, tag + ", prover mode, library tables")
    run_whole(ctx, oracle, kind, log_n, trace, aux, ch, True, random_tables(2 << log_n, seed), tag + ", raw mode, caller tables")


@pytest.fixture(scope="module")
def challenges():
    return qr.challenge_sets(seed=2025)


@pytest.mark.parametrize("log_n", [6, 7, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_whole_domain_shapes(gpu_ctx, oracle, challenges, kind, log_n):
    trace, aux = qr.dataset(kind, "random", 2 << log_n, seed=10 * kind + log_n)
    both_modes(gpu_ctx, oracle, kind, log_n, trace, aux, challenges["random"], "random columns", seed=log_n)


@pytest.mark.parametrize("name", ["zero", "pm1", "edge", "binary"])
@pytest.mark.parametrize("kind", KINDS)
def test_data_sets(gpu_ctx, oracle, challenges, kind, name):
    """All zero (only the constants that stand under no filter survive: the -1 of the helper constraints and the 65535 of the range
    counter's last row; 511, OFF * sum(u) and the a = 1 group of Fq are multiplied by a filter or flag and need the sets below),
    all p - 1 (maximal carries: the overflow word of conv16, the largest seeds), dense mixtures of boundary words, and random
    columns whose flag, filter and bit columns are 0 / 1 (1 - bit, filter - is_last, 2 iqp - 1 take the values 0, 1, p - 1; the
    constants meet a filter of exactly 1)."""
    log_n = 7
    trace, aux = qr.dataset(kind, name, 2 << log_n, seed=77 + kind)
    both_modes(gpu_ctx, oracle, kind, log_n, trace, aux, challenges["random"], f"data set {name}", seed=5)


CHALLENGE_NAMES = sorted(qr.challenge_sets(0))


@pytest.mark.parametrize("name", [c for c in CHALLENGE_NAMES if c != "random"])
@pytest.mark.parametrize("kind", KINDS)
def test_challenge_values(gpu_ctx, oracle, challenges, kind, name):
    """alpha = 0 leaves one weight, alpha = 1 all ones, alpha = p - 1 gives +-1 weights with full top limbs; beta and gamma at 0, 1
    and p - 1 in the lookup and CTL constraints.  The binary data set, so that the special values meet 0 / 1 flags."""
    log_n = 6
    trace, aux = qr.dataset(kind, "binary", 2 << log_n, seed=300 + kind)
    run_whole(gpu_ctx, oracle, kind, log_n, trace, aux, challenges[name], False, None, f"challenges {name}, prover mode")
    if name.startswith("alpha"):
        run_whole(gpu_ctx, oracle, kind, log_n, trace, aux, challenges[name], True, random_tables(2 << log_n, 8),
                  f"challenges {name}, raw mode, caller tables")


# ---- window mode -------------------------------------------------------------------------------------------------------------
WLOG, WCOUNT, WSTRIDE = 10, 300, 333
WK0 = (0, 212, (1 << WLOG) - WCOUNT)


def check_untouched(out, part, kind, h, k0, count, tag):
    mask = np.ones(out.shape, bool)
    mask[:, h, k0:k0 + count] = False
    assert (out[mask] == np.uint64(SENT)).all(), f"{tag}: output words outside rows {k0}..{k0 + count - 1} of coset {h} were written"
    assert (out[:, h, k0:k0 + count] != np.uint64(SENT)).all(), f"{tag}: output words of the window were not written"
    assert (part[:, :, count:] == np.uint64(SENT)).all(), f"{tag}: part words past the window's {count} points were written"


@pytest.mark.parametrize("k0", WK0)
@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_window_against_the_oracle(gpu_ctx, oracle, challenges, kind, h, k0):
    """Natural-order windows as the streaming prover cuts them: the library's window tables, z_last = x - w^-1, 1 / Z_H."""
    tag = f"kind {kind}, window of {WCOUNT} rows from {k0} of coset {h}"
    alphas, betas, gammas = challenges["random"]
    trace, aux = qr.dataset(kind, "random", WSTRIDE, seed=900 + 10 * kind + h)
    tab = qr.tables_window(WLOG, h, k0, WCOUNT)
    wi = qr.w_inv(WLOG)
    z_last = np.array([(int(x) - wi) % P for x in tab[0]], dtype=np.uint64)
    idx = np.arange(WCOUNT, dtype=np.uint64)
    values = qr.to_object(oracle_lib.vanishing_values_at(oracle, kind, trace, aux, idx, idx + np.uint64(1), betas, gammas, z_last,
                                                         tab[1], tab[2]))
    out, part = gpu_ctx.selftest_quotient(kind, WLOG, trace, aux, alphas, betas, gammas, window=(h, k0, WCOUNT), fill=SENT)
    check_untouched(out, part, kind, h, k0, WCOUNT, tag)
    zh = np.array([qr.zh_inv(WLOG, h)] * WCOUNT, dtype=object)
    compare(kind, tag, values, alphas, out[:, h, k0:k0 + WCOUNT], part[:, :, :WCOUNT], zh, False)


@pytest.fixture(scope="module")
def whole8(gpu_ctx, oracle, challenges):
    """Per kind: random leaf-order columns of a 2^8 domain, random caller tables, and the device's raw results on them (themselves
    checked against the oracle)."""
    res = {}
    for kind in KINDS:
        trace, aux = qr.dataset(kind, "random", 512, seed=4000 + kind)
        tab = random_tables(512, 41 + kind)
        out, part = run_whole(gpu_ctx, oracle, kind, 8, trace, aux, challenges["random"], True, tab, "window source, raw mode")
        res[kind] = (trace, aux, tab, out, part)
    return res


@pytest.mark.parametrize("k0", WK0)
@pytest.mark.parametrize("h", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_window_equals_whole_domain(gpu_ctx, challenges, whole8, kind, h, k0):
    """The two addressing modes on the same rows: a window's 301 rows are cut out of the leaf-order data of a 2^8 domain (rows
    s, s + 1, ... modulo 256 of coset h), with the caller tables of the same points; parts and outputs must be the words of the
    whole-domain launch."""
    tag = f"kind {kind}, window of {WCOUNT} rows from {k0} of coset {h} against leaf order"
    alphas, betas, gammas = challenges["random"]
    trace8, aux8, tab8, out8, part8 = whole8[kind]
    rows = [(k0 + j) % 256 for j in range(WCOUNT + 1)]
    pos = np.array([qr.leaf_index(8, h, r) for r in rows])
    trace = np.zeros((trace8.shape[0], WSTRIDE), np.uint64)
    aux = np.zeros((aux8.shape[0], WSTRIDE), np.uint64)
    trace[:, :WCOUNT + 1] = trace8[:, pos]
    aux[:, :WCOUNT + 1] = aux8[:, pos]
    tab = np.ascontiguousarray(tab8[:, pos[:WCOUNT]])
    out, part = gpu_ctx.selftest_quotient(kind, WLOG, trace, aux, alphas, betas, gammas, raw=True, window=(h, k0, WCOUNT),
                                          tables=tab, fill=SENT)
    check_untouched(out, part, kind, h, k0, WCOUNT, tag)
    for p in qr.PARTS[kind]:
        bad = np.argwhere(part[p][:, :WCOUNT] != part8[p][:, pos[:WCOUNT]])
        assert bad.size == 0, f"{tag}: part {p}: {bad.shape[0]} words differ, first at (alpha, point) {tuple(int(v) for v in bad[0])}"
    want = out8[:, h, rows[:WCOUNT]]
    bad = np.argwhere(out[:, h, k0:k0 + WCOUNT] != want)
    assert bad.size == 0, f"{tag}: output: {bad.shape[0]} words differ, first at (alpha, point) {tuple(int(v) for v in bad[0])}"


# ---- point tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [6, 10])
def test_point_tables(gpu_ctx, log_n):
    n = 1 << log_n
    leaf = gpu_ctx.selftest_point_tables(log_n)
    want = leaf_tables(log_n)
    bad = np.argwhere(leaf != want)
    assert bad.size == 0, f"leaf-order tables of 2^{log_n} rows: {bad.shape[0]} words differ, first at (table, leaf) {tuple(int(v) for v in bad[0])}"
    for h, k0, count in ((0, 0, 1), (1, 0, n), (0, n // 2 - 3, 37), (1, n - 45, 45), (0, n - 3, 9), (1, 17, min(300, n))):
        win = gpu_ctx.selftest_point_tables(log_n, window=(h, k0, count))
        assert np.array_equal(win, qr.tables_window(log_n, h, k0, count)), (h, k0, count)
        pos = [qr.leaf_index(log_n, h, (k0 + j) % n) for j in range(count)]
        assert np.array_equal(win, leaf[:, pos]), f"window ({h}, {k0}, {count}) disagrees with the leaf-order tables"


# ---- honest rows through the device -------------------------------------------------------------------------------------------
def test_honest_rows_vanish_on_the_device(gpu_ctx):
    """Fq-exp kind, no oracle: the device's trace and the device's auxiliary columns of 2^16 rows, windows of 257 rows with the
    true subgroup selectors as caller tables (raw mode: x is z_last = w^k - w^-1, L_first = [k = 0], L_last = [k = N - 1]).  Every
    part and every output is 0; after one corrupted cell the part that owns its constraint, or the output alone, is not."""
    kind, log_n = 2, 16
    n = 1 << log_n
    lay = qr.LAYOUTS[kind]
    s, x = synth.fq_inputs(128, seed=31)
    trace, _ = gpu_ctx.generate_trace(kind, s, x)
    assert trace.shape == (lay.W, n)
    rng = np.random.default_rng(17)
    alphas, betas, gammas = (tuple(int(v) for v in qr.rand_field(rng, 2)) for _ in range(3))
    aux = gpu_ctx.selftest_aux(kind, trace, betas, gammas)
    w, wi = qr.root_of_unity(log_n), qr.w_inv(log_n)

    def run(k0, t=trace, a=aux):
        rows = [(k0 + j) % n for j in range(257)]
        tab = np.zeros((3, 256), np.uint64)
        xk = pow(w, k0, P)
        for j in range(256):
            tab[0, j] = (xk - wi) % P
            tab[1, j] = int(rows[j] == 0)
            tab[2, j] = int(rows[j] == n - 1)
            xk = xk * w % P
        out, part = gpu_ctx.selftest_quotient(kind, log_n, np.ascontiguousarray(t[:, rows]), np.ascontiguousarray(a[:, rows]), alphas,
                                              betas, gammas, raw=True, window=(0, k0, 256), tables=tab, fill=SENT)
        return out[:, 0, k0:k0 + 256], part[:2, :, :256]

    for k0 in (0, 384, n - 256):   # row 0, around the instance boundary 511 / 512, the last rows with row 0 as their next
        out, part = run(k0)
        assert not part.any(), f"window at {k0}: non-zero part sums at (part, alpha, point) {np.argwhere(part != 0)[:4].tolist()}"
        assert not out.any(), f"window at {k0}: non-zero outputs at (alpha, point) {np.argwhere(out != 0)[:4].tolist()}"
    # a limb of the product's operand a: the multiplication block (part 0) of that row
    t = trace.copy()
    t[lay.A + 3, 400] ^= np.uint64(1)
    out, part = run(384, t=t)
    assert part[0, :, 16].all() and not np.delete(part[0], 16, axis=1).any()
    assert out[:, 16].all()
    # a bit of the scalar: the schedule (part 1)
    t = trace.copy()
    t[lay.BITS + 9, 1] ^= np.uint64(1)
    out, part = run(0, t=t)
    assert part[1].any() and not part[0].any() and out.any()
    # a CTL Z and a LogUp helper: no part, the output alone (finish_point adds the lookups and CTLs)
    for col, row in ((2 * (lay.m + 1) + 2, n - 1), (5, n - 200)):
        a = aux.copy()
        a[col, row] = (int(a[col, row]) + 1) % P
        out, part = run(n - 256, a=a)
        assert not part.any() and out[:, row - (n - 256)].all(), (col, row)


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu_ctx, challenges):
    kind, log_n = 2, 3
    alphas, betas, gammas = challenges["random"]
    trace, aux = qr.dataset(kind, "random", 16, seed=1)
    ok = gpu_ctx.selftest_quotient(kind, log_n, trace, aux, alphas, betas, gammas, fill=SENT)

    def refused(**kw):
        args = dict(kind=kind, log_n=log_n, trace=trace, aux=aux, alphas=alphas, betas=betas, gammas=gammas)
        args.update(kw)
        with pytest.raises(RuntimeError, match="failed with -1"):
            gpu_ctx.selftest_quotient(fill=SENT, **args)

    bad = trace.copy()
    bad[5, 3] = P
    refused(trace=bad)
    bad = aux.copy()
    bad[-1, -1] = 2**64 - 1
    refused(aux=bad)
    refused(alphas=(P, 1))
    refused(betas=(0, P))
    refused(gammas=(2**64 - 1, 0))
    tab = random_tables(16, 3)
    tab[1, 4] = P
    refused(tables=tab)
    wt, wa = qr.dataset(kind, "random", 6, seed=2)
    refused(trace=wt, aux=wa, window=(2, 0, 5))            # coset
    refused(trace=wt, aux=wa, window=(0, 4, 5))            # k0 + count > N
    refused(trace=wt, aux=wa, window=(0, 0, 6))            # stride < count + 1
    refused(trace=wt, aux=wa, window=(0, 0, 0))            # no point
    big_t, big_a = qr.dataset(kind, "random", 2 << 2, seed=2)
    refused(log_n=2, trace=big_t, aux=big_a)               # below the smallest domain
    with pytest.raises(RuntimeError, match="failed with -1"):
        gpu_ctx.selftest_point_tables(2)
    with pytest.raises(RuntimeError, match="failed with -1"):
        gpu_ctx.selftest_point_tables(6, window=(0, 64, 3))
    again = gpu_ctx.selftest_quotient(kind, log_n, trace, aux, alphas, betas, gammas, fill=SENT)
    assert np.array_equal(ok[0], again[0]) and np.array_equal(ok[1], again[1])
