"""The reference that tests/test_gpu_quotient_kernels.py and test_gpu_ctl_columns.py judge the device with, established without a
GPU: the oracle's per-constraint values (orc_eval_vanishing_values), its auxiliary columns (orc_aux_columns) and the Python side
of tools/quotient_ref.py (alpha weighting, point tables, the constraint ranges of the part kernels).

  * weighting: sum_e values[e] alpha^(K-1-e) in Python integers agrees with the Consumer's Horner accumulators on the AIR range;
  * an honest Fq-exp trace of 2^16 rows with the oracle's auxiliary columns makes all K values vanish on true subgroup points,
    and a one-bit corruption of a range-checked cell, a helper, a LogUp Z or a CTL Z does not;
  * power: on random data every local trace cell and every local auxiliary cell changes the weighted sum, and the next-row cells
    that matter are exactly the ones the layout says - so equality on random data exercises every column a kernel reads;
  * the point-table formulas against the oracle's own transforms of the Lagrange selectors;
  * the part table partitions [0, n_constraints)."""
import numpy as np
import pytest

from tests import oracle_lib
from tools import quotient_ref as qr
from tools import synth

P = qr.P
KINDS = (0, 1, 2)


def rand_point(kind, seed):
    lay = qr.LAYOUTS[kind]
    rng = np.random.default_rng(seed)
    return dict(local=qr.rand_field(rng, lay.W), nxt=qr.rand_field(rng, lay.W), aux_local=qr.rand_field(rng, lay.n_aux),
                aux_next=qr.rand_field(rng, lay.n_aux), betas=qr.rand_field(rng, 2), gammas=qr.rand_field(rng, 2),
                z_last=int(qr.rand_field(rng, 1)[0]), lfirst=int(qr.rand_field(rng, 1)[0]), llast=int(qr.rand_field(rng, 1)[0]))


def wsum(values, alpha, lo=0, hi=None):
    k = len(values)
    hi = k if hi is None else hi
    return sum(values[e] * pow(alpha, k - 1 - e, P) for e in range(lo, hi)) % P


@pytest.mark.parametrize("kind", KINDS)
def test_shapes_and_weighting_against_the_consumer(oracle, kind):
    lay = qr.LAYOUTS[kind]
    assert oracle.orc_stark_width(kind) == lay.W and oracle.orc_aux_width(kind) == lay.n_aux
    for seed in (1, 2):
        pt = rand_point(kind, 100 * kind + seed)
        values = oracle_lib.vanishing_values(oracle, kind, **pt)
        assert len(values) == lay.K and all(0 <= v < P for v in values)
        alphas = np.array([0x123456789ABCDEF % P, P - 2 - seed], dtype=np.uint64)
        accs = np.zeros(2, np.uint64)
        n = oracle.orc_eval_constraints(kind, oracle_lib.ptr(pt["local"]), oracle_lib.ptr(pt["nxt"]), oracle_lib.ptr(alphas),
                                        pt["z_last"], pt["lfirst"], pt["llast"], oracle_lib.ptr(accs))
        assert n == lay.n_constraints
        w = [qr.weights(int(a), lay.K) for a in alphas]
        vo = np.array(values, dtype=object)[None, :]
        for a in range(2):
            alpha = int(alphas[a])
            # the AIR range alone, Horner-folded by the Consumer: sum_{e < n} c_e alpha^(n-1-e)
            assert wsum(values[:n], alpha) == int(accs[a])
            # the same range inside the K-weighting carries alpha^(K-n) more
            assert wsum(values, alpha, 0, n) == int(accs[a]) * pow(alpha, lay.K - n, P) % P
            assert int(qr.weighted(vo, w[a], 0, n)[0]) == wsum(values, alpha, 0, n)
            assert int(qr.weighted(vo, w[a], n, lay.K)[0]) == wsum(values, alpha, n, lay.K)
            assert int(qr.weighted(vo, w[a], 0, lay.K)[0]) == wsum(values, alpha)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_export_equals_the_single_point_export(oracle, kind):
    lay = qr.LAYOUTS[kind]
    trace, aux = qr.dataset(kind, "random", 6, seed=5 + kind)
    rng = np.random.default_rng(9)
    betas, gammas = qr.rand_field(rng, 2), qr.rand_field(rng, 2)
    sel = qr.rand_field(rng, (3, 4))
    il, inx = np.array([0, 3, 5, 2], np.uint64), np.array([1, 4, 0, 2], np.uint64)
    got = oracle_lib.vanishing_values_at(oracle, kind, trace, aux, il, inx, betas, gammas, sel[0], sel[1], sel[2])
    assert got.shape == (4, lay.K)
    for i in range(4):
        one = oracle_lib.vanishing_values(oracle, kind, trace[:, il[i]], trace[:, inx[i]], aux[:, il[i]], aux[:, inx[i]], betas, gammas,
                                          sel[0, i], sel[1, i], sel[2, i])
        assert [int(v) for v in got[i]] == one


def test_parts_partition_the_air_constraints():
    for kind in KINDS:
        lay = qr.LAYOUTS[kind]
        ranges = sorted(qr.PARTS[kind].values())
        assert ranges[0][0] == 0 and ranges[-1][1] == lay.n_constraints
        for (lo, hi), (lo2, _) in zip(ranges, ranges[1:]):
            assert lo < hi == lo2
        assert sorted(qr.PARTS[kind]) == list(range(len(ranges)))
    assert [qr.LAYOUTS[k].K for k in KINDS] == [1573, 2605, 910]
    assert [qr.LAYOUTS[k].n_aux for k in KINDS] == [456, 906, 134]


@pytest.mark.parametrize("log_n", [3, 6])
def test_point_table_formulas_against_the_oracles_transforms(oracle, log_n):
    """L_first / L_last as the oracle's prover forms them: the unit vector through ifft, zero padding and a coset fft."""
    n = 1 << log_n
    m = 2 * n

    def selector(idx):
        v = np.zeros(m, np.uint64)
        v[idx] = 1
        oracle.orc_ntt(oracle_lib.ptr(v), n, 1, 0)
        oracle.orc_ntt(oracle_lib.ptr(v), m, 2, qr.GL_GEN)
        return v   # natural order of the 2N-point coset: index i = 2 k + h

    lf, ll = selector(0), selector(n - 1)
    leaf = qr.tables_leaf(log_n)
    w2n = qr.root_of_unity(log_n + 1)
    for h in (0, 1):
        win = qr.tables_window(log_n, h, 0, n)
        for k in range(n):
            i = 2 * k + h
            x, f, l, zh = qr.point(log_n, h, k)
            assert x == qr.GL_GEN * pow(w2n, i, P) % P
            assert (f, l) == (int(lf[i]), int(ll[i]))
            assert zh == (pow(x, n, P) - 1) % P
            j = qr.leaf_index(log_n, h, k)
            assert qr.leaf_point(log_n, j) == (h, k)
            assert [int(v) for v in leaf[:, j]] == [x, f, l] == [int(v) for v in win[:, k]]
            assert qr.next_leaf(log_n, j) == qr.leaf_index(log_n, h, (k + 1) % n)
        # a window wraps modulo N
        assert np.array_equal(qr.tables_window(log_n, h, n - 2, 4), np.concatenate([win[:, n - 2:], win[:, :2]], axis=1))
        assert qr.zh_inv(log_n, h) * qr.point(log_n, h, 0)[3] % P == 1


@pytest.fixture(scope="module")
def honest(oracle):
    kind, n_inst = 2, 128
    s, x = synth.fq_inputs(n_inst, seed=77)
    trace, _ = oracle_lib.generate_trace(oracle, kind, s, x, None)
    assert trace.shape == (qr.LAYOUTS[kind].W, 1 << 16)
    rng = np.random.default_rng(3)
    betas, gammas = qr.rand_field(rng, 2), qr.rand_field(rng, 2)
    aux = oracle_lib.aux_columns(oracle, kind, trace, betas, gammas)
    return kind, trace, aux, betas, gammas


def subgroup_values(oracle, kind, trace, aux, betas, gammas, rows):
    """values[len(rows)][K] on the TRUE subgroup points w^k: z_last = w^k - w^-1, L_first = [k == 0], L_last = [k == N - 1]."""
    n = trace.shape[1]
    log_n = n.bit_length() - 1
    w, wi = qr.root_of_unity(log_n), qr.w_inv(log_n)
    rows = np.array(rows, dtype=np.uint64)
    nxt = (rows + np.uint64(1)) % np.uint64(n)
    z_last = np.array([(pow(w, int(k), P) - wi) % P for k in rows], dtype=np.uint64)
    lfirst = (rows == 0).astype(np.uint64)
    llast = (rows == n - 1).astype(np.uint64)
    return oracle_lib.vanishing_values_at(oracle, kind, trace, aux, rows, nxt, betas, gammas, z_last, lfirst, llast)


def test_honest_trace_vanishes_and_corruptions_do_not(oracle, honest):
    kind, trace, aux, betas, gammas = honest
    lay = qr.LAYOUTS[kind]
    n = trace.shape[1]
    rows = [0, 1, 2, 3, 510, 511, 512, 513, n - 2, n - 1]
    v = subgroup_values(oracle, kind, trace, aux, betas, gammas, rows)
    assert v.shape == (len(rows), lay.K)
    assert not v.any(), f"non-zero constraints at (row position, index) {np.argwhere(v != 0)[:5].tolist()}"
    m = lay.m
    for name, which, col, row in (("range-checked cell", "trace", lay.RC_BEGIN + 5, 511), ("helper", "aux", 3, 2),
                                  ("LogUp Z", "aux", m, 512), ("LogUp Z of challenge 1", "aux", 2 * m + 1, n - 1),
                                  ("CTL Z", "aux", 2 * (m + 1) + 1, 1), ("last CTL Z", "aux", 2 * (m + 1) + 3, 0)):
        t, a = trace.copy(), aux.copy()
        (t if which == "trace" else a)[col, row] ^= np.uint64(1)
        assert (t if which == "trace" else a)[col, row] < P
        v = subgroup_values(oracle, kind, t, a, betas, gammas, [(row - 1) % n, row])
        assert v.any(), f"a corrupted {name} goes unnoticed"


def test_oracle_reports_a_non_binary_filter(oracle, honest):
    kind, trace, _, betas, gammas = honest
    t = np.ascontiguousarray(trace[:, :64]).copy()
    t[qr.LAYOUTS[kind].ctl_filter[1], 7] = 2
    with pytest.raises(RuntimeError, match="Non-binary filter"):
        oracle_lib.aux_columns(oracle, kind, t, betas, gammas)


@pytest.mark.parametrize("kind", KINDS)
def test_every_cell_read_changes_the_weighted_sum(oracle, kind):
    """Perturb one cell at a time of a random row pair.  Local cells: every one of the W + A must change the alpha-weighted sum.
    Next-row cells: the ones that change it are the same for two independent row pairs and are the list the layout gives."""
    lay = qr.LAYOUTS[kind]
    alpha = 0x0F1E2D3C4B5A6978 % P
    w = qr.weights(alpha, lay.K)
    found = []
    for seed in (11, 12):
        trace, aux = qr.dataset(kind, "random", 2, seed=1000 * kind + seed)
        rng = np.random.default_rng(seed)
        betas, gammas, sel = qr.rand_field(rng, 2), qr.rand_field(rng, 2), qr.rand_field(rng, 3)
        ncell = lay.W + lay.n_aux
        # point 0 = the unperturbed pair (local at position 0, next at 1); then one point per perturbed cell
        idx = np.arange(ncell + 1, dtype=np.uint64)

        def sums(position):
            """weighted sum of the pair with cell c of `position` (0 local, 1 next) perturbed, for every c, and unperturbed first"""
            # every perturbed copy is a column pair of its own: columns 2 i (local), 2 i + 1 (next) of a wide array
            tw = np.repeat(np.concatenate([trace, aux])[:, None, :], ncell + 1, axis=1).reshape(ncell, 2 * (ncell + 1))
            for c in range(ncell):
                col = 2 * (c + 1) + position
                tw[c, col] = (int(tw[c, col]) + 1) % P
            t, a = np.ascontiguousarray(tw[:lay.W]), np.ascontiguousarray(tw[lay.W:])
            ones = np.ones(ncell + 1, np.uint64)
            v = oracle_lib.vanishing_values_at(oracle, kind, t, a, 2 * idx, 2 * idx + np.uint64(1), betas, gammas, sel[0] * ones,
                                               sel[1] * ones, sel[2] * ones)
            s = qr.weighted(qr.to_object(v), w, 0, lay.K)
            return s[0], s[1:]

        base, local = sums(0)
        dead = [c for c in range(ncell) if local[c] == base]
        assert not dead, f"local cells that no constraint reads (trace column, or W + aux column): {dead[:10]}"
        base_n, nxt = sums(1)
        assert base_n == base
        found.append([c for c in range(ncell) if nxt[c] != base])
    assert found[0] == found[1] and found[0]
    assert found[0] == lay.next_trace_columns() + [lay.W + c for c in lay.aux_z_columns()]
