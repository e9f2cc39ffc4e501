"""Python-integer reference for the quotient (AIR constraint) kernels and their point tables.

What the device is compared with point by point (tests/test_gpu_quotient_kernels.py) and what tests/test_vanishing_ref_cpu.py
establishes first, without a GPU:
  * the layouts and shapes of the three STARK kinds (0 = G1, 1 = G2, 2 = Fq exp);
  * the point tables x_j, L_first(x_j), L_last(x_j) of the LDE domain, in leaf order and in window (natural) order;
  * which constraint indices each part kernel owns (PARTS), read from csrc/quotient_g1.hip / quotient_g2fq.hip;
  * the alpha weighting sum_e c_e alpha^(K-1-e) of starky's ConstraintConsumer over any index range, in Python integers;
  * the data sets and challenge sets of the GPU tests.
The constraint values c_e themselves come from the oracle (orc_eval_vanishing_values), which restates the reference's AIR.
"""
import numpy as np

from tools.fri_ref import GL_GEN, P, bitrev, inv, root_of_unity

# ---- shapes (csrc/layout.h, csrc/aux.h) ----------------------------------------------------------------------------------------


class Layout:
    """Column layout of one kind: LayoutT<PL, AUXL> of csrc/layout.h."""

    def __init__(self, pl, auxl, n_constraints, mz_iqp):
        self.PL, self.AUXL = pl, auxl
        self.DOUBLE, self.SUM, self.A, self.B, self.C, self.AUX = 0, pl, 2 * pl, 3 * pl, 4 * pl, 5 * pl
        self.BITS = self.AUX + auxl
        self.FLAGS = self.BITS + 256
        self.TIMESTAMP = self.FLAGS + 5
        self.IS_ADDING, self.IDNL, self.FILTER = self.TIMESTAMP + 1, self.TIMESTAMP + 2, self.TIMESTAMP + 3
        self.FREQ, self.RANGE = self.TIMESTAMP + 4, self.TIMESTAMP + 5
        self.W = self.RANGE + 1
        self.RC_BEGIN, self.RC_END = 2 * pl, 5 * pl + auxl
        self.n_rc = self.RC_END - self.RC_BEGIN
        self.m = (self.n_rc + 1) // 2                       # helper columns per challenge
        self.n_aux = 2 * (self.m + 1) + 4                   # A: per challenge helpers + Z, then 2 CTLs x 2 challenges
        self.n_constraints = n_constraints                  # AIR constraints
        self.K = n_constraints + 2 * (self.m + 2) + 8       # + lookups + CTLs
        self.mz_iqp = [self.AUX + o for o in mz_iqp]        # is_quot_positive of every eval_modulus_zero block
        self.ctl_filter = (self.FLAGS + 0, self.FLAGS + 1)  # is_first, is_last

    def aux_z_columns(self):
        """Auxiliary columns whose NEXT-row value enters a constraint: the two LogUp Z's and the four CTL Z's."""
        return [self.m, 2 * self.m + 1] + [2 * (self.m + 1) + i for i in range(4)]

    def next_trace_columns(self):
        """Trace columns whose NEXT-row value enters a constraint (the schedule of quotient_sched.h and the range counter)."""
        pl = self.PL
        cols = set()
        for base in (self.DOUBLE, self.SUM, self.A, self.B, self.C):
            cols.update(range(base, base + pl))
        cols.update(range(self.BITS, self.BITS + 256))
        cols.update((self.FLAGS + 1, self.FLAGS + 2, self.TIMESTAMP, self.IS_ADDING, self.IDNL, self.FILTER, self.RANGE))
        return sorted(cols)

    def binary_columns(self, aux_flags):
        """Columns an honest trace keeps in {0, 1}: the bits, is_first / is_last, is_adding, is_doubling_not_last, filter, the
        is-zero flags of the addition witness and every is_quot_positive."""
        return sorted(set(range(self.BITS, self.BITS + 256)) | {self.FLAGS, self.FLAGS + 1, self.IS_ADDING, self.IDNL, self.FILTER}
                      | {self.AUX + o for o in aux_flags} | set(self.mz_iqp))


# is_quot_positive offsets inside the addition witness: G1AddAux {is_x_eq_aux 1 + 16, lambda_aux 114, x_aux 194, y_aux 274};
# G2AddAux {c0_aux 3 + 16, c1_aux 99 + 16, lambda_aux 228 / 308, x_aux 388 / 468, y_aux 548 / 628}; Fq: the one block at 0
LAYOUTS = {0: Layout(32, 354, 1111, (17, 114, 194, 274)),
           1: Layout(64, 708, 1693, (19, 115, 228, 308, 388, 468, 548, 628)),
           2: Layout(16, 80, 770, (0,))}
AUX_FLAGS = {0: (0, 97), 1: (0, 1, 2, 195), 2: ()}   # is_x_eq, is_x_eq_filter / + is_c0_zero, is_c1_zero

# part kernel -> [lo, hi) of the AIR constraint indices whose weighted sum it stores (the lookups and CTLs, [n_constraints, K),
# are added in finish_point and appear in no part)
PARTS = {0: {0: (0, 50), 1: (50, 83), 2: (83, 132), 3: (132, 165), 4: (165, 198), 5: (198, 1111)},
         1: {0: (0, 50), 5: (50, 100), 1: (100, 166), 2: (166, 264), 3: (264, 330), 4: (330, 396), 6: (396, 1693)},
         2: {0: (0, 33), 1: (33, 770)}}

# ---- point tables --------------------------------------------------------------------------------------------------------------


def point(log_n, h, k):
    """(x, L_first(x), L_last(x), Z_H(x)) at x = g w_2N^h w_N^k, the point of row k on coset h.
    Z_H(x) = x^N - 1 = g^N (-1)^h - 1;  L_i(x) = w^i Z_H(x) / (N (x - w^i)) for i = 0 (first) and i = N - 1 (last, w^i = w^-1)."""
    n = 1 << log_n
    w_n, w_2n = root_of_unity(log_n), root_of_unity(log_n + 1)
    x = GL_GEN * pow(w_2n, h, P) * pow(w_n, k % n, P) % P
    zh = (pow(GL_GEN, n, P) * (P - 1 if h else 1) - 1) % P
    w_inv = inv(w_n)
    lfirst = zh * inv(n * (x - 1) % P) % P
    llast = zh * w_inv % P * inv(n * (x - w_inv) % P) % P
    return x, lfirst, llast, zh


def leaf_index(log_n, h, k):
    """Position of (coset h, row k) in leaf order."""
    return (h << log_n) | bitrev(k, log_n)


def leaf_point(log_n, j):
    """(h, k) of leaf j."""
    return j >> log_n, bitrev(j & ((1 << log_n) - 1), log_n)


def tables_leaf(log_n):
    """out[3][2N] uint64: x, L_first, L_last of the whole domain in leaf order (what quotient_point_tables writes)."""
    out = np.zeros((3, 2 << log_n), np.uint64)
    for j in range(2 << log_n):
        h, k = leaf_point(log_n, j)
        out[:, j] = point(log_n, h, k)[:3]
    return out


def tables_window(log_n, h, k0, count):
    """out[3][count]: the same for the rows k0 .. k0 + count - 1 (mod N) of coset h (quotient_point_tables_window)."""
    out = np.zeros((3, count), np.uint64)
    for j in range(count):
        out[:, j] = point(log_n, h, k0 + j)[:3]
    return out


def w_inv(log_n):
    return inv(root_of_unity(log_n))


def zh_inv(log_n, h):
    return inv(point(log_n, h, 0)[3])


def next_leaf(log_n, j):
    h, k = leaf_point(log_n, j)
    return leaf_index(log_n, h, (k + 1) & ((1 << log_n) - 1))


# ---- weighting -----------------------------------------------------------------------------------------------------------------


def weights(alpha, k):
    """w[e] = alpha^(K-1-e) as an object array of Python integers."""
    w = [1] * k
    for e in range(k - 2, -1, -1):
        w[e] = w[e + 1] * alpha % P
    return np.array(w, dtype=object)


def weighted(values, w, lo, hi):
    """sum_{lo <= e < hi} values[i][e] w[e] mod p for every point i; values: object array [n][K]."""
    if hi <= lo:
        return np.zeros(values.shape[0], dtype=object)
    return (values[:, lo:hi] * w[lo:hi]).sum(axis=1) % P


def to_object(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


# ---- data sets and challenges of the GPU tests ---------------------------------------------------------------------------------

EDGE = np.array([0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, P - 2**32, 2**63, 2**48, 0xFFFFFFFE00000001,
                 0xFFFFFFFEFFFFFFFF, 0x00000001FFFFFFFF, 0xFFFF0000FFFF0001], dtype=np.uint64)   # (tests/test_gpu_kernels.py)


def rand_field(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def dataset(kind, name, npoints, seed):
    """(trace[W][npoints], aux[A][npoints]) of the named data set."""
    lay = LAYOUTS[kind]
    shape = (lay.W + lay.n_aux, npoints)
    rng = np.random.default_rng(seed)
    if name == "random":
        d = rand_field(rng, shape)
    elif name == "zero":
        d = np.zeros(shape, np.uint64)
    elif name == "pm1":
        d = np.full(shape, P - 1, np.uint64)
    elif name == "edge":
        d = EDGE[rng.integers(0, EDGE.size, size=shape)]
    elif name == "binary":   # random, with the flag / filter / bit columns in {0, 1}
        d = rand_field(rng, shape)
        cols = lay.binary_columns(AUX_FLAGS[kind])
        d[cols] = rng.integers(0, 2, size=(len(cols), npoints), dtype=np.uint64)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(d[:lay.W]), np.ascontiguousarray(d[lay.W:])


def challenge_sets(seed):
    """name -> (alphas, betas, gammas): random, and each of alpha, beta, gamma at 0, 1 and p - 1 (every value in either slot)."""
    rng = np.random.default_rng(seed)
    rnd = lambda: tuple(int(v) for v in rand_field(rng, 2))   # noqa: E731
    base = {"alpha": rnd(), "beta": rnd(), "gamma": rnd()}
    sets = {"random": (base["alpha"], base["beta"], base["gamma"])}
    for who in ("alpha", "beta", "gamma"):
        for pair in ((0, 1), (1, P - 1), (P - 1, 0)):
            c = dict(base)
            c[who] = pair
            sets[f"{who}_{'_'.join('pm1' if v == P - 1 else str(v) for v in pair)}"] = (c["alpha"], c["beta"], c["gamma"])
    return sets
