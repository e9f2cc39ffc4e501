#!/usr/bin/env python3
"""Crafted Poseidon inputs that force the rare reduction paths (tests/golden/poseidon_adversarial.json).

The fast code of the hand-scheduled statements (tools/gen_poseidon_asm.py) is wrong for a few digit patterns; two checks detect
them and the wave repeats the permutation with the exact code.  The fold check fires about once per 100 wave-permutations, so
every run sees it.  The PRODUCT check (mul_task: the borrow-out of the final v_subb_co, OR-ed into a sticky scalar flag) fires
when w0 + w1 2^32 + w2 (2^32 - 1) < w3 + carry3, about 2^-33 per product (derived from the digit widths, not measured): no random
test reaches it.  The permutation is a bijection, so inputs that reach it can be constructed:

  product 1 (x * x):     x = m 2^48: x^2 = m^2 2^96 as integers, so w0 = w1 = w2 = 0 < w3;
  product 2 (x^2 * x^2): x = +-k 2^24, 1 <= k < 256: x^2 = k^2 2^48 (an integer below 2^64, its only representative below 2^64),
                         so product 1 stays quiet and product 2 is the case above with m = k^2;
  products 3 and 4 (x^2 * x, x^3 * x^4): no construction known; not covered.

state_for(round, lane, x) inverts the textbook rounds (inverse MDS matrix, y -> y^(1/7)) to the 12-lane input whose S-box input
at that round and lane is x.  Every case is executed in the generator's one-lane interpreter before it is written:
  * the unmodified statement gives the textbook result,
  * with exactly one repeat, raised at the intended flag site, the fold check's min / max in range (so the product flag alone
    is the cause; FOLD_FED below names the rounds where no first product can be isolated, and why),
  * and the fast code alone (flag check neutralised) gives a WRONG result;
a candidate that fails any of these is dropped and the next one tried.  Companions (the other lanes of a wave, the other leaves
of a launch) come from pools of random states / leaves for which the interpreter reports no repeat at all.

The same S-box inputs drive the `lo < hi_hi` borrow of gl_mul_lazy (the compiler's and the cooperative permutation); "lazy"
cases aim at its `r < t1` wrap at the extremes and at the `sum < x` branch of the lazy MDS fold (about 2^-23 per output, derived).
The fixture holds inputs only; the tests compute the expected outputs from the CPU oracle.
usage: python tools/gen_poseidon_adversarial.py [out = tests/golden/poseidon_adversarial.json]
       python tools/gen_poseidon_adversarial.py --search-fold SEED     (finds STAT_INDEX for STAT_SEED; minutes)
"""
import json
import multiprocessing
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_poseidon_asm as G  # noqa: E402
from derive_poseidon_constants import P, permute, round_constants  # noqa: E402

M64 = (1 << 64) - 1
EPS = (1 << 32) - 1
INV7 = pow(7, -1, P - 1)
RC = round_constants()
M = G.mat_M()                        # M[j][i]: coefficient of lane i in output j
LENS = (8, 9, 16, 17, 21, 24)        # leaf lengths of the sponge cases (tests/test_gpu_sponge_trim.py)
POOL = 32
# the statistical case: 4096 states from random.Random(STAT_SEED); state STAT_INDEX takes a fold-check repeat (--search-fold)
STAT_SEED, STAT_N, STAT_INDEX = 20240, 4096, 2848


def is_full(r):
    return r < 4 or r >= 26


def mat_inv(X):
    n = len(X)
    a = [[x % P for x in row] + [int(i == j) for j in range(n)] for i, row in enumerate(X)]
    for c in range(n):
        piv = next(r for r in range(c, n) if a[r][c])
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, P)
        a[c] = [x * inv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


MINV = mat_inv(M)
SQRT = {}


def sqrt_mod(a):
    """A square root of a mod p (Tonelli-Shanks: p - 1 = 2^32 (2^32 - 1), 7 generates the group), or None."""
    if a not in SQRT:
        SQRT[a] = None
        if pow(a, (P - 1) // 2, P) == 1:
            q, m, c = (1 << 32) - 1, 32, pow(7, (1 << 32) - 1, P)
            t, r = pow(a, q, P), pow(a, (q + 1) // 2, P)
            while t != 1:
                i, u = 0, t
                while u != 1:
                    u, i = u * u % P, i + 1
                b = pow(c, 1 << (m - i - 1), P)
                m, c, t, r = i, b * b % P, t * b * b % P, r * b % P
            assert r * r % P == a
            SQRT[a] = r
    return SQRT[a]


# ---- textbook rounds and their inverses -------------------------------------------------------------------------------------
def round_fwd(s, r):
    s = [(s[i] + RC[12 * r + i]) % P for i in range(12)]
    s = [pow(x, 7, P) for x in s] if is_full(r) else [pow(s[0], 7, P)] + s[1:]
    return G.mat_vec(M, s, P)


def round_inv(s, r):
    u = G.mat_vec(MINV, s, P)
    u = [pow(x, INV7, P) for x in u] if is_full(r) else [pow(u[0], INV7, P)] + u[1:]
    return [(u[i] - RC[12 * r + i]) % P for i in range(12)]


def sbox_inputs(state, r):
    """The twelve lanes right after round r's constants were added (in a partial round only lane 0 enters the S-box)."""
    s = list(state)
    for q in range(r):
        s = round_fwd(s, q)
    return [(s[i] + RC[12 * r + i]) % P for i in range(12)]


def state_of(r, vec):
    """The permutation input whose lanes after round r's constant addition are vec."""
    s = [(vec[i] - RC[12 * r + i]) % P for i in range(12)]
    for q in range(r - 1, -1, -1):
        s = round_inv(s, q)
    return s


def state_for(r, lane, x, base):
    """The 12-lane input whose S-box input at round r, lane `lane` is x; the other lanes of that round are those of `base`."""
    assert is_full(r) or lane == 0, "a partial round has one S-box"
    vec = sbox_inputs(base, r)
    vec[lane] = x % P
    return state_of(r, vec)


def hash_no_pad(leaf):
    st = [0] * 12
    for c in range(0, len(leaf), 8):
        st[:len(leaf[c:c + 8])] = leaf[c:c + 8]
        st = permute(st, RC)
    return st[:4]


# ---- the statements in the interpreter ------------------------------------------------------------------------------------------
TAB = G.init_table(RC)
MEM = {"tab": G.table_dwords(TAB), "rc": [w for c in RC[:12] for w in (c & G.M32, c >> 32)], "blk": G.block_tables(TAB)}
PERM = G.pad_hazards(G.build_permute().ins)
SPONGE = G.pad_hazards(G.build_sponge(store=True).ins)      # POSEIDON_ASM_SPONGE_STORE: the one k_leaf_hash runs


def lazy_add(a, b):
    """gl_add_lazy (poseidon_dev.h): what poseidon_permute() hands to the statement."""
    t = (a + b) & M64
    return (t + EPS) & M64 if t < a else t


def run_permute(state, **mode):
    st = dict(mode)
    try:
        got, _, _ = G.run(PERM, MEM, [lazy_add(x, RC[i]) for i, x in enumerate(state)], stats=st)
    except AssertionError:          # (the fast code alone on an input it does not cover may leave the interpreter's ranges)
        return None, st
    return [g % P for g in got], st


def run_sponge(leaf, **mode):
    st = dict(mode)
    try:
        got, _, _ = G.run(SPONGE, MEM, None, leaf, stats=st)
    except AssertionError:
        return None, st
    return [g % P for g in got[:4]], st


def flag_sites(ins):
    """Every product of the fast code that can raise the sticky flag: {instruction index: name}.  The names tell the S-box (full
    round body: its lane, which fixes stream and lane group; merged blocks: the static copy A->S, S->A, last A->S and the S-box
    0..2; the single partial round) and the product 1..4 inside it."""
    out, region, cnt = {}, None, [0] * G.N_STREAMS
    for k, t in enumerate(ins):
        if t[0] == "flagcheck":
            break
        if t[0] == "label" and t[1] in ("full", "part"):
            region, cnt = t[1], [0] * G.N_STREAMS
        elif t[0] == "loop":
            region, cnt = ("tail" if t[2] == "part" else None), [0] * G.N_STREAMS
        elif t[0] == "s_or" and t[1] == G.sp(G.S_FLAG):
            stream = (t[3][1] - G.SB_CARRY) // 4
            sbox, product = divmod(cnt[stream], 4)
            cnt[stream] += 1
            if region == "full":
                out[k] = "full/lane%d/p%d" % (3 * sbox + stream, product + 1)
            elif region == "part":
                out[k] = "block%d/sbox%d/p%d" % (sbox // 3, sbox % 3, product + 1)
            else:
                assert region == "tail"
                out[k] = "block2/sbox%d/p%d" % (sbox, product + 1) if sbox < 3 else "single/p%d" % (product + 1)
    return out


def site_name(r, lane, product):
    if is_full(r):
        return "full/lane%d/p%d" % (lane, product)
    if r == 25:
        return "single/p%d" % product
    blk, k = divmod(r - 4, 3)
    return "block%d/sbox%d/p%d" % (blk % 2 if blk < 6 else 2, k, product)


PERM_SITES = {name: k for k, name in flag_sites(PERM).items()}
SPONGE_SITES = {name: k for k, name in flag_sites(SPONGE).items()}


def triggers(product, n):
    """Candidate S-box inputs for the product, rotated by n so that the cases do not all use the same one."""
    if product == 1:
        ms = [1, 3, 65535, 2, 255, 4097, 40503, 7]
        return [m << 48 for m in ms[n % len(ms):] + ms[:n % len(ms)]]
    # x^2 = m 2^48 (its only representative below 2^64): x = +-k 2^24 for m = k^2, and x = +-2^24 sqrt(m) for the other quadratic
    # residues m - those look like any other 64-bit value, which matters where x comes out of a fast fold (FOLD_FED)
    ks = [1, 3, 255, 2, 17, 128, 201, 77]
    k = ks[n % len(ks)]
    ms = [m for m in range(2, 40) if sqrt_mod(m) is not None and int(m ** 0.5) ** 2 != m]
    ms = ms[n % len(ms):] + ms[:n % len(ms)]
    roots = [(sqrt_mod(m) << 24) % P for m in ms]
    return [k << 24, P - (k << 24)] + [x for r in roots for x in (r, P - r)]


# ---- verification ---------------------------------------------------------------------------------------------------------------
def quiet_state(state):
    got, st = run_permute(state)
    assert got == permute(state, RC), state
    return not st.get("repeats") and not st.get("flag_sites")


def quiet_leaf(leaf):
    for n in LENS:
        got, st = run_sponge(leaf[:n])
        assert got == hash_no_pad(leaf[:n]), (n, leaf)
        if st.get("repeats") or st.get("flag_sites"):
            return False
    return True


# Rounds whose S-box inputs come out of a FAST fold (fold_group: low digit al0 - ah1).  A product-1 underflow needs
# x^2 mod 2^96 < 2^32 (w2 = 0 and w0 + w1 2^32 < w3 + carry3; w2 = 1 needs x^2 = 2^64 mod 2^96), and every x < 2^64 with that
# property is a multiple of 2^32.  A zero low digit out of a fast fold means al0 = ah1 < 2^10: the fold check fires as well, for
# every such input, so at these rounds product 1 cannot be isolated - the hardware never sees its flag alone there either.  The
# same instructions run rounds 0 (full-round body) and 10, 16 (block 0's first S-box), where the cases are isolated.
FOLD_FED = (1, 2, 3, 4, 26, 27, 28, 29)


def isolated_possible(r, product):
    return not (product == 1 and r in FOLD_FED)


def permute_case_ok(state, site, isolated=True):
    want = permute(state, RC)
    got, st = run_permute(state)
    assert got == want, ("the statement is wrong", state)
    if st.get("repeats") != 1 or st.get("flag_sites") != [(0, site)] or st["fold_in_range"] != [isolated]:
        return False
    alone, _ = run_permute(state, never=1)
    return alone != want


def sponge_case_ok(leaf, chunk, site, isolated=True):
    want = hash_no_pad(leaf)
    got, st = run_sponge(leaf)
    assert got == want, ("the statement is wrong", leaf)
    in_range = [k != chunk or isolated for k in range(len(st["fold_in_range"]))]
    if st.get("repeats") != 1 or st.get("flag_sites") != [(chunk, site)] or st["fold_in_range"] != in_range:
        return False
    alone, _ = run_sponge(leaf, never=1)
    return alone != want


JOB = {}     # the quiet pools (set before the worker processes are forked)


def permute_job(job):
    n, r, lane, product = job
    site, iso = PERM_SITES[site_name(r, lane, product)], isolated_possible(r, product)
    for b in range(4):
        base = JOB["states"][(n + b) % POOL]
        for x in triggers(product, n):
            state = state_for(r, lane, x, base)
            if permute_case_ok(state, site, iso):
                return {"round": r, "lane": lane, "product": product, "site": site, "isolated": iso, "x": x, "state": state}
    raise AssertionError("no case for %r" % (job,))


def sponge_leaf_for(leaf, chunk, r, lane, x, free):
    """leaf with one element of chunk `chunk` replaced so that the S-box input of the chunk's permutation at round r (0 or 1),
    lane `lane` is x.  Round 0: the element of that lane.  Round 1: element `free` of the chunk, solved through the MDS row."""
    leaf = list(leaf)
    st = [0] * 12
    for c in range(0, 8 * chunk, 8):
        st[:8] = leaf[c:c + 8]
        st = permute(st, RC)
    part = leaf[8 * chunk:8 * chunk + 8]
    st[:len(part)] = part
    if r == 0:
        assert lane < len(part)
        leaf[8 * chunk + lane] = (x - RC[lane]) % P
        return leaf
    assert r == 1 and free < len(part)
    y = [pow((st[i] + RC[i]) % P, 7, P) for i in range(12)]
    rest = sum(M[lane][i] * y[i] for i in range(12) if i != free)
    y_free = (x - RC[12 + lane] - rest) * pow(M[lane][free], -1, P) % P
    leaf[8 * chunk + free] = (pow(y_free, INV7, P) - RC[free]) % P
    return leaf


def sponge_job(job):
    n, length, chunk, r, lane, product = job
    site, iso = SPONGE_SITES[site_name(r, lane, product)], isolated_possible(r, product)
    nfree = min(8, length - 8 * chunk)
    for b in range(4):
        base = JOB["leaves"][(n + b) % POOL][:length]
        for x in triggers(product, n):
            leaf = sponge_leaf_for(base, chunk, r, lane, x, (n + b) % nfree)
            if sponge_case_ok(leaf, chunk, site, iso):
                return {"len": length, "chunk": chunk, "round": r, "lane": lane, "product": product, "site": site, "isolated": iso, "x": x,
                        "leaf": leaf}
    raise AssertionError("no case for %r" % (job,))


def chunk_classes(length, chunk):
    """The classes of chunk the sponge statement's last round tells apart (a chunk can be in several)."""
    chunks = (length + 7) // 8
    ragged = length % 8 != 0
    out = set()
    if chunks == 1:
        out.add("only")
    if chunk == 0 and chunks > 1:
        out.add("first")
    if 0 < chunk < chunks - 1 and not (ragged and chunk == chunks - 2):
        out.add("middle")
    if ragged and chunk == chunks - 2:
        out.add("before_ragged")
    if ragged and chunk == chunks - 1:
        out.add("ragged")
    if chunk == chunks - 1 and chunks > 1:
        out.add("last")
    return out


# ---- the compiler's / cooperative code: gl_mul_lazy and the lazy MDS fold (poseidon_dev.h), restated -----------------------------
def mul_lazy(a, b):
    """-> (result, `lo < hi_hi` borrow taken, `r < t1` wrap taken)"""
    x = a * b
    lo, hi = x & M64, x >> 64
    hi_hi, hi_lo = hi >> 32, hi & EPS
    t0 = (lo - hi_hi) & M64
    borrow = lo < hi_hi
    if borrow:
        t0 = (t0 - EPS) & M64
    t1 = hi_lo * EPS
    r = (t0 + t1) & M64
    wrap = r < t1
    return ((r + EPS) & M64 if wrap else r), borrow, wrap


def mds_fold_wraps(y):
    """The output lanes of a full round's layer (poseidon_mds<false>) whose fold takes the `sum < x` branch; y: S-box outputs."""
    out = []
    for j in range(12):
        al = sum(M[j][i] * (y[i] & EPS) for i in range(12))
        ah = sum(M[j][i] * (y[i] >> 32) for i in range(12))
        t = (al + (ah >> 32) * EPS) & M64
        x = (ah << 32) & M64
        if (t + x) & M64 < x:
            out.append(j)
    return out


def lazy_cases(states):
    cases = []
    # gl_mul_lazy, product 1 of the S-box: the wrap with the largest t1 (hi_lo = 2^32 - 1), borrow and wrap in one product, the
    # wrap that lands on r = 0 .. and the sum that just does not wrap (2^64 - 1 is not reachable by a square: the nearest found)
    picks = {}
    for a in range(33, 64):
        for b in [None] + list(range(0, a)):
            for sign in (1, -1):
                x = (1 << a) + (sign * (1 << b) if b is not None else 0)
                if not EPS <= x < P:        # a single representative below 2^64: the kernels see these digits
                    continue
                r, borrow, wrap = mul_lazy(x, x)
                hi_lo = ((x * x) >> 64) & EPS
                if wrap and hi_lo == EPS:
                    picks.setdefault("wrap_max_t1", x)
                if wrap and borrow:
                    picks.setdefault("borrow_and_wrap", x)
                if wrap and r < (1 << 33):
                    picks.setdefault("wrap_to_small", x)
                if not wrap and not borrow and r > M64 - (1 << 33):
                    picks.setdefault("no_wrap_at_top", x)
    n = 0
    for kind in sorted(picks):
        for r, lane in ((0, 2), (1, 9), (3, 0), (13, 0), (27, 11)):
            cases.append({"kind": kind, "round": r, "lane": lane, "x": picks[kind], "state": state_for(r, lane, picks[kind], states[n % POOL])})
            n += 1
    # lazy MDS fold: S-box outputs with every high digit near 2^24 and all-ones low digits put ah's low word just below 2^32
    rnd = random.Random(77)
    found = 0
    while found < 6:
        y = [(((1 << 24) - 1 + rnd.randrange(0, 3)) << 32) | EPS for _ in range(12)]
        rows = mds_fold_wraps(y)
        if not rows:
            continue
        r = (0, 1, 2, 3, 26, 29)[found]
        vec = [pow(v, INV7, P) for v in y]
        assert [pow(v, 7, P) for v in vec] == y
        cases.append({"kind": "fold_wrap", "round": r, "lane": rows[0], "x": vec[rows[0]], "state": state_of(r, vec)})
        found += 1
    for c in cases:
        assert sbox_inputs(c["state"], c["round"])[c["lane"]] == c["x"]
    return cases


# ---- the statistical case ---------------------------------------------------------------------------------------------------------
def stat_states(seed=STAT_SEED, n=STAT_N):
    rnd = random.Random(seed)
    return [[rnd.randrange(P) for _ in range(12)] for _ in range(n)]


def fold_repeat(state):
    """True if the statement repeats this state because of the fold check alone (no product flag)."""
    got, st = run_permute(state)
    assert got == permute(state, RC), state
    return st.get("repeats") == 1 and not st.get("flag_sites") and st["fold_in_range"] == [False]


# ---- output -----------------------------------------------------------------------------------------------------------------------
def hexes(v):
    return ["%016x" % x for x in v]


def dump(doc):
    """One case per line: the file stays readable in a diff."""
    lines = ["{"]
    keys = list(doc)
    for key in keys:
        val = doc[key]
        end = "" if key == keys[-1] else ","
        if isinstance(val, list):
            lines.append(' "%s": [' % key)
            lines += ["  " + json.dumps(item) + ("" if k == len(val) - 1 else ",") for k, item in enumerate(val)]
            lines.append(" ]" + end)
        else:
            lines.append(' "%s": %s%s' % (key, json.dumps(val), end))
    lines.append("}")
    return "\n".join(lines) + "\n"


def permute_targets():
    jobs = [(r, lane, p) for r in (0, 3, 26, 29) for lane in range(12) for p in (1, 2)]      # first / last iteration of both loops
    jobs += [(4 + 3 * blk + k, 0, p) for blk in range(7) for k in range(3) for p in (1, 2)]  # every S-box of every merged block
    jobs += [(25, 0, p) for p in (1, 2)]                                                     # the single partial round
    return [(n,) + j for n, j in enumerate(jobs)]


def sponge_targets():
    combos = [(length, c) for length in LENS for c in range((length + 7) // 8)]
    jobs = []
    for q, (length, c) in enumerate(combos):
        nfree = min(8, length - 8 * c)
        jobs += [(length, c, 1, q % 12, 1), (length, c, 1, (q + 5) % 12, 2), (length, c, 0, q % nfree, 1), (length, c, 0, (q + 3) % nfree, 2)]
    return [(n,) + j for n, j in enumerate(jobs)]


def build(workers):
    ctx = multiprocessing.get_context("fork")
    rnd = random.Random(0x504F5345)
    cand_states = [[rnd.randrange(P) for _ in range(12)] for _ in range(POOL + 8)]
    cand_leaves = [[rnd.randrange(P) for _ in range(max(LENS))] for _ in range(POOL + 8)]
    with ctx.Pool(workers) as pool:
        qs = pool.map(quiet_state, cand_states, chunksize=1)
        ql = pool.map(quiet_leaf, cand_leaves, chunksize=1)
    states = [s for s, q in zip(cand_states, qs) if q][:POOL]
    leaves = [s for s, q in zip(cand_leaves, ql) if q][:POOL]
    assert len(states) == POOL and len(leaves) == POOL
    JOB.update(states=states, leaves=leaves)
    with ctx.Pool(workers) as pool:
        pcases = pool.map(permute_job, permute_targets(), chunksize=1)
        scases = pool.map(sponge_job, sponge_targets(), chunksize=1)
    lazy = lazy_cases(states)
    # coverage: every product-1 / product-2 flag site of the bare statement; of the sponge statement those of the full-round
    # body (only rounds 0 and 1 of a chunk's permutation can be steered: the capacity lanes are not free); every class of chunk
    want = {k for name, k in PERM_SITES.items() if name[-1] in "12"}
    assert {c["site"] for c in pcases} == want, sorted(want - {c["site"] for c in pcases})
    want = {k for name, k in SPONGE_SITES.items() if name[-1] in "12" and name.startswith("full/")}
    assert {c["site"] for c in scases} == want
    assert set().union(*(chunk_classes(c["len"], c["chunk"]) for c in scases)) == {"only", "first", "middle", "before_ragged", "ragged", "last"}
    assert STAT_INDEX is not None and fold_repeat(stat_states()[STAT_INDEX]), "run --search-fold and set STAT_INDEX"
    fmt = lambda c, key: dict(c, x="%016x" % c["x"], **{key: hexes(c[key])})
    return {
        "comment": "generated by tools/gen_poseidon_adversarial.py - inputs only, every word a 64-bit hexadecimal number",
        "stat": {"seed": STAT_SEED, "n": STAT_N, "fold_repeat_at": STAT_INDEX},
        "quiet_states": [hexes(s) for s in states],
        "quiet_leaves": [hexes(s) for s in leaves],
        "permute_cases": [fmt(c, "state") for c in pcases],
        "sponge_cases": [fmt(c, "leaf") for c in scases],
        "lazy_cases": [fmt(c, "state") for c in lazy],
    }


def search_fold(seed, workers):
    states = stat_states(seed)
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        for k, hit in enumerate(pool.imap(fold_repeat, states, chunksize=8)):
            if hit:
                print("seed %d: state %d takes a fold-check repeat" % (seed, k))
                pool.terminate()
                return k
    print("seed %d: no fold-check repeat in %d states" % (seed, len(states)))
    return None


def main():
    workers = min(16, os.cpu_count() or 1)
    if len(sys.argv) > 2 and sys.argv[1] == "--search-fold":
        search_fold(int(sys.argv[2]), workers)
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                                                             "poseidon_adversarial.json")
    doc = build(workers)
    with open(out, "w") as f:
        f.write(dump(doc))
    print("flag sites covered (products 1 and 2): %d of the bare statement, %d of the sponge statement's full-round body; "
          "products 3 and 4: not reached" % (len({c["site"] for c in doc["permute_cases"]}), len({c["site"] for c in doc["sponge_cases"]})))
    print("wrote %s: %d permute cases, %d sponge cases, %d lazy cases, %d + %d companions" %
          (os.path.basename(out), len(doc["permute_cases"]), len(doc["sponge_cases"]), len(doc["lazy_cases"]),
           len(doc["quiet_states"]), len(doc["quiet_leaves"])))


if __name__ == "__main__":
    main()
