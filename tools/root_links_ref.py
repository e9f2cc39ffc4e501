"""Reference for the root-link check (csrc/root_links.hip, bn254s_root_links_check_batch) and for the jobs that the five root
verifiers hand to bn254s_verify_batch, in Python integers.

  code_one(what, x, sgn, out, flags, root_ok, jobs)   the code of one input and its bases, ABI words in.  A claimed root is not
                                                      squared, as the kernel does: the roots of the radicand are COMPUTED
                                                      (Fq: g^((p+1)/4); Fq2: the complex method of tools/field_gadgets_ref.py) and
                                                      the claimed words compared with them
  codes(what, rows)                                   the same for the arrays of a call -> (codes [n], bases [n | 2n, 4])
  derived_outputs(what, bases, flags)                 the outputs that a verifier demands of the proofs
  honest(what, inputs, sgns)                          the arrays of a call as the front-end returns them (tools/synth.py,
                                                      tools/field_gadgets_ref.py, tools/map_to_g1_ref.py)
  device_rows(ctx, what, xs, sgns, per_proof)         the same from the device front-end itself, with its proofs (the GPU tests
                                                      and tools/run_verify_roots.py)
  cases(what)                                         crafted rows, accepted and rejected, each with the code it was made for and
                                                      no earlier one, and the edge inputs of the five front-ends

what: 0 G1_RECOVER, 1 G2_RECOVER, 2 FQ_SQRT, 3 FQ2_SQRT, 4 MAP_TO_G1.  The code of an input is the first that applies of
  1 a job's scalar != (p-1)/2      2 a job's base != the base computed here     3 a byte above 1, or (sqrt) square on a zero base,
  or root_ok != (base != 0 ? square : sgn == 0)      4 the point's x is not x_i / not the candidate that the flags select
  5 no root claimed and the y / root words not zero  6 y^2 != radicand          7 y squares back and has the other sign
and 0 where all hold."""
from __future__ import annotations

import collections

import numpy as np

from tools import field_gadgets_ref as fg
from tools import map_to_g1_ref as m1
from tools import synth

P = synth.P
LEGENDRE_EXP = (P - 1) // 2
WHATS = (G1_RECOVER, G2_RECOVER, FQ_SQRT, FQ2_SQRT, MAP_TO_G1) = range(5)
(OK, JOB_SCALAR, JOB_BASE, FLAG, CARRY, NOT_ZERO, SQUARE, SIGN) = range(8)
IN_WORDS = (4, 8, 4, 8, 4)
OUT_WORDS = (8, 16, 4, 8, 8)
JOBS = (1, 1, 1, 1, 2)
POSSIBLE = {G1_RECOVER: {0, 1, 2, 3, 4, 5, 6, 7}, G2_RECOVER: {0, 1, 2, 3, 4, 5, 6, 7}, FQ_SQRT: {0, 1, 2, 3, 5, 6, 7},
            FQ2_SQRT: {0, 1, 2, 3, 5, 6, 7}, MAP_TO_G1: {0, 1, 2, 3, 4, 6, 7}}
# at least four u of every map_to_g1_ref.branch, found with branch()
U_BRANCH = {0: (7, 12, 15, 19, 22), 1: (2, 5, 8, 10, 17), 2: (3, 4, 6, 9, 11)}

# the arrays of a call: xs [n, IW], sgns [n], out [n, OW], flags [n | 2n], root_ok [n], jobs [n | 2n, 8]
Rows = collections.namedtuple("Rows", "xs sgns out flags root_ok jobs")


def _elem(w):
    """4 words -> int, 8 words -> (c0, c1)"""
    v = tuple(synth.words_to_int(w[4 * k:4 * k + 4]) for k in range(len(w) // 4))
    return v[0] if len(v) == 1 else v


def _words(v):
    return synth._to_words(v) if isinstance(v, int) else synth._to_words(v[0]) + synth._to_words(v[1])


def _norm(a):
    return (a[0] * a[0] + a[1] * a[1]) % P


def _sgn(y) -> int:
    return y & 1 if isinstance(y, int) else int(synth.f2_sgn(y))


def _neg(y):
    return (P - y) % P if isinstance(y, int) else ((P - y[0]) % P, (P - y[1]) % P)


def roots_of(radicand):
    """The set of all y with y^2 == radicand, by computing them."""
    if isinstance(radicand, int):
        r = pow(radicand, (P + 1) // 4, P)
        return {r, P - r if r else 0} if r * r % P == radicand else set()
    if radicand == (0, 0):
        return {(0, 0)}
    y = fg._fq2_any_root(fg.Fq2(*radicand))
    return set() if y is None else {y.pair(), (-y).pair()}


def radicand_and_bases(what, x, flags):
    """(radicand, [bases]) of an input; for MAP_TO_G1 the radicand is g of the candidate that `flags` select."""
    if what == G1_RECOVER:
        g = (x * x * x + 3) % P
        return g, [g]
    if what == G2_RECOVER:
        g = synth.g2_rhs(x)
        return g, [_norm(g)]
    if what == FQ_SQRT:
        return x, [x]
    if what == FQ2_SQRT:
        return x, [_norm(x)]
    x1, x2, x3 = m1.candidates(x)
    xc = x1 if flags[0] else x2 if flags[1] else x3
    return m1.g(xc), [m1.g(x1), m1.g(x2)]


def code_one(what, x, sgn, out, flags, root_ok=None, jobs=None):
    """x: the IW words of the input; sgn: its byte (ignored for what 0, 4); out: the OW words of its point or root; flags: its
    one byte (two for MAP_TO_G1); root_ok: its byte (what 2, 3); jobs: None or its one (two) rows of 8 words
    -> (code, [base, ...] as integers)."""
    iw = IN_WORDS[what]
    xv = _elem(x)
    flags = [int(f) for f in flags]
    radicand, bases = radicand_and_bases(what, xv, flags)
    done = lambda code: (code, bases)
    if jobs is not None:
        if any(synth.words_to_int(j[:4]) != LEGENDRE_EXP for j in jobs):
            return done(JOB_SCALAR)
        if any(synth.words_to_int(j[4:]) != b for j, b in zip(jobs, bases)):
            return done(JOB_BASE)
    sgn = 0 if what == G1_RECOVER else int(xv & 1) if what == MAP_TO_G1 else int(sgn)
    if any(f > 1 for f in flags) or sgn > 1:
        return done(FLAG)
    if what in (FQ_SQRT, FQ2_SQRT):
        ok = int(root_ok)
        if ok > 1 or (flags[0] and bases[0] == 0) or ok != int(flags[0] if bases[0] else sgn == 0):
            return done(FLAG)
        claimed, yw = bool(ok), out
    else:
        carried = [int(w) for w in x] if what != MAP_TO_G1 else _words(
            m1.candidates(xv)[0 if flags[0] else 1 if flags[1] else 2])
        if [int(w) for w in out[:iw]] != carried:
            return done(CARRY)
        claimed, yw = what == MAP_TO_G1 or bool(flags[0]), out[iw:]
    if not claimed:
        return done(NOT_ZERO if any(int(w) for w in yw) else OK)
    y = _elem(yw)
    if y not in roots_of(radicand):
        return done(SQUARE)
    return done(OK if _sgn(y) == sgn else SIGN)


def codes(what, rows: Rows, with_jobs=True):
    """-> (codes [n] uint8, bases [n | 2n, 4] uint64) of a call."""
    J, n = JOBS[what], len(rows.xs)
    out_codes, out_bases = np.zeros(n, np.uint8), np.zeros((J * n, 4), np.uint64)
    for i in range(n):
        c, b = code_one(what, rows.xs[i], rows.sgns[i], rows.out[i], rows.flags[J * i:J * i + J], rows.root_ok[i],
                        rows.jobs[J * i:J * i + J] if with_jobs else None)
        out_codes[i] = c
        out_bases[J * i:J * i + J] = [synth._to_words(v) for v in b]
    return out_codes, out_bases


def derived_outputs(what, bases, flags):
    """bases [nj, 4], flags [nj] -> outputs [nj, 4] that a verifier demands of the proofs: 0 for a zero base (the sqrt kinds; a
    set flag there is code 3), else 1 where the flag is set and p - 1 where it is clear."""
    out = np.zeros((len(flags), 4), np.uint64)
    for j, f in enumerate(flags):
        zero = what in (FQ_SQRT, FQ2_SQRT) and not np.asarray(bases[j]).any()
        out[j] = synth._to_words(0 if zero else 1 if f else P - 1)
    return out


def honest_one(what, xv, sgn):
    """(out words, flags list, root_ok, jobs rows) of one input as its front-end returns them."""
    job = lambda b: synth._to_words(LEGENDRE_EXP) + synth._to_words(b)
    if what == G1_RECOVER:
        r = synth.g1_recover_from_x(xv)
        return _words(xv) + _words(r[1] if r else 0), [int(r is not None)], 0, [job((xv ** 3 + 3) % P)]
    if what == G2_RECOVER:
        r = synth.g2_recover_from_x(xv, sgn)
        return _words(xv) + _words(r[1] if r else (0, 0)), [int(r is not None)], 0, [job(_norm(synth.g2_rhs(xv)))]
    if what == FQ_SQRT:
        y, sq, ok = fg.fq_sqrt(xv, sgn)
        return _words(y), [int(sq)], int(ok), [job(xv)]
    if what == FQ2_SQRT:
        y, sq, ok = fg.fq2_sqrt(xv, sgn)
        return _words(y), [int(sq)], int(ok), [job(_norm(xv))]
    pts, fl, jobs = m1.front_end([xv])
    return [int(w) for w in pts[0]], [int(f) for f in fl], 0, [[int(w) for w in j] for j in jobs]


def _rows(what, items):
    """items: (x words, sgn, out words, flags, root_ok, jobs rows) per input -> Rows"""
    iw, ow = IN_WORDS[what], OUT_WORDS[what]
    return Rows(np.array([r[0] for r in items], np.uint64).reshape(len(items), iw), np.array([r[1] for r in items], np.uint8),
                np.array([r[2] for r in items], np.uint64).reshape(len(items), ow),
                np.array([f for r in items for f in r[3]], np.uint8), np.array([r[4] for r in items], np.uint8),
                np.array([j for r in items for j in r[5]], np.uint64).reshape(-1, 8))


def honest(what, inputs, sgns=None) -> Rows:
    """inputs: integers (pairs for the Fq2 kinds) -> the arrays of the call."""
    sgns = [0] * len(inputs) if sgns is None else [int(s) for s in sgns]
    return _rows(what, [(_words(x), s) + honest_one(what, x, s) for x, s in zip(inputs, sgns)])


def random_inputs(what, n, seed=0x726C6B):
    """(inputs, sgns): n uniform inputs of the kind with uniform wanted signs."""
    rng = synth.Xoshiro256ss(seed + what)
    fq = lambda: rng.next_u256() % P
    xs = [(fq(), fq()) if IN_WORDS[what] == 8 else fq() for _ in range(n)]
    return xs, [int(rng.next_u256() & 1) for _ in range(n)]


def cases(what, seed=0x726C6B):
    """(Rows, want [k] uint8, names [k]): the edge inputs of the front-end as honest rows, then every rejected row made from an
    honest one by the one change that reaches its code (a row named "... and ..." has a later fault too: the first applies)."""
    iw = IN_WORDS[what]
    items, want, names = [], [], []

    def put(name, x, sgn, code, out=None, flags=None, root_ok=None, jobs=None):
        """The honest row of (x, sgn) with the given parts replaced.  out / jobs: a function of the honest words."""
        h_out, h_flags, h_ok, h_jobs = honest_one(what, x, sgn)
        o = out(list(h_out)) if out else h_out
        j = jobs([list(r) for r in h_jobs]) if jobs else h_jobs
        items.append((_words(x), sgn, o, h_flags if flags is None else flags, h_ok if root_ok is None else root_ok, j))
        want.append(code)
        names.append(name)

    def y_set(v):  # the y / root words replaced by the value v (an int for the low coordinate, the others zero; or raw words)
        at = 0 if what in (FQ_SQRT, FQ2_SQRT) else iw

        def f(o):
            w = v if isinstance(v, list) else synth._to_words(v) + [0] * (len(o) - at - 4)
            return o[:at] + w
        return f

    def y_map(fn):  # the y / root replaced by fn(y)
        at = 0 if what in (FQ_SQRT, FQ2_SQRT) else iw
        return lambda o: o[:at] + _words(fn(_elem(o[at:])))

    def bump(word):
        def f(o):
            o[word] ^= 1
            return o
        return f

    def job_bump(row, word):
        def f(j):
            j[row][word] ^= 1
            return j
        return f

    plus_one = lambda y: (y + 1) % P if isinstance(y, int) else ((y[0] + 1) % P, y[1])
    xs, sg = random_inputs(what, 64, seed)
    if what == MAP_TO_G1:
        for b, us in U_BRANCH.items():
            for u in us:
                assert m1.branch(u) == b
                put(f"branch {b}: u = {u}", u, 0, OK)
        for name, u in (("u = 0", 0), ("u = 1/2 (tv3 = inv(0) = 0)", (P + 1) // 2), ("u = -1/2", (P - 1) // 2), ("u = 1", 1), ("u = -1", P - 1)):
            put(name, u, 0, OK)
        put("a random u", xs[0], 0, OK)
        b0, b1, b2 = U_BRANCH[0][0], U_BRANCH[1][0], U_BRANCH[2][0]
        for b, u in ((0, b0), (1, b1), (2, b2), (0, xs[1])):
            put(f"branch {b}: y + 1", u, 0, SQUARE, out=y_map(plus_one))
            put(f"branch {b}: y -> p - y", u, 0, SIGN, out=y_map(_neg))
            put(f"branch {b}: an x word of the point", u, 0, CARRY, out=bump(1))
        put("y = 1", b0, 0, SQUARE, out=y_set(1))
        put("y = p - 1", b1, 0, SQUARE, out=y_set(P - 1))
        put("u = 1/2: y -> p - y", (P + 1) // 2, 0, SIGN, out=y_map(_neg))
        put("scalar of job 2i", b0, 0, JOB_SCALAR, jobs=job_bump(0, 0))
        put("scalar of job 2i + 1", b1, 0, JOB_SCALAR, jobs=job_bump(1, 3))
        put("scalar of job 2i + 1 and base of job 2i", b2, 0, JOB_SCALAR, jobs=lambda j: job_bump(1, 0)(job_bump(0, 4)(j)))
        put("base of job 2i", b1, 0, JOB_BASE, jobs=job_bump(0, 4))
        put("base of job 2i + 1", b2, 0, JOB_BASE, jobs=job_bump(1, 7))
        put("base of job 2i and flag 2 and y + 1", b2, 0, JOB_BASE, jobs=job_bump(0, 5), flags=[2, 0], out=y_map(plus_one))
        put("flag 2 on g(x1), no square", b1, 0, FLAG, flags=[2, 1])
        put("flag 2 on g(x2), no square", b2, 0, FLAG, flags=[0, 2])
        put("flag 2 on g(x2) and an x word", b2, 0, FLAG, flags=[0, 2], out=bump(0))
        x1, x2, x3 = m1.candidates(b0)
        assert not m1.is_square(m1.g(x2)) and not m1.is_square(m1.g(x3))
        put("branch 0 with its first flag cleared: the point carries x1, the flags select x3", b0, 0, CARRY, flags=[0, 0])
        put("both flags clear, the point (x3, 1): g(x3) has no root", b0, 0, SQUARE, flags=[0, 0],
            out=lambda o: synth._to_words(x3) + synth._to_words(1))
        put("branch 1 with its first flag set: the flags select x1", b1, 0, CARRY, flags=[1, 1])
    elif what in (G1_RECOVER, G2_RECOVER):
        if what == G1_RECOVER:
            edge = [(f"x = {v if v < 9 else 'p - %d' % (P - v)}", v, 0) for v in (0, 1, 2, 4, P - 1, P - 2)]
        else:
            exs, esg = synth.g2_recover_inputs(12, seed)
            edge = [(f"edge input {i} of synth.g2_recover_inputs", _elem(exs[i]), int(esg[i])) for i in range(12)]
        for name, x, s in edge:
            put(name, x, s, OK)
        flag_of = lambda x, s: honest_one(what, x, s)[1][0]
        sq = [(x, s) for x, s in zip(xs, sg) if flag_of(x, s)][:8]
        nsq = [(x, s) for x, s in zip(xs, sg) if not flag_of(x, s)][:8]
        if what == G2_RECOVER:  # the root (0, t), whose sign comes from c1, and the root (t, 0)
            sq[6], sq[7] = (synth._g2_recover_real_g(7), 1), (synth._g2_recover_real_g(2), 0)
            assert _elem(honest_one(what, *sq[6])[0][8:])[0] == 0 and _elem(honest_one(what, *sq[7])[0][8:])[1] == 0
        for k in range(2):
            put(f"a square g {k}", *sq[k], OK)
            put(f"no square g {k}", *nsq[k], OK)
        put("y + 1", *sq[0], SQUARE, out=y_map(plus_one))
        put("y = 1", *sq[1], SQUARE, out=y_set(1))
        put("y = p - 1", *sq[2], SQUARE, out=y_set(P - 1))
        put("y = 0 under a set flag", *sq[3], SQUARE, out=y_set(0))
        put("a clear flag set, y forged", *nsq[0], SQUARE, flags=[1], out=y_set(5))
        put("y -> -y", *sq[0], SIGN, out=y_map(_neg))
        put("y -> -y again", *sq[4], SIGN, out=y_map(_neg))
        if what == G2_RECOVER:
            put("y = (0, t) -> (0, -t)", *sq[6], SIGN, out=y_map(_neg))
            put("y = (t, 0) -> (-t, 0)", *sq[7], SIGN, out=y_map(_neg))
            put("the sign byte flipped", sq[5][0], 1 - sq[5][1], SIGN, out=lambda o: honest_one(what, *sq[5])[0])
            put("y.c1 + 1", *sq[1], SQUARE, out=y_map(lambda y: (y[0], (y[1] + 1) % P)))
            put("sgn 2", sq[2][0], 2, FLAG, out=lambda o: honest_one(what, *sq[2])[0])
            put("y.c1 = 1 under a clear flag", *nsq[3], NOT_ZERO, out=bump(12))
        put("y = 1 under a clear flag", *nsq[1], NOT_ZERO, out=y_set(1))
        put("y words of all ones under a clear flag", *nsq[2], NOT_ZERO, out=y_set([synth.MASK64] * iw))
        put("a set flag cleared with its y left", *sq[3], NOT_ZERO, flags=[0])
        put("an x word of the point", *sq[1], CARRY, out=bump(0))
        put("the top x word of the point, flag clear", *nsq[1], CARRY, out=bump(iw - 1))
        put("an x word and y + 1", *sq[2], CARRY, out=lambda o: y_map(plus_one)(bump(1)(o)))
        put("flag 2, no square", *nsq[2], FLAG, flags=[2])
        put("flag 2, no square, and an x word", *nsq[3], FLAG, flags=[2], out=bump(0))
        put("scalar of the job", *sq[0], JOB_SCALAR, jobs=job_bump(0, 0))
        put("scalar of the job and its base", *nsq[0], JOB_SCALAR, jobs=lambda j: job_bump(0, 2)(job_bump(0, 6)(j)))
        put("base of the job", *sq[1], JOB_BASE, jobs=job_bump(0, 4))
        put("base of the job and flag 2 and y -> -y", *sq[2], JOB_BASE, jobs=job_bump(0, 7), flags=[2], out=y_map(_neg))
    else:
        crafted = fg.crafted_fq() if what == FQ_SQRT else fg.crafted_fq2()
        for name, x in crafted.items():  # x = 0 with both signs; 1 with the roots p - 1 and 1; c0 = 0, c1 = 0; the roots (0, t)
            for s in (0, 1):
                put(f"{name}, sgn {s}", x, s, OK)
        flag_of = lambda x, s: honest_one(what, x, s)[1][0]
        sq = [(x, s) for x, s in zip(xs, sg) if flag_of(x, s)][:8]
        nsq = [(x, s) for x, s in zip(xs, sg) if not flag_of(x, s)][:8]
        zero = 0 if what == FQ_SQRT else (0, 0)
        one = 1 if what == FQ_SQRT else (1, 0)
        for k in range(2):
            put(f"a square {k}", *sq[k], OK)
            put(f"no square {k}", *nsq[k], OK)
        put("root + 1", *sq[0], SQUARE, out=y_map(plus_one))
        put("root = 1", *sq[1], SQUARE, out=y_set(1))
        put("root = p - 1", *sq[2], SQUARE, out=y_set(P - 1))
        put("x = 0, sgn 0: root 1", zero, 0, SQUARE, out=y_set(1))
        put("no square with both flags set, root forged", *nsq[0], SQUARE, flags=[1], root_ok=1, out=y_set(5))
        put("root -> -root", *sq[0], SIGN, out=y_map(_neg))
        put("x = 1, sgn 0: the root 1", one, 0, SIGN, out=y_set(1))
        put("x = 1, sgn 1: the root p - 1", one, 1, SIGN, out=y_set(P - 1))
        put("the sign byte flipped", sq[3][0], 1 - sq[3][1], SIGN, out=lambda o: honest_one(what, *sq[3])[0])
        if what == FQ2_SQRT:
            x0t = crafted["(n,0), n a non-residue"]  # its roots are (0, +-t): the sign comes from c1
            assert honest_one(what, x0t, 0)[0][:4] == [0, 0, 0, 0]
            put("root (0, t) -> (0, -t)", x0t, 0, SIGN, out=y_map(_neg))
            put("root (0, t) -> (0, -t), sgn 1", x0t, 1, SIGN, out=y_map(_neg))
            put("root c1 + 1", *sq[4], SQUARE, out=y_map(lambda y: (y[0], (y[1] + 1) % P)))
            put("root c1 = 1 under a clear root_ok", *nsq[3], NOT_ZERO, out=bump(4))
        put("root = 1 under a clear root_ok", *nsq[1], NOT_ZERO, out=y_set(1))
        put("root words of all ones under a clear root_ok", *nsq[2], NOT_ZERO, out=y_set([synth.MASK64] * iw))
        put("x = 0, sgn 1: root 1 under a clear root_ok", zero, 1, NOT_ZERO, out=y_set(1))
        put("square 2, no square", *nsq[2], FLAG, flags=[2])
        put("root_ok 2", *sq[1], FLAG, root_ok=2)
        put("sgn 2", sq[2][0], 2, FLAG, out=lambda o: honest_one(what, *sq[2])[0], flags=[1], root_ok=1)
        put("square set on x = 0, sgn 0", zero, 0, FLAG, flags=[1])
        put("square set on x = 0, sgn 1, with root_ok", zero, 1, FLAG, flags=[1], root_ok=1)
        put("x = 0, sgn 1 with root_ok set", zero, 1, FLAG, root_ok=1)
        put("x = 0, sgn 0 with root_ok clear", zero, 0, FLAG, root_ok=0)
        put("a square with root_ok clear", *sq[3], FLAG, root_ok=0)
        put("no square with root_ok set", *nsq[3], FLAG, root_ok=1)
        put("root_ok clear and root + 1", *sq[5], FLAG, root_ok=0, out=y_map(plus_one))
        put("scalar of the job", *sq[0], JOB_SCALAR, jobs=job_bump(0, 0))
        put("scalar of the job and its base", *nsq[0], JOB_SCALAR, jobs=lambda j: job_bump(0, 3)(job_bump(0, 6)(j)))
        put("base of the job", *sq[1], JOB_BASE, jobs=job_bump(0, 4))
        put("base of the job of x = 0", zero, 0, JOB_BASE, jobs=job_bump(0, 4))
        put("base of the job and square 2 and root -> -root", *sq[2], JOB_BASE, jobs=job_bump(0, 7), flags=[2], out=y_map(_neg))
    return _rows(what, items), np.array(want, np.uint8), names


def to_words(what, inputs) -> np.ndarray:
    return np.array([_words(x) for x in inputs], np.uint64).reshape(len(inputs), IN_WORDS[what])


def device_rows(ctx, what, xs, sgns=None, per_proof=None):
    """The arrays of a call as the front-end of `what` returns them on the device, xs in words: its *_batch form, or with
    per_proof its proven form -> (Rows, proofs or None)."""
    n = len(xs)
    sgns = np.zeros(n, np.uint8) if sgns is None else np.asarray(sgns, np.uint8)
    kw = {} if per_proof is None else {"per_proof": per_proof}
    ok = np.zeros(n, np.uint8)
    if what == G1_RECOVER:
        got = (ctx.g1_recover_from_x_batch if per_proof is None else ctx.g1_recover_from_x)(xs, **kw)
    elif what == G2_RECOVER:
        got = (ctx.g2_recover_from_x_batch if per_proof is None else ctx.g2_recover_from_x)(xs, sgns, **kw)
    elif what == MAP_TO_G1:
        got = (ctx.map_to_g1_batch if per_proof is None else ctx.map_to_g1)(xs, **kw)
    else:
        fn = {(FQ_SQRT, True): ctx.fq_sqrt_batch, (FQ_SQRT, False): ctx.fq_sqrt, (FQ2_SQRT, True): ctx.fq2_sqrt_batch,
              (FQ2_SQRT, False): ctx.fq2_sqrt}[(what, per_proof is None)]
        out, flags, ok, jobs, *rest = fn(xs, sgns, **kw)
        got = (out, flags, jobs, *rest)
    return Rows(np.ascontiguousarray(xs, dtype=np.uint64), sgns, got[0], got[1], ok, got[2]), (got[3] if per_proof is not None else None)
