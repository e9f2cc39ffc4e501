"""The five root statement verifiers on the GPU (csrc/root_links.hip: bn254s_verify_g1_recover, _g2_recover, _fq_sqrt, _fq2_sqrt,
_map_to_g1): a call of every front-end, proven once per module as two Fq-exp proofs, is accepted as it is, with its fq_jobs and
without, and rejected with the exact link codes, proof verdicts and message once a job word, a flag, a point or a root is not what
it was; the two forgeries that only the proofs can catch or that the proofs catch too; a flipped proof word; a call whose two
proofs differ in height, so that bn254s_verify_batch runs twice; and the Python checkers of plonky2_bn254_amd.lib agree on the
accepted call and on three rejected ones.  The Python side does array surgery and negations only."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import map_to_g1_ref as m1
from tools import root_links_ref as rl
from tools import synth

P = synth.P
PER = 128
TAG = ("verify_g1_recover", "verify_g2_recover", "verify_fq_sqrt", "verify_fq2_sqrt", "verify_map_to_g1")
ROOT = ("y of the point", "y of the point", "the root", "the root", "y of the point")
RADICAND = ("x^3 + 3", "x^3 + b'", "x", "x", "g of the candidate that the flags select")
BASE = ("x^3 + 3", "norm(x^3 + b')", "x", "norm(x)", None)
FLAG = ("the flag", "the flag", "square", "square", None)
SQRT = (rl.FQ_SQRT, rl.FQ2_SQRT)
U_BOTH = 22  # the u whose g(x1) and g(x2) are both squares


def _inputs(what):
    """130 inputs (65 for map_to_g1: 130 jobs) with a square at 128 and a non-square at 129, for the roots the zero at 5 (sgn 0)
    and 6 (sgn 1), for the map U_BOTH at 3."""
    n = 65 if what == rl.MAP_TO_G1 else 130
    xs, sgns = rl.random_inputs(what, n + 40, seed=0x767274)
    if what == rl.MAP_TO_G1:
        xs[3] = U_BOTH
        return xs[:n], sgns[:n]
    flag = lambda k: rl.honest_one(what, xs[k], sgns[k])[1][0]
    spare = list(range(n, n + 40))
    for place, want in ((128, 1), (129, 0)):
        k = next(k for k in spare if flag(k) == want)
        spare.remove(k)
        xs[place], sgns[place] = xs[k], sgns[k]
    if what in SQRT:
        zero = 0 if what == rl.FQ_SQRT else (0, 0)
        xs[5], sgns[5], xs[6], sgns[6] = zero, 0, zero, 1
    return xs[:n], sgns[:n]


@pytest.fixture(scope="module")
def calls(gpu_ctx):
    """what -> (Rows, proofs) of the proven front-end: two proofs, of 128 and of 2 jobs, both of 2^16 rows."""
    out = {}
    for what in rl.WHATS:
        xs, sgns = _inputs(what)
        rows, proofs = rl.device_rows(gpu_ctx, what, rl.to_words(what, xs), sgns, per_proof=PER)
        for a in rows:
            a.setflags(write=False)
        out[what] = (rows, proofs)
    return out


def _verify(ctx, what, proofs, r, jobs=True):
    j = r.jobs if jobs else None
    if what == rl.G1_RECOVER:
        return ctx.verify_g1_recover(proofs, PER, r.xs, r.out, r.flags, j)
    if what == rl.G2_RECOVER:
        return ctx.verify_g2_recover(proofs, PER, r.xs, r.sgns, r.out, r.flags, j)
    if what == rl.MAP_TO_G1:
        return ctx.verify_map_to_g1(proofs, PER, r.xs, r.out, r.flags, j)
    return (ctx.verify_fq_sqrt if what == rl.FQ_SQRT else ctx.verify_fq2_sqrt)(proofs, PER, r.xs, r.sgns, r.out, r.flags, r.root_ok, j)


def _python_checker(ctx, what, proofs, r):
    if what == rl.G1_RECOVER:
        return pk.verify_g1_recover(r.xs, r.out, r.flags, r.jobs, proofs, PER, ctx=ctx)
    if what == rl.G2_RECOVER:
        return pk.verify_g2_recover(r.xs, r.sgns, r.out, r.flags, r.jobs, proofs, PER, ctx=ctx)
    if what == rl.MAP_TO_G1:
        return pk.verify_map_to_g1(r.xs, r.out, r.flags, r.jobs, proofs, PER, ctx=ctx)
    return (pk.verify_fq_sqrt if what == rl.FQ_SQRT else pk.verify_fq2_sqrt)(r.xs, r.sgns, r.out, r.flags, r.root_ok, r.jobs, proofs, PER, ctx=ctx)


def _rejected(call):
    with pytest.raises(pk.VerifyError) as e:
        call()
    return str(e.value), {i: int(v) for i, v in enumerate(e.value.link_codes) if v}, [int(v) for v in e.value.proof_status]


class _Surgery:
    """Copies of the arrays of a call with one input changed."""

    def __init__(self, what, rows):
        self.what, self.rows = what, rows
        self.J, self.iw = rl.JOBS[what], rl.IN_WORDS[what]
        self.at = 0 if what in SQRT else self.iw  # where the y / root begins in a row of out

    def y(self, i):
        return rl._elem(self.rows.out[i, self.at:])

    def with_y(self, i, y, rows=None):
        r = rows or self.rows
        out = r.out.copy()
        out[i, self.at:] = rl._words(y) if not isinstance(y, list) else y
        return r._replace(out=out)

    def with_out_word(self, i, word):
        out = self.rows.out.copy()
        out[i, word] ^= np.uint64(1)
        return self.rows._replace(out=out)

    def with_job_word(self, j, word):
        jobs = self.rows.jobs.copy()
        jobs[j, word] ^= np.uint64(1)
        return self.rows._replace(jobs=jobs)

    def with_flag(self, j, v, root_ok=None, rows=None):
        r = rows or self.rows
        flags = r.flags.copy()
        flags[j] = v
        r = r._replace(flags=flags)
        if root_ok is not None:
            ok = r.root_ok.copy()
            ok[j] = root_ok
            r = r._replace(root_ok=ok)
        return r


def _one(y):
    return 1 if isinstance(y, int) else (1, 0)


def _plus_one(y):
    return (y + 1) % P if isinstance(y, int) else ((y[0] + 1) % P, y[1])


@pytest.mark.gpu
@pytest.mark.parametrize("what", rl.WHATS)
def test_accepted_with_and_without_jobs_and_by_the_python_checker(gpu_ctx, calls, what):
    rows, proofs = calls[what]
    n = len(rows.xs)
    assert [p.degree_bits for p in proofs] == [16, 16]  # 128 jobs and 2 jobs: no proof has fewer than 2^16 rows; test_two_heights
    assert set(int(f) for f in rows.flags) == {0, 1}
    if what in SQRT:
        assert not rows.xs[5:7].any() and list(rows.flags[5:7]) == [0, 0] and list(rows.root_ok[5:7]) == [1, 0] and not rows.out[5:7].any()
    for jobs in (True, False):
        link, status = _verify(gpu_ctx, what, proofs, rows, jobs=jobs)
        assert link.shape == (n,) and link.dtype == np.uint8 and not link.any()
        assert status.shape == (2,) and status.dtype == np.int32 and not status.any()
    pairs = [(p.words, p.degree_bits) for p in proofs]  # the other form of `proofs`
    link, status = _verify(gpu_ctx, what, pairs, rows)
    assert not link.any() and not status.any()
    _python_checker(gpu_ctx, what, proofs, rows)
    # the jobs that the verifier makes are the front-end's, and the outputs it demands are the proven ones
    codes, bases = gpu_ctx.root_links_check_batch(what, rows.xs, rows.out, rows.flags, sgns=rows.sgns, root_ok=rows.root_ok, fq_jobs=rows.jobs)
    assert not codes.any() and np.array_equal(bases, rows.jobs[:, 4:])
    proven = np.concatenate([np.asarray(p.outputs).reshape(-1, 4) for p in proofs])
    assert np.array_equal(rl.derived_outputs(what, bases, rows.flags), proven)


@pytest.mark.gpu
@pytest.mark.parametrize("what", rl.WHATS)
def test_one_change_at_a_time(gpu_ctx, calls, what):
    rows, proofs = calls[what]
    cut, J, tag = _Surgery(what, rows), rl.JOBS[what], TAG[what]
    n = len(rows.xs)
    verify = lambda r, **kw: _verify(gpu_ctx, what, proofs, r, **kw)
    claimed = rows.root_ok if what in SQRT else rows.flags[::2] if what == rl.MAP_TO_G1 else rows.flags
    lo = 7  # past the crafted inputs
    s0 = next(i for i in range(lo, 64) if claimed[i])        # a claimed root in proof 0 (map_to_g1: an input that takes x1)
    c0 = next(i for i in range(lo, 64) if not claimed[i])    # no root claimed (map_to_g1: g(x1) is no square)
    s1 = n - 1 if what == rl.MAP_TO_G1 else 128                 # a claimed root in proof 1
    assert (J * s1) // PER == 1 and (J * s0) // PER == 0
    python_agrees = []

    # a job's scalar word, a job's base word: the proofs are judged against the verifier's own jobs and stay accepted
    j = J * s0 + J - 1
    name = BASE[what] or "g(x2)"
    r = cut.with_job_word(j, 3)
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: the scalar of job {j}" + (" (g(x2))" if J == 2 else "") + " is not (p - 1)/2",
                                            {s0: 1}, [0, 0])
    r = cut.with_job_word(j, 4)
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: the base of job {j} is not {name}", {s0: 2}, [0, 0])
    python_agrees.append(r)
    link, status = verify(r, jobs=False)  # ... and without the jobs there is nothing to compare
    assert not link.any() and not status.any()
    # a flag byte 2 on a set flag: the proof still says "a square"
    flag_name = FLAG[what] or "the flag of g(x1)"
    r = cut.with_flag(J * s0, 2)
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: {flag_name} is 2, neither 0 nor 1", {s0: 3}, [0, 0])
    # an x word of a point
    if what not in SQRT:
        text = "x of the point is not the candidate that the flags select" if what == rl.MAP_TO_G1 else "the point does not carry x"
        assert _rejected(lambda: verify(cut.with_out_word(s0, 0))) == (f"{tag}: input {s0}: {text}", {s0: 4}, [0, 0])
    # the y of a clear flag set to 1
    if what != rl.MAP_TO_G1:
        r = cut.with_y(c0, _one(cut.y(c0)))
        clear = "root_ok" if what in SQRT else "the flag"
        assert _rejected(lambda: verify(r)) == (f"{tag}: input {c0}: {clear} is clear and {ROOT[what]} is not zero words", {c0: 5}, [0, 0])
    # y + 1; y -> -y
    r = cut.with_y(s0, _plus_one(cut.y(s0)))
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: {ROOT[what]} does not square to {RADICAND[what]}", {s0: 6}, [0, 0])
    python_agrees.append(r)
    r = cut.with_y(s0, rl._neg(cut.y(s0)))
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: {ROOT[what]} squares to {RADICAND[what]} but has the other sign", {s0: 7}, [0, 0])
    python_agrees.append(r)
    # two changes in inputs of different proofs: both are named in the codes, the lower one in the message
    r = cut.with_y(s1, _plus_one(cut.y(s1)), rows=r)
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {s0}: {ROOT[what]} squares to {RADICAND[what]} but has the other sign",
                                            {s0: 7, s1: 6}, [0, 0])
    # the Python checkers reject the same three calls
    for r in python_agrees:
        with pytest.raises(pk.VerifyError):
            _python_checker(gpu_ctx, what, proofs, r)
    # and the unmodified call is still accepted by the same context
    link, status = verify(rows)
    assert not link.any() and not status.any()


@pytest.mark.gpu
@pytest.mark.parametrize("what", rl.WHATS)
def test_what_only_the_proofs_can_catch(gpu_ctx, calls, what):
    rows, proofs = calls[what]
    cut, J, tag = _Surgery(what, rows), rl.JOBS[what], TAG[what]
    verify = lambda r: _verify(gpu_ctx, what, proofs, r)
    # a set flag cleared with its y zeroed: every link holds, the output p - 1 that the verifier now demands contradicts proof 0
    if what == rl.MAP_TO_G1:  # ... for the map: the first flag of U_BOTH cleared with the point of x2 put in
        s0 = 3
        assert list(rows.flags[6:8]) == [1, 1]
        x2, y2 = m1.select_point(U_BOTH, False, True)
        out = rows.out.copy()
        out[s0] = synth._to_words(x2) + synth._to_words(y2)
        r = cut.with_flag(2 * s0, 0, rows=rows._replace(out=out))
    else:
        claimed = rows.root_ok if what in SQRT else rows.flags
        s0 = next(i for i in range(7, 64) if claimed[i])
        r = cut.with_flag(s0, 0, root_ok=0 if what in SQRT else None, rows=cut.with_y(s0, [0] * cut.iw))
    msg, link, status = _rejected(lambda: verify(r))
    assert msg.startswith("proof 0: ") and len(msg) > len("proof 0: ") and link == {} and status == [-8, 0]
    with pytest.raises(pk.VerifyError):
        _python_checker(gpu_ctx, what, proofs, r)
    # a clear flag set with y forged: the link says so (code 6), and proof 0 says so too
    if what == rl.MAP_TO_G1:
        c0 = next(i for i in range(7, 64) if not rows.flags[2 * i])
        x1 = m1.candidates(rl._elem(rows.xs[c0]))[0]
        out = rows.out.copy()
        out[c0] = synth._to_words(x1) + synth._to_words(5)
        r = cut.with_flag(2 * c0, 1, rows=rows._replace(out=out))
    else:
        claimed = rows.root_ok if what in SQRT else rows.flags
        c0 = next(i for i in range(7, 64) if not claimed[i])
        r = cut.with_flag(c0, 1, root_ok=1 if what in SQRT else None, rows=cut.with_y(c0, 5 if cut.iw == 4 else (5, 0)))
    assert _rejected(lambda: verify(r)) == (f"{tag}: input {c0}: {ROOT[what]} does not square to {RADICAND[what]}", {c0: 6}, [-8, 0])
    # one word of the query rounds of proof 1 flipped: that proof alone is rejected, the linkage is whole
    w1 = proofs[1].words.copy()
    sec = proofs[1].section("query_round_proofs")
    tail = sum(proofs[1].section(name).size for name in ("final_poly", "pow_witness", "init_challenger_state"))  # what follows
    off = w1.size - tail - sec.size
    assert np.array_equal(w1[off:off + sec.size], sec)
    w1[off + 5] ^= np.uint64(1)
    msg, link, status = _rejected(lambda: _verify(gpu_ctx, what, [proofs[0], (w1, proofs[1].degree_bits)], rows))
    assert msg.startswith("proof 1: ") and len(msg) > len("proof 1: ") and link == {} and status == [0, -8]


@pytest.mark.gpu
@pytest.mark.parametrize("what", SQRT)
def test_square_set_on_zero(gpu_ctx, calls, what):
    """square set on x = 0: code 3, and the proofs stay accepted, because the output demanded for a zero base is 0 whatever the
    flag says."""
    rows, proofs = calls[what]
    r = _Surgery(what, rows).with_flag(5, 1)
    assert _rejected(lambda: _verify(gpu_ctx, what, proofs, r)) == (
        f"{TAG[what]}: input 5: square is set on the base zero, whose Legendre symbol is 0", {5: 3}, [0, 0])
    with pytest.raises(pk.VerifyError):
        _python_checker(gpu_ctx, what, proofs, r)
    # root_ok against the sign of the one root of zero
    r = _Surgery(what, rows).with_flag(6, 0, root_ok=1)
    assert _rejected(lambda: _verify(gpu_ctx, what, proofs, r)) == (
        f"{TAG[what]}: input 6: root_ok is set, but a root with the sign 1 does not exist (the one root of zero has the sign 0)", {6: 3}, [0, 0])


@pytest.mark.gpu
def test_two_heights(gpu_ctx):
    """300 roots at 256 per proof: proofs of 2^17 and 2^16 rows, one bn254s_verify_batch call each; a verdict and a code land at
    the index of the whole call."""
    what = rl.FQ_SQRT
    xs, sgns = rl.random_inputs(what, 300, seed=0x686774)
    rows, proofs = rl.device_rows(gpu_ctx, what, rl.to_words(what, xs), sgns, per_proof=256)
    assert [p.degree_bits for p in proofs] == [17, 16]
    args = lambda r, pr=proofs: (pr, 256, r.xs, r.sgns, r.out, r.flags, r.root_ok, r.jobs)
    link, status = gpu_ctx.verify_fq_sqrt(*args(rows))
    assert link.shape == (300,) and not link.any() and list(status) == [0, 0]
    cut = _Surgery(what, rows)
    a, b = (next(i for i in range(lo, 300) if rows.root_ok[i]) for lo in (3, 290))
    r = cut.with_y(b, _plus_one(cut.y(b)), rows=cut.with_y(a, rl._neg(cut.y(a))))
    assert _rejected(lambda: gpu_ctx.verify_fq_sqrt(*args(r))) == (
        f"verify_fq_sqrt: input {a}: the root squares to x but has the other sign", {a: 7, b: 6}, [0, 0])
    for k in (0, 1):  # a word of either proof flipped: that proof alone is rejected, under its index in the call
        w = proofs[k].words.copy()
        w[w.size // 2] ^= np.uint64(1)
        pr = [(w, p.degree_bits) if j == k else p for j, p in enumerate(proofs)]
        msg, link, status = _rejected(lambda: gpu_ctx.verify_fq_sqrt(*args(rows, pr)))
        assert msg.startswith(f"proof {k}: ") and link == {} and status == [-8 if j == k else 0 for j in (0, 1)]


@pytest.mark.gpu
def test_arguments_with_a_context(gpu_ctx, calls):
    rows, proofs = calls[rl.G2_RECOVER]
    with pytest.raises(RuntimeError, match="failed with -1"):  # three proofs for 130 jobs of 128
        _verify(gpu_ctx, rl.G2_RECOVER, proofs + [proofs[0]], rows)
    s0 = next(i for i in range(7, 64) if rows.flags[i])
    out = rows.out.copy()
    out[s0, 8:12] = synth._to_words(P)
    with pytest.raises(RuntimeError, match=f"failed with -1: verify_g2_recover: points_{s0} has y.c0 not below p"):
        _verify(gpu_ctx, rl.G2_RECOVER, proofs, rows._replace(out=out))
    xs = rows.xs.copy()
    xs[100, 4:] = synth._to_words(P + 1)
    with pytest.raises(RuntimeError, match="failed with -1: verify_g2_recover: x_100 has c1 not below p"):
        _verify(gpu_ctx, rl.G2_RECOVER, proofs, rows._replace(xs=xs))
