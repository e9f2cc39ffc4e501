"""The root-link check and the five root statement verifiers, the parts that need no GPU: the crafted rows of
tools/root_links_ref.py against the five Python checkers of plonky2_bn254_amd.lib (a row has the code 0 exactly when the checker
accepts a call made of that row alone with honestly computed Legendre outputs), that every code a front-end can have is among
them, the outputs that a verifier demands of the proofs, and the argument checks of bn254s_root_links_check_batch and
bn254s_verify_{g1_recover, g2_recover, fq_sqrt, fq2_sqrt, map_to_g1}, which are all answered before any device work and before
the context is looked at."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from plonky2_bn254_amd import lib as pkl
from tools import map_to_g1_ref as m1
from tools import root_links_ref as rl
from tools import synth

P = synth.P
E_ARG = -1
VERIFIERS = ("bn254s_verify_g1_recover", "bn254s_verify_g2_recover", "bn254s_verify_fq_sqrt", "bn254s_verify_fq2_sqrt",
             "bn254s_verify_map_to_g1")


@pytest.fixture(scope="module")
def crafted():
    return {what: rl.cases(what) for what in rl.WHATS}


def test_the_symbols_and_constants_exist():
    lib = pk.load_library()
    for name in ("bn254s_root_links_check_batch",) + VERIFIERS:
        assert hasattr(lib, name), name
    assert lib.bn254s_abi_version() == 1
    assert (pkl.ROOT_OK, pkl.ROOT_JOB_SCALAR, pkl.ROOT_JOB_BASE, pkl.ROOT_FLAG, pkl.ROOT_CARRY, pkl.ROOT_NOT_ZERO, pkl.ROOT_SQUARE,
            pkl.ROOT_SIGN) == tuple(range(8))
    assert (pkl.G1_RECOVER, pkl.G2_RECOVER, pkl.FQ_SQRT, pkl.FQ2_SQRT, pkl.MAP_TO_G1) == tuple(rl.WHATS) == tuple(range(5))
    assert (rl.OK, rl.JOB_SCALAR, rl.JOB_BASE, rl.FLAG, rl.CARRY, rl.NOT_ZERO, rl.SQUARE, rl.SIGN) == tuple(range(8))
    for name in ("root_links_check_batch", "verify_g1_recover", "verify_g2_recover", "verify_fq_sqrt", "verify_fq2_sqrt", "verify_map_to_g1"):
        assert callable(getattr(pk.Context, name)), name


class _HonestProver:
    """Stands where a context stands in the Python checkers: a proof is accepted exactly when its outputs are x^s of its jobs."""

    @staticmethod
    def verify(kind, words, degree_bits, scalars, x, offset, outputs, params=None):
        assert kind == 2 and offset is None
        for s, b, o in zip(scalars, x, np.asarray(outputs).reshape(-1, 4)):
            if pow(synth.words_to_int(b), synth.words_to_int(s), P) != synth.words_to_int(o):
                raise pk.VerifyError("the outputs are not those of the jobs")


def _python_checker_accepts(what, rows, i, bases):
    """The Python checker of the front-end on row i alone, its one proof holding the Legendre symbols of the true bases."""
    J = rl.JOBS[what]
    xs, sgns, out, ok = (a[i:i + 1] for a in (rows.xs, rows.sgns, rows.out, rows.root_ok))
    flags, jobs = rows.flags[J * i:J * i + J], rows.jobs[J * i:J * i + J]
    outputs = np.array([synth._to_words(pow(b, rl.LEGENDRE_EXP, P)) for b in bases], np.uint64).reshape(-1)
    proofs = [SimpleNamespace(words=np.zeros(1, np.uint64), degree_bits=16, outputs=outputs)]
    ctx = _HonestProver()
    try:
        if what == rl.G1_RECOVER:
            pk.verify_g1_recover(xs, out, flags, jobs, proofs, J, ctx=ctx)
        elif what == rl.G2_RECOVER:
            pk.verify_g2_recover(xs, sgns, out, flags, jobs, proofs, J, ctx=ctx)
        elif what == rl.FQ_SQRT:
            pk.verify_fq_sqrt(xs, sgns, out, flags, ok, jobs, proofs, J, ctx=ctx)
        elif what == rl.FQ2_SQRT:
            pk.verify_fq2_sqrt(xs, sgns, out, flags, ok, jobs, proofs, J, ctx=ctx)
        else:
            pk.verify_map_to_g1(xs, out, flags, jobs, proofs, J, ctx=ctx)
    except pk.VerifyError:
        return False
    return True


@pytest.mark.parametrize("what", rl.WHATS)
def test_crafted_codes_agree_with_the_python_checkers(crafted, what):
    rows, want, names = crafted[what]
    J = rl.JOBS[what]
    got, bases = rl.codes(what, rows)
    assert np.array_equal(got, want), [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]
    for i, name in enumerate(names):
        b = [synth.words_to_int(w) for w in bases[J * i:J * i + J]]
        assert _python_checker_accepts(what, rows, i, b) == (want[i] == rl.OK), name
        # the codes from 3 on do not need the caller's jobs; 1 and 2 are only ever about them
        code, _ = rl.code_one(what, rows.xs[i], rows.sgns[i], rows.out[i], rows.flags[J * i:J * i + J], rows.root_ok[i], None)
        assert (code == want[i]) if want[i] not in (rl.JOB_SCALAR, rl.JOB_BASE) else (code not in (rl.JOB_SCALAR, rl.JOB_BASE)), name
        # what the entry point takes: every input coordinate is below p, and so is every root that is claimed
        assert all(synth.words_to_int(rows.xs[i, 4 * k:4 * k + 4]) < P for k in range(rl.IN_WORDS[what] // 4)), name


@pytest.mark.parametrize("what", rl.WHATS)
def test_every_possible_code_occurs(crafted, what):
    rows, want, names = crafted[what]
    assert set(int(v) for v in want) == rl.POSSIBLE[what]
    assert rl.POSSIBLE[what] == set(range(8)) - ({rl.CARRY} if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else {rl.NOT_ZERO} if what == rl.MAP_TO_G1 else set())
    code = dict(zip(names, (int(v) for v in want)))
    if what == rl.MAP_TO_G1:
        for b, us in rl.U_BRANCH.items():
            assert len(us) >= 4 and all(m1.branch(u) == b and code[f"branch {b}: u = {u}"] == 0 for u in us)
        assert code["u = 0"] == 0 and code["u = 1/2 (tv3 = inv(0) = 0)"] == 0 and code["u = -1/2"] == 0
        assert code["scalar of job 2i + 1 and base of job 2i"] == 1  # a scalar before a base, whichever job
    if what in (rl.FQ_SQRT, rl.FQ2_SQRT):
        zero = "0" if what == rl.FQ_SQRT else "(0,0)"
        assert code[f"{zero}, sgn 0"] == 0 and code[f"{zero}, sgn 1"] == 0
        assert code["square set on x = 0, sgn 0"] == 3 and code["x = 0, sgn 1 with root_ok set"] == 3
        assert code["x = 1, sgn 0: the root 1"] == 7 and code["x = 1, sgn 1: the root p - 1"] == 7
    if what == rl.FQ2_SQRT:
        assert code["root (0, t) -> (0, -t)"] == 7 and code["(0,c1), c1 a residue, sgn 1"] == 0 and code["(a^2,0), sgn 1"] == 0
    if what == rl.G2_RECOVER:
        assert code["y = (0, t) -> (0, -t)"] == 7 and code["y = (t, 0) -> (-t, 0)"] == 7


def test_derived_outputs():
    one, pm1, zero = synth._to_words(1), synth._to_words(P - 1), [0, 0, 0, 0]
    bases = np.array([synth._to_words(5), zero, synth._to_words(7), zero], np.uint64)
    for what in rl.WHATS:
        sqrt = what in (rl.FQ_SQRT, rl.FQ2_SQRT)
        got = rl.derived_outputs(what, bases, [1, 0, 0, 1])
        assert [list(r) for r in got] == [one, zero if sqrt else pm1, pm1, zero if sqrt else one]


# ---- the argument ladders, without a context -------------------------------------------------------------------------------------
N, PER = 4, 3  # inputs and jobs per proof: two proofs (three for map_to_g1, whose jobs number 8)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Proofs:
    """Proof slots of four words each: the verifiers look at nothing of them before the context."""

    def __init__(self, k):
        self.arr = [np.zeros(4, np.uint64) for _ in range(k)]
        self.table = (C.c_void_p * k)(*[w.ctypes.data for w in self.arr])
        self.n_words = (C.c_size_t * k)(*([4] * k))
        self.bits = (C.c_uint32 * k)(*([16] * k))


def _args(what):
    """A valid shape: every flag set, so that every y / root is claimed and range-checked."""
    J = rl.JOBS[what]
    return dict(xs=np.ones((N, rl.IN_WORDS[what]), np.uint64), sgns=np.zeros(N, np.uint8), out=np.ones((N, rl.OUT_WORDS[what]), np.uint64),
                flags=np.ones(J * N, np.uint8), root_ok=np.ones(N, np.uint8), jobs=np.ones((J * N, 8), np.uint64),
                code=np.full(N, 9, np.uint8), bases=np.full((J * N, 4), 9, np.uint64), status=np.full(3, 9, np.int32))


def _n_proofs(what):
    return (rl.JOBS[what] * N + PER - 1) // PER


def _check(lib, what, a, n=N, what_=None, null=(), **over):
    p = {k: (None if k in null else _vp(over.get(k, v))) for k, v in a.items()}
    return lib.bn254s_root_links_check_batch(None, what if what_ is None else what_, p["xs"], p["sgns"], n, p["out"], p["flags"], p["root_ok"],
                                             p["jobs"], p["code"], p["bases"])


def _verify(lib, what, a, pr, n=N, n_proofs=None, per_proof=PER, null=(), params=None, no_params=False, **over):
    p = {k: (None if k in null else _vp(over.get(k, v))) for k, v in a.items()}
    params = params or pk.default_params()
    mid = ([p["xs"]] + ([] if what in (rl.G1_RECOVER, rl.MAP_TO_G1) else [p["sgns"]]) + [n, p["out"], p["flags"]] +
           ([p["root_ok"]] if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else []) + [p["jobs"]])
    return getattr(lib, VERIFIERS[what])(None, None if no_params else C.byref(params), None if "words" in null else pr.table,
                                         None if "n_words" in null else pr.n_words, None if "degree_bits" in null else pr.bits,
                                         _n_proofs(what) if n_proofs is None else n_proofs, per_proof, *mid, p["code"], p["status"])


def _coordinate_faults(what, a):
    """(array, copy with one coordinate at p or p + 1): every coordinate of an input, and of the y / root of a claimed row."""
    at = {rl.G1_RECOVER: 4, rl.G2_RECOVER: 8, rl.FQ_SQRT: 0, rl.FQ2_SQRT: 0, rl.MAP_TO_G1: 4}[what]
    for v in (P, P + 1):
        for k, lo, hi in (("xs", 0, rl.IN_WORDS[what]), ("out", at, rl.OUT_WORDS[what])):
            for c in range(lo, hi, 4):
                bad = a[k].copy()
                bad[N - 1, c:c + 4] = synth._to_words(v)
                yield k, bad


@pytest.mark.parametrize("what", rl.WHATS)
def test_argument_ladder_of_root_links_check(what):
    lib, a = pk.load_library(), _args(what)
    assert _check(lib, what, a) == E_ARG  # a valid shape: only the context is missing
    assert _check(lib, what, a, null=("sgns", "jobs", "bases")) == E_ARG  # (the three optional arrays)
    for k in ("xs", "out", "flags", "code") + (("root_ok",) if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else ()):
        assert _check(lib, what, a, null=(k,)) == E_ARG, k
    assert _check(lib, what, a, n=0) == E_ARG and _check(lib, what, a, n=2**32 - 1) == E_ARG and _check(lib, what, a, n=2**32) == E_ARG
    if what == rl.MAP_TO_G1:
        assert _check(lib, what, a, n=2**31) == E_ARG
    assert _check(lib, what, a, what_=5) == E_ARG and _check(lib, what, a, what_=-1) == E_ARG
    for k, bad in _coordinate_faults(what, a):
        assert _check(lib, what, a, **{k: bad}) == E_ARG, k
    assert (a["code"] == 9).all() and (a["bases"] == 9).all()


@pytest.mark.parametrize("what", rl.WHATS)
def test_argument_ladder_of_the_verifiers(what):
    lib, a, pr = pk.load_library(), _args(what), _Proofs(_n_proofs(what))
    call = lambda **kw: _verify(lib, what, a, pr, **kw)
    assert call() == E_ARG  # a valid shape: only the context is missing
    assert call(null=("code", "status", "jobs", "sgns")) == E_ARG  # (the optional ones)
    for k in ("xs", "out", "flags", "words", "n_words", "degree_bits") + (("root_ok",) if what in (rl.FQ_SQRT, rl.FQ2_SQRT) else ()):
        assert call(null=(k,)) == E_ARG, k
    assert call(no_params=True) == E_ARG
    hole = _Proofs(_n_proofs(what))
    hole.table[1] = None
    assert _verify(lib, what, a, hole) == E_ARG
    assert call(n=0, n_proofs=0) == E_ARG and call(per_proof=0) == E_ARG
    assert call(n_proofs=_n_proofs(what) - 1) == E_ARG and call(n_proofs=_n_proofs(what) + 1) == E_ARG
    assert call(n=2**32 - 1, per_proof=2**31, n_proofs=2 * rl.JOBS[what]) == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert call(params=bad) == E_ARG
    for k, arr in _coordinate_faults(what, a):
        assert call(**{k: arr}) == E_ARG, k
    assert (a["code"] == 9).all() and (a["status"] == 9).all()
