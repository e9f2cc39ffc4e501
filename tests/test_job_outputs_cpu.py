"""Proof-free job outputs without a GPU: the window-ladder model (tools/job_outputs_ref.py ladder, the shape of
csrc/window_ladder.h) against the big-integer definition and the exceptional cases of the group law it meets, the definition
against the outputs of the CPU oracle's traces, the argument checks of the two C entry points, and verify_job_outputs on proofs
made by the CPU oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import job_outputs_ref as jr
from tools import synth

P, R = synth.P, synth.R_ORDER
KINDS = (0, 1, 2)
NAMES = {0: "G1", 1: "G2", 2: "Fq exp"}


@pytest.fixture(scope="module")
def edge():
    """kind -> (scalars, x, offset, classes, outputs, finite) of edge_jobs and the definition: computed once, read-only."""
    out = {}
    for kind in KINDS:
        s, x, o, classes = jr.edge_jobs(kind)
        outs, fin = jr.outputs(kind, s, x, o)
        for a in (s, x, o, outs, fin):
            if a is not None:
                a.setflags(write=False)
        out[kind] = (s, x, o, classes, outs, fin)
    return out


def _values(kind, s, x, o, i):
    return synth.words_to_int(s[i]), jr.from_words(kind, x[i]), None if kind == 2 else jr.from_words(kind, o[i])


def test_edge_jobs_hold_every_class(edge):
    for kind in KINDS:
        s, x, o, classes, outs, fin = edge[kind]
        assert s.shape == (64, 4) and x.shape == (64, jr.POINT_WORDS[kind]) and len(classes) == 64
        have = set(classes)
        assert "random" in have and {"s = 2^w - 1", "s = 2^w", "s = 2^255", "alternating digits"} <= have
        w = jr.WINDOW[kind]
        svals = {synth.words_to_int(v) for v in s}
        assert {(1 << w) - 1, 1 << w, 1 << 255, jr.alternating(w, True), jr.alternating(w, False)} <= svals
        if kind == 2:
            assert o is None and fin.all()
            for xv in (0, 1, 2, P - 1):
                for sv in (0, 1, P - 1, P, 2**256 - 1):
                    assert any(synth.words_to_int(s[i]) == sv and synth.words_to_int(x[i]) == xv for i in range(64)), (xv, sv)
            continue
        assert {0, 1, 2, 2**256 - 1, R - 1, R, R + 1, (2**256 - 1) // R * R} <= svals
        assert {"offset = x, s = 1", "offset = -x, s = 1", "offset = -[2]x, s = 2", "offset = [s]x"} <= have
        infinite = {classes[i] for i in range(64) if not fin[i]}
        assert infinite == {c for c in jr.INFINITE if c in have} and len(infinite) == (3 if kind == 0 else 2)
        assert not outs[fin == 0].any()
        # special lanes stand beside ordinary ones: the crafted jobs are not all in front
        assert "random" in classes[:16] and any(c != "random" for c in classes[48:])
        if kind == 0:
            assert {"offset = x, s = r - 1", "accumulator equals an entry, s = r + 2d"} <= have
        else:
            assert set(jr.SMALL_ORDER) <= have
            off = [i for i in range(64) if classes[i] == "off the subgroup, s >= r"]
            assert len(off) == 3
            for i in off:  # the full 256-bit scalar matters: s x differs from (s mod r) x
                sv, xv, ov = _values(kind, s, x, o, i)
                assert sv >= R and not synth.g2_in_subgroup(xv)
                assert jr.output_one(kind, sv, xv, ov) != jr.output_one(kind, sv % R, xv, ov)
            i = classes.index("order 10069, s = 10069")
            assert np.array_equal(outs[i], o[i])  # [10069]x = O: the output is the offset


def test_ladder_model_equals_the_definition(edge):
    """Every window 2..4, on edge_jobs and on 200 seeded random jobs per kind; the exceptional additions the model reports."""
    for kind in KINDS:
        s, x, o, classes, outs, fin = edge[kind]
        rs, rx, ro = jr.random_jobs(kind, 200, seed=977 + kind)
        routs, rfin = jr.outputs(kind, rs, rx, ro)
        seen, where = set(), {}
        for w in (2, 3, 4):
            for i in range(64):
                got, ev = jr.ladder(kind, *_values(kind, s, x, o, i), w)
                assert jr.to_words(kind, got) == [int(v) for v in outs[i]] and (got is not None) == bool(fin[i]), (kind, w, classes[i])
                for e in ev:
                    seen.add(e)
                    where.setdefault(e, set()).add(classes[i])
            for i in range(200):
                got, ev = jr.ladder(kind, *_values(kind, rs, rx, ro, i), w)
                assert jr.to_words(kind, got) == [int(v) for v in routs[i]] and rfin[i] == 1, (kind, w, i)
                # a random job meets nothing but zero digits and leading zero windows
                assert all(e == ("ladder", "O") for e in ev), (kind, w, i, ev)
        print(NAMES[kind], {e: sorted(c) for e, c in sorted(where.items())})
        if kind == 2:
            assert not seen
            continue
        assert not any(e[0] == "table" for e in seen)  # the table's additions are ordinary
        assert {case for _, case in seen} == {"O", "equal", "opposite"}
        assert {("offset", "O"), ("offset", "equal"), ("offset", "opposite"), ("ladder", "O"), ("ladder", "opposite")} <= seen
        assert ("ladder", "equal") in seen  # the accumulator meets the table entry that is added to it
        if kind == 0:
            assert "accumulator equals an entry, s = r + 2d" in where[("ladder", "equal")]
            # ... with the window of the kernel, so that the G1 instance of the law doubles inside its ladder
            i = classes.index("accumulator equals an entry, s = r + 2d")
            assert any(("ladder", "equal") in jr.ladder(kind, *_values(kind, s, x, o, j))[1]
                       for j in range(64) if classes[j] == classes[i])
        else:
            assert "order 10069, accumulator equals an entry" in where[("ladder", "equal")]
            assert "order 10069, accumulator is minus an entry" in where[("ladder", "opposite")]
        assert "s = r" in where[("ladder", "opposite")]  # [r - 1]x + x


def test_digits_cover_the_scalar():
    for w in (2, 3, 4):
        for s in (0, 1, 2**256 - 1, 2**255, R, jr.alternating(w, True)):
            ds = jr.digits(s, w)
            assert len(ds) == (256 + w - 1) // w and ds[0] < 1 << (256 - w * (len(ds) - 1))
            v = 0
            for d in ds:
                v = (v << w) | d
            assert v == s


def _oracle_accepts(orc, kind, s, x, o, i):
    """One job through the oracle's trace generator at 512 rows: True if its walk ends, False if it meets a + (-a).  (A trace
    that short cannot hold the range-check column: the call fails after the walk in either case, which is all that is asked.)"""
    tr = np.zeros((orc.orc_stark_width(kind), 512), np.uint64)
    out = np.zeros(jr.POINT_WORDS[kind], np.uint64)
    s1, x1 = np.ascontiguousarray(s[i:i + 1]), np.ascontiguousarray(x[i:i + 1])
    o1 = None if o is None else np.ascontiguousarray(o[i:i + 1])
    rc = orc.orc_generate_trace(kind, oracle_lib.ptr(s1), oracle_lib.ptr(x1), oracle_lib.ptr(o1), 1, 9, oracle_lib.ptr(tr), oracle_lib.ptr(out))
    msg = orc.orc_last_error().decode() if rc != 0 else ""
    if "point at infinity" in msg:
        return False
    assert rc == 0 or "fewer than 2^16 rows" in msg, msg
    return True


@pytest.mark.parametrize("kind", KINDS)
def test_definition_equals_the_oracle_trace(edge, kind):
    s, x, o, classes, outs, fin = edge[kind]
    orc = oracle_lib.load()
    ok = [i for i in range(64) if _oracle_accepts(orc, kind, s, x, o, i)]
    rejected = sorted({classes[i] for i in range(64) if i not in ok})
    print(NAMES[kind], "rejected by the oracle:", rejected)
    # what the oracle cannot walk: an infinite output, or (order 10069) a running sum that passes through O on a finite one
    assert set(rejected) <= set(jr.INFINITE) | set(jr.SMALL_ORDER)
    assert all(i not in ok for i in range(64) if not fin[i])
    s_, x_ = np.ascontiguousarray(s[ok]), np.ascontiguousarray(x[ok])
    o_ = None if o is None else np.ascontiguousarray(o[ok])
    _, got = oracle_lib.generate_trace(orc, kind, s_, x_, o_)  # one trace of 2^16 rows for all of them
    want = outs[ok]
    assert np.array_equal(got, want), [classes[ok[j]] for j in np.nonzero(np.any(got != want, axis=1))[0]]
    compared = {classes[i] for i in ok}
    assert set(classes) - set(jr.INFINITE) - set(jr.SMALL_ORDER) <= compared
    if kind == 2:
        assert len(ok) == 64
        i = classes.index("x = 0, s = 0")
        assert synth.words_to_int(got[ok.index(i)]) == 1 == pow(0, 0, P)  # 0^0: the oracle and Python agree


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.mark.parametrize("kind", KINDS)
def test_entry_points_check_their_arguments(kind):
    lib = pk.load_library()
    pw = jr.POINT_WORDS[kind]
    s, x, o = jr.random_jobs(kind, 3, seed=3)
    o_arg = o if kind != 2 else None
    outs, finite = np.zeros((3, pw), np.uint64), np.zeros(3, np.uint8)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(kind=kind, s=s, x=x, o=o_arg, n=3, outs=outs, finite=finite):
        return lib.bn254s_job_outputs_batch(None, kind, _vp(s), _vp(x), _vp(o), n, _vp(outs), _vp(finite))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(s=None) == E_ARG and front(x=None) == E_ARG and front(outs=None) == E_ARG
    assert front(finite=None) == E_ARG and front(n=0) == E_ARG and front(kind=3) == E_ARG and front(kind=-1) == E_ARG

    def full(ctx=None, kind=kind, params=params, s=s, x=x, o=o_arg, n=3, per_proof=20000, outs=outs, slots=True):
        pr = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_job_outputs(ctx, kind, C.byref(params) if params is not None else None, _vp(s), _vp(x), _vp(o), n, per_proof,
                                    _vp(outs), pr if slots else None)
        return rc, list(pr)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), slots are cleared
    rc, pr = full()
    assert rc == E_UNSUP and pr[0] is None and pr[1] == 1
    assert full(per_proof=16385)[0] == E_UNSUP
    assert full(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    rc, pr = full(per_proof=2)
    assert rc == E_ARG and pr[0] is None and pr[1] is None and pr[2] == 1
    # each invalid argument alone is reported before the shape
    assert full(s=None)[0] == E_ARG
    assert full(x=None)[0] == E_ARG
    assert full(outs=None)[0] == E_ARG
    assert full(slots=False)[0] == E_ARG
    assert full(params=None)[0] == E_ARG
    assert full(n=0)[0] == E_ARG
    assert full(per_proof=0)[0] == E_ARG
    assert full(kind=3)[0] == E_ARG and full(kind=-1)[0] == E_ARG
    rc, pr = full(n=2**32 - 1)  # the first bad index travels as a 32-bit word; no slot is touched
    assert rc == E_ARG and pr[0] == 1
    assert front(n=2**32 - 1) == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert full(params=bad)[0] == E_ARG
    if kind == 2:
        assert full(o=x)[0] == E_UNSUP  # an offset is not read for Fq exp, NULL or not
    else:
        assert full(o=None)[0] == E_ARG and front(o=None) == E_ARG
    assert not outs.any() and not finite.any()


@pytest.fixture(scope="module", params=KINDS)
def oracle_jobs(request):
    """3 jobs of one kind, per_proof = 4: one 2^16-row proof made by the CPU oracle (the cut into several proofs is the GPU
    test's, n = 130)."""
    kind = request.param
    s, x, o = jr.random_jobs(kind, 3, seed=59 + kind)
    orc = oracle_lib.load()
    words, outs, _, db = oracle_lib.prove(orc, kind, s, x, o)
    assert np.array_equal(outs, jr.outputs(kind, s, x, o)[0])
    return kind, s, x, o, outs, [SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1))]


def test_verify_job_outputs_accepts_oracle_proofs(oracle_jobs):
    kind, s, x, o, outs, proofs = oracle_jobs
    pk.verify_job_outputs(kind, s, x, o, outs, proofs, 4)


def test_verify_job_outputs_rejects_tampering(oracle_jobs):
    kind, s, x, o, outs, proofs = oracle_jobs

    def check(match, outs=outs, proofs=proofs, per_proof=4, s=s):
        with pytest.raises(pk.VerifyError, match=match):
            pk.verify_job_outputs(kind, s, x, o, outs, proofs, per_proof)

    flipped = outs.copy()  # a flipped output word
    flipped[1, 2] ^= 1
    check(r"^job_outputs: output 1 ", outs=flipped)
    swapped = outs.copy()  # a swapped pair of outputs
    swapped[[0, 2]] = outs[[2, 0]]
    check(r"^job_outputs: output 0 ", outs=swapped)
    words = proofs[0].words.copy()  # a flipped proof word (the trace cap)
    words[0] ^= 1
    check(r"^job_outputs: proof 0 .*rejected", proofs=[SimpleNamespace(words=words, degree_bits=proofs[0].degree_bits,
                                                                      outputs=proofs[0].outputs)])
    other = s.copy()  # a claimed scalar that is not the proof's
    other[2, 0] ^= 1
    check(r"^job_outputs: proof 0 .*rejected", s=other)
    check("1 proofs for 3 jobs", per_proof=2)
