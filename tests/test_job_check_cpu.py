"""The job check without a GPU: the stepwise definition (tools/job_check_ref.py check_one) against the closed form
offset == -[2^k + (s mod 2^k)] x, the expected result of every class of edge_jobs, the definition against the walk of the CPU
oracle's trace generator, and the argument checks of the two C entry points without a context.

The closed form costs one scalar multiplication per step, 256 per job (0.4 s on G1, 1.3 s on G2 in Python): every job is
compared on the steps of STEPS, which hold every step a crafted job hits at and the word boundaries of the scalar, and FULL jobs
per set on all 256."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import synth

CURVES = (0, 1)
NAMES = {0: "G1", 1: "G2"}
NONE = jc.STEP_NONE
STEPS = sorted({0, 7, 20, 130, 252, 253, 254} | set(jc.BOUNDARIES))
FULL = 3
E_ARG, E_UNSUP = -1, -5


@pytest.fixture(scope="module")
def edge():
    """kind -> (scalars, x, offset, classes, expected) of edge_jobs: computed once, read-only."""
    out = {}
    for kind in CURVES:
        s, x, o, classes, expected = jc.edge_jobs(kind)
        for a in (s, x, o):
            a.setflags(write=False)
        out[kind] = (s, x, o, classes, expected)
    return out


def _values(kind, s, x, o, i):
    return synth.words_to_int(s[i]), jr.from_words(kind, x[i]), jr.from_words(kind, o[i])


def test_pk_exports_the_sentinel():
    assert pk.JOB_STEP_NONE == NONE == 0xFFFF


def test_edge_jobs_have_their_expected_results(edge):
    for kind in CURVES:
        s, x, o, classes, expected = edge[kind]
        assert s.shape == (64, 4) and x.shape == o.shape == (64, jr.POINT_WORDS[kind]) and len(classes) == len(expected) == 64
        prov, step = jc.check(kind, s, x, o)
        assert prov.dtype == np.uint8 and step.dtype == np.uint16
        bad = [(classes[i], expected[i], (int(prov[i]), int(step[i]))) for i in range(64) if expected[i] != (prov[i], step[i])]
        assert not bad, bad
        have = set(classes)
        want = {"random", "offset = -x, s odd", "offset = -x, s = 2", "offset = x, s = 1", "s = 0, offset = -[2^7]x", "s = 2^256 - 1",
                "s = 2^256 - 1, hit at step 255"}
        want |= {f"{what} at step {k}" for what in ("hit", "doubling") for k in (1, 63, 64, 127, 128, 191, 192, 255)}
        if kind == 0:
            want |= {f"s = {v}{h}" for v in ("r - 1", "r", "r + 1") for h in ("", ", hit at step 252")}
        else:
            want |= {f"off the subgroup, s >= 2^255, hit at step {k}" for k in (255, 254, 130)}
            want |= {"order 10069, hit at step 20", "order 10069, subgroup offset"}
        assert have == want, have ^ want
        # every expected step is one the closed form is compared at
        assert {e[1] for e in expected} - {NONE} <= set(STEPS)
        # special lanes stand beside ordinary ones: the crafted jobs are not all in front
        assert "random" in classes[:16] and any(c != "random" for c in classes[48:])
        # a finite output is necessary, not sufficient: offset = -x with s = 2 has the output x and cannot be proven
        i = classes.index("offset = -x, s = 2")
        outs, fin = jr.outputs(kind, s[i:i + 1], x[i:i + 1], o[i:i + 1])
        assert fin[0] == 1 and np.array_equal(outs[0], x[i]) and expected[i] == (0, 0)
        fin = jr.outputs(kind, s, x, o)[1]
        assert all(prov[i] == 0 for i in range(64) if not fin[i]) and int((prov == 0).sum()) > int((fin == 0).sum())
        # the doubling classes do double where they say, with the bit set, and go on
        for i, c in enumerate(classes):
            if c.startswith("doubling at step "):
                k = int(c.split()[-1])
                sv, xv, ov = _values(kind, s, x, o, i)
                assert (sv >> k) & 1 and (k, "double") in list(jc.walk(kind, sv, xv, ov)), c
        if kind == 1:
            for i, c in enumerate(classes):
                if c.startswith("off the subgroup"):
                    sv, xv, _ = _values(kind, s, x, o, i)
                    assert sv >= 1 << 255 and not synth.g2_in_subgroup(xv)
            i = classes.index("order 10069, hit at step 20")
            assert synth.g2_mul_unreduced(jc.SMALL, jr.from_words(1, x[i])) is None


@pytest.mark.parametrize("kind", CURVES)
def test_stepwise_definition_equals_the_closed_form(edge, kind):
    s, x, o, classes, _ = edge[kind]
    rs, rx, ro = jr.random_jobs(kind, 64, seed=1301 + kind)
    for name, (s_, x_, o_), cls in (("edge", (s, x, o), classes), ("random", (rs, rx, ro), ["random"] * 64)):
        hits = [i for i in range(64) if "hit" in cls[i]]
        full = set((hits[:FULL - 1] + [i for i in range(64) if cls[i] == "random"])[:FULL])
        for i in range(64):
            sv, xv, ov = _values(kind, s_, x_, o_, i)
            prov, step = jc.check_one(kind, sv, xv, ov)
            ks = range(256) if i in full else STEPS
            closed = jc.closed_form(kind, sv, xv, ov, ks)
            # the closed form knows no "first": it names every k whose multiple is minus the offset; the walk ends at the first
            want = [step] if not prov else []
            assert [k for k in closed if prov or k <= step] == want and prov == (step == NONE), (name, cls[i], closed, step)
    assert jc.multiplier(0b1011, 2) == 0b111 and jc.multiplier(5, 0) == 1 and jc.multiplier(2**256 - 1, 255) == 2**256 - 1


def test_fq_exp_jobs_are_all_provable():
    s, x, _ = jr.random_jobs(2, 5, seed=9)
    prov, step = jc.check(2, s, x)
    assert prov.all() and (step == NONE).all()


@pytest.mark.parametrize("kind", CURVES)
def test_definition_is_the_oracle_walk(edge, kind):
    """All provable crafted jobs in one trace of 2^16 rows: the oracle walks them, and its outputs are the definition's.  One job
    of each of four unprovable classes alone: the oracle's addition meets b == -a."""
    s, x, o, classes, expected = edge[kind]
    orc = oracle_lib.load()
    ok = [i for i in range(64) if classes[i] != "random" and expected[i][0]]
    assert len(ok) == (13 if kind == 0 else 11)  # offset = x; 8 doublings; s = 2^256 - 1; s = r - 1, r, r + 1 | the subgroup offset
    pick = (lambda a: np.ascontiguousarray(a[ok]))
    _, got = oracle_lib.generate_trace(orc, kind, pick(s), pick(x), pick(o))
    assert np.array_equal(got, jr.outputs(kind, pick(s), pick(x), pick(o))[0])
    tail = ("s = r, hit at step 252",) if kind == 0 else ("order 10069, hit at step 20",)
    for c in ("offset = -x, s = 2", "hit at step 64", "s = 0, offset = -[2^7]x") + tail:
        i = classes.index(c)
        with pytest.raises(RuntimeError, match="b == -a"):
            oracle_lib.generate_trace(orc, kind, *(np.ascontiguousarray(a[i:i + 1]) for a in (s, x, o)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_entry_points_check_their_arguments(kind):
    lib = pk.load_library()
    pw = jr.POINT_WORDS[kind]
    s, x, o = jr.random_jobs(kind, 3, seed=3)
    prov, step = np.full(3, 7, np.uint8), np.full(3, 7, np.uint16)
    params = pk.default_params()

    def front(kind=kind, s=s, x=x, o=o, n=3, prov=prov, step=step):
        return lib.bn254s_job_check_batch(None, kind, _vp(s), _vp(x), _vp(o), n, _vp(prov), _vp(step))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(s=None) == E_ARG and front(x=None) == E_ARG and front(prov=None) == E_ARG
    assert front(step=None) == E_ARG and front(n=0) == E_ARG and front(kind=3) == E_ARG and front(kind=-1) == E_ARG
    assert front(n=2**32 - 1) == E_ARG

    def full(kind=kind, params=params, s=s, x=x, o=o, n=3, per_proof=16385, prov=prov, step=step, slots=True):
        pr = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_prove_batch_checked(None, kind, C.byref(params) if params is not None else None, _vp(s), _vp(x), _vp(o), n,
                                            per_proof, _vp(prov), _vp(step), pr if slots else None)
        return rc, list(pr)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), slots are cleared
    rc, pr = full()
    assert rc == E_UNSUP and pr[0] is None and pr[1] == 1
    assert full(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    rc, pr = full(per_proof=2)
    assert rc == E_ARG and pr[0] is None and pr[1] is None and pr[2] == 1
    # the two outputs of the check may be NULL
    assert full(prov=None)[0] == E_UNSUP and full(step=None)[0] == E_UNSUP
    # each invalid argument alone is reported before the shape and touches no slot
    for bad in (dict(s=None), dict(x=None), dict(params=None), dict(n=0), dict(per_proof=0), dict(kind=3), dict(kind=-1),
                dict(n=2**32 - 1)):
        assert full(**bad) == (E_ARG, [1] * 4), bad
    assert full(slots=False)[0] == E_ARG
    other = pk.default_params()
    other.struct_size += 4
    assert full(params=other) == (E_ARG, [1] * 4)
    if kind == 2:
        assert full(o=x)[0] == E_UNSUP  # an offset is not read for Fq exp, NULL or not
    else:
        assert full(o=None)[0] == E_ARG and front(o=None) == E_ARG
    assert (prov == 7).all() and (step == 7).all()
