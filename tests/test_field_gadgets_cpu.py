"""The field gadgets without a GPU: the reference tool (tools/field_gadgets_ref.py) against the definitions on its crafted sets and
on 200 random elements per field, and the argument ladder of bn254s_fq_sqrt / bn254s_fq2_sqrt and of the four batch calls without
a context, in the manner of tests/test_proven_args_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import field_gadgets_ref as ref

P = ref.P
E_ARG, E_UNSUP = -1, -5
N = 3


def _fq_cases():
    vals = list(ref.crafted_fq().values()) + ref.random_fq(200, seed=11)
    return ref.both_signs(vals)


def _fq2_cases():
    vals = list(ref.crafted_fq2().values()) + ref.random_fq2(200, seed=12)
    return ref.both_signs(vals)


def test_reference_fq_roots_obey_the_definitions():
    vals, sgns = _fq_cases()
    seen = set()
    for x, s in zip(vals, sgns):
        y, square, ok = ref.fq_sqrt(x, int(s))
        leg = pow(x, (P - 1) // 2, P)
        assert leg in (0, 1, P - 1) and (leg == 0) == (x == 0)
        assert square == (leg == 1)
        assert ok == (square if x else s == 0)
        if ok:
            assert 0 <= y < P and y * y % P == x and (y & 1) == s
        else:
            assert y == 0
        seen.add((square, ok))
    assert seen == {(True, True), (False, False), (False, True)}  # squares, non-squares and the even root of zero


def test_reference_fq2_roots_obey_the_definitions():
    vals, sgns = _fq2_cases()
    shapes = set()
    for x, s in zip(vals, sgns):
        y, square, ok = ref.fq2_sqrt(x, int(s))
        nrm = (x[0] * x[0] + x[1] * x[1]) % P
        leg = pow(nrm, (P - 1) // 2, P)
        assert (leg == 0) == (x == (0, 0))
        assert square == (leg == 1)
        assert ok == (square if x != (0, 0) else s == 0)
        if ok:
            assert max(y) < P
            assert ((y[0] * y[0] - y[1] * y[1]) % P, 2 * y[0] * y[1] % P) == x
            assert ((y[0] & 1) if y[0] else (y[1] & 1)) == s
            shapes.add((y[0] == 0, y[1] == 0))
        else:
            assert y == (0, 0)
    # roots (t, 0), (0, t) - the sign falls to c1 -, general ones and the zero
    assert shapes == {(False, True), (True, False), (False, False), (True, True)}


def test_reference_crafted_sets_hold_what_their_names_say():
    fq = ref.crafted_fq()
    assert ref.legendre(fq["p-1"]) == P - 1 and ref.legendre(fq["smallest non-residue"]) == P - 1
    assert all(ref.legendre(v) == 1 for v in range(1, fq["smallest non-residue"]))
    y, _, _ = ref.fq_sqrt(fq["root with the top limb at its maximum"], 0)
    assert max(y, P - y) >> 192 == P >> 192
    fq2 = ref.crafted_fq2()
    assert ref.fq2_sqrt(fq2["(p-1,0)"], 1)[0] == (0, 1) and ref.fq2_sqrt(fq2["(p-1,0)"], 0)[0] == (0, P - 1)
    assert ref.fq2_sqrt(fq2["(n,0), n a non-residue"], 0)[0][0] == 0
    assert sum(name.startswith("delta a residue") for name in fq2) == 2 and sum(name.startswith("delta a non-residue") for name in fq2) == 2
    for name, v in fq2.items():
        if name.startswith("non-residue norm"):
            assert ref.fq2_sqrt(v, 0) == ((0, 0), False, False)
        if name.startswith("delta"):
            assert ref.fq2_delta_is_residue(v) == name.startswith("delta a residue")


def test_reference_inverses():
    for x in ref.crafted_inv_fq() + ref.random_fq(200, seed=13):
        assert ref.fq_inv(x) * x % P == (1 if x else 0) and (x or ref.fq_inv(x) == 0)
    for x in ref.crafted_inv_fq2() + ref.random_fq2(200, seed=14):
        i = ref.fq2_inv(x)
        prod = ((x[0] * i[0] - x[1] * i[1]) % P, (x[0] * i[1] + x[1] * i[0]) % P)
        assert prod == ((1, 0) if x != (0, 0) else (0, 0)) and (x != (0, 0) or i == (0, 0))


def test_reference_words_round_trip():
    vals, sgns = ref.both_signs([0, 4, P - 1])
    roots, square, ok, jobs = ref.fq_sqrt_words(ref.fq_words(vals), sgns)
    assert square.tolist() == [0, 0, 1, 1, 0, 0] and ok.tolist() == [1, 0, 1, 1, 0, 0]
    assert [ref.from_words(r) for r in roots] == [0, 0, 2, P - 2, 0, 0]
    assert all(ref.from_words(j[:4]) == (P - 1) // 2 and ref.from_words(j[4:]) == v for j, v in zip(jobs, vals))
    roots, square, ok, jobs = ref.fq2_sqrt_words(ref.fq2_words([(0, 0), (P - 1, 0)]), [1, 1])
    assert square.tolist() == [0, 1] and ok.tolist() == [0, 1] and ref.from_words(roots[1, 4:]) == 1 and not roots[1, :4].any()
    assert ref.from_words(jobs[1, 4:]) == 1  # norm((p-1, 0)) = 1


# ---- the argument ladder without a context ----------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _proven(lib, name, w, per_proof, null=None, params=None, xs=None, sgns="zeros", n=N):
    """The proven call without a context, every slot preset to the marker 1; `null` names the argument passed as NULL.
    -> (return code, slots, the output arrays)."""
    params = params or pk.default_params()
    slots = (C.c_void_p * 8)(*([1] * 8))
    a = {"xs": np.zeros((N, w), np.uint64) if xs is None else xs, "sgns": np.zeros(N, np.uint8) if isinstance(sgns, str) else sgns,
         "roots": np.zeros((N, w), np.uint64), "square": np.zeros(N, np.uint8), "ok": np.zeros(N, np.uint8), "jobs": np.zeros((N, 8), np.uint64)}
    p = {k: (None if k == null else _vp(v)) for k, v in a.items()}
    rc = getattr(lib, name)(None, None if null == "params" else C.byref(params), p["xs"], p["sgns"], n, per_proof, p["roots"],
                            p["square"], p["ok"], p["jobs"], None if null == "slots" else slots)
    return rc, list(slots), [a[k] for k in ("roots", "square", "ok", "jobs")]


@pytest.mark.parametrize("name,w", [("bn254s_fq_sqrt", 4), ("bn254s_fq2_sqrt", 8)])
def test_proven_calls_check_their_arguments(name, w):
    lib = pk.load_library()
    # a valid shape: only the context is missing; the slots of the call are cleared, the next one is not touched
    rc, slots, _ = _proven(lib, name, w, 16384)
    assert rc == E_ARG and slots[0] is None and slots[1] == 1
    rc, slots, _ = _proven(lib, name, w, 2)
    assert rc == E_ARG and slots[:2] == [None, None] and slots[2] == 1
    # per_proof above the limit answers before the context, with the slots cleared
    rc, slots, _ = _proven(lib, name, w, 16385)
    assert rc == E_UNSUP and slots[0] is None and slots[1:] == [1] * 7
    # each NULL pointer alone answers before the shape and touches no slot; sgns and fq_jobs may be NULL
    for null in ("params", "xs", "roots", "square", "ok", "slots"):
        rc, slots, _ = _proven(lib, name, w, 16385, null=null)
        assert rc == E_ARG and slots == [1] * 8, null
    for null in ("sgns", "jobs"):
        assert _proven(lib, name, w, 16385, null=null)[0] == E_UNSUP, null
    # n = 0, per_proof = 0 and parameters of another size likewise
    assert _proven(lib, name, w, 16385, n=0)[:2] == (E_ARG, [1] * 8)
    assert _proven(lib, name, w, 0)[:2] == (E_ARG, [1] * 8)
    bad = pk.default_params()
    bad.struct_size += 4
    assert _proven(lib, name, w, 16385, params=bad)[:2] == (E_ARG, [1] * 8)
    # an sgns byte of 2 and a coordinate of p: invalid arguments, and nothing is written
    rc, _, outs = _proven(lib, name, w, 2, sgns=np.array([0, 2, 1], np.uint8))
    assert rc == E_ARG and not any(o.any() for o in outs)
    xs = np.zeros((N, w), np.uint64)
    xs[1, w - 4:] = ref.to_words(P)
    rc, _, outs = _proven(lib, name, w, 2, xs=xs)
    assert rc == E_ARG and not any(o.any() for o in outs)


def test_batch_calls_without_a_context_are_invalid():
    lib = pk.load_library()
    for name, w in (("bn254s_fq_sqrt_batch", 4), ("bn254s_fq2_sqrt_batch", 8)):
        xs, roots, jobs = np.zeros((N, w), np.uint64), np.full((N, w), 7, np.uint64), np.full((N, 8), 7, np.uint64)
        sgns, square, ok = np.zeros(N, np.uint8), np.full(N, 7, np.uint8), np.full(N, 7, np.uint8)
        assert getattr(lib, name)(None, _vp(xs), _vp(sgns), N, _vp(roots), _vp(square), _vp(ok), _vp(jobs)) == E_ARG
        assert (roots == 7).all() and (jobs == 7).all() and (square == 7).all() and (ok == 7).all()
    for name, w in (("bn254s_fq_inv_batch", 4), ("bn254s_fq2_inv_batch", 8)):
        xs, out = np.ones((N, w), np.uint64), np.full((N, w), 7, np.uint64)
        assert getattr(lib, name)(None, _vp(xs), N, _vp(out)) == E_ARG and (out == 7).all()


def test_package_exports_the_checkers():
    assert callable(pk.verify_fq_sqrt) and callable(pk.verify_fq2_sqrt)
    for m in ("fq_sqrt_batch", "fq2_sqrt_batch", "fq_sqrt", "fq2_sqrt", "fq_inv_batch", "fq2_inv_batch"):
        assert callable(getattr(pk.Context, m))
