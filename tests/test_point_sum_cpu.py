"""The point-sum check and the two statement verifiers, the parts that need no GPU: the crafted relations of
tools/point_sum_ref.py against a second route to their codes (a + b by the complete law, compared as integers), that every code
and every exceptional relation is among them, and the argument checks of bn254s_point_sum_check_batch, bn254s_verify_scalar_mul
and bn254s_verify_msm_multi, which are all answered before any device work and before the context is looked at."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from plonky2_bn254_amd import lib as pkl
from tools import job_outputs_ref as jr
from tools import point_sum_ref as ps
from tools import synth

P = synth.P
CURVES = (0, 1)
PW = jr.POINT_WORDS
E_ARG = -1
N, M, PER = 5, 3, 2  # jobs, MSMs and jobs per proof of the argument ladders: three proofs


@pytest.fixture(scope="module")
def crafted():
    return {kind: ps.cases(kind) for kind in CURVES}


def test_the_symbols_and_constants_exist():
    lib = pk.load_library()
    for name in ("bn254s_point_sum_check_batch", "bn254s_verify_scalar_mul", "bn254s_verify_msm_multi"):
        assert hasattr(lib, name), name
    assert lib.bn254s_abi_version() == 1
    assert (pkl.SUM_OK, pkl.SUM_A_NOT_ZERO, pkl.SUM_A_OFF_CURVE, pkl.SUM_B_OFF_CURVE, pkl.SUM_C_OFF_CURVE, pkl.SUM_INFINITE, pkl.SUM_X,
            pkl.SUM_Y, pkl.SUM_X_OFF_CURVE, pkl.SUM_HEAD, pkl.SUM_CHAIN) == tuple(range(11))
    assert (ps.OK, ps.A_NOT_ZERO, ps.A_OFF_CURVE, ps.B_OFF_CURVE, ps.C_OFF_CURVE, ps.INFINITE, ps.SUM_X, ps.SUM_Y) == tuple(range(8))


@pytest.mark.parametrize("kind", CURVES)
def test_crafted_codes_agree_with_the_complete_law(crafted, kind):
    a, fin, b, c, want, names = crafted[kind]
    add, neg = jr._law(kind)
    assert set(range(8)) <= set(int(v) for v in want)
    assert np.array_equal(ps.codes(kind, a, fin, b, c), want)
    for i, name in enumerate(names):  # the second route, written out here: curve membership, then integers against integers
        pa = jr.from_words(kind, a[i]) if fin[i] else None
        pb, pc = jr.from_words(kind, b[i]), jr.from_words(kind, c[i])
        if not fin[i] and a[i].any():
            got = 1
        elif pa is not None and not ps.on_curve(kind, pa):
            got = 2
        elif not ps.on_curve(kind, pb):
            got = 3
        elif not ps.on_curve(kind, pc):
            got = 4
        else:
            total = add(pa, pb)
            got = 5 if total is None else 0 if total == pc else 7 if total == neg(pc) else 6
            assert got != 6 or total[0] != pc[0]
        assert got == want[i], name
        for w in (b[i], c[i]) + ((a[i],) if fin[i] else ()):  # what the entry point takes: every coordinate read is below p
            assert all(synth.words_to_int(w[4 * k:4 * k + 4]) < P for k in range(PW[kind] // 4)), name


@pytest.mark.parametrize("kind", CURVES)
def test_the_exceptional_relations_are_present(crafted, kind):
    a, fin, b, c, want, names = crafted[kind]
    code = dict(zip(names, (int(v) for v in want)))
    row = names.index
    accepted = {"general", "a = O", "a == b"} | ({"twist points outside the subgroup", "a == b outside the subgroup"} if kind == 1 else set())
    assert all(code[k] == 0 for k in accepted)
    i = row("a = O")
    assert fin[i] == 0 and not a[i].any() and np.array_equal(b[i], c[i])
    i = row("a == b")
    assert np.array_equal(a[i], b[i]) and list(c[i]) == jr.to_words(kind, jr._law(kind)[0](*(jr.from_words(kind, a[i]),) * 2))
    if kind == 1:
        i = row("twist points outside the subgroup")
        assert not any(synth.g2_in_subgroup(jr.from_words(1, w)) for w in (a[i], b[i]))
    assert code["c = -(a + b)"] == 7 and code["a == b, c = -(2a)"] == 7
    assert code["a = -b"] == 5 and code["a = -b, c = a"] == 5
    assert code["a = O, c = -b"] == 7 and code["a = O, c another point"] == 6 and code["c another point"] == 6
    assert code["finite = 0, the words of a point"] == 1 and code["finite = 0, one word"] == 1
    for coord in range(PW[kind] // 4):
        assert [code[f"{t} off its curve ({coord})"] for t in "abc"] == [2, 3, 4]
    assert code["a and c off their curves"] == 2


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _point(kind):
    return jr.to_words(kind, synth.G1_GEN if kind == 0 else synth.G2_GEN)


def _p_at(arr, row, coord):
    out = arr.copy()
    out[row, 4 * coord:4 * coord + 4] = synth._to_words(P)
    return out


@pytest.mark.parametrize("kind", CURVES)
def test_argument_ladder_of_point_sum_check(kind):
    lib = pk.load_library()
    pt = np.array([_point(kind)] * N, np.uint64)
    a = dict(a=pt, a_finite=np.ones(N, np.uint8), b=pt.copy(), c=pt.copy(), code=np.full(N, 7, np.uint8))

    def call(kind_=kind, n=N, null=(), **over):
        p = {k: (None if k in null else _vp(over.get(k, v))) for k, v in a.items()}
        return lib.bn254s_point_sum_check_batch(None, kind_, p["a"], p["a_finite"], p["b"], p["c"], n, p["code"])

    assert call() == E_ARG  # a valid shape: only the context is missing
    for k in a:
        assert call(null=(k,)) == E_ARG
    assert call(n=0) == E_ARG and call(n=2**32 - 1) == E_ARG and call(n=2**32) == E_ARG
    assert call(kind_=2) == E_ARG and call(kind_=-1) == E_ARG
    for k in "abc":
        for coord in range(PW[kind] // 4):
            assert call(**{k: _p_at(pt, N - 1, coord)}) == E_ARG
    assert (a["code"] == 7).all()


class _Proofs:
    """Three proof slots of four words each: the verifiers look at nothing of them before the context."""

    def __init__(self, k=3):
        self.arr = [np.zeros(4, np.uint64) for _ in range(k)]
        self.table = (C.c_void_p * k)(*[w.ctypes.data for w in self.arr])
        self.n_words = (C.c_size_t * k)(*([4] * k))
        self.bits = (C.c_uint32 * k)(*([16] * k))


def _verifier_args(kind):
    pt = np.array([_point(kind)] * N, np.uint64)
    return dict(scalars=np.ones((N, 4), np.uint64), x=pt, seg_len=np.array([1, 3, 1], np.uintp), R=pt[:M].copy(),
                products=pt.copy(), results=pt[:M].copy(), finite=np.ones(N, np.uint8), offsets=pt.copy(), outputs=pt.copy(),
                link=np.full(N, 7, np.uint8), status=np.full(3, 7, np.int32))


def _smul(lib, kind, a, pr, n=N, n_proofs=3, per_proof=PER, null=(), params=None, no_params=False, **over):
    p = {k: (None if k in null else _vp(over.get(k, v))) for k, v in a.items()}
    params = params or pk.default_params()
    return lib.bn254s_verify_scalar_mul(None, kind, None if no_params else C.byref(params), None if "words" in null else pr.table,
                                        None if "n_words" in null else pr.n_words, None if "degree_bits" in null else pr.bits, n_proofs,
                                        per_proof, p["scalars"], p["x"], n, p["products"], p["finite"], p["offsets"], p["outputs"],
                                        p["link"], p["status"])


def _msm(lib, kind, a, pr, n=N, m=M, n_proofs=3, per_proof=PER, null=(), params=None, no_params=False, **over):
    p = {k: (None if k in null else _vp(over.get(k, v))) for k, v in a.items()}
    params = params or pk.default_params()
    return lib.bn254s_verify_msm_multi(None, kind, None if no_params else C.byref(params), None if "words" in null else pr.table,
                                       None if "n_words" in null else pr.n_words, None if "degree_bits" in null else pr.bits, n_proofs,
                                       per_proof, p["scalars"], p["x"], p["seg_len"], m, n, p["R"], p["results"], p["finite"], p["offsets"],
                                       p["outputs"], p["link"], p["status"])


@pytest.mark.parametrize("kind", CURVES)
def test_argument_ladder_of_verify_scalar_mul(kind):
    lib, a, pr = pk.load_library(), _verifier_args(kind), _Proofs()
    call = lambda **kw: _smul(lib, kind, a, pr, **kw)
    assert call() == E_ARG  # a valid shape: only the context is missing
    assert call(null=("link", "status")) == E_ARG  # (the two optional outputs)
    for k in ("scalars", "x", "products", "finite", "offsets", "outputs", "words", "n_words", "degree_bits"):
        assert call(null=(k,)) == E_ARG, k
    assert call(no_params=True) == E_ARG
    hole = _Proofs()
    hole.table[1] = None
    assert _smul(lib, kind, a, hole) == E_ARG
    assert call(n=0, n_proofs=0) == E_ARG and call(per_proof=0) == E_ARG
    assert call(n_proofs=2) == E_ARG and call(n_proofs=4) == E_ARG
    assert _smul(lib, 2, a, pr) == E_ARG and _smul(lib, -1, a, pr) == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert call(params=bad) == E_ARG
    for k in ("x", "products", "offsets", "outputs"):
        for coord in range(PW[kind] // 4):
            assert call(**{k: _p_at(a[k], 3, coord)}) == E_ARG, k
    assert (a["link"] == 7).all() and (a["status"] == 7).all()


@pytest.mark.parametrize("kind", CURVES)
def test_argument_ladder_of_verify_msm_multi(kind):
    lib, a, pr = pk.load_library(), _verifier_args(kind), _Proofs()
    call = lambda **kw: _msm(lib, kind, a, pr, **kw)
    assert call() == E_ARG  # a valid shape: only the context is missing
    assert call(null=("link", "status")) == E_ARG
    for k in ("scalars", "x", "seg_len", "R", "results", "finite", "offsets", "outputs", "words", "n_words", "degree_bits"):
        assert call(null=(k,)) == E_ARG, k
    assert call(no_params=True) == E_ARG
    assert call(n=0, n_proofs=0) == E_ARG and call(m=0) == E_ARG and call(per_proof=0) == E_ARG
    assert call(n_proofs=2) == E_ARG and call(n_proofs=4) == E_ARG
    for seg in ([1, 0, 4], [1, 3, 2], [1, 2, 1], [5, 2**64 - 1, 1]):  # a zero; a sum above n; one below; one that wraps round to n
        assert call(seg_len=np.array(seg, np.uintp)) == E_ARG, seg
    assert _msm(lib, 2, a, pr) == E_ARG and _msm(lib, -1, a, pr) == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert call(params=bad) == E_ARG
    for k, row in (("x", 3), ("R", 2), ("results", 2), ("offsets", 3), ("outputs", 3)):
        for coord in range(PW[kind] // 4):
            assert call(**{k: _p_at(a[k], row, coord)}) == E_ARG, k
    assert (a["link"] == 7).all() and (a["status"] == 7).all()
