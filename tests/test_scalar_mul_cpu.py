"""Scalar multiplication without an offset argument, the parts that need no GPU: the Python definition (tools/scalar_mul_ref.py)
against the plain complete-law s x and its crafted jobs against both forms of the job check (tools/job_check_ref.py: the walk
and the closed form); and the argument checks of bn254s_scalar_mul_batch / bn254s_scalar_mul that are answered before any device
work, without a context where the order of the checks allows it."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import scalar_mul_ref as sm
from tools import synth

P, R = synth.P, synth.R_ORDER
E_ARG, E_UNSUP = -1, -5
CURVES = (0, 1)
PW = jr.POINT_WORDS
SEED = (0x5EED, 1, 2, 0xFFFFFFFF00000000)  # the last word is the largest canonical Goldilocks element
GL_P = 0xFFFFFFFF00000001
STEPS = (0, 1, 63, 64, 255)
N = 3


def _mul(kind):
    return jr.g1_mul_complete if kind == 0 else synth.g2_mul_unreduced


@pytest.mark.parametrize("kind", CURVES)
def test_product_is_the_plain_scalar_multiple(kind):
    """12 jobs per kind: random ones, s = 0 / 1 / r + 1 / r / 2^256 - 1, and on the twist an x off the subgroup."""
    s, x, _ = jr.provable_jobs(kind, 12, seed=97 + kind)
    for j, v in enumerate((0, 1, R + 1, R, (1 << 256) - 1)):
        s[j] = synth._to_words(v)
    prods, finite, offs, outs, att = sm.scalar_mul(kind, s, x, SEED)
    assert (att == 0).all()
    for i in range(12):
        si, xi = synth.words_to_int(s[i]), jr.from_words(kind, x[i])
        want = _mul(kind)(si, xi)
        assert list(prods[i]) == jr.to_words(kind, want) and finite[i] == (want is not None)
        off = sm.offset(kind, SEED, i, 0)
        assert list(offs[i]) == jr.to_words(kind, off)
        assert list(outs[i]) == jr.to_words(kind, jr.output_one(kind, si, xi, off))
    assert [int(finite[j]) for j in (0, 1, 3)] == [0, 1, kind]  # s = 0; s = 1; s = r: O on G1, finite on the twist, where x_3 is off the subgroup


@pytest.mark.parametrize("kind", CURVES)
def test_offsets_depend_on_seed_index_attempt_and_kind_only(kind):
    assert sm.hash_inputs(kind, SEED, (1 << 32) + 5, 3) == list(SEED) + [5, 1, 3, 0x62736D00 + kind]
    a = sm.offset(kind, SEED, 7, 0)
    assert a != sm.offset(kind, SEED, 7, 1) and a != sm.offset(kind, SEED, 8, 0) and a != sm.offset(kind, (0x5EED, 1, 2, 4), 7, 0)
    if kind == 0:
        assert (a[1] * a[1] - a[0] ** 3 - 3) % P == 0
    else:
        assert synth.g2_on_curve(a) and synth.g2_in_subgroup(a)


@pytest.mark.parametrize("k", STEPS)
@pytest.mark.parametrize("kind", CURVES)
def test_crafted_jobs_hit_at_attempt_0_only(kind, k):
    i = 11 + k
    s = synth.Xoshiro256ss(1000 * kind + k).next_u256()
    x = sm.crafted_x(kind, SEED, i, s, k)
    assert x is not None
    r0, r1 = sm.offset(kind, SEED, i, 0), sm.offset(kind, SEED, i, 1)
    assert jc.check_one(kind, s, x, r0) == (0, k)
    assert jc.check_one(kind, s, x, r1) == (1, jc.STEP_NONE)
    ks = sorted(set(STEPS) | {k})
    assert jc.closed_form(kind, s, x, r0, ks) == [k]
    assert jc.closed_form(kind, s, x, r1, ks) == []
    prod, off, out, a = sm.scalar_mul_one(kind, s, x, SEED, i)
    assert a == 1 and off == r1 and prod == _mul(kind)(s, x)
    with pytest.raises(sm.Exhausted) as e:
        sm.scalar_mul_one(kind, s, x, SEED, i, max_attempts=1)
    assert (e.value.i, e.value.step, e.value.attempt) == (i, k, 0)


@pytest.mark.parametrize("kind", CURVES)
def test_crafted_job_skips_a_multiplier_that_is_a_multiple_of_r(kind):
    assert jc.multiplier(R - (1 << 253), 253) == R
    assert sm.crafted_x(kind, SEED, 0, R - (1 << 253), 253) is None
    assert sm.opposite_x(kind, SEED, 0, 2 * R) is None


@pytest.mark.parametrize("kind", CURVES)
def test_opposite_job_doubles_in_the_subtraction(kind):
    _, neg = jr._law(kind)
    s = 5
    x = sm.opposite_x(kind, SEED, 3, s)
    prod, off, out, a = sm.scalar_mul_one(kind, s, x, SEED, 3)
    assert a == 0 and out == neg(off) and prod == _mul(kind)(s, x) and prod is not None


# ---- the argument checks of the C entry points ------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _args(kind, n=N):
    """scalars, x (a valid point n times), seed, products, finite, offsets, outputs, attempts: outputs pre-filled with 7."""
    x1 = jr.to_words(kind, sm.offset(kind, SEED, 0, 0))
    return dict(scalars=np.ones((n, 4), np.uint64), x=np.array([x1] * n, np.uint64), seed=np.array(SEED, np.uint64),
                products=np.full((n, PW[kind]), 7, np.uint64), finite=np.full(n, 7, np.uint8), offsets=np.full((n, PW[kind]), 7, np.uint64),
                outputs=np.full((n, PW[kind]), 7, np.uint64), attempts=np.full(n, 7, np.uint8))


OUT = ("products", "finite", "offsets", "outputs", "attempts")


def _batch(lib, kind, a, ctx=None, n=N, max_attempts=4, null=()):
    p = {k: (None if k in null else _vp(v)) for k, v in a.items()}
    return lib.bn254s_scalar_mul_batch(ctx, kind, p["scalars"], p["x"], n, p["seed"], max_attempts, p["products"], p["finite"],
                                       p["offsets"], p["outputs"], p["attempts"])


def _full(lib, kind, a, per_proof, ctx=None, n=N, max_attempts=4, null=(), params=None, no_params=False, no_slots=False):
    p = {k: (None if k in null else _vp(v)) for k, v in a.items()}
    params = params or pk.default_params()
    slots = (C.c_void_p * 8)(*([1] * 8))
    rc = lib.bn254s_scalar_mul(ctx, kind, None if no_params else C.byref(params), p["scalars"], p["x"], n, per_proof, p["seed"],
                               max_attempts, p["products"], p["finite"], p["offsets"], p["outputs"], p["attempts"],
                               None if no_slots else slots)
    return rc, list(slots)


def _untouched(a):
    return all((a[k] == 7).all() for k in OUT)


def test_the_symbols_exist():
    lib = pk.load_library()
    assert hasattr(lib, "bn254s_scalar_mul_batch") and hasattr(lib, "bn254s_scalar_mul")


@pytest.mark.parametrize("kind", CURVES)
def test_argument_ladder_of_the_proven_call(kind):
    """As tests/test_proven_args_cpu.py has it for the other proven calls: invalid arguments first, then per_proof, the context last."""
    lib = pk.load_library()
    a = _args(kind)
    rc, slots = _full(lib, kind, a, 16384)  # a valid shape: only the context is missing
    assert rc == E_ARG and slots[0] is None and slots[1] == 1
    rc, slots = _full(lib, kind, a, 2)
    assert rc == E_ARG and slots[:2] == [None, None] and slots[2] == 1
    rc, slots = _full(lib, kind, a, 16385)  # the shape answers before the context
    assert rc == E_UNSUP and slots[0] is None and slots[1:] == [1] * 7
    for name in ("scalars", "x", "seed", "products", "finite", "offsets"):  # each required pointer alone, before the shape
        assert _full(lib, kind, a, 16385, null=(name,)) == (E_ARG, [1] * 8), name
    assert _full(lib, kind, a, 16385, no_params=True) == (E_ARG, [1] * 8)
    assert _full(lib, kind, a, 16385, no_slots=True)[0] == E_ARG
    for name in ("outputs", "attempts"):  # these may be NULL
        assert _full(lib, kind, a, 16385, null=(name,))[0] == E_UNSUP, name
    assert _full(lib, kind, a, 0) == (E_ARG, [1] * 8)
    bad = pk.default_params()
    bad.struct_size += 4
    assert _full(lib, kind, a, 16385, params=bad) == (E_ARG, [1] * 8)
    assert _full(lib, kind, a, 16385, n=0) == (E_ARG, [1] * 8)
    assert _full(lib, kind, a, 16385, n=2**32 - 1) == (E_ARG, [1] * 8)  # n >= UINT_MAX, before any array is read
    for m in (0, -1, 9):
        assert _full(lib, kind, a, 16385, max_attempts=m) == (E_ARG, [1] * 8), m
    assert _full(lib, kind, a, 16385, max_attempts=8)[0] == E_UNSUP and _full(lib, kind, a, 16385, max_attempts=1)[0] == E_UNSUP
    for w in range(4):  # a seed word that is not canonical
        b = dict(a, seed=a["seed"].copy())
        b["seed"][w] = GL_P
        assert _full(lib, kind, b, 16385) == (E_ARG, [1] * 8), w
    for c in range(PW[kind] // 4):  # a coordinate of x that is p
        b = dict(a, x=a["x"].copy())
        b["x"][1, 4 * c:4 * c + 4] = synth._to_words(P)
        assert _full(lib, kind, b, 16385) == (E_ARG, [1] * 8), c
    assert _untouched(a)


@pytest.mark.parametrize("kind", (-1, 2, 3))
def test_kinds_other_than_the_curves_are_invalid(kind):
    lib = pk.load_library()
    a = _args(0)
    assert _full(lib, kind, a, 16385) == (E_ARG, [1] * 8)
    assert _batch(lib, kind, a) == E_ARG and _untouched(a)


@pytest.mark.parametrize("kind", CURVES)
def test_batch_call_without_a_context(kind):
    lib = pk.load_library()
    a = _args(kind)
    assert _batch(lib, kind, a) == E_ARG
    assert _batch(lib, kind, a, null=("outputs", "attempts")) == E_ARG
    assert _untouched(a)


def test_wrappers_check_shapes():
    ctx = pk.Context.__new__(pk.Context)  # no device: the shape checks come before the library is entered
    ctx._h = None
    a = _args(0)
    with pytest.raises(ValueError, match="seed"):
        ctx.scalar_mul_batch(0, a["scalars"], a["x"], [1, 2, 3])
    with pytest.raises(ValueError, match="job_outputs"):
        ctx.scalar_mul(0, a["scalars"], a["x"][:, :4], list(SEED))
