"""Many MSMs as one segmented chain without a GPU: the Python reference (tools/msm_multi_ref.py) against the naive sequential fold
and against scalar algebra on multiples of the generators, crafted_x against the walk of the job check, the argument ladder of
the two C entry points with ctx = NULL, and verify_msm_multi on proofs made by the CPU oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import msm_multi_ref as mm
from tools import synth

P, R_ORD = synth.P, synth.R_ORDER
CURVES = (0, 1)
PW = jr.POINT_WORDS
SEED = (0x6D6D, 0xFFFFFFFF00000000, 0, 5)
GL_P = 0xFFFFFFFF00000001
E_ARG, E_UNSUP = -1, -5
GEN = {0: synth.G1_GEN, 1: synth.G2_GEN}


def _inputs(kind, n, seed):
    return (synth.g1_inputs if kind == 0 else synth.g2_inputs)(n, seed)


def _words(kind, pts):
    return np.array([jr.to_words(kind, p) for p in pts], np.uint64).reshape(len(pts), PW[kind])


def _swords(ss):
    return np.array([synth._to_words(s) for s in ss], np.uint64).reshape(-1, 4)


def _mulg(kind, k):
    """[k mod r] of the generator, None for the point at infinity."""
    return jr.g1_mul_complete(k, GEN[0]) if kind == 0 else synth.g2_mul_unreduced(k % R_ORD, GEN[1])


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CURVES)
def test_reference_matches_the_naive_fold(kind):
    s, x, o = _inputs(kind, 7, seed=31 + kind)
    seg = [1, 4, 2]
    R = np.ascontiguousarray(o[:3])
    got = mm.msm_multi(kind, s, x, seg, R=R)
    assert (got.bad_link == mm.LINK_NONE).all() and (got.bad_step == mm.STEP_NONE).all() and (got.attempts == 0).all() and got.finite.all()
    assert np.array_equal(got.R, R)
    add, neg = jr._law(kind)
    lo = 0
    for j, ln in enumerate(seg):
        ss = [synth.words_to_int(v) for v in s[lo:lo + ln]]
        xs = [jr.from_words(kind, v) for v in x[lo:lo + ln]]
        offs = mm.naive_fold(kind, ss, xs, jr.from_words(kind, R[j]))
        assert np.array_equal(got.offsets[lo:lo + ln], _words(kind, offs[:-1])), j
        assert np.array_equal(got.outputs[lo:lo + ln], _words(kind, offs[1:])), j
        assert list(got.results[j]) == jr.to_words(kind, add(offs[-1], neg(offs[0]))), j
        lo += ln


@pytest.mark.parametrize("kind", CURVES)
def test_reference_matches_scalar_algebra(kind):
    """x_i = [k_i] G: T_{j,t} = [sum s k] G.  MSM 1 passes through infinity inside and MSM 2 ends there; a head cuts the sum."""
    rng = synth.Xoshiro256ss(77 + kind)
    ks = [rng.next_u256() % (R_ORD - 1) + 1 for _ in range(8)]
    ss = [rng.next_u256() % R_ORD for _ in range(8)]
    ks[3], ss[3] = ks[2], R_ORD - ss[2]            # MSM 1 = inputs 2 .. 5: T_{1,2} is infinity
    ks[7], ss[7] = ks[6], R_ORD - ss[6]            # MSM 2 = inputs 6, 7: the result is infinity
    seg, rk = [2, 4, 2], [11, 12, 13]
    x = _words(kind, [_mulg(kind, k) for k in ks])
    R = _words(kind, [_mulg(kind, k) for k in rk])
    got = mm.msm_multi(kind, _swords(ss), x, seg, R=R)
    assert list(got.finite) == [1, 1, 0] and not got.results[2].any() and (got.bad_link == mm.LINK_NONE).all()
    lo = 0
    for j, ln in enumerate(seg):
        acc = 0
        for t in range(ln):
            assert list(got.offsets[lo + t]) == jr.to_words(kind, _mulg(kind, rk[j] + acc)), (j, t)
            acc += ss[lo + t] * ks[lo + t]
            assert list(got.outputs[lo + t]) == jr.to_words(kind, _mulg(kind, rk[j] + acc)), (j, t)
        assert list(got.results[j]) == jr.to_words(kind, _mulg(kind, acc)), j
        lo += ln
    assert np.array_equal(got.offsets[4], R[1]) and np.array_equal(got.outputs[7], R[2])


@pytest.mark.parametrize("kind", CURVES)
def test_drawn_points_and_acceptance(kind):
    s, x, _ = _inputs(kind, 5, seed=41 + kind)
    s[:, 3] &= np.uint64((1 << 62) - 1)
    seg = [2, 3]
    plain = mm.msm_multi(kind, s, x, seg, seed=SEED)
    assert (plain.attempts == 0).all() and list(plain.R[1]) == jr.to_words(kind, mm.drawn(kind, SEED, 1, 0))
    assert mm.hash_inputs(kind, SEED, (1 << 32) + 5, 3) == list(SEED) + [5, 1, 3, 0x626D6D00 + kind]
    # link 1 of MSM 1 made to hit step 64 under the point of attempt 0
    R0 = mm.drawn(kind, SEED, 1, 0)
    T = mm.chain_one(kind, mm.products(kind, s[2:3], x[2:3]), None)[2]
    x2 = x.copy()
    x2[3] = jr.to_words(kind, mm.crafted_x(kind, R0, T, synth.words_to_int(s[3]), 64))
    one = mm.msm_multi(kind, s, x2, seg, seed=SEED, max_attempts=1)
    assert list(one.attempts) == [0, 1] and list(one.bad_link) == [mm.LINK_NONE, 1] and list(one.bad_step) == [mm.STEP_NONE, 64]
    assert not one.offsets[2:].any() and not one.outputs[2:].any() and one.finite[1] and np.array_equal(one.offsets[:2], plain.offsets[:2])
    assert list(one.R[1]) == jr.to_words(kind, R0)
    two = mm.msm_multi(kind, s, x2, seg, seed=SEED)
    assert list(two.attempts) == [0, 1] and (two.bad_link == mm.LINK_NONE).all() and np.array_equal(two.results, one.results)
    assert list(two.offsets[2]) == list(two.R[1]) == jr.to_words(kind, mm.drawn(kind, SEED, 1, 1))


@pytest.mark.parametrize("kind", CURVES)
@pytest.mark.parametrize("link,step", [(0, 0), (2, 64), (1, 255)])
def test_crafted_x_hits_the_asked_link_and_step(kind, link, step):
    s, x, o = _inputs(kind, 4, seed=51 + kind)
    s[:, 3] &= np.uint64((1 << 62) - 1)
    R = jr.from_words(kind, o[0])
    T = mm.chain_one(kind, mm.products(kind, s[:link], x[:link]), None)[2]
    si = synth.words_to_int(s[link])
    cx = mm.crafted_x(kind, R, T, si, step)
    add, _ = jr._law(kind)
    assert jc.check_one(kind, si, cx, add(R, T)) == (0, step)
    assert jc.closed_form(kind, si, cx, add(R, T), ks=(step,)) == [step]
    x[link] = jr.to_words(kind, cx)
    got = mm.msm_multi(kind, s, x, [4], R=np.ascontiguousarray(o[:1]))
    assert (int(got.bad_link[0]), int(got.bad_step[0]), int(got.attempts[0])) == (link, step, 0)
    assert not got.offsets.any() and not got.outputs.any() and got.finite[0]


# ---- the argument checks of the C entry points ------------------------------------------------------------------------------
def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


N, M = 5, 3
OUT = ("results", "finite", "offsets", "outputs", "R_out", "attempts", "bad_link", "bad_step")


def _args(kind):
    """Valid arguments for 3 MSMs of 5 inputs; every output pre-filled with 7."""
    pt = jr.to_words(kind, GEN[kind])
    pw = PW[kind]
    return dict(scalars=np.ones((N, 4), np.uint64), x=np.array([pt] * N, np.uint64), seg_len=np.array([1, 3, 1], np.uintp),
                R=np.array([pt] * M, np.uint64), seed=np.array(SEED, np.uint64), results=np.full((M, pw), 7, np.uint64),
                finite=np.full(M, 7, np.uint8), offsets=np.full((N, pw), 7, np.uint64), outputs=np.full((N, pw), 7, np.uint64),
                R_out=np.full((M, pw), 7, np.uint64), attempts=np.full(M, 7, np.uint8), bad_link=np.full(M, 7, np.uint32),
                bad_step=np.full(M, 7, np.uint16))


def _chain(lib, kind, a, ctx=None, m=M, n=N, max_attempts=4, null=()):
    p = {k: (None if k in null else _vp(v)) for k, v in a.items()}
    return lib.bn254s_msm_multi_chain(ctx, kind, p["scalars"], p["x"], p["seg_len"], m, n, p["R"], p["seed"], max_attempts,
                                      *(p[k] for k in OUT))


def _full(lib, kind, a, per_proof, ctx=None, m=M, n=N, max_attempts=4, null=(), params=None, no_params=False, no_slots=False):
    p = {k: (None if k in null else _vp(v)) for k, v in a.items()}
    params = params or pk.default_params()
    slots = (C.c_void_p * 8)(*([1] * 8))
    rc = lib.bn254s_msm_multi(ctx, kind, None if no_params else C.byref(params), p["scalars"], p["x"], p["seg_len"], m, n, p["R"],
                              p["seed"], max_attempts, per_proof, *(p[k] for k in OUT), None if no_slots else slots)
    return rc, list(slots)


def _untouched(a):
    return all((a[k] == 7).all() for k in OUT)


def test_the_symbols_exist():
    lib = pk.load_library()
    assert hasattr(lib, "bn254s_msm_multi_chain") and hasattr(lib, "bn254s_msm_multi")
    assert lib.bn254s_abi_version() == 1 and pk.MSM_LINK_NONE == 0xFFFFFFFF


@pytest.mark.parametrize("kind", CURVES)
def test_argument_ladder_of_the_proven_call(kind):
    """Invalid arguments first, then per_proof, the context last."""
    lib = pk.load_library()
    a = _args(kind)
    untouched = (E_ARG, [1] * 8)
    rc, slots = _full(lib, kind, a, 16384)  # a valid shape: only the context is missing
    assert rc == E_ARG and slots[0] is None and slots[1] == 1
    rc, slots = _full(lib, kind, a, 2)
    assert rc == E_ARG and slots[:3] == [None] * 3 and slots[3] == 1
    rc, slots = _full(lib, kind, a, 16385)  # the shape answers before the context
    assert rc == E_UNSUP and slots[0] is None and slots[1:] == [1] * 7
    for name in ("scalars", "x", "seg_len", "results", "finite", "offsets", "outputs", "bad_link"):  # each required pointer alone
        assert _full(lib, kind, a, 16385, null=(name,)) == untouched, name
    assert _full(lib, kind, a, 16385, no_params=True) == untouched
    assert _full(lib, kind, a, 16385, no_slots=True)[0] == E_ARG
    for name in ("R_out", "attempts", "bad_step", "R", "seed"):  # these may be NULL, R and seed each alone
        assert _full(lib, kind, a, 16385, null=(name,))[0] == E_UNSUP, name
    assert _full(lib, kind, a, 16385, null=("R", "seed")) == untouched
    assert _full(lib, kind, a, 0) == untouched
    bad = pk.default_params()
    bad.struct_size += 4
    assert _full(lib, kind, a, 16385, params=bad) == untouched
    assert _full(lib, kind, a, 16385, m=0) == untouched
    assert _full(lib, kind, a, 16385, n=N + 1) == untouched and _full(lib, kind, a, 16385, n=N - 1) == untouched  # sum seg_len != n
    assert _full(lib, kind, a, 16385, m=2, n=4)[0] == E_UNSUP  # the first two MSMs alone
    assert _full(lib, kind, a, 16385, n=2**32 - 1) == untouched  # n >= UINT_MAX
    assert _full(lib, kind, dict(a, seg_len=np.array([2, 0, 3], np.uintp)), 16385) == untouched  # an empty MSM
    assert _full(lib, kind, dict(a, seg_len=np.array([2**64 - 1, 3, 3], np.uintp)), 16385) == untouched  # a sum that wraps
    # max_attempts and the seed are read for drawn points only
    for att in (0, -1, 9):
        assert _full(lib, kind, a, 16385, max_attempts=att, null=("R",)) == untouched, att
        assert _full(lib, kind, a, 16385, max_attempts=att)[0] == E_UNSUP, att
    assert _full(lib, kind, a, 16385, max_attempts=8, null=("R",))[0] == E_UNSUP
    for w in range(4):
        b = dict(a, seed=a["seed"].copy())
        b["seed"][w] = GL_P
        assert _full(lib, kind, b, 16385, null=("R",)) == untouched, w
        assert _full(lib, kind, b, 16385)[0] == E_UNSUP, w
    for c in range(PW[kind] // 4):  # a coordinate of x or of R that is p
        for name, row in (("x", 4), ("R", 2)):
            b = dict(a, **{name: a[name].copy()})
            b[name][row, 4 * c:4 * c + 4] = synth._to_words(P)
            assert _full(lib, kind, b, 16385) == untouched, (name, c)
    assert _untouched(a)


@pytest.mark.parametrize("kind", (-1, 2, 3))
def test_kinds_other_than_the_curves_are_invalid(kind):
    lib = pk.load_library()
    a = _args(0)
    assert _full(lib, kind, a, 16385) == (E_ARG, [1] * 8)
    assert _chain(lib, kind, a) == E_ARG and _untouched(a)


@pytest.mark.parametrize("kind", CURVES)
def test_chain_call_without_a_context(kind):
    lib = pk.load_library()
    a = _args(kind)
    assert _chain(lib, kind, a) == E_ARG
    assert _chain(lib, kind, a, null=("R_out", "attempts", "bad_step", "R")) == E_ARG
    assert _chain(lib, kind, a, null=("R", "seed")) == E_ARG and _chain(lib, kind, a, m=0) == E_ARG
    assert _untouched(a)


def test_wrappers_check_shapes():
    ctx = pk.Context.__new__(pk.Context)  # no device: the shape checks come before the library is entered
    ctx._h = None
    a = _args(0)
    with pytest.raises(ValueError, match="msm_multi: R"):
        ctx.msm_multi_chain(0, a["scalars"], a["x"], [1, 3, 1], R=a["R"][:2])
    with pytest.raises(ValueError, match="seed"):
        ctx.msm_multi(0, a["scalars"], a["x"], [1, 3, 1], seed=[1, 2, 3])


# ---- verify_msm_multi on oracle-made proofs -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_multi():
    """G1, seg_len [2, 1], per_proof = 2: two 2^16-row proofs made by the CPU oracle from the reference's offsets; MSM 0 fills
    proof 0 and the head of MSM 1 opens proof 1."""
    s, x, o = synth.g1_inputs(3, seed=61)
    seg, R = [2, 1], np.ascontiguousarray(o[:2])
    ref = mm.msm_multi(0, s, x, seg, R=R)
    assert (ref.bad_link == mm.LINK_NONE).all()
    orc = oracle_lib.load()
    proofs = []
    for lo, hi in ((0, 2), (2, 3)):
        words, outs, _, db = oracle_lib.g1_prove(orc, s[lo:hi], x[lo:hi], np.ascontiguousarray(ref.offsets[lo:hi]))
        proofs.append(SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1)))
    return s, x, seg, R, ref, proofs


def test_verify_accepts_oracle_proofs(oracle_multi):
    s, x, seg, R, ref, proofs = oracle_multi
    assert np.array_equal(np.concatenate([p.outputs for p in proofs]).reshape(3, 8), ref.outputs)
    pk.verify_msm_multi(0, s, x, seg, R, ref.results, ref.finite, ref.offsets, ref.outputs, proofs, 2)


def test_verify_names_what_is_broken(oracle_multi):
    s, x, seg, R, ref, proofs = oracle_multi

    def verify(R=R, results=ref.results, finite=ref.finite, offsets=ref.offsets, outputs=ref.outputs, proofs=proofs, seg=seg):
        pk.verify_msm_multi(0, s, x, seg, R, results, finite, offsets, outputs, proofs, 2)

    with pytest.raises(pk.VerifyError, match=r"offsets\[0\] != R_0 \(the head of msm 0\)"):  # R_0 and R_1 swapped
        verify(R=np.ascontiguousarray(R[::-1]))
    chained = ref.offsets.copy()
    chained[2] = ref.outputs[1]  # MSM 1 made to go on from MSM 0: a link across the head
    with pytest.raises(pk.VerifyError, match=r"offsets\[2\] != R_1 \(the head of msm 1\)"):
        verify(offsets=chained)
    inside = ref.offsets.copy()
    inside[1] = ref.offsets[0]
    with pytest.raises(pk.VerifyError, match=r"offsets\[1\] != outputs\[0\] \(link 0 -> 1 of msm 0\)"):
        verify(offsets=inside)
    wrong = ref.results.copy()
    wrong[1] = ref.results[0]
    with pytest.raises(pk.VerifyError, match=r"results\[1\] != outputs\[2\] - R_1"):
        verify(results=wrong)
    with pytest.raises(pk.VerifyError, match=r"finite\[0\] is 0, outputs\[1\] - R_0 is finite"):
        verify(finite=np.array([0, 1], np.uint8))
    # an MSM said to be finite whose last output is R itself (with a consistent chain, so that the flag is what is wrong)
    outs = ref.outputs.copy()
    outs[2] = R[1]
    with pytest.raises(pk.VerifyError, match="output 2 of proof 1"):
        verify(outputs=outs)
    fake = [proofs[0], SimpleNamespace(words=proofs[1].words, degree_bits=proofs[1].degree_bits, outputs=R[1].copy())]
    with pytest.raises(pk.VerifyError, match=r"finite\[1\] is 1, outputs\[2\] - R_1 is the point at infinity"):
        verify(outputs=outs, proofs=fake)
    with pytest.raises(pk.VerifyError, match="shapes"):
        verify(seg=[3, 1])
    with pytest.raises(pk.VerifyError, match="1 proofs for 3 jobs"):
        verify(proofs=proofs[:1])
    # consistent arrays, but a word of proof 1 changed: the verifier rejects that proof
    words = proofs[1].words.copy()
    words[0] ^= 1
    tampered = [proofs[0], SimpleNamespace(words=words, degree_bits=proofs[1].degree_bits, outputs=proofs[1].outputs)]
    with pytest.raises(pk.VerifyError, match="proof 1"):
        verify(proofs=tampered)
