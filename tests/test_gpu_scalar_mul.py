"""Scalar multiplication without an offset argument on the GPU (csrc/scalar_mul.hip): the drawn offsets against hash_to_g1 /
hash_to_g2 of the defined inputs, the outputs against job_outputs_batch and the products against the Python definition
(tools/scalar_mul_ref.py) at the wave and block boundaries; a job's independence of the call it is in; the edge scalars and the
three cases of the subtraction; crafted jobs that must be repaired with the offset of attempt 1, proven and verified; exhaustion
with one attempt; a point off its curve found on the device; and the front-end inside an open batch."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import scalar_mul_ref as sm
from tools import synth

P, R = synth.P, synth.R_ORDER
CURVES = (0, 1)
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block of 64, one block, one over, past a block of 256 with a ragged tail
PW = jr.POINT_WORDS
SEED = (0x73636D, 0xFFFFFFFF00000000, 0, 77)
REF_JOBS = 64  # jobs per kind that the pure-Python definition is run for
CRAFTED = {3: 0, 64: 1, 77: 63, 128: 64, 129: 255}  # index -> step, in a call of 130 jobs: both proofs and a block boundary


def _mul(kind):
    return jr.g1_mul_complete if kind == 0 else synth.g2_mul_unreduced


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def jobs():
    """kind -> (scalars, x): 257 jobs, 65 random ones (on G2 every other x off the subgroup with a scalar above r) repeated - the
    same job at another index has another offset.  Computed once, read-only."""
    out = {}
    for kind in CURVES:
        s, x, _ = jr.provable_jobs(kind, 65, seed=411 + kind)
        out[kind] = _frozen(*(np.ascontiguousarray(np.tile(a, (4, 1))[:257]) for a in (s, x)))
    return out


@pytest.fixture(scope="module")
def ref(jobs):
    """kind -> (products, finite, offsets, outputs, attempts) of jobs 0 .. 63 by the Python definition.  Computed once, read-only."""
    return {kind: _frozen(*sm.scalar_mul(kind, jobs[kind][0][:REF_JOBS], jobs[kind][1][:REF_JOBS], SEED)) for kind in CURVES}


@pytest.fixture(scope="module")
def crafted(jobs):
    """kind -> (scalars, x): 130 jobs, those of CRAFTED made to hit their step with the offset of attempt 0.  Read-only."""
    out = {}
    for kind in CURVES:
        s, x = (a[:130].copy() for a in jobs[kind])
        for i, k in CRAFTED.items():
            s[i, 3] &= np.uint64((1 << 62) - 1)  # below 2^254: the crafted x is in the subgroup, nothing needs the top bits
            x[i] = jr.to_words(kind, sm.crafted_x(kind, SEED, i, synth.words_to_int(s[i]), k))
        out[kind] = _frozen(s, x)
    return out


def _inputs(kind, n, attempts=None):
    """The hash inputs of jobs 0 .. n - 1 as the definition has them."""
    a = np.zeros((n, 8), np.uint64)
    a[:, :4] = np.array(SEED, np.uint64)
    a[:, 4] = np.arange(n, dtype=np.uint64)
    a[:, 6] = 0 if attempts is None else attempts
    a[:, 7] = 0x62736D00 + kind
    return a


def _hash(ctx, kind, inputs):
    return ctx.hash_to_g1_batch(inputs) if kind == 0 else ctx.hash_to_g2_batch(inputs)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(n, kind):
    """Output buffers pre-filled with 7."""
    return (np.full((n, PW[kind]), 7, np.uint64), np.full(n, 7, np.uint8), np.full((n, PW[kind]), 7, np.uint64),
            np.full((n, PW[kind]), 7, np.uint64), np.full(n, 7, np.uint8))


def _raw_batch(ctx, kind, s, x, n, max_attempts, bufs):
    seed = np.array(SEED, np.uint64)
    return ctx._lib.bn254s_scalar_mul_batch(ctx._h, kind, _vp(s), _vp(x), n, _vp(seed), max_attempts, *(_vp(b) for b in bufs))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", CURVES)
def test_sizes(gpu_ctx, jobs, ref, kind, n):
    s, x = (np.ascontiguousarray(a[:n]) for a in jobs[kind])
    prods, finite, offs, outs, att = gpu_ctx.scalar_mul_batch(kind, s, x, SEED)
    assert prods.shape == offs.shape == outs.shape == (n, PW[kind]) and finite.shape == att.shape == (n,)
    assert (att == 0).all() and (finite == 1).all()
    assert np.array_equal(offs, _hash(gpu_ctx, kind, _inputs(kind, n)))
    want_outs, want_fin = gpu_ctx.job_outputs_batch(kind, s, x, offs)
    assert np.array_equal(outs, want_outs) and want_fin.all()
    m = min(n, REF_JOBS)
    for got, want in zip((prods, finite, offs, outs, att), ref[kind]):
        assert np.array_equal(got[:m], want[:m])
    # every lane writes its own rows and no others; outputs_out and attempts_out may be NULL
    bufs = _raw(n + 2, kind)
    assert _raw_batch(gpu_ctx, kind, s, x, n, 4, bufs) == 0
    for b, want in zip(bufs, (prods, finite, offs, outs, att)):
        assert np.array_equal(b[:n], want) and (b[n:] == 7).all()
    bufs = _raw(n, kind)
    assert _raw_batch(gpu_ctx, kind, s, x, n, 1, bufs[:3] + (None, None)) == 0
    assert np.array_equal(bufs[0], prods) and np.array_equal(bufs[2], offs) and (bufs[3] == 7).all() and (bufs[4] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_a_job_does_not_depend_on_its_call(gpu_ctx, jobs, kind):
    s, x = jobs[kind]
    small = gpu_ctx.scalar_mul_batch(kind, np.ascontiguousarray(s[:65]), np.ascontiguousarray(x[:65]), SEED)
    large = gpu_ctx.scalar_mul_batch(kind, s, x, SEED)
    for a, b in zip(small, large):
        assert np.array_equal(a, b[:65])
    other = gpu_ctx.scalar_mul_batch(kind, np.ascontiguousarray(s[:65]), np.ascontiguousarray(x[:65]), (1,) + SEED[1:])
    assert np.array_equal(other[0], small[0]) and not (other[2] == small[2]).all(axis=1).any()  # the products stay, every offset moves


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_edge_scalars(gpu_ctx, jobs, kind):
    w = jr.WINDOW[kind]
    top = (1 << 256) - 1
    scalars = [0, 1, 2, R - 1, R, R + 1, top, jr.alternating(w, True), jr.alternating(w, False), top // R * R]
    xs = [jr.from_words(kind, jobs[kind][1][2 * j]) for j in range(len(scalars))]  # even indices: points of order r on both curves
    if kind == 1:
        off_subgroup = jr.from_words(1, jobs[1][1][1])
        assert not synth.g2_in_subgroup(off_subgroup)
        scalars += [R, 0]
        xs += [off_subgroup, off_subgroup]
        es, ex, _, classes = jr.edge_jobs(1)
        small = jr.from_words(1, ex[classes.index("order 10069, s = 10069")])
        assert synth.g2_mul_unreduced(jr.SMALL, small) is None
        scalars += [jr.SMALL, jr.SMALL * (1 << 200), jr.SMALL + 1]
        xs += [small] * 3
    # output == -offset: s x = -2 R0, the subtraction doubles; s is taken so that the trace can prove the job
    i_opp = len(scalars)
    s_opp = next(v for v in range(5, 50) if jc.check_one(kind, v, sm.opposite_x(kind, SEED, i_opp, v), sm.offset(kind, SEED, i_opp, 0))[0])
    scalars.append(s_opp)
    xs.append(sm.opposite_x(kind, SEED, i_opp, s_opp))
    n = len(scalars)
    s = np.array([synth._to_words(v) for v in scalars], np.uint64).reshape(n, 4)
    x = np.array([jr.to_words(kind, v) for v in xs], np.uint64).reshape(n, PW[kind])
    want = [_mul(kind)(scalars[i], xs[i]) for i in range(n)]
    prods, finite, offs, outs, att = gpu_ctx.scalar_mul_batch(kind, s, x, SEED)
    assert (att == 0).all()
    assert [int(f) for f in finite] == [int(v is not None) for v in want]
    assert np.array_equal(prods, np.array([jr.to_words(kind, v) for v in want], np.uint64).reshape(n, PW[kind]))
    infinite = [0, 4, 9] + ([11, 12, 13] if kind == 1 else [])
    assert [i for i in range(n) if not finite[i]] == infinite
    assert np.array_equal(outs[infinite], offs[infinite])  # s x = O: the output is the offset
    _, neg = jr._law(kind)
    assert list(outs[i_opp]) == jr.to_words(kind, neg(jr.from_words(kind, offs[i_opp]))) and finite[i_opp] == 1
    ref_all = sm.scalar_mul(kind, s, x, SEED)
    for got, exp in zip((prods, finite, offs, outs, att), ref_all):
        assert np.array_equal(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_repair_and_proofs(gpu_ctx, crafted, kind):
    s, x = crafted[kind]
    prods, finite, offs, outs, att, proofs = gpu_ctx.scalar_mul(kind, s, x, SEED, per_proof=128)
    want_att = np.zeros(130, np.uint8)
    want_att[list(CRAFTED)] = 1
    assert np.array_equal(att, want_att) and finite.all()
    assert np.array_equal(offs, _hash(gpu_ctx, kind, _inputs(kind, 130, want_att)))
    off0 = _hash(gpu_ctx, kind, _inputs(kind, 130))
    assert [i for i in range(130) if not np.array_equal(offs[i], off0[i])] == sorted(CRAFTED)
    prov, step = gpu_ctx.job_check_batch(kind, s, x, off0)
    assert {i: int(step[i]) for i in range(130) if not prov[i]} == CRAFTED
    assert np.array_equal(outs, gpu_ctx.job_outputs_batch(kind, s, x, offs)[0])
    for i in CRAFTED:
        si, xi = synth.words_to_int(s[i]), jr.from_words(kind, x[i])
        assert list(prods[i]) == jr.to_words(kind, _mul(kind)(si, xi))
        assert list(offs[i]) == jr.to_words(kind, sm.offset(kind, SEED, i, 1))
    assert len(proofs) == 2 and proofs[1].outputs.size == 2 * PW[kind]
    assert np.array_equal(np.concatenate([p.outputs for p in proofs]).reshape(130, PW[kind]), outs)
    for p, (lo, hi) in zip(proofs, ((0, 128), (128, 130))):
        gpu_ctx.verify(kind, p.words, p.degree_bits, *(np.ascontiguousarray(a[lo:hi]) for a in (s, x, offs)), p.outputs)
    with pytest.raises(RuntimeError, match="failed with -4"):  # without the repair the same jobs cannot be proven
        gpu_ctx.prove_batch(kind, s, x, off0, per_proof=128)
    batch = gpu_ctx.scalar_mul_batch(kind, s, x, SEED)
    for a, b in zip(batch, (prods, finite, offs, outs, att)):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_exhaustion(gpu_ctx, crafted, kind):
    s, x = crafted[kind]
    lib = gpu_ctx._lib
    bufs = _raw(130, kind)
    assert _raw_batch(gpu_ctx, kind, s, x, 130, 1, bufs) == -4
    msg = lib.bn254s_last_error(gpu_ctx._h).decode()
    assert msg == "scalar_mul_batch: job 3 cannot be proven: sum == -double at step 0 (row 0 of its frame) with the offset of attempt 0, the last of 1"
    assert all((b == 7).all() for b in bufs)
    slots = (C.c_void_p * 3)(1, 1, 1)
    params = pk.default_params()
    seed = np.array(SEED, np.uint64)
    rc = lib.bn254s_scalar_mul(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x), 130, 128, _vp(seed), 1, *(_vp(b) for b in bufs), slots)
    assert rc == -4 and list(slots) == [None, None, 1] and all((b == 7).all() for b in bufs)
    assert lib.bn254s_last_error(gpu_ctx._h).decode().startswith("scalar_mul: job 3 cannot be proven: sum == -double at step 0 (row 0 of")
    # a crafted x at another index than the one it was made for is an ordinary job: one attempt is enough for jobs 64 .. 129 alone
    tail = np.ascontiguousarray(s[64:]), np.ascontiguousarray(x[64:])
    assert (gpu_ctx.scalar_mul_batch(kind, *tail, SEED, max_attempts=1)[4] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_point_off_its_curve_is_found_on_the_device(gpu_ctx, jobs, kind):
    s, x = (a[:130].copy() for a in jobs[kind])
    for i in (128, 70):  # the smallest index is the one reported
        x[i, PW[kind] // 2] += 1  # y (y.c0) + 1: below p still
        assert synth.words_to_int(x[i, PW[kind] // 2:PW[kind] // 2 + 4]) < P
    bufs = _raw(130, kind)
    assert _raw_batch(gpu_ctx, kind, s, x, 130, 4, bufs) == -1
    msg = gpu_ctx._lib.bn254s_last_error(gpu_ctx._h).decode()
    assert msg.startswith("scalar_mul_batch: x_70 is not on the "), msg
    assert all((b == 7).all() for b in bufs)
    x[9, :4] = synth._to_words(P)  # a coordinate that is p is found on the host, before the device is asked
    assert _raw_batch(gpu_ctx, kind, s, x, 130, 4, bufs) == -1
    assert gpu_ctx._lib.bn254s_last_error(gpu_ctx._h).decode().startswith("scalar_mul_batch: x_9 has x")
    assert all((b == 7).all() for b in bufs)
    with pytest.raises(RuntimeError, match="failed with -1: scalar_mul: x_9 "):
        gpu_ctx.scalar_mul(kind, s, x, SEED)
    # the same context answers a valid call correctly afterwards
    good = gpu_ctx.scalar_mul_batch(kind, *(np.ascontiguousarray(a[:8]) for a in jobs[kind]), SEED)
    assert good[1].all() and (good[4] == 0).all()


@pytest.mark.gpu
def test_front_end_inside_an_open_batch(gpu_ctx, jobs, crafted):
    """bn254s_scalar_mul_batch between bn254s_prove_batch_begin and _end of a G1 batch of four proofs: it uses the context's own
    stream and its own pooled buffer, so both give what they give alone."""
    s, x = jobs[0]
    idle = [gpu_ctx.scalar_mul_batch(k, *crafted[k], SEED) for k in CURVES]
    s4, x4 = (np.ascontiguousarray(np.tile(a[:128], (4, 1))) for a in (s, x))
    o4 = np.ascontiguousarray(np.tile(idle[0][2][:128], (4, 1)))
    alone = [pr.words.copy() for pr in gpu_ctx.prove_batch(0, s4, x4, o4, per_proof=128)]
    batch = gpu_ctx.prove_batch_begin(0, s4, x4, o4, per_proof=128)
    inside = [gpu_ctx.scalar_mul_batch(k, *crafted[k], SEED) for k in CURVES]
    proofs = batch.end()
    assert len(proofs) == 4
    for pr, w in zip(proofs, alone):
        assert np.array_equal(pr.words, w)
    for a, b in zip(idle, inside):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert int(inside[1][4].sum()) == len(CRAFTED)
