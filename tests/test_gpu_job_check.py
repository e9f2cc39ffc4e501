"""The job check on the GPU (csrc/job_check.hip): the device front-end on random jobs, which are all provable, and on the crafted
jobs of edge_jobs against the Python definition (tools/job_check_ref.py); the definition against the prover itself - the
provable crafted jobs in one proof, unprovable ones refused with -4; the rejection of unreduced coordinates and of points off
their curve before any output; prove_batch_checked with one bad job among 130 and on 130 good ones; a link of an msm chain that
cannot be proven although every offset is finite; and the front-end between the two halves of an open batch."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import synth

P = synth.P
KINDS = (0, 1, 2)
CURVES = (0, 1)
SIZES = [1, 63, 64, 65, 130]  # one lane, one short of a block, one block, one over, three blocks with a ragged tail
PW = jr.POINT_WORDS
NONE = pk.JOB_STEP_NONE


@pytest.fixture(scope="module")
def jobs():
    """kind -> (scalars, x, offset): 130 random jobs (every smaller case is a prefix; on G2 every other x is off the subgroup
    with a scalar above r).  Computed once, read-only."""
    out = {}
    for kind in KINDS:
        s, x, o = jr.provable_jobs(kind, max(SIZES), seed=311 + kind)
        for a in (s, x, o):
            if a is not None:
                a.setflags(write=False)
        out[kind] = (s, x, o)
    return out


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


def _head(a, n):
    return None if a is None else np.ascontiguousarray(a[:n])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _hit_at(kind, s, x, k):
    """The offset words with which step k of the job (s, x) hits."""
    _, neg = jr._law(kind)
    return jr.to_words(kind, neg(jc._mul(kind)(jc.multiplier(synth.words_to_int(s), k), jr.from_words(kind, x))))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_random_jobs_are_provable(gpu_ctx, jobs, kind, n):
    s, x, o = (_head(a, n) for a in jobs[kind])
    prov, step = gpu_ctx.job_check_batch(kind, s, x, o)
    assert prov.dtype == np.uint8 and prov.shape == (n,) and step.dtype == np.uint16 and step.shape == (n,)
    assert (prov == 1).all() and (step == NONE).all()
    # every lane writes its own byte and half-word and no others; step_out may be NULL
    raw, raw_step = np.full(n + 8, 7, np.uint8), np.full(n + 8, 7, np.uint16)
    lib = gpu_ctx._lib
    assert lib.bn254s_job_check_batch(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(o), n, _vp(raw), _vp(raw_step)) == 0
    assert (raw[:n] == 1).all() and (raw[n:] == 7).all() and (raw_step[:n] == NONE).all() and (raw_step[n:] == 7).all()
    raw[:] = 7
    assert lib.bn254s_job_check_batch(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(o), n, _vp(raw), None) == 0
    assert (raw[:n] == 1).all() and (raw[n:] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_edge_jobs(gpu_ctx, edge, kind):
    """The 64 jobs of edge_jobs in one wave: hits and doublings at the word boundaries of the scalar, s = 0, 2^256 - 1 and around
    r, twist points off the subgroup and of order 10069, beside random jobs."""
    s, x, o, classes, expected = edge[kind]
    want_prov, want_step = jc.check(kind, s, x, o)
    assert [(int(a), int(b)) for a, b in zip(want_prov, want_step)] == expected
    prov, step = gpu_ctx.job_check_batch(kind, s, x, o)
    bad = [(classes[i], int(prov[i]), int(step[i]), expected[i]) for i in np.nonzero((prov != want_prov) | (step != want_step))[0]]
    assert not bad, bad
    assert 0 < int((prov == 0).sum()) < 64


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_the_definition_is_the_provers(gpu_ctx, edge, kind):
    s, x, o, classes, expected = edge[kind]
    ok = [i for i in range(64) if classes[i] != "random" and expected[i][0]]
    s_, x_, o_ = (np.ascontiguousarray(a[ok]) for a in (s, x, o))
    assert gpu_ctx.job_check_batch(kind, s_, x_, o_)[0].all()
    proofs = gpu_ctx.prove_batch(kind, s_, x_, o_, per_proof=128)
    assert len(proofs) == 1 and proofs[0].degree_bits == 16
    want = jr.outputs(kind, s_, x_, o_)[0]
    assert np.array_equal(proofs[0].outputs.reshape(-1, PW[kind]), want)
    gpu_ctx.verify(kind, proofs[0].words, 16, s_, x_, o_, proofs[0].outputs)
    tail = ("s = r, hit at step 252", "s = 2^256 - 1, hit at step 255") if kind == 0 else \
        ("order 10069, hit at step 20", "off the subgroup, s >= 2^255, hit at step 254")
    for c in ("offset = -x, s = 2", "offset = -x, s odd", "hit at step 64", "s = 0, offset = -[2^7]x") + tail:
        i = classes.index(c)
        one = [np.ascontiguousarray(a[i:i + 1]) for a in (s, x, o)]
        assert gpu_ctx.job_check_batch(kind, *one)[0][0] == 0, c
        with pytest.raises(RuntimeError, match="failed with -4"):
            gpu_ctx.prove_batch(kind, *one)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,case", [(k, "coordinate == p") for k in KINDS] +
                         [(k, c) for k in CURVES for c in ("x off the curve", "offset off the curve")])
def test_bad_input_is_rejected_before_any_output(gpu_ctx, jobs, kind, case):
    n = 72
    s, x, o = (None if a is None else a[:n].copy() for a in jobs[kind])
    if case == "coordinate == p":
        x[5, -4:] = synth._to_words(P)  # the last coordinate of x_5
        names = ["x_5 ", "not below p"]
    elif case == "x off the curve":
        for i in (70, 3):  # the smallest index is the one reported
            x[i, PW[kind] // 2] += 1  # y (y.c0) + 1: below p still
            assert synth.words_to_int(x[i, PW[kind] // 2:PW[kind] // 2 + 4]) < P
        names = ["x_3 ", "not on the"]
    else:
        o[66, PW[kind] // 2] += 1
        names = ["offset_66 ", "not on the"]
    prov, step = np.full(n, 7, np.uint8), np.full(n, 7, np.uint16)
    lib = gpu_ctx._lib
    assert lib.bn254s_job_check_batch(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(o), n, _vp(prov), _vp(step)) == -1
    msg = lib.bn254s_last_error(gpu_ctx._h).decode()
    assert msg.startswith("job_check: ") and all(t in msg for t in names), msg
    assert (prov == 7).all() and (step == 7).all()
    slots = (C.c_void_p * 2)(1, 1)
    params = pk.default_params()
    assert lib.bn254s_prove_batch_checked(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x), _vp(o), n, 64, _vp(prov), _vp(step),
                                          slots) == -1
    assert all(t in lib.bn254s_last_error(gpu_ctx._h).decode() for t in names) and list(slots) == [None, None]
    assert (prov == 7).all() and (step == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: job_check: " + names[0]):
        gpu_ctx.job_check_batch(kind, s, x, o)
    # the same context answers a valid batch correctly afterwards
    assert gpu_ctx.job_check_batch(kind, *(_head(a, 8) for a in jobs[kind]))[0].all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_checked_batch_names_the_bad_job(gpu_ctx, jobs, kind):
    s, x, o = (a.copy() for a in jobs[kind])
    o[77] = _hit_at(kind, s[77], x[77], 64)
    prov, step = np.full(130, 7, np.uint8), np.full(130, 7, np.uint16)
    slots = (C.c_void_p * 2)(1, 1)
    params = pk.default_params()
    lib = gpu_ctx._lib
    rc = lib.bn254s_prove_batch_checked(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x), _vp(o), 130, 128, _vp(prov), _vp(step), slots)
    assert rc == -4
    assert lib.bn254s_last_error(gpu_ctx._h).decode() == \
        "prove_batch_checked: job 77 cannot be proven: sum == -double at step 64 (row 128 of its frame)"
    assert list(slots) == [None, None]
    assert list(np.nonzero(prov == 0)[0]) == [77] and int(prov.sum()) == 129
    assert step[77] == 64 and (np.delete(step, 77) == NONE).all()
    with pytest.raises(pk.UnprovableJobs, match="failed with -4: prove_batch_checked: job 77 .* step 64 ") as e:
        gpu_ctx.prove_batch_checked(kind, s, x, o, per_proof=128)
    assert np.array_equal(e.value.provable, prov) and np.array_equal(e.value.step, step)
    # both outputs may be NULL: the message alone is the answer then
    assert lib.bn254s_prove_batch_checked(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x), _vp(o), 130, 128, None, None, slots) == -4
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.prove_batch_checked(kind, s, x, o, per_proof=16385)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_checked_batch_gives_the_proofs_of_prove_batch(gpu_ctx, jobs, kind):
    s, x, o = jobs[kind]
    proofs, prov, step = gpu_ctx.prove_batch_checked(kind, s, x, o, per_proof=128)
    assert prov.all() and (step == NONE).all()
    plain = gpu_ctx.prove_batch(kind, s, x, o, per_proof=128)
    assert len(proofs) == len(plain) == 2 and proofs[1].outputs.size == 2 * PW[kind]
    for a, b in zip(proofs, plain):
        assert np.array_equal(a.words, b.words) and np.array_equal(a.outputs, b.outputs)


@pytest.mark.gpu
def test_msm_link_with_finite_offsets_that_cannot_be_proven(gpu_ctx, jobs):
    """x_1 = -offset_1 with s_1 = 2: offset_2 = -offset_1 is finite, the chain succeeds, and link 1 hits at step 0."""
    s, x, o = (a[:4].copy() for a in jobs[0])
    R = o[0]
    off1 = jr.output_one(0, synth.words_to_int(s[0]), jr.from_words(0, x[0]), jr.from_words(0, R))
    x[1] = jr.to_words(0, jr.g1_neg(off1))
    s[1] = [2, 0, 0, 0]
    offsets, _ = gpu_ctx.g1_msm_chain(s, x, R)
    assert offsets.shape == (5, 8) and offsets.any(axis=1).all()
    assert np.array_equal(offsets[1], jr.to_words(0, off1)) and np.array_equal(offsets[2], x[1])
    prov, step = gpu_ctx.job_check_batch(0, s, x, np.ascontiguousarray(offsets[:-1]))
    assert list(prov) == [1, 0, 1, 1] and list(step) == [NONE, 0, NONE, NONE]
    with pytest.raises(RuntimeError, match="failed with -4"):
        gpu_ctx.g1_msm(s, x, R)


@pytest.mark.gpu
def test_front_end_inside_an_open_batch(gpu_ctx, jobs, edge):
    """bn254s_job_check_batch between bn254s_prove_batch_begin and _end of a G1 batch of four proofs: it uses the context's own
    stream and its own pooled buffer, so both give what they give alone."""
    s, x, o = jobs[0]
    s4, x4, o4 = (np.ascontiguousarray(np.tile(a, (4, 1))[:512]) for a in (s, x, o))
    alone = [pr.words.copy() for pr in gpu_ctx.prove_batch(0, s4, x4, o4, per_proof=128)]
    batch = gpu_ctx.prove_batch_begin(0, s4, x4, o4, per_proof=128)
    inside = [gpu_ctx.job_check_batch(k, *edge[k][:3]) for k in CURVES] + [gpu_ctx.job_check_batch(2, *jobs[2])]
    proofs = batch.end()
    assert len(proofs) == 4
    for pr, w in zip(proofs, alone):
        assert np.array_equal(pr.words, w)
    for k in CURVES:
        assert [(int(a), int(b)) for a, b in zip(*inside[k])] == edge[k][4]
    assert inside[2][0].all() and (inside[2][1] == NONE).all()
