"""Proof-free job outputs on the GPU (csrc/job_outputs.hip): the device front-end against the Python definition
(tools/job_outputs_ref.py) word for word on random jobs and on the crafted jobs of edge_jobs, against the outputs of the proofs
of the same jobs, the rejection of unreduced coordinates and of points off their curve before any output, the full call checked
with verify_job_outputs, and the front-end between the two halves of an open batch."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_outputs_ref as jr
from tools import synth

P, R = synth.P, synth.R_ORDER
KINDS = (0, 1, 2)
SIZES = [1, 63, 64, 65, 130]  # one lane, one short of a block, one block, one over, three blocks with a ragged tail
PW = jr.POINT_WORDS


@pytest.fixture(scope="module")
def jobs():
    """kind -> (scalars, x, offset, outputs, finite): 130 provable jobs (every smaller case is a prefix; on G2 every other x is
    off the subgroup with a scalar above r) and the outputs of the Python definition.  Computed once, read-only."""
    out = {}
    for kind in KINDS:
        s, x, o = jr.provable_jobs(kind, max(SIZES), seed=211 + kind)
        outs, fin = jr.outputs(kind, s, x, o)
        assert fin.all()
        for a in (s, x, o, outs, fin):
            if a is not None:
                a.setflags(write=False)
        out[kind] = (s, x, o, outs, fin)
    return out


def _head(a, n):
    return None if a is None else np.ascontiguousarray(a[:n])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_front_end_matches_python(gpu_ctx, jobs, kind, n):
    s, x, o, want, want_fin = (_head(a, n) for a in jobs[kind])
    outs, finite = gpu_ctx.job_outputs_batch(kind, s, x, o)
    assert outs.dtype == np.uint64 and outs.shape == (n, PW[kind]) and finite.dtype == np.uint8 and finite.shape == (n,)
    assert np.array_equal(finite, want_fin)
    assert outs.tobytes() == want.tobytes(), f"outputs differ at {np.nonzero(np.any(outs != want, axis=1))[0][:4]}"
    # every lane writes its own words and byte and no others
    raw, raw_fin = np.full((n + 2, PW[kind]), 7, np.uint64), np.full(n + 8, 7, np.uint8)
    assert gpu_ctx._lib.bn254s_job_outputs_batch(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(o), n, _vp(raw), _vp(raw_fin)) == 0
    assert np.array_equal(raw[:n], want) and (raw[n:] == 7).all()
    assert np.array_equal(raw_fin[:n], want_fin) and (raw_fin[n:] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_edge_jobs(gpu_ctx, kind):
    """The 64 jobs of edge_jobs in one wave: small scalars, multiples of r, offsets that double or cancel, twist points off the
    subgroup and of order 10069; zero words and finite = 0 where the output is the point at infinity."""
    s, x, o, classes = jr.edge_jobs(kind)
    want, want_fin = jr.outputs(kind, s, x, o)
    outs, finite = gpu_ctx.job_outputs_batch(kind, s, x, o)
    bad = [classes[i] for i in np.nonzero(np.any(outs != want, axis=1) | (finite != want_fin))[0]]
    assert not bad, bad
    if kind != 2:
        assert 0 < int((finite == 0).sum()) and not outs[finite == 0].any()
    for i in range(0, 64, 9):  # and alone in their launch
        one = gpu_ctx.job_outputs_batch(kind, *(_head(a[i:], 1) if a is not None else None for a in (s, x, o)))
        assert np.array_equal(one[0][0], want[i]) and one[1][0] == want_fin[i], classes[i]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_front_end_equals_the_proven_outputs(gpu_ctx, jobs, kind):
    s, x, o, want, _ = jobs[kind]
    if kind == 1:  # every other point is off the subgroup and multiplied by more than r: the reduced scalar gives another point
        sv, xv, ov = synth.words_to_int(s[1]), jr.from_words(1, x[1]), jr.from_words(1, o[1])
        assert sv >= R and not synth.g2_in_subgroup(xv) and jr.output_one(1, sv % R, xv, ov) != jr.output_one(1, sv, xv, ov)
    proofs = gpu_ctx.prove_batch(kind, s, x, o, per_proof=128)
    assert len(proofs) == 2 and proofs[1].outputs.size == 2 * PW[kind]
    proven = np.concatenate([pr.outputs.reshape(-1, PW[kind]) for pr in proofs])
    outs, finite = gpu_ctx.job_outputs_batch(kind, s, x, o)
    assert finite.all() and outs.tobytes() == proven.tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,case", [(k, "coordinate == p") for k in KINDS] +
                         [(k, c) for k in (0, 1) for c in ("x off the curve", "offset off the curve")])
def test_bad_input_is_rejected_before_any_output(gpu_ctx, jobs, kind, case):
    n = 72
    s, x, o = (None if a is None else a[:n].copy() for a in jobs[kind][:3])
    if case == "coordinate == p":
        x[5, -4:] = synth._to_words(P)  # the last coordinate of x_5
        names = ["x_5 "]
    elif case == "x off the curve":
        for i in (70, 3):  # the smallest index is the one reported
            x[i, PW[kind] // 2] += 1  # y (y.c0) + 1: below p still
            assert synth.words_to_int(x[i, PW[kind] // 2:PW[kind] // 2 + 4]) < P
        names = ["x_3 ", "not on the"]
    else:
        o[66, PW[kind] // 2] += 1
        names = ["offset_66 ", "not on the"]
    outs, finite = np.full((n, PW[kind]), 7, np.uint64), np.full(n, 7, np.uint8)
    lib = gpu_ctx._lib
    assert lib.bn254s_job_outputs_batch(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(o), n, _vp(outs), _vp(finite)) == -1
    msg = lib.bn254s_last_error(gpu_ctx._h).decode()
    assert all(t in msg for t in names), msg
    assert (outs == 7).all() and (finite == 7).all()
    slots = (C.c_void_p * 2)(1, 1)
    params = pk.default_params()
    assert lib.bn254s_job_outputs(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x), _vp(o), n, 64, _vp(outs), slots) == -1
    assert all(t in lib.bn254s_last_error(gpu_ctx._h).decode() for t in names) and list(slots) == [None, None]
    assert (outs == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: job_outputs: " + names[0]):
        gpu_ctx.job_outputs_batch(kind, s, x, o)
    # the same context answers a valid batch correctly afterwards
    good = gpu_ctx.job_outputs_batch(kind, *(_head(a, 8) for a in jobs[kind][:3]))
    assert np.array_equal(good[0], jobs[kind][3][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_full_call_two_proofs(gpu_ctx, jobs, kind):
    s, x, o, want, _ = jobs[kind]
    outs, proofs = gpu_ctx.job_outputs(kind, s, x, o, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 128 * PW[kind] and proofs[1].outputs.size == 2 * PW[kind]
    assert np.array_equal(outs, want)
    pk.verify_job_outputs(kind, s, x, o, outs, proofs, 128, ctx=gpu_ctx)
    flipped = outs.copy()
    flipped[129, 0] ^= 1
    with pytest.raises(pk.VerifyError, match="output 129 "):
        pk.verify_job_outputs(kind, s, x, o, flipped, proofs, 128, ctx=gpu_ctx)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.job_outputs(kind, s, x, o, per_proof=16385)
    if kind == 2:
        return  # every Fq-exp output is finite
    # one job whose output is the point at infinity (offset = -x, s = 1) among them: nothing is proven
    s2, x2, o2 = s.copy(), x.copy(), o.copy()
    s2[77] = [1, 0, 0, 0]
    neg = jr.g1_neg if kind == 0 else synth.g2_neg
    o2[77] = jr.to_words(kind, neg(jr.from_words(kind, x2[77])))
    buf = np.full((130, PW[kind]), 7, np.uint64)
    slots = (C.c_void_p * 2)(1, 1)
    params = pk.default_params()
    rc = gpu_ctx._lib.bn254s_job_outputs(gpu_ctx._h, kind, C.byref(params), _vp(s2), _vp(x2), _vp(o2), 130, 128, _vp(buf), slots)
    assert rc == -4 and "job 77 " in gpu_ctx._lib.bn254s_last_error(gpu_ctx._h).decode()
    assert list(slots) == [None, None] and (buf == 7).all()
    alone, fin = gpu_ctx.job_outputs_batch(kind, s2, x2, o2)
    assert fin[77] == 0 and int(fin.sum()) == 129 and not alone[77].any()


@pytest.mark.gpu
def test_front_end_inside_an_open_batch(gpu_ctx, jobs):
    """bn254s_job_outputs_batch between bn254s_prove_batch_begin and _end of a G1 batch of four proofs: it uses the context's own
    stream and its own pooled buffer, so both give what they give alone."""
    s, x, o, want, _ = jobs[0]
    s4, x4, o4 = (np.ascontiguousarray(np.tile(a, (4, 1))[:512]) for a in (s, x, o))
    alone = [pr.words.copy() for pr in gpu_ctx.prove_batch(0, s4, x4, o4, per_proof=128)]
    batch = gpu_ctx.prove_batch_begin(0, s4, x4, o4, per_proof=128)
    inside = [gpu_ctx.job_outputs_batch(k, *jobs[k][:3]) for k in KINDS]
    proofs = batch.end()
    assert len(proofs) == 4
    for pr, w in zip(proofs, alone):
        assert np.array_equal(pr.words, w)
    for k, (outs, fin) in zip(KINDS, inside):
        assert np.array_equal(outs, jobs[k][3]) and fin.all()
    proven = np.concatenate([pr.outputs.reshape(-1, 8) for pr in proofs])
    assert np.array_equal(proven, np.tile(want, (4, 1))[:512])
