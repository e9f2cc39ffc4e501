"""The point-sum check on the GPU (csrc/point_sum.hip, bn254s_point_sum_check_batch): the relations product + offset == output of
one scalar_mul_batch call at the lane and block boundaries; the crafted relations of tools/point_sum_ref.py, accepted and
rejected, at both ends of a wave and across a block boundary among valid ones, against the reference's codes; a relation's
independence of the call it is in; the range check of the host with a context to hold its text; and the front-end inside an open
batch."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_outputs_ref as jr
from tools import point_sum_ref as ps
from tools import synth

P = synth.P
CURVES = (0, 1)
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block of 64, one block, one over, a ragged tail past 256
PLACES = (0, 63, 64, 65, 129)  # where the crafted relations go in a call of 130
PW = jr.POINT_WORDS
SEED = (0x70736D, 0xFFFFFFFF00000000, 0, 5)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def relations(gpu_ctx):
    """kind -> (products, finite, offsets, outputs) of 257 provable jobs (on G2 every other x off the subgroup): 257 relations
    that hold.  One scalar_mul_batch per kind, read-only."""
    out = {}
    for kind in CURVES:
        s, x, _ = jr.provable_jobs(kind, 257, seed=911 + kind)
        prods, finite, offs, outs, _ = gpu_ctx.scalar_mul_batch(kind, s, x, SEED)
        assert finite.all()
        out[kind] = _frozen(prods, finite, offs, outs)
    return out


@pytest.fixture(scope="module")
def crafted():
    return {kind: ps.cases(kind) for kind in CURVES}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _cut(rel, n):
    return tuple(np.ascontiguousarray(a[:n]) for a in rel)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", CURVES)
def test_sizes(gpu_ctx, relations, kind, n):
    a, fin, b, c = _cut(relations[kind], n)
    codes = gpu_ctx.point_sum_check_batch(kind, a, fin, b, c)
    assert codes.shape == (n,) and codes.dtype == np.uint8 and not codes.any()
    if n == 65:  # the definition agrees that they hold (Python integers: a handful is enough, the device has said it of all)
        assert not ps.codes(kind, a[60:], fin[60:], b[60:], c[60:]).any()
    raw = np.full(n + 3, 7, np.uint8)  # every lane writes its own byte and no other
    assert gpu_ctx._lib.bn254s_point_sum_check_batch(gpu_ctx._h, kind, _vp(a), _vp(fin), _vp(b), _vp(c), n, _vp(raw)) == 0
    assert not raw[:n].any() and (raw[n:] == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_crafted_relations_among_valid_ones(gpu_ctx, relations, crafted, kind):
    ca, cfin, cb, cc, want, names = crafted[kind]
    k = len(names)
    seen = set()
    for lo in range(0, k, len(PLACES)):  # five crafted relations per call of 130, until each has had its turn
        a, fin, b, c = (v.copy() for v in _cut(relations[kind], 130))
        expect = np.zeros(130, np.uint8)
        for place, i in zip(PLACES, range(lo, min(k, lo + len(PLACES)))):
            a[place], fin[place], b[place], c[place], expect[place] = ca[i], cfin[i], cb[i], cc[i], want[i]
            seen.add(i)
        got = gpu_ctx.point_sum_check_batch(kind, a, fin, b, c)
        bad = np.nonzero(got != expect)[0]
        assert not bad.size, [(int(j), int(got[j]), int(expect[j])) for j in bad]
        if lo == 0:  # once: all 130 against the definition
            assert np.array_equal(got, ps.codes(kind, a, fin, b, c))
    assert seen == set(range(k))
    # all of them in one call, the other way round: a code depends on its relation alone
    got = gpu_ctx.point_sum_check_batch(kind, ca[::-1], cfin[::-1], cb[::-1], cc[::-1])
    assert np.array_equal(got, want[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_a_code_does_not_depend_on_its_call(gpu_ctx, relations, crafted, kind):
    a, fin, b, c = (v.copy() for v in relations[kind])
    ca, cfin, cb, cc, want, _ = crafted[kind]
    rows = np.arange(len(want)) * 3  # 0, 3, 6, ...: below 65 for the first 22
    a[rows], fin[rows], b[rows], c[rows] = ca, cfin, cb, cc
    large = gpu_ctx.point_sum_check_batch(kind, a, fin, b, c)
    small = gpu_ctx.point_sum_check_batch(kind, *_cut((a, fin, b, c), 65))
    assert np.array_equal(small, large[:65]) and small.any()
    assert np.array_equal(large[rows], want) and not np.delete(large, rows).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_a_coordinate_not_below_p_is_named(gpu_ctx, relations, kind):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    a, fin, b, c = (v.copy() for v in _cut(relations[kind], 70))
    raw = np.full(70, 7, np.uint8)
    call = lambda a_, b_, c_, kind_=kind, n=70: lib.bn254s_point_sum_check_batch(h, kind_, _vp(a_), _vp(fin), _vp(b_), _vp(c_), n, _vp(raw))
    last = PW[kind] // 4 - 1
    coord = ("x", "y") if kind == 0 else ("x.c0", "x.c1", "y.c0", "y.c1")
    for name, k in (("a", 0), ("b", 1), ("c", 2)):
        arrs = [a.copy(), b.copy(), c.copy()]
        arrs[k][66, 4 * last:] = synth._to_words(P)
        arrs[k][68, :4] = synth._to_words(P)  # the first such row is the one named
        assert call(*arrs) == -1
        assert lib.bn254s_last_error(h).decode() == f"point_sum_check: {name}_66 has {coord[last]} not below p"
    arrs = [a.copy(), b.copy(), c.copy()]
    arrs[2][1, :4] = arrs[1][2, :4] = arrs[0][3, :4] = synth._to_words(P)  # a before b before c, whatever the row
    assert call(*arrs) == -1 and lib.bn254s_last_error(h).decode().startswith("point_sum_check: a_3 has x")
    assert call(a, b, c, kind_=2) == -1 and call(a, b, c, n=0) == -1  # (no text: the shape answers first)
    assert (raw == 7).all()
    fin[3] = 0  # a row that is not a point is not range-checked: it is code 1
    assert call(arrs[0], b, c) == 0 and list(np.nonzero(raw)[0]) == [3] and raw[3] == 1


@pytest.mark.gpu
def test_front_end_inside_an_open_batch(gpu_ctx, relations, crafted):
    """bn254s_point_sum_check_batch between bn254s_prove_batch_begin and _end of a G1 batch of two proofs: it uses the context's
    own stream and its own pooled buffer, so both give what they give alone."""
    s, x, o = synth.g1_inputs(256, seed=0x70736D)
    alone = [pr.words.copy() for pr in gpu_ctx.prove_batch(0, s, x, o, per_proof=128)]
    calls = [crafted[k][:4] for k in CURVES] + [relations[k] for k in CURVES]
    idle = [gpu_ctx.point_sum_check_batch(k % 2, *v) for k, v in enumerate(calls)]
    batch = gpu_ctx.prove_batch_begin(0, s, x, o, per_proof=128)
    inside = [gpu_ctx.point_sum_check_batch(k % 2, *v) for k, v in enumerate(calls)]
    proofs = batch.end()
    assert len(proofs) == 2
    for pr, w in zip(proofs, alone):
        assert np.array_equal(pr.words, w)
    for u, v in zip(idle, inside):
        assert np.array_equal(u, v)
    for k in CURVES:
        assert np.array_equal(inside[k], crafted[k][4]) and not inside[2 + k].any()
