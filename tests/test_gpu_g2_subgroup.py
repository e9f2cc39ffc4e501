"""G2 subgroup check on the GPU: the device front-end (csrc/g2_subgroup.hip, the endomorphism criterion) against the Python
definition [r]P = O (tools/synth.py g2_in_subgroup) byte for byte, points of every small order of the cofactor, the rejection of
unreduced coordinates and of points off the curve before any output, the proven jobs (r, P_i, R_i) checked with
verify_g2_subgroup, and the chain recover -> subgroup check -> g2_msm."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import synth

P, R = synth.P, synth.R_ORDER
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail


@pytest.fixture(scope="module")
def reference():
    """The 257 inputs of seed 41 (every smaller case is a prefix; what they cover: tests/test_g2_subgroup_cpu.py), their expected
    flags and the flags of the Python definition."""
    pts, flags = synth.g2_subgroup_inputs(max(SIZES), seed=41)
    definition = np.array([synth.g2_in_subgroup(synth.g2_from_words(w)) for w in pts], np.uint8)
    assert np.array_equal(definition, flags)
    for a in (pts, definition):
        a.setflags(write=False)
    return pts, definition


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_python(gpu_ctx, reference, n):
    pts, want = (np.ascontiguousarray(a[:n]) for a in reference)
    flags = gpu_ctx.g2_subgroup_check_batch(pts)
    assert flags.dtype == np.uint8 and flags.shape == (n,)
    assert np.array_equal(flags, want), f"flags differ at {np.nonzero(flags != want)[0][:4]}"
    assert gpu_ctx.g2_subgroup_check_batch(pts).tobytes() == flags.tobytes()
    # every lane writes its byte and no other (the wrapper's buffer starts as zeros, the flag of a non-member)
    raw = np.full(n + 8, 7, np.uint8)
    assert gpu_ctx._lib.bn254s_g2_subgroup_check_batch(gpu_ctx._h, _vp(pts), n, _vp(raw)) == 0
    assert np.array_equal(raw[:n], want) and (raw[n:] == 7).all()


@pytest.mark.gpu
def test_small_order_and_edge_points(gpu_ctx, reference):
    """One point of each prime order of the cofactor, one of order 10069 * 5864401, a member plus a point of order 10069, and
    G2_GEN, -G2_GEN, [r - 1]G2_GEN: every one alone in its launch, and all together."""
    pts_all, _ = reference
    _, _, classes = synth.g2_subgroup_inputs(32, seed=41, with_classes=True)
    prime = [next(i for i, (c, d) in enumerate(classes) if c == 3 and d == f) for f in synth.G2_COFACTOR_PRIMES]
    pick = prime + [classes.index((4, 10069 * 5864401)), classes.index((5, 10069))]
    gen = synth.G2_GEN
    edge = synth.g2_points_to_words([gen, synth.g2_neg(gen), synth.g2_mul(R - 1, gen)])
    assert np.array_equal(edge[1], edge[2])  # [r - 1]G = -G
    pts = np.ascontiguousarray(np.concatenate([pts_all[pick], edge]))
    want = [0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert [synth.g2_in_subgroup(synth.g2_from_words(w)) for w in pts] == [bool(v) for v in want]
    assert gpu_ctx.g2_subgroup_check_batch(pts).tolist() == want
    for i in range(9):
        assert gpu_ctx.g2_subgroup_check_batch(np.ascontiguousarray(pts[i:i + 1])).tolist() == [want[i]], i


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["x.c0 == p", "y.c1 == 2^256 - 1", "off the curve"])
def test_bad_input_is_rejected_before_any_output(gpu_ctx, reference, case):
    pts = reference[0][:8].copy()
    offs = synth.g2_inputs(8, seed=43)[2]
    if case == "x.c0 == p":
        pts[5, :4] = synth._to_words(P)
    elif case == "y.c1 == 2^256 - 1":
        pts[5, 12:] = synth._to_words(2**256 - 1)
    else:
        pts[5, 8] += 1  # y.c0 + 1: below p still, off the curve
        assert synth.words_to_int(pts[5, 8:12]) < P and not synth.g2_on_curve(synth.g2_from_words(pts[5]))
    flags, jobs = np.full(8, 7, np.uint8), np.full((8, 20), 7, np.uint64)
    lib = gpu_ctx._lib
    rc = lib.bn254s_g2_subgroup_check_batch(gpu_ctx._h, _vp(pts), 8, _vp(flags))
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode()
    assert (flags == 7).all()
    outs = (C.c_void_p * 4)(*([1] * 4))
    params = pk.default_params()
    rc = lib.bn254s_g2_subgroup_check(gpu_ctx._h, C.byref(params), _vp(pts), _vp(offs), 8, 2, _vp(flags), _vp(jobs), outs)
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode() and list(outs) == [None] * 4
    assert (flags == 7).all() and (jobs == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: .*point_5 "):
        gpu_ctx.g2_subgroup_check_batch(pts)
    with pytest.raises(RuntimeError, match="failed with -1: .*point_5 "):
        gpu_ctx.g2_subgroup_check(pts, offs, per_proof=8)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.g2_subgroup_check(reference[0][:8], offs, per_proof=16385)
    # the same context checks a valid batch correctly afterwards
    good = np.ascontiguousarray(reference[0][:8])
    assert np.array_equal(gpu_ctx.g2_subgroup_check_batch(good), reference[1][:8])


@pytest.mark.gpu
def test_full_call_two_proofs(gpu_ctx, reference):
    n = 130
    pts, want = (np.ascontiguousarray(a[:n]) for a in reference)
    offs = synth.g2_inputs(n, seed=47)[2]
    flags, jobs, proofs = gpu_ctx.g2_subgroup_check(pts, offs, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 16 * 128 and proofs[1].outputs.size == 16 * 2
    assert np.array_equal(flags, want)
    r_words = np.array(synth._to_words(R), np.uint64)
    assert np.array_equal(jobs[:, :4], np.tile(r_words, (n, 1))) and np.array_equal(jobs[:, 4:], pts)
    outs = np.concatenate([pr.outputs.reshape(-1, 16) for pr in proofs])
    for i in range(n):
        if want[i]:
            assert np.array_equal(outs[i], offs[i]), i
        else:  # R_i + [r]P_i over the unreduced 254-bit r, as the trace walks it
            rp = synth.g2_mul_unreduced(R, synth.g2_from_words(pts[i]))
            assert np.array_equal(outs[i], synth.g2_points_to_words([synth.g2_add(synth.g2_from_words(offs[i]), rp)])[0]), i
            assert not np.array_equal(outs[i], offs[i]), i
    pk.verify_g2_subgroup(pts, offs, flags, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    pk.verify_g2_subgroup(pts, offs, flags, jobs, proofs, 128)               # the host verifier
    flipped = flags.copy()
    flipped[129] ^= 1
    with pytest.raises(pk.VerifyError, match="flag 129 "):
        pk.verify_g2_subgroup(pts, offs, flipped, jobs, proofs, 128)


@pytest.mark.gpu
def test_recover_check_msm_chain(gpu_ctx, reference):
    """recover -> subgroup check -> g2_msm: the x of three members and of two random twist points."""
    s, x, o = synth.g2_inputs(3, seed=77)
    rnd = np.ascontiguousarray(reference[0][[1, 8]])  # class 1 of the inputs: random twist points
    full = np.concatenate([x, rnd])
    sgns = np.array([synth.f2_sgn(synth.g2_from_words(w)[1]) for w in full], np.uint8)
    pts, rec, _ = gpu_ctx.g2_recover_from_x_batch(np.ascontiguousarray(full[:, :8]), sgns)
    assert rec.all() and np.array_equal(pts, full)  # the x of a curve point recovers the point, given the sign of its y
    flags = gpu_ctx.g2_subgroup_check_batch(pts)
    assert flags.tolist() == [1, 1, 1, 0, 0]
    members = np.ascontiguousarray(pts[flags == 1])
    R0 = np.ascontiguousarray(o[0])
    res, offs, proofs = gpu_ctx.g2_msm(s, members, R0, per_proof=128)
    want, msm = synth.g2_msm_chain(s, members, R0)
    assert np.array_equal(offs, synth.g2_points_to_words(want)) and np.array_equal(res, synth.g2_points_to_words([msm])[0])
    pk.verify_g2_msm(s, members, R0, res, offs, proofs, 128, ctx=gpu_ctx)
