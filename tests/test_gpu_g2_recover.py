"""G2 point recovery from x on the GPU (reference src/curves/g2.rs:42-54, src/fields/fq2.rs:209-241): the device front-end
(csrc/root_front.hip) against the Python reference (tools/synth.py g2_recover_from_x, ark's complex method: another algorithm than
the kernel's) word for word, the rejection of unreduced coordinates and of sign bytes above 1, the proven Legendre symbols checked
with verify_g2_recover, and the recovered points as the inputs of g2_msm."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import map_to_g2_ref, synth

P = synth.P
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail


def python_recover(xs, sgns):
    """(points [n,16], flags [n], fq_jobs [n,8]) from Python integers."""
    pts, flags, jobs = [], [], []
    for w, s in zip(xs, sgns):
        x = (synth.words_to_int(w[:4]), synth.words_to_int(w[4:]))
        rec = synth.g2_recover_from_x(x, int(s))
        flags.append(rec is not None)
        y = rec[1] if rec else (0, 0)
        pts.append([int(v) for v in w] + synth._to_words(y[0]) + synth._to_words(y[1]))
        jobs.append(synth._to_words((P - 1) // 2) + synth._to_words(map_to_g2_ref.f2_norm(synth.g2_rhs(x))))
    return np.array(pts, np.uint64), np.array(flags, np.uint8), np.array(jobs, np.uint64)


@pytest.fixture(scope="module")
def reference():
    """The 257 inputs of seed 31 (every smaller case is a prefix; what they cover: tests/test_g2_recover_cpu.py) and what Python
    makes of them."""
    xs, sgns = synth.g2_recover_inputs(max(SIZES), seed=31)
    pts, flags, jobs = python_recover(xs, sgns)
    for a in (xs, sgns, pts, flags, jobs):
        a.setflags(write=False)
    return xs, sgns, pts, flags, jobs


def _neg_words(w):
    return synth._to_words((-synth.words_to_int(w)) % P)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_python(gpu_ctx, reference, n):
    xs, sgns, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a[:n]) for a in reference)
    pts, flags, jobs = gpu_ctx.g2_recover_from_x_batch(xs, sgns)
    assert flags.dtype == np.uint8 and np.array_equal(flags, want_flags), f"flags differ at {np.nonzero(flags != want_flags)[0][:4]}"
    assert np.array_equal(jobs, want_jobs), f"jobs differ at {np.nonzero(np.any(jobs != want_jobs, axis=1))[0][:4]}"
    assert np.array_equal(pts, want_pts), f"points differ at {np.nonzero(np.any(pts != want_pts, axis=1))[0][:4]}"
    again = gpu_ctx.g2_recover_from_x_batch(xs, sgns)
    assert all(np.array_equal(a, b) for a, b in zip((pts, flags, jobs), again))


@pytest.mark.gpu
def test_default_and_opposite_signs(gpu_ctx, reference):
    xs = np.ascontiguousarray(reference[0][:64])
    pts0, flags0, jobs0 = gpu_ctx.g2_recover_from_x_batch(xs)  # sgns=None: all 0
    want = python_recover(xs, np.zeros(64, np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip((pts0, flags0, jobs0), want))
    pts1, flags1, jobs1 = gpu_ctx.g2_recover_from_x_batch(xs, np.ones(64, np.uint8))
    assert np.array_equal(flags1, flags0) and np.array_equal(jobs1, jobs0) and 0 < flags0.sum() < 64
    assert np.array_equal(pts1[:, :8], xs) and np.array_equal(pts0[:, :8], xs)
    for i in range(64):
        if flags0[i]:
            assert list(pts1[i, 8:12]) == _neg_words(pts0[i, 8:12]) and list(pts1[i, 12:]) == _neg_words(pts0[i, 12:]), i
            assert pts0[i, 8:].any()
        else:
            assert not pts0[i, 8:].any() and not pts1[i, 8:].any(), i


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c0 == p", "c1 == 2^256 - 1", "sgn == 2"])
def test_bad_input_is_rejected_before_any_output(gpu_ctx, reference, case):
    xs, sgns = reference[0][:8].copy(), reference[1][:8].copy()
    if case == "c0 == p":
        xs[5, :4] = synth._to_words(P)
    elif case == "c1 == 2^256 - 1":
        xs[5, 4:] = synth._to_words(2**256 - 1)
    else:
        sgns[5] = 2
    pts, flags, jobs = np.full((8, 16), 7, np.uint64), np.full(8, 7, np.uint8), np.full((8, 8), 7, np.uint64)
    lib = gpu_ctx._lib

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    rc = lib.bn254s_g2_recover_from_x_batch(gpu_ctx._h, vp(xs), vp(sgns), 8, vp(pts), vp(flags), vp(jobs))
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode()
    assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
    outs = (C.c_void_p * 4)(*([1] * 4))
    params = pk.default_params()
    rc = lib.bn254s_g2_recover_from_x(gpu_ctx._h, C.byref(params), vp(xs), vp(sgns), 8, 2, vp(pts), vp(flags), vp(jobs), outs)
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode() and list(outs) == [None] * 4
    assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: .*(x|sgn)_5 "):
        gpu_ctx.g2_recover_from_x_batch(xs, sgns)
    with pytest.raises(RuntimeError, match="failed with -1: .*(x|sgn)_5 "):
        gpu_ctx.g2_recover_from_x(xs, sgns, per_proof=8)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.g2_recover_from_x(reference[0][:8], reference[1][:8], per_proof=16385)
    # the context still recovers: p - 1 is the largest valid coordinate
    xs[5], sgns[5] = synth._to_words(P - 1) * 2, 1
    got = gpu_ctx.g2_recover_from_x_batch(xs, sgns)
    assert all(np.array_equal(a, b) for a, b in zip(got, python_recover(xs, sgns)))


@pytest.mark.gpu
def test_full_call_two_proofs(gpu_ctx, reference):
    n = 130
    xs, sgns, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a[:n]) for a in reference)
    pts, flags, jobs, proofs = gpu_ctx.g2_recover_from_x(xs, sgns, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 4 * 128 and proofs[1].outputs.size == 4 * 2
    assert np.array_equal(jobs, want_jobs) and np.array_equal(flags, want_flags) and np.array_equal(pts, want_pts)
    for pr in proofs:
        assert all(synth.words_to_int(o) in (1, P - 1) for o in pr.outputs.reshape(-1, 4))
    pk.verify_g2_recover(xs, sgns, pts, flags, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    pk.verify_g2_recover(xs, sgns, pts, flags, jobs, proofs, 128)               # the host verifier
    flipped = flags.copy()
    flipped[129] ^= 1
    with pytest.raises(pk.VerifyError, match="flag 129 "):
        pk.verify_g2_recover(xs, sgns, pts, flipped, jobs, proofs, 128)


@pytest.mark.gpu
def test_recovered_points_feed_g2_msm(gpu_ctx):
    s, x, o = synth.g2_inputs(3, seed=77)
    sgns = np.array([synth.f2_sgn(synth.g2_from_words(w)[1]) for w in x], np.uint8)
    pts, flags, _ = gpu_ctx.g2_recover_from_x_batch(np.ascontiguousarray(x[:, :8]), sgns)
    assert flags.all()  # the x of a curve point is always recoverable
    assert np.array_equal(pts, x)  # ... to the point itself, given the sign of its y
    R = np.ascontiguousarray(o[0])
    res, offs, proofs = gpu_ctx.g2_msm(s, pts, R, per_proof=128)
    want, msm = synth.g2_msm_chain(s, pts, R)
    assert np.array_equal(offs, synth.g2_points_to_words(want)) and np.array_equal(res, synth.g2_points_to_words([msm])[0])
    pk.verify_g2_msm(s, pts, R, res, offs, proofs, 128, ctx=gpu_ctx)
