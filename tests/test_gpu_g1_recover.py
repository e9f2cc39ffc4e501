"""G1 point recovery from x on the GPU (reference src/curves/g1.rs:76-95, src/fields/recover.rs): the device front-end
(csrc/root_front.hip) against the Python reference (tools/synth.py g1_recover_from_x) word for word, the rejection of x >= p, the
proven Legendre symbols checked with verify_g1_recover, and the recovered points as the inputs of g1_msm."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import synth

P = synth.P
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail


def python_recover(xs):
    """(points [n,8], flags [n], fq_jobs [n,8]) from Python integers."""
    pts, flags, jobs = [], [], []
    for w in xs:
        x = synth.words_to_int(w)
        rec = synth.g1_recover_from_x(x)
        flags.append(rec is not None)
        pts.append(synth._to_words(x) + synth._to_words(rec[1] if rec else 0))
        jobs.append(synth._to_words((P - 1) // 2) + synth._to_words((x * x * x + 3) % P))
    return np.array(pts, np.uint64), np.array(flags, np.uint8), np.array(jobs, np.uint64)


@pytest.fixture(scope="module")
def reference():
    """The 257 inputs of seed 31 (every smaller case is a prefix) and what Python makes of them."""
    xs = synth.g1_recover_inputs(max(SIZES), seed=31)
    pts, flags, jobs = python_recover(xs)
    assert min(int(flags.sum()), len(flags) - int(flags.sum())) >= len(flags) // 4 + 1  # both flag values are well covered
    for a in (xs, pts, flags, jobs):
        a.setflags(write=False)
    return xs, pts, flags, jobs


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_python(gpu_ctx, reference, n):
    xs, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a[:n]) for a in reference)
    pts, flags, jobs = gpu_ctx.g1_recover_from_x_batch(xs)
    assert flags.dtype == np.uint8 and np.array_equal(flags, want_flags), f"flags differ at {np.nonzero(flags != want_flags)[0][:4]}"
    assert np.array_equal(jobs, want_jobs), f"jobs differ at {np.nonzero(np.any(jobs != want_jobs, axis=1))[0][:4]}"
    assert np.array_equal(pts, want_pts), f"points differ at {np.nonzero(np.any(pts != want_pts, axis=1))[0][:4]}"
    again = gpu_ctx.g1_recover_from_x_batch(xs)
    assert all(np.array_equal(a, b) for a, b in zip((pts, flags, jobs), again))


@pytest.mark.gpu
def test_unreduced_x_is_rejected_before_any_output(gpu_ctx, reference):
    import ctypes as C
    xs = reference[0][:8].copy()
    xs[5] = synth._to_words(P)
    pts, flags, jobs = np.full((8, 8), 7, np.uint64), np.full(8, 7, np.uint8), np.full((8, 8), 7, np.uint64)
    lib = gpu_ctx._lib

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    rc = lib.bn254s_g1_recover_from_x_batch(gpu_ctx._h, vp(xs), 8, vp(pts), vp(flags), vp(jobs))
    assert rc == -1 and "5" in lib.bn254s_last_error(gpu_ctx._h).decode()
    assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
    outs = (C.c_void_p * 4)(*([1] * 4))
    params = pk.default_params()
    rc = lib.bn254s_g1_recover_from_x(gpu_ctx._h, C.byref(params), vp(xs), 8, 2, vp(pts), vp(flags), vp(jobs), outs)
    assert rc == -1 and "5" in lib.bn254s_last_error(gpu_ctx._h).decode() and list(outs) == [None] * 4
    assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: .*x_5 "):
        gpu_ctx.g1_recover_from_x_batch(xs)
    xs[5] = synth._to_words(2**256 - 1)
    with pytest.raises(RuntimeError, match="failed with -1: .*x_5 "):
        gpu_ctx.g1_recover_from_x(xs, per_proof=8)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.g1_recover_from_x(reference[0][:8], per_proof=16385)
    # the context still recovers: p - 1 is the largest valid x
    xs[5] = synth._to_words(P - 1)
    got = gpu_ctx.g1_recover_from_x_batch(xs)
    assert all(np.array_equal(a, b) for a, b in zip(got, python_recover(xs)))


@pytest.mark.gpu
def test_full_call_two_proofs(gpu_ctx, reference):
    n = 130
    xs, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a[:n]) for a in reference)
    pts, flags, jobs, proofs = gpu_ctx.g1_recover_from_x(xs, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 4 * 128 and proofs[1].outputs.size == 4 * 2
    assert np.array_equal(jobs, want_jobs) and np.array_equal(flags, want_flags) and np.array_equal(pts, want_pts)
    for pr in proofs:
        assert all(synth.words_to_int(o) in (1, P - 1) for o in pr.outputs.reshape(-1, 4))
    pk.verify_g1_recover(xs, pts, flags, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    pk.verify_g1_recover(xs, pts, flags, jobs, proofs, 128)               # the host verifier
    flipped = flags.copy()
    flipped[129] ^= 1
    with pytest.raises(pk.VerifyError, match="flag 129 "):
        pk.verify_g1_recover(xs, pts, flipped, jobs, proofs, 128)


@pytest.mark.gpu
def test_recovered_points_feed_g1_msm(gpu_ctx):
    s, x, o = synth.g1_inputs(3, seed=77)
    pts, flags, _ = gpu_ctx.g1_recover_from_x_batch(np.ascontiguousarray(x[:, :4]))
    assert flags.all()  # the x of a curve point is always recoverable
    for got, orig in zip(pts, x):
        y, y0 = synth.words_to_int(got[4:]), synth.words_to_int(orig[4:])
        assert y % 2 == 0 and y in (y0, P - y0)
    R = np.ascontiguousarray(o[0])
    res, offs, proofs = gpu_ctx.g1_msm(s, pts, R, per_proof=128)
    want, msm = synth.g1_msm_chain(s, pts, R)
    assert np.array_equal(offs, synth.g1_points_to_words(want)) and np.array_equal(res, synth.g1_points_to_words([msm])[0])
    pk.verify_g1_msm(s, pts, R, res, offs, proofs, 128, ctx=gpu_ctx)
