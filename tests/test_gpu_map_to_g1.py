"""map_to_g1 / hash_to_g1 on the GPU (csrc/map_to_g1.hip): the device front-end against the Python definition
(tools/map_to_g1_ref.py) word for word, the rejection of u >= p, hash_to_fq on the device against the host function, the proven
Legendre symbols checked with verify_map_to_g1, and the mapped points as the inputs of g1_msm."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import map_to_g1_ref as m2g1
from tools import map_to_g2_ref as m2g
from tools import synth

P = synth.P
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail


@pytest.fixture(scope="module")
def reference():
    """The crafted inputs followed by seeded ones, 257 in all (every smaller case is a prefix), and what Python makes of them."""
    us = list(m2g1.CRAFTED) + m2g1.inputs(max(SIZES) - len(m2g1.CRAFTED))
    u = m2g1.to_words(us)
    pts, flags, jobs = m2g1.front_end(us)
    picks = [m2g1.branch(v) for v in us]
    assert min(picks.count(b) for b in (0, 1, 2)) >= 32  # every branch is well covered
    for a in (u, pts, flags, jobs):
        a.setflags(write=False)
    return u, pts, flags, jobs


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_python(gpu_ctx, reference, n):
    u, want_pts, want_flags, want_jobs = reference
    u, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a) for a in (u[:n], want_pts[:n], want_flags[:2 * n], want_jobs[:2 * n]))
    pts, flags, jobs = gpu_ctx.map_to_g1_batch(u)
    assert flags.dtype == np.uint8 and flags.shape == (2 * n,) and jobs.shape == (2 * n, 8) and pts.shape == (n, 8)
    assert np.array_equal(flags, want_flags), f"flags differ at {np.nonzero(flags != want_flags)[0][:4]}"
    assert np.array_equal(jobs, want_jobs), f"jobs differ at {np.nonzero(np.any(jobs != want_jobs, axis=1))[0][:4]}"
    assert np.array_equal(pts, want_pts), f"points differ at {np.nonzero(np.any(pts != want_pts, axis=1))[0][:4]}"
    again = gpu_ctx.map_to_g1_batch(u)
    assert all(np.array_equal(a, b) for a, b in zip((pts, flags, jobs), again))


@pytest.mark.gpu
def test_unreduced_u_is_rejected_before_any_output(gpu_ctx, reference):
    u = reference[0][:8].copy()
    lib = gpu_ctx._lib

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    for bad in (P, 2**256 - 1):
        u[5] = synth._to_words(bad)
        pts, flags, jobs = np.full((8, 8), 7, np.uint64), np.full(16, 7, np.uint8), np.full((16, 8), 7, np.uint64)
        rc = lib.bn254s_map_to_g1_batch(gpu_ctx._h, vp(u), 8, vp(pts), vp(flags), vp(jobs))
        assert rc == -1 and "u_5 " in lib.bn254s_last_error(gpu_ctx._h).decode()
        assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
        outs = (C.c_void_p * 8)(*([1] * 8))
        params = pk.default_params()
        rc = lib.bn254s_map_to_g1(gpu_ctx._h, C.byref(params), vp(u), 8, 2, vp(pts), vp(flags), vp(jobs), outs)
        assert rc == -1 and "u_5 " in lib.bn254s_last_error(gpu_ctx._h).decode() and list(outs) == [None] * 8
        assert (pts == 7).all() and (flags == 7).all() and (jobs == 7).all()
        with pytest.raises(RuntimeError, match="failed with -1: .*u_5 "):
            gpu_ctx.map_to_g1_batch(u)
        with pytest.raises(RuntimeError, match="failed with -1: .*u_5 "):
            gpu_ctx.map_to_g1(u, per_proof=8)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.map_to_g1(reference[0][:8], per_proof=16385)
    # the context still maps: p - 1 is the largest valid u
    u[5] = synth._to_words(P - 1)
    got = gpu_ctx.map_to_g1_batch(u)
    assert all(np.array_equal(a, b) for a, b in zip(got, m2g1.front_end([synth.words_to_int(w) for w in u])))


@pytest.mark.gpu
def test_hash_to_fq_and_hash_to_g1_on_device(gpu_ctx):
    from plonky2_bn254_amd import lib as L
    lib = L.load_library()
    rng = np.random.default_rng(78)
    n = 65
    for ln in (1, 8, 9):
        inp = rng.integers(0, m2g.GL_P, size=(n, ln), dtype=np.uint64)
        inp[0, :] = m2g.GL_P - 1
        got = gpu_ctx.hash_to_fq_batch(inp)
        want = np.zeros((n, 4), np.uint64)
        for i in range(n):
            row = np.ascontiguousarray(inp[i])
            assert lib.bn254s_hash_to_fq(L._ptr(row), ln, L._ptr(want[i])) == 0
        assert np.array_equal(got, want), f"len {ln}: rows {np.nonzero(np.any(got != want, axis=1))[0][:4]}"
        assert np.array_equal(got, gpu_ctx.hash_to_fq2_batch(inp)[:, :4])  # the first coordinate of hash_to_fq2
        assert np.array_equal(gpu_ctx.hash_to_g1_batch(inp), gpu_ctx.map_to_g1_batch(got)[0])
    assert synth.words_to_int(got[3]) == m2g1.hash_to_fq(inp[3].tolist())  # one row against the pure-Python mirror


@pytest.mark.gpu
def test_full_call_two_proofs(gpu_ctx, reference):
    n = 65
    u, want_pts, want_flags, want_jobs = reference
    u, want_pts, want_flags, want_jobs = (np.ascontiguousarray(a) for a in (u[:n], want_pts[:n], want_flags[:2 * n], want_jobs[:2 * n]))
    pts, flags, jobs, proofs = gpu_ctx.map_to_g1(u, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 4 * 128 and proofs[1].outputs.size == 4 * 2
    assert np.array_equal(jobs, want_jobs) and np.array_equal(flags, want_flags) and np.array_equal(pts, want_pts)
    for pr in proofs:
        assert all(synth.words_to_int(o) in (1, P - 1) for o in pr.outputs.reshape(-1, 4))
    pk.verify_map_to_g1(u, pts, flags, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    pk.verify_map_to_g1(u, pts, flags, jobs, proofs, 128)               # the host verifier
    flipped = flags.copy()
    flipped[129] ^= 1
    with pytest.raises(pk.VerifyError, match=r"flag 129 .*input 64\)"):
        pk.verify_map_to_g1(u, pts, flipped, jobs, proofs, 128)
    other = pts.copy()
    other[7, 4:] = synth._to_words(P - synth.words_to_int(pts[7, 4:]))  # on the curve, but of the other parity
    with pytest.raises(pk.VerifyError, match="input 7:"):
        pk.verify_map_to_g1(u, other, flags, jobs, proofs, 128)


@pytest.mark.gpu
def test_mapped_points_feed_g1_msm(gpu_ctx, reference):
    s, _, o = synth.g1_inputs(3, seed=77)
    pts, _, _ = gpu_ctx.map_to_g1_batch(np.ascontiguousarray(reference[0][3:6]))  # u = 2, 3, 1/2: one point per branch
    R = np.ascontiguousarray(o[0])
    res, offs, proofs = gpu_ctx.g1_msm(s, pts, R, per_proof=128)
    want, msm = synth.g1_msm_chain(s, pts, R)
    assert np.array_equal(offs, synth.g1_points_to_words(want)) and np.array_equal(res, synth.g1_points_to_words([msm])[0])
    pk.verify_g1_msm(s, pts, R, res, offs, proofs, 128, ctx=gpu_ctx)
