"""g1_msm on the GPU (reference src/utils/g1_msm.rs:22-36): the device chain (csrc/msm.hip) against the Python fold
(tools/synth.py g1_msm_chain), the chained proofs checked with verify_g1_msm, and the error cases."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import synth

P, R_ORD, G = synth.P, synth.R_ORDER, synth.G1_GEN


def words(pts):
    return synth.g1_points_to_words(pts)


def swords(ss):
    return np.array([synth._to_words(s) for s in ss], np.uint64).reshape(-1, 4)


def pt(w):
    return (synth.words_to_int(w[:4]), synth.words_to_int(w[4:]))


def neg(p):
    return (p[0], (-p[1]) % P)


def check_chain(ctx, s, x, R):
    offs, res = ctx.g1_msm_chain(s, x, R)
    want, msm = synth.g1_msm_chain(s, x, R)
    assert all(p is not None for p in want)
    assert np.array_equal(offs, words(want)), f"first differing offset: {np.nonzero(np.any(offs != words(want), axis=1))[0][:4]}"
    assert np.array_equal(res, words([msm])[0])
    return offs, res


@pytest.fixture(scope="module")
def jobs():
    return synth.g1_inputs(1000, seed=0x6D736D)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 300, 1000])
def test_chain_matches_python(gpu_ctx, jobs, n):
    s, x, o = jobs
    check_chain(gpu_ctx, np.ascontiguousarray(s[:n]), np.ascontiguousarray(x[:n]), np.ascontiguousarray(o[n % 1000]))


@pytest.mark.gpu
def test_chain_special_cases(gpu_ctx, jobs):
    s0, x0, o = jobs
    R = pt(o[0])
    xs = [pt(x0[i]) for i in range(6)]
    a = synth.words_to_int(s0[0]) % R_ORD
    ss = [0, R_ORD, R_ORD + 5, 2**256 - 1, a, R_ORD - a, 7, 7, synth.words_to_int(s0[1]), 1, 2, R_ORD]
    xx = [xs[0], xs[1], xs[2], xs[2], xs[3], xs[3], xs[4], xs[4], xs[5], xs[0], xs[0], xs[1]]
    # s = 0 and s = r: no change; unreduced s; repeated x; s x, (r - s) x: the partial sum returns to offset_4;
    # two adjacent equal inputs (7 x_4 twice): the first scan step adds a point to itself
    s, x = swords(ss), words(xx)
    offs, _ = check_chain(gpu_ctx, s, x, words([R])[0])
    assert np.array_equal(offs[1], offs[0]) and np.array_equal(offs[2], offs[0]) and np.array_equal(offs[6], offs[4])
    # x_1 = offset_1, s_1 = 1: the sequential fold doubles offset_1
    off1 = synth.g1_scalar_mul_offset(synth.words_to_int(s0[2]), pt(x0[2]), R)
    s2, x2 = swords([synth.words_to_int(s0[2]), 1, 3]), words([pt(x0[2]), off1, pt(x0[3])])
    offs2, _ = check_chain(gpu_ctx, s2, x2, words([R])[0])
    assert pt(offs2[2]) == synth.g1_add(off1, off1)
    # the same configurations across a block boundary of the scan (inputs 254 .. 257 of 300)
    s3, x3, _ = synth.g1_inputs(300, seed=99)
    s3[254], x3[254] = s3[253], x3[253]
    s3[255] = synth._to_words(R_ORD - synth.words_to_int(s3[254]) % R_ORD)
    x3[255] = x3[254]
    check_chain(gpu_ctx, s3, x3, words([R])[0])


def arithmetic_inputs(n, a, d, seed):
    """x_i = (a + i d) G by one affine addition per input, random 256-bit scalars, and the expected sum (sum s_i k_i mod r) G."""
    rng = synth.Xoshiro256ss(seed)
    dG = synth.g1_mul(d, G)
    cur = synth.g1_mul(a, G)
    xs, ss, acc = [], [], 0
    for i in range(n):
        xs.append(cur)
        sv = rng.next_u256()
        ss.append(sv)
        acc += sv * (a + i * d)
        cur = synth.g1_add(cur, dG)
    return swords(ss), words(xs), synth.g1_mul(acc % R_ORD, G)


@pytest.mark.gpu
def test_large_chain_three_levels(gpu_ctx):
    n = 70000  # > 256^2 + 1 points: the scan has three levels
    s, x, want = arithmetic_inputs(n, 0x1234567, 0x9E3779B9, seed=70000)
    R = words([synth.g1_mul(0xC0FFEE, G)])[0]
    offs, res = gpu_ctx.g1_msm_chain(s, x, R)
    assert offs.shape == (n + 1, 8) and np.array_equal(offs[0], R)
    assert pt(res) == want
    rng = np.random.default_rng(1)
    for i in list(rng.choice(n, 62, replace=False)) + [0, n - 1]:
        assert pt(offs[i + 1]) == synth.g1_scalar_mul_offset(synth.words_to_int(s[i]), pt(x[i]), pt(offs[i])), f"link {i}"


@pytest.mark.gpu
def test_msm_proofs_per_proof_128(gpu_ctx, jobs):
    s, x, o = jobs
    R = np.ascontiguousarray(o[500])
    res, offs, proofs = gpu_ctx.g1_msm(s, x, R, per_proof=128)
    assert len(proofs) == 8 and proofs[-1].outputs.size == 8 * (1000 - 7 * 128)
    pk.verify_g1_msm(s, x, R, res, offs, proofs, 128, ctx=gpu_ctx)
    want, msm = synth.g1_msm_chain(s, x, R)
    assert pt(res) == msm and np.array_equal(offs, words(want))


@pytest.mark.gpu
def test_msm_one_proof_hook_shape(gpu_ctx):
    n = 4096
    s, x, want = arithmetic_inputs(n, 0x77, 0x10001, seed=4096)
    R = words([synth.g1_mul(0xBEEF, G)])[0]
    res, offs, proofs = gpu_ctx.g1_msm(s, x, R, per_proof=4096)
    assert len(proofs) == 1 and proofs[0].degree_bits == 21
    pk.verify_g1_msm(s, x, R, res, offs, proofs, 4096, ctx=gpu_ctx)
    assert pt(res) == want


def expect_error(fn, code, text):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert f"failed with {code}" in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_msm_errors_then_a_normal_msm(gpu_ctx, jobs):
    s0, x0, o = jobs
    s, x = np.ascontiguousarray(s0[:3]), np.ascontiguousarray(x0[:3])
    # R = -(s_0 x_0): offset_1 is infinity
    R = words([neg(synth.g1_mul(synth.words_to_int(s[0]) % R_ORD, pt(x[0])))])[0]
    expect_error(lambda: gpu_ctx.g1_msm_chain(s, x, R), -4, "offset_1 ")
    expect_error(lambda: gpu_ctx.g1_msm(s, x, R, per_proof=2), -4, "offset_1 ")
    # a zero sum: offset_n == R, the result would be infinity
    k = synth.words_to_int(s[1]) % R_ORD
    sz, xz = swords([k, R_ORD - k]), words([pt(x[1]), pt(x[1])])
    expect_error(lambda: gpu_ctx.g1_msm_chain(sz, xz, np.ascontiguousarray(o[0])), -4, "offset_n equals R")
    expect_error(lambda: gpu_ctx.g1_msm(sz, xz, np.ascontiguousarray(o[0])), -4, "offset_n equals R")
    # offset_n == -R is accepted: the result is the doubling -2R
    Rp = pt(o[1])
    offs, res = gpu_ctx.g1_msm_chain(swords([R_ORD - 2]), words([Rp]), np.ascontiguousarray(o[1]))
    assert pt(offs[1]) == neg(Rp) and pt(res) == neg(synth.g1_add(Rp, Rp))
    # shapes the batch cannot prove, before any device work
    expect_error(lambda: gpu_ctx.g1_msm(s, x, np.ascontiguousarray(o[0]), per_proof=16385), -5, "per_proof")
    # the context still proves a normal MSM
    R = np.ascontiguousarray(o[2])
    res, offs, proofs = gpu_ctx.g1_msm(s, x, R, per_proof=2)
    assert len(proofs) == 2
    pk.verify_g1_msm(s, x, R, res, offs, proofs, 2, ctx=gpu_ctx)
    assert pt(res) == synth.g1_msm_chain(s, x, R)[1]
