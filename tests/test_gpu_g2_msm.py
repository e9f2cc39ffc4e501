"""g2_msm on the GPU (the g1_msm circuit, src/utils/g1_msm.rs:22-36, with the G2 gadgets): the device chain (csrc/msm.hip)
against the Python fold (tools/synth.py g2_msm_chain), the chained G2 proofs checked with verify_g2_msm, and the error cases."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import map_to_g2_ref as m2g
from tools import synth

P, R_ORD, G = synth.P, synth.R_ORDER, synth.G2_GEN


def words(pts):
    return synth.g2_points_to_words(pts)


def swords(ss):
    return np.array([synth._to_words(s) for s in ss], np.uint64).reshape(-1, 4)


def pt(w):
    return synth.g2_from_words(w)


def neg(p):
    return (p[0], ((-p[1][0]) % P, (-p[1][1]) % P))


def check_chain(ctx, s, x, R, want=None):
    offs, res = ctx.g2_msm_chain(s, x, R)
    want, msm = want or synth.g2_msm_chain(s, x, R)
    assert all(p is not None for p in want)
    assert np.array_equal(offs, words(want)), f"first differing offset: {np.nonzero(np.any(offs != words(want), axis=1))[0][:4]}"
    assert np.array_equal(res, words([msm])[0])
    return offs, res


def twist_point_outside_subgroup(seed):
    """A map_to_g2 point before cofactor clearing: on the twist, not in the r-torsion subgroup."""
    u = m2g.inputs(1, seed=seed)[0]
    x1, x2, _ = m2g.candidates(u)
    p = m2g.select_point(u, m2g.fq_is_square(m2g.f2_norm(m2g.g(x1))), m2g.fq_is_square(m2g.f2_norm(m2g.g(x2))))
    assert synth.g2_mul_unreduced(R_ORD, p) is not None
    return p


@pytest.fixture(scope="module")
def jobs():
    s, x, o = synth.g2_inputs(300, seed=0x67326D)
    R = np.ascontiguousarray(o[0])
    offs, _ = synth.g2_msm_chain(s, x, R)
    return s, x, R, offs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 300])
def test_chain_matches_python(gpu_ctx, jobs, n):
    s, x, R, offs = jobs
    want = (offs[:n + 1], synth.g2_add(offs[n], neg(pt(R))))  # the fold of the first n inputs
    check_chain(gpu_ctx, np.ascontiguousarray(s[:n]), np.ascontiguousarray(x[:n]), R, want)


@pytest.mark.gpu
def test_chain_special_cases(gpu_ctx, jobs):
    s0, x0, R0, _ = jobs
    R = pt(R0)
    xs = [pt(x0[i]) for i in range(6)]
    a = synth.words_to_int(s0[0]) % R_ORD
    ss = [0, R_ORD, R_ORD + 5, 2**256 - 1, a, R_ORD - a, 7, 7, synth.words_to_int(s0[1]), 1, 2, R_ORD]
    xx = [xs[0], xs[1], xs[2], xs[2], xs[3], xs[3], xs[4], xs[4], xs[5], xs[0], xs[0], xs[1]]
    # s = 0 and s = r: no change (subgroup points); unreduced s; s x, (r - s) x: the partial sum returns to offset_4;
    # two adjacent equal inputs (7 x_4 twice): the first scan step adds a point to itself
    offs, _ = check_chain(gpu_ctx, swords(ss), words(xx), R0)
    assert np.array_equal(offs[1], offs[0]) and np.array_equal(offs[2], offs[0]) and np.array_equal(offs[6], offs[4])
    # x_1 = offset_1, s_1 = 1: the sequential fold doubles offset_1
    off1 = synth.g2_scalar_mul_offset(synth.words_to_int(s0[2]), pt(x0[2]), R)
    offs2, _ = check_chain(gpu_ctx, swords([synth.words_to_int(s0[2]), 1, 3]), words([pt(x0[2]), off1, pt(x0[3])]), R0)
    assert pt(offs2[2]) == synth.g2_add(off1, off1)
    # the same configurations across the first block boundary of the scan (inputs 250 .. 258 of 300)
    s3, x3 = s0.copy(), x0.copy()
    s3[250], s3[251], s3[252], s3[253] = (synth._to_words(v) for v in (0, R_ORD, 2**256 - 1, R_ORD + 5))
    s3[254], x3[254] = s3[253], x3[253]                                        # equal to the input before
    s3[255], x3[255] = s3[254], x3[254]                                        # and once more
    s3[256], x3[256] = synth._to_words(R_ORD - (R_ORD + 5) % R_ORD), x3[255]   # back to offset_255
    pref, _ = synth.g2_msm_chain(s3[:257], x3[:257], R0)
    s3[257], x3[257] = synth._to_words(1), words([pref[257]])[0]               # x_257 = offset_257: doubles
    s3[258], x3[258] = synth._to_words(R_ORD + 0xABCDEF), words([twist_point_outside_subgroup(0x258)])[0]
    offs3, _ = check_chain(gpu_ctx, s3, x3, R0)
    assert np.array_equal(offs3[257], offs3[255]) and pt(offs3[258]) == synth.g2_add(pref[257], pref[257])


@pytest.mark.gpu
def test_chain_outside_the_subgroup(gpu_ctx):
    # the products are s x for the full 256-bit s: for a twist point outside the subgroup (s mod r) x is another point
    pts = [twist_point_outside_subgroup(seed) for seed in (1, 2, 3)]
    ss = [R_ORD + 0x1234567, 2**256 - 1, 3 * R_ORD]
    R = words([synth.g2_mul(0xC0FFEE, G)])[0]
    offs, res = check_chain(gpu_ctx, swords(ss), words(pts), R)
    reduced, _ = synth.g2_msm_chain([s % R_ORD for s in ss], pts, R)
    assert not np.array_equal(offs[1], words([reduced[1]])[0])


def arithmetic_inputs(n, a, d, seed):
    """x_i = (a + i d) G by one affine addition per input, random 256-bit scalars, and the expected sum (sum s_i k_i mod r) G."""
    rng = synth.Xoshiro256ss(seed)
    dG = synth.g2_mul(d, G)
    cur = synth.g2_mul(a, G)
    xs, ss, acc = [], [], 0
    for i in range(n):
        xs.append(cur)
        sv = rng.next_u256()
        ss.append(sv)
        acc += sv * (a + i * d)
        cur = synth.g2_add(cur, dG)
    return swords(ss), words(xs), synth.g2_mul(acc % R_ORD, G)


@pytest.mark.gpu
def test_large_chain_three_levels(gpu_ctx):
    n = 70000  # > 256^2 + 1 points: the scan has three levels; more than one product chunk (8192 inputs)
    s, x, want = arithmetic_inputs(n, 0x1234567, 0x9E3779B9, seed=70000)
    R = words([synth.g2_mul(0xC0FFEE, G)])[0]
    offs, res = gpu_ctx.g2_msm_chain(s, x, R)
    assert offs.shape == (n + 1, 16) and np.array_equal(offs[0], R)
    assert pt(res) == want
    rng = np.random.default_rng(1)
    for i in list(rng.choice(n, 62, replace=False)) + [0, n - 1]:
        assert pt(offs[i + 1]) == synth.g2_scalar_mul_offset(synth.words_to_int(s[i]), pt(x[i]), pt(offs[i])), f"link {i}"


@pytest.mark.gpu
def test_msm_proofs_per_proof_128(gpu_ctx, jobs):
    s, x, _, _ = jobs
    R = words([synth.g2_mul(0x5EED, G)])[0]
    res, offs, proofs = gpu_ctx.g2_msm(s, x, R, per_proof=128)
    assert len(proofs) == 3 and proofs[-1].outputs.size == 16 * (300 - 2 * 128)
    pk.verify_g2_msm(s, x, R, res, offs, proofs, 128, ctx=gpu_ctx)
    want, msm = synth.g2_msm_chain(s, x, R)
    assert pt(res) == msm and np.array_equal(offs, words(want))


@pytest.mark.gpu
def test_msm_one_proof_hook_shape(gpu_ctx):
    n = 1024
    s, x, want = arithmetic_inputs(n, 0x77, 0x10001, seed=1024)
    R = words([synth.g2_mul(0xBEEF, G)])[0]
    res, offs, proofs = gpu_ctx.g2_msm(s, x, R, per_proof=1024)
    assert len(proofs) == 1 and proofs[0].degree_bits == 19
    pk.verify_g2_msm(s, x, R, res, offs, proofs, 1024, ctx=gpu_ctx)
    assert pt(res) == want


def expect_error(fn, code, text):
    with pytest.raises(RuntimeError) as e:
        fn()
    assert f"failed with {code}" in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_msm_errors_then_a_normal_msm(gpu_ctx, jobs):
    s0, x0, _, _ = jobs
    s, x = np.ascontiguousarray(s0[:3]), np.ascontiguousarray(x0[:3])
    # R = -(s_0 x_0): offset_1 is infinity
    R = words([neg(synth.g2_mul(synth.words_to_int(s[0]) % R_ORD, pt(x[0])))])[0]
    expect_error(lambda: gpu_ctx.g2_msm_chain(s, x, R), -4, "offset_1 ")
    expect_error(lambda: gpu_ctx.g2_msm(s, x, R, per_proof=2), -4, "offset_1 ")
    # a zero sum: offset_n == R, the result would be infinity
    R1 = words([synth.g2_mul(0x1111, G)])[0]
    k = synth.words_to_int(s[1]) % R_ORD
    sz, xz = swords([k, R_ORD - k]), words([pt(x[1]), pt(x[1])])
    expect_error(lambda: gpu_ctx.g2_msm_chain(sz, xz, R1), -4, "offset_n equals R")
    expect_error(lambda: gpu_ctx.g2_msm(sz, xz, R1), -4, "offset_n equals R")
    # offset_n == -R is accepted: the result is the doubling -2R
    Rp = pt(R1)
    offs, res = gpu_ctx.g2_msm_chain(swords([R_ORD - 2]), words([Rp]), R1)
    assert pt(offs[1]) == neg(Rp) and pt(res) == neg(synth.g2_add(Rp, Rp))
    # shapes the batch cannot prove, before any device work
    expect_error(lambda: gpu_ctx.g2_msm(s, x, R1, per_proof=16385), -5, "per_proof")
    # the context still proves a normal MSM
    R2 = words([synth.g2_mul(0x2222, G)])[0]
    res, offs, proofs = gpu_ctx.g2_msm(s, x, R2, per_proof=2)
    assert len(proofs) == 2
    pk.verify_g2_msm(s, x, R2, res, offs, proofs, 2, ctx=gpu_ctx)
    assert pt(res) == synth.g2_msm_chain(s, x, R2)[1]
