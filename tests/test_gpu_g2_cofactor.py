"""G2 cofactor clearing on the GPU: the device front-end (csrc/g2_cofactor.hip, the form with psi) against the Python definition
[h]P (tools/synth.py g2_clear_cofactor) byte for byte, points of every small order of the cofactor, closure under the subgroup
check, the rejection of unreduced coordinates and of points off the curve before any output, the proven jobs (h, P_i, R_i) checked
with verify_g2_clear_cofactor, the proof-free map_to_g2 / hash_to_g2, and the chain recover -> clear -> check -> g2_msm."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import map_to_g2_ref as m2g
from tools import synth

P, R, H = synth.P, synth.R_ORDER, synth.G2_COFACTOR
SIZES = [1, 63, 64, 65, 257]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail


def _images(points):
    """(images [n,16], finite [n]) of the Python definition for affine points."""
    imgs = [synth.g2_clear_cofactor(pt) for pt in points]
    words = np.zeros((len(imgs), 16), np.uint64)
    for i, img in enumerate(imgs):
        if img is not None:
            words[i] = synth.g2_points_to_words([img])[0]
    return words, np.array([img is not None for img in imgs], np.uint8)


@pytest.fixture(scope="module")
def reference():
    """The 257 inputs of seed 41 (every smaller case is a prefix; what they cover: tests/test_g2_cofactor_cpu.py) and the images
    and bytes of the Python definition."""
    pts, _ = synth.g2_subgroup_inputs(max(SIZES), seed=41)
    images, finite = _images([synth.g2_from_words(w) for w in pts])
    for a in (pts, images, finite):
        a.setflags(write=False)
    return pts, images, finite


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _u_words(us):
    return np.array([synth._to_words(a[0]) + synth._to_words(a[1]) for a in us], dtype=np.uint64).reshape(-1, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_python(gpu_ctx, reference, n):
    pts, want, want_fin = (np.ascontiguousarray(a[:n]) for a in reference)
    images, finite = gpu_ctx.g2_clear_cofactor_batch(pts)
    assert images.dtype == np.uint64 and images.shape == (n, 16) and finite.dtype == np.uint8 and finite.shape == (n,)
    assert np.array_equal(finite, want_fin), f"finite differs at {np.nonzero(finite != want_fin)[0][:4]}"
    assert images.tobytes() == want.tobytes(), f"images differ at {np.nonzero(np.any(images != want, axis=1))[0][:4]}"
    again = gpu_ctx.g2_clear_cofactor_batch(pts)
    assert again[0].tobytes() == images.tobytes() and again[1].tobytes() == finite.tobytes()
    # every lane writes its own 16 words and byte and no others (an infinite image is written as zeros, not left alone)
    raw_img, raw_fin = np.full((n + 2, 16), 7, np.uint64), np.full(n + 8, 7, np.uint8)
    assert gpu_ctx._lib.bn254s_g2_clear_cofactor_batch(gpu_ctx._h, _vp(pts), n, _vp(raw_img), _vp(raw_fin)) == 0
    assert np.array_equal(raw_img[:n], want) and (raw_img[n:] == 7).all()
    assert np.array_equal(raw_fin[:n], want_fin) and (raw_fin[n:] == 7).all()


@pytest.mark.gpu
def test_small_order_and_edge_points(gpu_ctx, reference):
    """One point of each prime order of the cofactor, one of order 10069 * 5864401, a member plus a point of order 10069, G2_GEN
    and -G2_GEN: every one alone in its launch, and all together.  (A point with psi(P) == +-P does not exist on the twist other
    than O: tests/test_g2_cofactor_cpu.py test_cofactor_numbers; none was constructed.)"""
    pts_all = reference[0]
    _, _, classes = synth.g2_subgroup_inputs(32, seed=41, with_classes=True)
    prime = [next(i for i, (c, d) in enumerate(classes) if c == 3 and d == f) for f in synth.G2_COFACTOR_PRIMES]
    pick = prime + [classes.index((4, 10069 * 5864401)), classes.index((5, 10069))]
    gen = synth.G2_GEN
    pts = np.ascontiguousarray(np.concatenate([pts_all[pick], synth.g2_points_to_words([gen, synth.g2_neg(gen)])]))
    want = np.concatenate([reference[1][pick], synth.g2_points_to_words([synth.g2_mul(H % R, gen), synth.g2_neg(synth.g2_mul(H % R, gen))])])
    want_fin = [0, 0, 0, 0, 0, 1, 1, 1]
    assert reference[2][pick].tolist() == want_fin[:6]
    images, finite = gpu_ctx.g2_clear_cofactor_batch(pts)
    assert finite.tolist() == want_fin and np.array_equal(images, want)
    for i in range(8):
        img, fin = gpu_ctx.g2_clear_cofactor_batch(np.ascontiguousarray(pts[i:i + 1]))
        assert fin.tolist() == [want_fin[i]] and np.array_equal(img[0], want[i]), i


@pytest.mark.gpu
def test_images_are_members(gpu_ctx, reference):
    pts = np.ascontiguousarray(reference[0][:65])
    images, finite = gpu_ctx.g2_clear_cofactor_batch(pts)
    members = np.ascontiguousarray(images[finite == 1])
    assert 0 < members.shape[0] < 65
    assert gpu_ctx.g2_subgroup_check_batch(members).all()
    assert not gpu_ctx.g2_subgroup_check_batch(pts).all()  # (the inputs are not all members)


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
    images, finite, jobs = np.full((8, 16), 7, np.uint64), np.full(8, 7, np.uint8), np.full((8, 20), 7, np.uint64)
    lib = gpu_ctx._lib
    rc = lib.bn254s_g2_clear_cofactor_batch(gpu_ctx._h, _vp(pts), 8, _vp(images), _vp(finite))
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode()
    assert (images == 7).all() and (finite == 7).all()
    outs = (C.c_void_p * 4)(*([1] * 4))
    params = pk.default_params()
    rc = lib.bn254s_g2_clear_cofactor(gpu_ctx._h, C.byref(params), _vp(pts), _vp(offs), 8, 2, _vp(images), _vp(finite), _vp(jobs), outs)
    assert rc == -1 and "_5 " in lib.bn254s_last_error(gpu_ctx._h).decode() and list(outs) == [None] * 4
    assert (images == 7).all() and (finite == 7).all() and (jobs == 7).all()
    with pytest.raises(RuntimeError, match="failed with -1: .*point_5 "):
        gpu_ctx.g2_clear_cofactor_batch(pts)
    with pytest.raises(RuntimeError, match="failed with -1: .*point_5 "):
        gpu_ctx.g2_clear_cofactor(pts, offs, per_proof=8)
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        gpu_ctx.g2_clear_cofactor(reference[0][:8], offs, per_proof=16385)
    # the same context clears a valid batch correctly afterwards
    images, finite = gpu_ctx.g2_clear_cofactor_batch(np.ascontiguousarray(reference[0][:8]))
    assert np.array_equal(images, reference[1][:8]) and np.array_equal(finite, reference[2][:8])


@pytest.mark.gpu
def test_full_call_two_proofs(gpu_ctx, reference):
    n = 130
    pts, want, want_fin = (np.ascontiguousarray(a[:n]) for a in reference)
    offs = synth.g2_inputs(n, seed=47)[2]
    images, finite, jobs, proofs = gpu_ctx.g2_clear_cofactor(pts, offs, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 16 * 128 and proofs[1].outputs.size == 16 * 2
    assert np.array_equal(images, want) and np.array_equal(finite, want_fin)
    h_words = np.array(synth._to_words(H), np.uint64)
    assert np.array_equal(jobs[:, :4], np.tile(h_words, (n, 1))) and np.array_equal(jobs[:, 4:], pts)
    outs = np.concatenate([pr.outputs.reshape(-1, 16) for pr in proofs])
    for i in range(n):
        if want_fin[i]:  # R_i + image_i, with Python's image
            rp = synth.g2_add(synth.g2_from_words(offs[i]), synth.g2_from_words(want[i]))
            assert np.array_equal(outs[i], synth.g2_points_to_words([rp])[0]), i
        else:
            assert np.array_equal(outs[i], offs[i]), i
    pk.verify_g2_clear_cofactor(pts, offs, images, finite, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    pk.verify_g2_clear_cofactor(pts, offs, images, finite, jobs, proofs, 128)               # the host verifier
    flipped = finite.copy()
    flipped[129] ^= 1
    with pytest.raises(pk.VerifyError, match="image 129 "):
        pk.verify_g2_clear_cofactor(pts, offs, images, flipped, jobs, proofs, 128)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65])
def test_map_to_g2_batch_matches_python(gpu_ctx, n):
    us = m2g.inputs(n, seed=41) + [(0, 0), (P - 1, P - 1)]
    want = synth.g2_points_to_words([m2g.map_to_g2(u) for u in us])
    got = gpu_ctx.map_to_g2_batch(_u_words(us))
    assert got.shape == (n + 2, 16) and got.tobytes() == want.tobytes(), f"differ at {np.nonzero(np.any(got != want, axis=1))[0][:4]}"


@pytest.mark.gpu
def test_map_to_g2_batch_equals_the_proven_pipeline(gpu_ctx):
    u = _u_words(m2g.inputs(5, seed=23))
    offs = synth.g2_inputs(5, seed=29)[2]
    proven = gpu_ctx.map_to_g2(u, offs)[0]
    assert np.array_equal(gpu_ctx.map_to_g2_batch(u), proven)
    big = u.copy()
    big[3, 4:] = synth._to_words(P)  # u_3.c1 == p
    out = np.full((5, 16), 7, np.uint64)
    assert gpu_ctx._lib.bn254s_map_to_g2_batch(gpu_ctx._h, _vp(big), 5, _vp(out)) == -1
    assert "u_3 has c1" in gpu_ctx._lib.bn254s_last_error(gpu_ctx._h).decode() and (out == 7).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ln", [0, 3, 8, 11])
def test_hash_to_g2_batch(gpu_ctx, ln):
    rng = synth.Xoshiro256ss(100 + ln)
    x = np.array([[rng.next_u64() % m2g.GL_P for _ in range(ln)] for _ in range(4)], dtype=np.uint64).reshape(4, ln)
    got = gpu_ctx.hash_to_g2_batch(x)
    assert np.array_equal(got, gpu_ctx.map_to_g2_batch(gpu_ctx.hash_to_fq2_batch(x)))
    assert got[0].tobytes() == synth.g2_points_to_words([m2g.map_to_g2(m2g.hash_to_fq2(x[0]))])[0].tobytes()


@pytest.mark.gpu
def test_recover_clear_check_msm_chain(gpu_ctx, reference):
    """recover -> clear the cofactor -> subgroup check -> g2_msm: the x of two random twist points."""
    rnd = np.ascontiguousarray(reference[0][[1, 8]])  # class 1 of the inputs: random twist points
    sgns = np.array([synth.f2_sgn(synth.g2_from_words(w)[1]) for w in rnd], np.uint8)
    pts, rec, _ = gpu_ctx.g2_recover_from_x_batch(np.ascontiguousarray(rnd[:, :8]), sgns)
    assert rec.all() and np.array_equal(pts, rnd)
    assert gpu_ctx.g2_subgroup_check_batch(pts).tolist() == [0, 0]
    images, finite = gpu_ctx.g2_clear_cofactor_batch(pts)
    assert finite.tolist() == [1, 1] and np.array_equal(images, reference[1][[1, 8]])
    assert gpu_ctx.g2_subgroup_check_batch(images).tolist() == [1, 1]
    s, _, o = synth.g2_inputs(2, seed=77)
    R0 = np.ascontiguousarray(o[0])
    res, offs, proofs = gpu_ctx.g2_msm(s, images, R0, per_proof=128)
    want, msm = synth.g2_msm_chain(s, images, R0)
    assert np.array_equal(offs, synth.g2_points_to_words(want)) and np.array_equal(res, synth.g2_points_to_words([msm])[0])
    pk.verify_g2_msm(s, images, R0, res, offs, proofs, 128, ctx=gpu_ctx)
