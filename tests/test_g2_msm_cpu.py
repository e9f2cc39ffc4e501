"""g2_msm without a GPU (the g1_msm circuit, src/utils/g1_msm.rs:22-36, with the G2 gadgets): the Python reference chain, on
subgroup points and on a twist point outside the subgroup, the argument checks of the two C entry points, and verify_g2_msm on
proofs made by the CPU oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import map_to_g2_ref as m2g
from tools import synth

P, R_ORD, G = synth.P, synth.R_ORDER, synth.G2_GEN


def neg(p):
    return (p[0], ((-p[1][0]) % P, (-p[1][1]) % P))


def swords(ss):
    return np.array([synth._to_words(s) for s in ss], np.uint64).reshape(-1, 4)


def naive_fold(ss, xs, r):
    """offset_{i+1} = s_i x_i + offset_i with affine arithmetic, as the reference's g2_scalar_mul generator computes each link."""
    offs = [r]
    for s, x in zip(ss, xs):
        offs.append(synth.g2_scalar_mul_offset(s, x, offs[-1]))
    return offs, synth.g2_add(offs[-1], neg(r))


def test_python_chain_matches_naive_fold():
    rng = synth.Xoshiro256ss(6)
    pts = [synth.g2_mul(rng.next_u256() % (R_ORD - 1) + 1, G) for _ in range(8)]
    r = synth.g2_mul(rng.next_u256() % (R_ORD - 1) + 1, G)
    ss = [rng.next_u256(), 0, R_ORD, R_ORD + 1, rng.next_u256(), 2**256 - 1, 1, rng.next_u256()]
    offs, msm = synth.g2_msm_chain(swords(ss), synth.g2_points_to_words(pts), synth.g2_points_to_words([r])[0])
    want, want_msm = naive_fold(ss, pts, r)
    assert offs == want and msm == want_msm
    assert offs[2] == offs[1] and offs[3] == offs[2]  # s = 0 and s = r leave the offset alone on subgroup points
    assert offs[4] == synth.g2_add(offs[3], pts[3])   # s = r + 1 adds x once
    # int scalars and point tuples are accepted too, and a partial sum may pass through infinity
    offs2, _ = synth.g2_msm_chain([3, R_ORD - 3, 5], [pts[0], pts[0], pts[1]], r)
    assert offs2[2] == r and offs2[3] == synth.g2_add(synth.g2_mul(5, pts[1]), r)
    offs3, msm3 = synth.g2_msm_chain([1, 1], [neg(r), pts[2]], r)
    assert offs3[1] is None and offs3[2] == pts[2] and msm3 == synth.g2_add(pts[2], neg(r))


def twist_point_outside_subgroup(seed=0x6732):
    """A map_to_g2 point before cofactor clearing (hash_to_g2.rs:128-145): on the twist, not in the r-torsion subgroup."""
    u = m2g.inputs(1, seed=seed)[0]
    x1, x2, _ = m2g.candidates(u)
    pt = m2g.select_point(u, m2g.fq_is_square(m2g.f2_norm(m2g.g(x1))), m2g.fq_is_square(m2g.f2_norm(m2g.g(x2))))
    assert synth.g2_mul_unreduced(R_ORD, pt) is not None
    return pt


def test_python_chain_uses_the_unreduced_scalar():
    pt = twist_point_outside_subgroup()
    r = synth.g2_mul(0xC0FFEE, G)
    s = R_ORD + 0x1234567  # >= r
    offs, msm = synth.g2_msm_chain(swords([s]), synth.g2_points_to_words([pt]), synth.g2_points_to_words([r])[0])
    want = synth.g2_mul(s, pt)  # affine double-and-add over every bit of s
    assert offs[1] == synth.g2_add(want, r) and msm == want
    assert synth.g2_mul(s % R_ORD, pt) != want  # the reduced scalar gives another point
    # the same through the full range of the ABI scalar
    s2 = 2**256 - 1
    assert synth.g2_msm_chain([s2], [pt], r)[1] == synth.g2_mul(s2, pt) != synth.g2_mul(s2 % R_ORD, pt)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_check_their_arguments():
    lib = pk.load_library()
    s, x, o = synth.g2_inputs(3, seed=3)
    R = np.ascontiguousarray(o[0])
    offs, res = np.zeros((4, 16), np.uint64), np.zeros(16, np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5
    # no context: the chain needs one
    assert lib.bn254s_g2_msm_chain(None, _vp(s), _vp(x), _vp(R), 3, _vp(offs), _vp(res)) == E_ARG

    def msm(ctx=None, params=params, s=s, x=x, R=R, n=3, per_proof=20000, res=res, offs=offs, slots=True):
        outs = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_g2_msm(ctx, C.byref(params) if params is not None else None, _vp(s), _vp(x), _vp(R), n, per_proof, _vp(res),
                               _vp(offs), outs if slots else None)
        return rc, list(outs)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), slots are cleared
    rc, outs = msm()
    assert rc == E_UNSUP and outs[0] is None and outs[1] == 1
    assert msm(per_proof=16385)[0] == E_UNSUP
    assert msm(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    # each invalid argument alone is reported before the shape
    assert msm(s=None)[0] == E_ARG
    assert msm(x=None)[0] == E_ARG
    assert msm(R=None)[0] == E_ARG
    assert msm(res=None)[0] == E_ARG
    assert msm(slots=False)[0] == E_ARG
    assert msm(params=None)[0] == E_ARG
    assert msm(n=0)[0] == E_ARG
    assert msm(per_proof=0)[0] == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert msm(params=bad)[0] == E_ARG
    assert msm(offs=None)[0] == E_UNSUP  # offsets_out may be NULL


@pytest.fixture(scope="module")
def oracle_msm():
    """n = 3, per_proof = 2: two 2^16-row G2 proofs made by the CPU oracle from the Python chain's offsets."""
    s, x, o = synth.g2_inputs(3, seed=22)
    R = np.ascontiguousarray(o[0])
    offs_pts, msm = synth.g2_msm_chain(s, x, R)
    offs = synth.g2_points_to_words(offs_pts)
    res = synth.g2_points_to_words([msm])[0]
    orc = oracle_lib.load()
    proofs = []
    for lo, hi in ((0, 2), (2, 3)):
        words, outs, _, db = oracle_lib.prove(orc, 1, s[lo:hi], x[lo:hi], np.ascontiguousarray(offs[lo:hi]))
        proofs.append(SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1)))
    return s, x, R, res, offs, proofs


def test_verify_g2_msm_accepts_oracle_proofs(oracle_msm):
    s, x, R, res, offs, proofs = oracle_msm
    assert np.array_equal(proofs[0].outputs.reshape(-1, 16), offs[1:3]) and np.array_equal(proofs[1].outputs.reshape(-1, 16), offs[3:])
    pk.verify_g2_msm(s, x, R, res, offs, proofs, 2)


def test_verify_g2_msm_rejects_broken_links(oracle_msm):
    s, x, R, res, offs, proofs = oracle_msm
    swapped = offs.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    with pytest.raises(pk.VerifyError, match=r"^g2_msm: output 0 of proof 0 != offsets\[1\]"):
        pk.verify_g2_msm(s, x, R, res, swapped, proofs, 2)
    R2 = synth.g2_points_to_words([synth.g2_mul(7, G)])[0]
    with pytest.raises(pk.VerifyError, match=r"^g2_msm: offsets\[0\] != R"):
        pk.verify_g2_msm(s, x, R2, res, offs, proofs, 2)
    wrong = synth.g2_points_to_words([synth.g2_add(synth.g2_mul(2, G), synth.g2_from_words(res))])[0]
    with pytest.raises(pk.VerifyError, match="^g2_msm: result"):
        pk.verify_g2_msm(s, x, R, wrong, offs, proofs, 2)
    # consistent linkage, but a word of proof 1's trace cap changed: the verifier rejects that proof
    words = proofs[1].words.copy()
    words[0] ^= 1
    tampered = [proofs[0], SimpleNamespace(words=words, degree_bits=proofs[1].degree_bits, outputs=proofs[1].outputs)]
    with pytest.raises(pk.VerifyError, match="^g2_msm: proof 1"):
        pk.verify_g2_msm(s, x, R, res, offs, tampered, 2)
