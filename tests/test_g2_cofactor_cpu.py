"""G2 cofactor clearing without a GPU: the numbers the kernel's form rests on (h = 2p - r = p - 1 + t, the multipliers of its two
ladders and their prefixes), the Python reference (tools/synth.py: the definition [h]P and, independently, the form with psi), the
inputs of the GPU parity test and what they cover, the generated constants, the argument checks of the four C entry points,
map_to_g2_ref.map_to_g2 against the model of the proven pipeline, and verify_g2_clear_cofactor on a G2 proof made by the CPU
oracle."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import map_to_g2_ref as m2g
from tools import synth

P, R, X0 = synth.P, synth.R_ORDER, synth.X0
H, PRIMES = synth.G2_COFACTOR, synth.G2_COFACTOR_PRIMES
T = 6 * X0 * X0 + 1
SEED = 41  # the seed of the GPU parity test (tests/test_gpu_g2_cofactor.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2_bn254_amd", "csrc")


@pytest.fixture(scope="module")
def inputs():
    pts, _, classes = synth.g2_subgroup_inputs(257, seed=SEED, with_classes=True)
    points = [synth.g2_from_words(w) for w in pts]
    return pts, classes, points, [synth.g2_clear_cofactor(pt) for pt in points]


def _inc_words(name, fname):
    with open(os.path.join(CSRC, fname)) as f:
        m = re.search(r"%s\[4\] = \{([^}]*)\}" % name, f.read())
    return synth.words_to_int([int(w.strip().rstrip("ULL"), 16) for w in m.group(1).split(",")])


def test_cofactor_numbers():
    assert R == P + 1 - T and H == 2 * P - R == P - 1 + T == m2g.COFACTOR
    assert _inc_words("M2G_COFACTOR", "map_to_g2_constants.inc") == H == _inc_words("G2C_H", "g2_cofactor_constants.inc")
    assert math.prod(PRIMES) == H
    assert (6 * X0) * X0 == T - 1 and (6 * X0).bit_length() == 65
    for f in PRIMES + (R,):  # none of x0, 6 x0^2 and h is 0 modulo a prime of r h (h: modulo r)
        assert X0 % f and (6 * X0 * X0) % f
    assert H % R
    # psi has no fixed and no negated point other than O on E'(Fq2): psi(P) = +-P gives (1 -+ t + p) P = O by psi^2 - t psi + p = 0;
    # 1 - t + p = r, and on the r-torsion psi is multiplication by p != 1; 1 + t + p is coprime to r h.  So the GPU test cannot
    # hold a point with psi(P) == +-P: none exists.
    assert math.gcd(1 + T + P, R * H) == 1 and P + 1 - T == R and P % R != 1


def test_ladders_meet_no_exceptional_case():
    """The accumulator [k]B over the prefixes k of x0 (base P) and of 6 x0 (base [x0]P): 2k is never 0, 1 or -1 modulo a prime of
    r h, so [2k]B is never O, B or -B for a base of any order d > 1 dividing r h (csrc/g2_cofactor.hip)."""
    for mult in (X0, 6 * X0):
        bits, k = bin(mult)[2:], 1
        for b in bits[1:]:
            for f in PRIMES + (R,):
                assert 2 * k % f not in (0, 1, f - 1), (mult, k, f)
            k = 2 * k + int(b)
        assert k == mult
    assert min(PRIMES[3], R) > 12 * X0 + 1 > max(PRIMES[:3])  # only the three small primes can divide 2k or 2k +- 1 at all


def test_form_with_psi_is_the_definition_on_the_parity_inputs(inputs):
    pts, classes, points, images = inputs
    for i, (pt, img) in enumerate(zip(points, images)):
        assert synth.g2_clear_cofactor_psi(pt) == img, (i, classes[i])
        if classes[i][0] in (3, 4):  # an order that divides h
            assert img is None, (i, classes[i])
        else:
            assert img is not None and synth.g2_on_curve(img) and synth.g2_in_subgroup(img), (i, classes[i])
    assert synth.g2_clear_cofactor(synth.G2_GEN) == synth.g2_mul(H % R, synth.G2_GEN)
    assert synth.g2_clear_cofactor_psi(synth.g2_neg(synth.G2_GEN)) == synth.g2_neg(synth.g2_mul(H % R, synth.G2_GEN))


def test_parity_inputs_cover_both_values_at_the_block_edges(inputs):
    _, classes, _, images = inputs
    finite = np.array([img is not None for img in images], np.uint8)
    assert finite[:7].tolist() == [1, 1, 1, 0, 0, 1, 1]
    for n in (63, 64, 65, 257):  # every parity size above 1 holds both values
        assert 0 < int(finite[:n].sum()) < n
    # lanes 63 | 64 are classes 0 and 1, both finite; the infinite images next to the block edge are 59, 60 and 66, 67, and the
    # window 62..65 holds only finite ones (62 = class 6, 65 = class 2).  The GPU test therefore relies on 59/60 and 66/67 for
    # the two values around the edge of the first block, on 255 | 256 (classes 3 and 4: infinite) against 254 (class 2: finite)
    # for the ragged last lane, and runs every size against a pre-filled buffer.
    assert finite[62:66].tolist() == [1, 1, 1, 1]
    assert finite[[59, 60, 66, 67]].tolist() == [0, 0, 0, 0] and finite[[58, 61, 68]].tolist() == [1, 1, 1]
    assert finite[[254, 255, 256]].tolist() == [1, 0, 0]


def test_constants_are_generated():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_g2_cofactor_constants.py")], capture_output=True, text=True,
                         check=True).stdout
    with open(os.path.join(CSRC, "g2_cofactor_constants.inc")) as f:
        assert f.read() == out


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_check_their_arguments():
    lib = pk.load_library()
    pts, _ = synth.g2_subgroup_inputs(3, seed=3)
    offs = synth.g2_inputs(3, seed=3)[2]
    images, finite, jobs = np.zeros((3, 16), np.uint64), np.zeros(3, np.uint8), np.zeros((3, 20), np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(pts=pts, n=3, images=images, finite=finite):
        return lib.bn254s_g2_clear_cofactor_batch(None, _vp(pts), n, _vp(images), _vp(finite))

    # no context: the front-ends need one, whatever else is passed
    assert front() == E_ARG and front(pts=None) == E_ARG and front(images=None) == E_ARG and front(finite=None) == E_ARG
    assert front(n=0) == E_ARG
    u = np.zeros((3, 8), np.uint64)
    assert lib.bn254s_map_to_g2_batch(None, _vp(u), 3, _vp(images)) == E_ARG
    assert lib.bn254s_hash_to_g2_batch(None, _vp(u), 3, 8, _vp(images)) == E_ARG

    def full(ctx=None, params=params, pts=pts, offs=offs, n=3, per_proof=20000, images=images, finite=finite, jobs=jobs, slots=True):
        outs = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_g2_clear_cofactor(ctx, C.byref(params) if params is not None else None, _vp(pts), _vp(offs), n, per_proof,
                                          _vp(images), _vp(finite), _vp(jobs), outs if slots else None)
        return rc, list(outs)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), slots are cleared
    rc, outs = full()
    assert rc == E_UNSUP and outs[0] is None and outs[1] == 1
    assert full(per_proof=16385)[0] == E_UNSUP
    assert full(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    rc, outs = full(per_proof=2)
    assert rc == E_ARG and outs[0] is None and outs[1] is None and outs[2] == 1
    # each invalid argument alone is reported before the shape
    assert full(pts=None)[0] == E_ARG
    assert full(offs=None)[0] == E_ARG
    assert full(images=None)[0] == E_ARG
    assert full(finite=None)[0] == E_ARG
    assert full(slots=False)[0] == E_ARG
    assert full(params=None)[0] == E_ARG
    assert full(n=0)[0] == E_ARG
    assert full(per_proof=0)[0] == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert full(params=bad)[0] == E_ARG
    assert full(jobs=None)[0] == E_UNSUP  # g2_jobs may be NULL
    assert not images.any() and not finite.any() and not jobs.any()


def test_map_to_g2_model_equals_the_proven_pipeline_model():
    """map_to_g2(u) is the point the proven pipeline's model ends with: finish(R + [h](x, y), R) for the jobs g2_jobs derives
    from the Legendre results."""
    us = m2g.inputs(4, seed=11) + [(0, 0), (P - 1, P - 1)]
    _, fx = m2g.fq_exp_jobs(us)
    legendre = [pow(synth.words_to_int(w), (P - 1) // 2, P) for w in fx]
    _, _, goff, pts = m2g.g2_jobs(us, legendre, seed=3)
    picks = set()
    for k, (u, (pt, off)) in enumerate(zip(us, pts)):
        out = synth.g2_add(synth.g2_mul_unreduced(H, pt), off)  # what the G2 trace computes for the job (h, pt, off)
        got = m2g.map_to_g2(u)
        assert got == m2g.finish(synth.g2_points_to_words([out])[0], off), k
        assert synth.g2_on_curve(got) and synth.g2_in_subgroup(got), k
        picks.add(0 if legendre[2 * k] == 1 else 1 if legendre[2 * k + 1] == 1 else 2)
    assert len(picks) >= 2


@pytest.fixture(scope="module")
def oracle_cofactor(inputs):
    """n = 3, per_proof = 4: one 2^16-row G2 proof of the jobs (h, P_i, R_i) made by the CPU oracle (the cut into several proofs
    is the GPU test's, n = 130).  A member, a point of order 10069 and a random twist point: finite 1 / 0 / 1."""
    pts_all, classes, _, images_all = inputs
    pick = [0, 3, 1]
    assert [classes[i][0] for i in pick] == [0, 3, 1] and classes[3] == (3, 10069)
    pts = np.ascontiguousarray(pts_all[pick])
    finite = np.array([images_all[i] is not None for i in pick], np.uint8)
    images = np.zeros((3, 16), np.uint64)
    for j, i in enumerate(pick):
        if images_all[i] is not None:
            images[j] = synth.g2_points_to_words([images_all[i]])[0]
    offs = synth.g2_inputs(3, seed=SEED + 1)[2]
    jobs = np.array([synth._to_words(H) + [int(v) for v in w] for w in pts], np.uint64)
    orc = oracle_lib.load()
    words, outs, _, db = oracle_lib.prove(orc, 1, np.ascontiguousarray(jobs[:, :4]), pts, np.ascontiguousarray(offs))
    proofs = [SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1))]
    return pts, offs, images, finite, jobs, proofs


def test_verify_g2_clear_cofactor_accepts_oracle_proofs(oracle_cofactor):
    pts, offs, images, finite, jobs, proofs = oracle_cofactor
    outs = proofs[0].outputs.reshape(-1, 16)
    assert finite.tolist() == [1, 0, 1] and not images[1].any()
    assert np.array_equal(outs[1], offs[1])  # R + [h]P = R for the point of order 10069: the trace walks through [h]P = O
    for i in (0, 2):
        want = synth.g2_add(synth.g2_from_words(offs[i]), synth.g2_from_words(images[i]))
        assert np.array_equal(outs[i], synth.g2_points_to_words([want])[0])
    pk.verify_g2_clear_cofactor(pts, offs, images, finite, jobs, proofs, 4)


def test_verify_g2_clear_cofactor_rejects_tampering(oracle_cofactor):
    pts, offs, images, finite, jobs, proofs = oracle_cofactor

    def check(match, pts=pts, offs=offs, images=images, finite=finite, jobs=jobs, proofs=proofs, per_proof=4):
        with pytest.raises(pk.VerifyError, match=match):
            pk.verify_g2_clear_cofactor(pts, offs, images, finite, jobs, proofs, per_proof)

    for i in range(3):  # a flipped finite: zeros are no image, an image is not zeros
        flipped = finite.copy()
        flipped[i] ^= 1
        check(rf"^g2_clear_cofactor: image {i} ", finite=flipped)
    moved = images.copy()  # a moved image word: off the curve
    moved[2, 9] ^= 1
    check(r"^g2_clear_cofactor: image 2 ", images=moved)
    other = images.copy()  # another point of the curve as the image
    other[0] = images[2]
    check(r"^g2_clear_cofactor: image 0: ", images=other)
    scal = jobs.copy()  # h - 1 in place of h
    scal[1, 0] -= 1
    check(r"scalar of job 1 ", jobs=scal)
    foreign = jobs.copy()
    foreign[2, 4:] = pts[0]
    check(r"x of job 2 ", jobs=foreign)
    off = pts.copy()  # a point off the curve, consistently in the points and in the jobs
    off[1, 8] += 1
    jobs_off = jobs.copy()
    jobs_off[1, 4:] = off[1]
    check(r"point 1 is not on the twist curve", pts=off, jobs=jobs_off)
    big = pts.copy()
    big[0, :4] = synth._to_words(P)
    check(r"point 0 has a coordinate", pts=big)
    shifted = offs.copy()  # a claimed offset that is not the proof's: the verifier rejects the proof that holds the job
    shifted[2] = offs[0]
    check("^g2_clear_cofactor: proof 0 ", offs=shifted)
    words = proofs[0].words.copy()  # a word of the trace cap changed
    words[0] ^= 1
    tampered = [SimpleNamespace(words=words, degree_bits=proofs[0].degree_bits, outputs=proofs[0].outputs)]
    check("^g2_clear_cofactor: proof 0 ", proofs=tampered)
    check("1 proofs for 3 jobs", per_proof=2)
