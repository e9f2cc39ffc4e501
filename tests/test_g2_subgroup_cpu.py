"""G2 subgroup check without a GPU: the numbers the kernel's argument rests on (the cofactor of the twist, the BN parameter, the
soundness condition of the endomorphism criterion, the ladder's prefixes), the Python reference (tools/synth.py: the definition
[r]P = O and, independently, the criterion with psi), the inputs of the GPU parity test and what they cover, the generated
constants, the argument checks of the two C entry points, and verify_g2_subgroup on G2 proofs made by the CPU oracle."""
import ctypes as C
import math
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import synth

P, R, X0 = synth.P, synth.R_ORDER, synth.X0
H, PRIMES = synth.G2_COFACTOR, synth.G2_COFACTOR_PRIMES
SEED = 41  # the seed of the GPU parity test (tests/test_gpu_g2_subgroup.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def inputs():
    pts, flags, classes = synth.g2_subgroup_inputs(257, seed=SEED, with_classes=True)
    return pts, flags, classes, [synth.g2_from_words(w) for w in pts]


def test_curve_numbers():
    assert P == 36 * X0**4 + 36 * X0**3 + 24 * X0**2 + 6 * X0 + 1 and X0.bit_length() == 63 and bin(X0).count("1") == 28
    assert H == 2 * P - R and math.prod(PRIMES) == H == 10069 * 5864401 * 1875725156269 * PRIMES[3]
    assert PRIMES[:3] == (10069, 5864401, 1875725156269) and PRIMES[3].bit_length() == 178
    for f in PRIMES + (R,):  # Fermat tests to a few bases: the factors pass as primes
        assert all(pow(a, f - 1, f) == 1 for a in (2, 3, 5, 7, 11, 13))
    assert (P - 6 * X0 * X0) % R == 0  # p = 6 x0^2 (mod r)
    assert H % 2 == 1 and R % 2 == 1   # odd order: no point with y = 0


def test_criterion_is_sound_on_the_whole_twist():
    """a(psi) P = O with a(X) = (x0 + 1) + x0 X + x0 X^2 - 2 x0 X^3 and chi(psi) = psi^2 - t psi + p = 0: modulo chi, a is
    c0 + c1 X, and its norm N = c0^2 + c0 c1 t + c1^2 p = (c0 + c1 psi)(c0 + c1 (t - psi)) kills P.  So does #E'(Fq2) = r h.
    gcd(N, r h) == r: every P that passes has [r]P = O.  a(p) = 0 (mod r): every member passes (psi acts as p on it)."""
    t = 6 * X0 * X0 + 1
    assert P + 1 - t == R
    a = [X0 + 1, X0, X0, -2 * X0]
    assert sum(c * pow(P, i, R) for i, c in enumerate(a)) % R == 0
    c = a[:]
    for d in (3, 2):  # X^d = t X^(d-1) - p X^(d-2)
        c[d - 1] += c[d] * t
        c[d - 2] -= c[d] * P
    c0, c1 = c[0], c[1]
    norm = c0 * c0 + c0 * c1 * t + c1 * c1 * P
    assert math.gcd(norm, R * H) == R


def test_ladder_meets_no_exceptional_case():
    """The accumulator [k]P over the prefixes k of x0: 2k is never 0, 1 or -1 modulo a prime of r h, so [2k]P is never O, P or
    -P for a point of any order d > 1 dividing r h (csrc/g2_subgroup.hip)."""
    bits, k = bin(X0)[2:], 1
    for b in bits[1:]:
        for f in PRIMES + (R,):
            assert 2 * k % f not in (0, 1, f - 1), (k, f)
        k = 2 * k + int(b)
    assert k == X0


def test_psi():
    assert synth.f2_pow(synth.PSI_X, 3) == synth.f2_pow(synth.PSI_Y, 2) == synth.f2_pow(synth.XI, P - 1)
    _, pts, _ = synth.g2_inputs(3, seed=SEED)
    for w in pts:  # members: psi is multiplication by p
        q = synth.g2_from_words(w)
        assert synth.g2_on_curve(synth.psi(q)) and synth.psi(q) == synth.g2_mul(P % R, q)
    rng = synth.Xoshiro256ss(SEED)
    t = 6 * X0 * X0 + 1
    for _ in range(3):  # any point of the twist: on the curve again, and psi^2 - t psi + p = 0
        q = synth._g2_random_twist_point(rng)
        s1, s2 = synth.psi(q), synth.psi(synth.psi(q))
        assert synth.g2_on_curve(s1) and s1 != synth.g2_mul_unreduced(P % R, q)
        assert synth.g2_add_complete(s2, synth.g2_mul_unreduced(P, q)) == synth.g2_mul_unreduced(t, s1)
    assert synth.psi(None) is None


def test_definition_and_criterion_agree_on_the_parity_inputs(inputs):
    pts, flags, classes, points = inputs
    assert pts.shape == (257, 16) and pts.dtype == np.uint64 and flags.shape == (257,) and flags.dtype == np.uint8
    for i, (pt, fl) in enumerate(zip(points, flags)):
        assert max(pt[0] + pt[1]) < P and synth.g2_on_curve(pt), i
        assert synth.g2_in_subgroup(pt) == synth.g2_in_subgroup_psi(pt) == bool(fl), (i, classes[i])
    short = synth.g2_subgroup_inputs(9, seed=SEED)  # prefix-stable
    assert np.array_equal(short[0], pts[:9]) and np.array_equal(short[1], flags[:9])


def test_parity_inputs_cover_every_class(inputs):
    pts, flags, classes, points = inputs
    assert [c for c, _ in classes] == [i % 7 for i in range(257)] and len(synth.G2_SUBGROUP_CLASSES) == 7
    assert flags[:7].tolist() == [1, 0, 1, 0, 0, 0, 1]
    for n in range(2, 258):  # every prefix of length >= 2 holds both flag values
        assert 0 < int(flags[:n].sum()) < n
    orders = [d for c, d in classes if c == 3]
    assert set(orders) == set(PRIMES) and orders[:4] == list(PRIMES)
    for (c, d), pt in zip(classes[:70], points[:70]):  # the orders are what the class says
        if c in (3, 4):
            assert synth.g2_mul_unreduced(d, pt) is None
            assert all(synth.g2_mul_unreduced(d // f, pt) is not None for f in PRIMES if d % f == 0)
        elif c == 5:  # r kills the member part, 10069 the other: neither alone kills the sum
            assert synth.g2_mul_unreduced(R, pt) is not None and synth.g2_mul_unreduced(d, pt) is not None
            assert synth.g2_mul_unreduced(R * d, pt) is None
        elif c == 2:  # a member that does not come from the generator by a known scalar
            assert synth.g2_mul_unreduced(R, pt) is None
    assert [d for c, d in classes if c == 4][0] == 10069 * 5864401
    # the block edges of a 64-lane launch: a member and a non-member on the two sides of lane 63 | 64, and both values among
    # 62..65 and among the edge lanes taken together (255 and 256, classes 3 and 4 of the cycle, are both non-members: the
    # GPU test therefore also runs the ragged last lane against a pre-filled buffer)
    assert flags[63] == 1 and flags[64] == 0
    assert set(flags[62:66].tolist()) == {0, 1} and set(flags[[62, 63, 64, 65, 255, 256]].tolist()) == {0, 1}
    assert flags[255] == 0 and flags[256] == 0


def test_constants_are_generated():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_g2_subgroup_constants.py")], capture_output=True, text=True,
                         check=True).stdout
    with open(os.path.join(ROOT, "plonky2_bn254_amd", "csrc", "g2_subgroup_constants.inc")) as f:
        assert f.read() == out


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_check_their_arguments():
    lib = pk.load_library()
    pts, _ = synth.g2_subgroup_inputs(3, seed=3)
    offs = synth.g2_inputs(3, seed=3)[2]
    flags, jobs = np.zeros(3, np.uint8), np.zeros((3, 20), np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(pts=pts, n=3, flags=flags):
        return lib.bn254s_g2_subgroup_check_batch(None, _vp(pts), n, _vp(flags))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(pts=None) == E_ARG and front(flags=None) == E_ARG and front(n=0) == E_ARG

    def full(ctx=None, params=params, pts=pts, offs=offs, n=3, per_proof=20000, flags=flags, jobs=jobs, slots=True):
        outs = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_g2_subgroup_check(ctx, C.byref(params) if params is not None else None, _vp(pts), _vp(offs), n, per_proof,
                                          _vp(flags), _vp(jobs), outs if slots else None)
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
    assert full(flags=None)[0] == E_ARG
    assert full(slots=False)[0] == E_ARG
    assert full(params=None)[0] == E_ARG
    assert full(n=0)[0] == E_ARG
    assert full(per_proof=0)[0] == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert full(params=bad)[0] == E_ARG
    assert full(jobs=None)[0] == E_UNSUP  # g2_jobs may be NULL
    assert not flags.any() and not jobs.any()


@pytest.fixture(scope="module")
def oracle_subgroup(inputs):
    """n = 3, per_proof = 4: one 2^16-row G2 proof of the jobs (r, P_i, R_i) made by the CPU oracle (the cut into several
    proofs is the GPU test's, n = 130).  A member (k G2_GEN), a
    point of order 10069 and a member plus a point of order 10069: flags 1 / 0 / 0."""
    pts_all, flags_all, classes, _ = inputs
    pick = [0, 3, 5]
    assert [classes[i] for i in pick] == [(0, 1), (3, 10069), (5, 10069)]
    pts, flags = np.ascontiguousarray(pts_all[pick]), np.ascontiguousarray(flags_all[pick])
    offs = synth.g2_inputs(3, seed=SEED + 1)[2]
    jobs = np.array([synth._to_words(R) + [int(v) for v in w] for w in pts], np.uint64)
    orc = oracle_lib.load()
    proofs = []
    words, outs, _, db = oracle_lib.prove(orc, 1, np.ascontiguousarray(jobs[:, :4]), pts, np.ascontiguousarray(offs))
    proofs.append(SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1)))
    return pts, offs, flags, jobs, proofs


def test_verify_g2_subgroup_accepts_oracle_proofs(oracle_subgroup):
    pts, offs, flags, jobs, proofs = oracle_subgroup
    outs = np.concatenate([pr.outputs.reshape(-1, 16) for pr in proofs])
    assert flags.tolist() == [1, 0, 0]
    assert np.array_equal(outs[0], offs[0])  # R + [r]P = R for the member: the trace walks through [r]P = O
    for i in (1, 2):  # ... and Python's R + [r]P for the others
        want = synth.g2_add(synth.g2_from_words(offs[i]), synth.g2_mul_unreduced(R, synth.g2_from_words(pts[i])))
        assert np.array_equal(outs[i], synth.g2_points_to_words([want])[0]) and not np.array_equal(outs[i], offs[i])
    pk.verify_g2_subgroup(pts, offs, flags, jobs, proofs, 4)


def test_verify_g2_subgroup_rejects_tampering(oracle_subgroup):
    pts, offs, flags, jobs, proofs = oracle_subgroup
    for i in range(3):
        flipped = flags.copy()
        flipped[i] ^= 1
        with pytest.raises(pk.VerifyError, match=rf"^g2_subgroup: flag {i} "):
            pk.verify_g2_subgroup(pts, offs, flipped, jobs, proofs, 4)
    scal = jobs.copy()  # r - 1 in place of r
    scal[1, 0] -= 1
    with pytest.raises(pk.VerifyError, match=r"scalar of job 1 "):
        pk.verify_g2_subgroup(pts, offs, flags, scal, proofs, 4)
    other = jobs.copy()
    other[2, 4:] = pts[0]
    with pytest.raises(pk.VerifyError, match=r"x of job 2 "):
        pk.verify_g2_subgroup(pts, offs, flags, other, proofs, 4)
    off = pts.copy()  # a point off the curve, consistently in the points and in the jobs
    off[1, 8] += 1
    jobs_off = jobs.copy()
    jobs_off[1, 4:] = off[1]
    with pytest.raises(pk.VerifyError, match=r"point 1 is not on the twist curve"):
        pk.verify_g2_subgroup(off, offs, flags, jobs_off, proofs, 4)
    big = pts.copy()
    big[0, :4] = synth._to_words(P)
    with pytest.raises(pk.VerifyError, match=r"point 0 has a coordinate"):
        pk.verify_g2_subgroup(big, offs, flags, jobs, proofs, 4)
    # a claimed offset that is not the proof's: the verifier rejects the proof that holds the job
    moved = offs.copy()
    moved[2] = offs[0]
    with pytest.raises(pk.VerifyError, match="^g2_subgroup: proof 0 "):
        pk.verify_g2_subgroup(pts, moved, flags, jobs, proofs, 4)
    words = proofs[0].words.copy()  # a word of the trace cap changed
    words[0] ^= 1
    tampered = [SimpleNamespace(words=words, degree_bits=proofs[0].degree_bits, outputs=proofs[0].outputs)]
    with pytest.raises(pk.VerifyError, match="^g2_subgroup: proof 0 "):
        pk.verify_g2_subgroup(pts, offs, flags, jobs, tampered, 4)
    with pytest.raises(pk.VerifyError, match="1 proofs for 3 jobs"):
        pk.verify_g2_subgroup(pts, offs, flags, jobs, proofs, 2)
