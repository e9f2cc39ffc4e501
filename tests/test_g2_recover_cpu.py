"""G2 point recovery from x without a GPU (reference src/curves/g2.rs:42-54, src/fields/fq2.rs:209-241, src/fields/sgn.rs:20-27):
the Python reference, the inputs of the GPU parity test and what they cover, the argument checks of the two C entry points, and
verify_g2_recover on Fq-exp proofs made by the CPU oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import map_to_g2_ref, synth

P = synth.P
SEED = 31  # the seed of the GPU parity test (tests/test_gpu_g2_recover.py), the one the G1 tests use


def _x(w):
    return (synth.words_to_int(w[:4]), synth.words_to_int(w[4:]))


def _f2_pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = synth.f2_mul(r, r)
        if bit == "1":
            r = synth.f2_mul(r, a)
    return r


def _real_g_x(c):
    """x = (sqrt((c^3 - b'.c1)/(3c)), c): x^3 + b' has no imaginary part."""
    s = (c ** 3 - synth.G2_B[1]) * pow(3 * c, -1, P) % P
    x0 = pow(s, (P + 1) // 4, P)
    assert x0 * x0 % P == s
    return (x0, c)


def test_python_reference():
    # -b' is not a cube in Fq2: x^3 + b' is never zero, and neither is its norm (-1 is a non-residue of Fq)
    assert _f2_pow(((-synth.G2_B[0]) % P, (-synth.G2_B[1]) % P), (P * P - 1) // 3) != (1, 0)
    assert P % 4 == 3
    xs, sgns = synth.g2_recover_inputs(40, seed=5)
    found = 0
    for w, s in zip(xs, sgns):
        x = _x(w)
        g = synth.g2_rhs(x)
        assert g != (0, 0)
        pt = synth.g2_recover_from_x(x, int(s))
        square = pow(map_to_g2_ref.f2_norm(g), (P - 1) // 2, P) == 1
        assert (pt is not None) == square
        if pt is None:
            assert synth.g2_recover_from_x(x, 1 - int(s)) is None
            continue
        found += 1
        y = pt[1]
        assert pt[0] == x and y[0] < P and y[1] < P and synth.f2_mul(y, y) == g and synth.f2_sgn(y) == bool(s)
        other = synth.g2_recover_from_x(x, 1 - int(s))  # flipping sgn negates y
        assert other == (x, ((-y[0]) % P, (-y[1]) % P)) and synth.f2_sgn(other[1]) != bool(s)
    assert 10 <= found <= 35
    _, pts, _ = synth.g2_inputs(3, seed=17)
    for w in pts:  # the x of a curve point gives back y with the sign of y, -y with the other
        x, y = synth.g2_from_words(w)
        assert synth.g2_recover_from_x(x, synth.f2_sgn(y)) == (x, y)
        assert synth.g2_recover_from_x(x, not synth.f2_sgn(y)) == (x, ((-y[0]) % P, (-y[1]) % P))
    # sgn.rs:20-27: the parity of c0, or of c1 when c0 is zero
    assert synth.f2_sgn((1, 0)) and not synth.f2_sgn((2, 1)) and synth.f2_sgn((0, 1)) and not synth.f2_sgn((0, 2))


def test_recover_inputs_start_with_the_edge_cases():
    xs, sgns = synth.g2_recover_inputs(15, seed=SEED)
    assert xs.shape == (15, 8) and xs.dtype == np.uint64 and sgns.shape == (15,) and sgns.dtype == np.uint8
    vals = [_x(w) for w in xs]
    assert all(a < P and b < P for a, b in vals) and set(sgns.tolist()) <= {0, 1}
    assert vals[:4] == [(0, 0), (1, 0), (0, 1), (P - 1, P - 1)]
    assert vals[4:6] == [_real_g_x(2), _real_g_x(7)]
    g2, g7 = synth.g2_rhs(vals[4]), synth.g2_rhs(vals[5])
    assert g2[1] == 0 and g7[1] == 0 and map_to_g2_ref.fq_is_square(g2[0]) and not map_to_g2_ref.fq_is_square(g7[0])
    y2, y7 = synth.g2_recover_from_x(vals[4], int(sgns[4]))[1], synth.g2_recover_from_x(vals[5], int(sgns[5]))[1]
    assert y2[1] == 0 and y2[0] != 0 and y7[0] == 0 and y7[1] != 0  # roots (t, 0) and (0, t): both flags are 1
    assert sgns[5] == 1 and y7[1] & 1  # the sign of (0, t) is the parity of c1
    known = [synth.g2_from_words(w) for w in synth.g2_inputs(3, seed=SEED)[1]]
    assert vals[6:9] == [x for x, _ in known] and sgns[6:9].tolist() == [int(synth.f2_sgn(y)) for _, y in known]
    assert vals[9:12] == [x for x, _ in known] and sgns[9:12].tolist() == [1 - int(synth.f2_sgn(y)) for _, y in known]
    rng = synth.Xoshiro256ss(SEED)
    for i in range(12, 15):
        assert vals[i] == (rng.next_u256() % P, rng.next_u256() % P) and sgns[i] == rng.next_u256() & 1
    short = synth.g2_recover_inputs(5, seed=SEED)  # prefix-stable
    assert np.array_equal(short[0], xs[:5]) and np.array_equal(short[1], sgns[:5])


def test_parity_inputs_cover_every_branch():
    """The 257 inputs of the GPU parity test: both flag values, both branches of the second exponentiation (delta a square of
    Fq or not), both wanted signs and a root with c0 == 0, so that the GPU test cannot pass on a one-sided sample."""
    xs, sgns = synth.g2_recover_inputs(257, seed=SEED)
    flags, delta_square, c0_zero = [], [], 0
    for w, s in zip(xs, sgns):
        x = _x(w)
        pt = synth.g2_recover_from_x(x, int(s))
        flags.append(pt is not None)
        if pt is None:
            continue
        g = synth.g2_rhs(x)
        alpha = pow(map_to_g2_ref.f2_norm(g), (P + 1) // 4, P)
        delta = g[0] if g[1] == 0 else (alpha + g[0]) * ((P + 1) // 2) % P
        delta_square.append(map_to_g2_ref.fq_is_square(delta))
        c0_zero += pt[1][0] == 0
    assert min(sum(flags), 257 - sum(flags)) >= 65
    assert min(sum(delta_square), len(delta_square) - sum(delta_square)) >= 16
    assert min(int(sgns.sum()), 257 - int(sgns.sum())) >= 65
    assert c0_zero >= 1


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_check_their_arguments():
    lib = pk.load_library()
    xs, sgns = synth.g2_recover_inputs(3, seed=3)
    pts, flags, jobs = np.zeros((3, 16), np.uint64), np.zeros(3, np.uint8), np.zeros((3, 8), np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(xs=xs, sgns=sgns, n=3, pts=pts, flags=flags, jobs=jobs):
        return lib.bn254s_g2_recover_from_x_batch(None, _vp(xs), _vp(sgns), n, _vp(pts), _vp(flags), _vp(jobs))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(jobs=None) == E_ARG and front(sgns=None) == E_ARG
    assert front(xs=None) == E_ARG and front(pts=None) == E_ARG and front(flags=None) == E_ARG and front(n=0) == E_ARG

    def full(ctx=None, params=params, xs=xs, sgns=sgns, n=3, per_proof=20000, pts=pts, flags=flags, jobs=jobs, slots=True):
        outs = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_g2_recover_from_x(ctx, C.byref(params) if params is not None else None, _vp(xs), _vp(sgns), n, per_proof,
                                          _vp(pts), _vp(flags), _vp(jobs), outs if slots else None)
        return rc, list(outs)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), slots are cleared
    rc, outs = full()
    assert rc == E_UNSUP and outs[0] is None and outs[1] == 1
    assert full(per_proof=16385)[0] == E_UNSUP
    assert full(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    rc, outs = full(per_proof=2)
    assert rc == E_ARG and outs[0] is None and outs[1] is None and outs[2] == 1
    # each invalid argument alone is reported before the shape
    assert full(xs=None)[0] == E_ARG
    assert full(pts=None)[0] == E_ARG
    assert full(flags=None)[0] == E_ARG
    assert full(slots=False)[0] == E_ARG
    assert full(params=None)[0] == E_ARG
    assert full(n=0)[0] == E_ARG
    assert full(per_proof=0)[0] == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert full(params=bad)[0] == E_ARG
    assert full(jobs=None)[0] == E_UNSUP  # fq_jobs may be NULL
    assert full(sgns=None)[0] == E_UNSUP  # sgns may be NULL
    assert not pts.any() and not flags.any() and not jobs.any()


@pytest.fixture(scope="module")
def oracle_recover():
    """n = 3, per_proof = 2: two 2^16-row Fq-exp proofs made by the CPU oracle from the Python-derived Legendre jobs.  Flags
    1 / 0 / 1: the x with a real g and root (0, t) wanted odd, a random x off the curve, the x of a g2_inputs point wanted with
    the sign opposite to its y."""
    xs_all, sgns_all = synth.g2_recover_inputs(257, seed=SEED)
    off = next(i for i in range(12, 257) if synth.g2_recover_from_x(_x(xs_all[i]), 0) is None)
    pick = [5, off, 9]
    xs, sgns = np.ascontiguousarray(xs_all[pick]), np.ascontiguousarray(sgns_all[pick])
    rec = [synth.g2_recover_from_x(_x(w), int(s)) for w, s in zip(xs, sgns)]
    flags = np.array([r is not None for r in rec], np.uint8)
    assert list(flags) == [1, 0, 1]
    points = np.array([list(w) + synth._to_words(r[1][0] if r else 0) + synth._to_words(r[1][1] if r else 0) for w, r in zip(xs, rec)],
                      np.uint64)
    jobs = np.array([synth._to_words((P - 1) // 2) + synth._to_words(map_to_g2_ref.f2_norm(synth.g2_rhs(_x(w)))) for w in xs], np.uint64)
    orc = oracle_lib.load()
    proofs = []
    for lo, hi in ((0, 2), (2, 3)):
        words, outs, _, db = oracle_lib.prove(orc, 2, np.ascontiguousarray(jobs[lo:hi, :4]), np.ascontiguousarray(jobs[lo:hi, 4:]))
        proofs.append(SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1)))
    return xs, sgns, points, flags, jobs, proofs


def test_verify_g2_recover_accepts_oracle_proofs(oracle_recover):
    xs, sgns, points, flags, jobs, proofs = oracle_recover
    legendre = [synth.words_to_int(o) for pr in proofs for o in pr.outputs.reshape(-1, 4)]
    assert legendre == [1, P - 1, 1]
    pk.verify_g2_recover(xs, sgns, points, flags, jobs, proofs, 2)


def test_verify_g2_recover_rejects_tampering(oracle_recover):
    xs, sgns, points, flags, jobs, proofs = oracle_recover
    for i in range(3):
        flipped = flags.copy()
        flipped[i] ^= 1
        with pytest.raises(pk.VerifyError, match=rf"flag {i} "):
            pk.verify_g2_recover(xs, sgns, points, flipped, jobs, proofs, 2)
    other = points.copy()  # the other root: on the curve, with the sign that was not asked for
    other[2, 8:12] = synth._to_words((-synth.words_to_int(points[2, 8:12])) % P)
    other[2, 12:] = synth._to_words((-synth.words_to_int(points[2, 12:])) % P)
    with pytest.raises(pk.VerifyError, match=r"sign 2 "):
        pk.verify_g2_recover(xs, sgns, other, flags, jobs, proofs, 2)
    swapped = sgns.copy()  # ... and the right root for the other wanted sign
    swapped[0] ^= 1
    with pytest.raises(pk.VerifyError, match=r"sign 0 "):
        pk.verify_g2_recover(xs, swapped, points, flags, jobs, proofs, 2)
    wrong = points.copy()  # one coordinate of y changed: no root at all
    wrong[2, 12] ^= 2
    with pytest.raises(pk.VerifyError, match=r"point 2 "):
        pk.verify_g2_recover(xs, sgns, wrong, flags, jobs, proofs, 2)
    nonzero = points.copy()
    nonzero[1, 12] = 2
    with pytest.raises(pk.VerifyError, match=r"point 1 "):
        pk.verify_g2_recover(xs, sgns, nonzero, flags, jobs, proofs, 2)
    off = jobs.copy()
    off[2, 4] += 1
    with pytest.raises(pk.VerifyError, match=r"x of job 2 "):
        pk.verify_g2_recover(xs, sgns, points, flags, off, proofs, 2)
    scal = jobs.copy()
    scal[1, 0] += 1
    with pytest.raises(pk.VerifyError, match=r"scalar of job 1 "):
        pk.verify_g2_recover(xs, sgns, points, flags, scal, proofs, 2)
    # consistent jobs and flags, but a word of proof 1's trace cap changed: the verifier rejects that proof
    words = proofs[1].words.copy()
    words[0] ^= 1
    tampered = [proofs[0], SimpleNamespace(words=words, degree_bits=proofs[1].degree_bits, outputs=proofs[1].outputs)]
    with pytest.raises(pk.VerifyError, match="proof 1 "):
        pk.verify_g2_recover(xs, sgns, points, flags, jobs, tampered, 2)
