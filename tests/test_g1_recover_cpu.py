"""G1 point recovery from x without a GPU (reference src/curves/g1.rs:76-95, src/fields/recover.rs): the Python reference, the
argument checks of the two C entry points, and verify_g1_recover on Fq-exp proofs made by the CPU oracle."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tests import oracle_lib
from tools import synth

P = synth.P


def test_python_reference():
    assert pow(P - 3, (P - 1) // 3, P) != 1  # -3 is not a cube: x^3 + 3 is never zero, "square" and "Legendre symbol 1" agree
    assert synth.g1_recover_from_x(1) == synth.G1_GEN == (1, 2)
    assert synth.g1_recover_from_x(0) is None and synth.g1_recover_from_x(4) is None
    for x in (1, 2, P - 1, P - 2):
        pt = synth.g1_recover_from_x(x)
        assert pt is not None and pt[0] == x and pt[1] < P and pt[1] % 2 == 0 and pt[1] * pt[1] % P == (x ** 3 + 3) % P
    _, pts, _ = synth.g1_inputs(3, seed=17)
    for w in pts:
        x, y = synth.words_to_int(w[:4]), synth.words_to_int(w[4:])
        assert synth.g1_recover_from_x(x) in ((x, y), (x, P - y))


def test_recover_inputs_start_with_the_edge_cases():
    xs = synth.g1_recover_inputs(12, seed=31)
    assert xs.shape == (12, 4) and xs.dtype == np.uint64
    vals = [synth.words_to_int(w) for w in xs]
    assert vals[:6] == [0, 1, 2, 4, P - 1, P - 2] and all(v < P for v in vals)
    assert vals[6:9] == [synth.words_to_int(w[:4]) for w in synth.g1_inputs(3, seed=31)[1]]
    rng = synth.Xoshiro256ss(31)
    assert vals[9:] == [rng.next_u256() % P for _ in range(3)]
    assert np.array_equal(synth.g1_recover_inputs(5, seed=31), xs[:5])
    # both flag values cover at least a quarter of the 257 inputs of the GPU parity test
    flags = [synth.g1_recover_from_x(synth.words_to_int(w)) is not None for w in synth.g1_recover_inputs(257, seed=31)]
    assert min(sum(flags), 257 - sum(flags)) >= 65


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_check_their_arguments():
    lib = pk.load_library()
    xs = synth.g1_recover_inputs(3, seed=3)
    pts, flags, jobs = np.zeros((3, 8), np.uint64), np.zeros(3, np.uint8), np.zeros((3, 8), np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(xs=xs, n=3, pts=pts, flags=flags, jobs=jobs):
        return lib.bn254s_g1_recover_from_x_batch(None, _vp(xs), n, _vp(pts), _vp(flags), _vp(jobs))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(jobs=None) == E_ARG
    assert front(xs=None) == E_ARG and front(pts=None) == E_ARG and front(flags=None) == E_ARG and front(n=0) == E_ARG

    def full(ctx=None, params=params, xs=xs, n=3, per_proof=20000, pts=pts, flags=flags, jobs=jobs, slots=True):
        outs = (C.c_void_p * 4)(*([1] * 4))
        rc = lib.bn254s_g1_recover_from_x(ctx, C.byref(params) if params is not None else None, _vp(xs), n, per_proof, _vp(pts),
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
    assert not pts.any() and not flags.any() and not jobs.any()


@pytest.fixture(scope="module")
def oracle_recover():
    """n = 3, per_proof = 2: two 2^16-row Fq-exp proofs made by the CPU oracle from the Python-derived Legendre jobs.
    x = 1 and p - 2 are recoverable, x = 4 is not."""
    vals = [1, 4, P - 2]
    xs = np.array([synth._to_words(v) for v in vals], np.uint64)
    rec = [synth.g1_recover_from_x(v) for v in vals]
    flags = np.array([r is not None for r in rec], np.uint8)
    assert list(flags) == [1, 0, 1]
    points = np.array([synth._to_words(v) + synth._to_words(r[1] if r else 0) for v, r in zip(vals, rec)], np.uint64)
    jobs = np.array([synth._to_words((P - 1) // 2) + synth._to_words((v ** 3 + 3) % P) for v in vals], np.uint64)
    orc = oracle_lib.load()
    proofs = []
    for lo, hi in ((0, 2), (2, 3)):
        words, outs, _, db = oracle_lib.prove(orc, 2, np.ascontiguousarray(jobs[lo:hi, :4]), np.ascontiguousarray(jobs[lo:hi, 4:]))
        proofs.append(SimpleNamespace(words=words, degree_bits=db, outputs=outs.reshape(-1)))
    return xs, points, flags, jobs, proofs


def test_verify_g1_recover_accepts_oracle_proofs(oracle_recover):
    xs, points, flags, jobs, proofs = oracle_recover
    legendre = [synth.words_to_int(o) for pr in proofs for o in pr.outputs.reshape(-1, 4)]
    assert legendre == [1, P - 1, 1]
    pk.verify_g1_recover(xs, points, flags, jobs, proofs, 2)


def test_verify_g1_recover_rejects_tampering(oracle_recover):
    xs, points, flags, jobs, proofs = oracle_recover
    for i in range(3):
        flipped = flags.copy()
        flipped[i] ^= 1
        with pytest.raises(pk.VerifyError, match=rf"flag {i} "):
            pk.verify_g1_recover(xs, points, flipped, jobs, proofs, 2)
    odd = points.copy()
    odd[2, 4:] = synth._to_words(P - synth.words_to_int(points[2, 4:]))  # the other root: on the curve, but odd
    with pytest.raises(pk.VerifyError, match=r"point 2 "):
        pk.verify_g1_recover(xs, odd, flags, jobs, proofs, 2)
    nonzero = points.copy()
    nonzero[1, 4] = 2
    with pytest.raises(pk.VerifyError, match=r"point 1 "):
        pk.verify_g1_recover(xs, nonzero, flags, jobs, proofs, 2)
    off = jobs.copy()
    off[2, 4] += 1
    with pytest.raises(pk.VerifyError, match=r"x of job 2 "):
        pk.verify_g1_recover(xs, points, flags, off, proofs, 2)
    scal = jobs.copy()
    scal[1, 0] += 1
    with pytest.raises(pk.VerifyError, match=r"scalar of job 1 "):
        pk.verify_g1_recover(xs, points, flags, scal, proofs, 2)
    # consistent jobs and flags, but a word of proof 1's trace cap changed: the verifier rejects that proof
    words = proofs[1].words.copy()
    words[0] ^= 1
    tampered = [proofs[0], SimpleNamespace(words=words, degree_bits=proofs[1].degree_bits, outputs=proofs[1].outputs)]
    with pytest.raises(pk.VerifyError, match="proof 1 "):
        pk.verify_g1_recover(xs, points, flags, jobs, tampered, 2)
