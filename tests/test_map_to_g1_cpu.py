"""map_to_g1 / hash_to_fq without a GPU: the constants and the Python definition (tools/map_to_g1_ref.py: the reference's
map_to_g2, src/utils/hash_to_g2.rs:113-148, read over Fq on y^2 = x^3 + 3), the host function bn254s_hash_to_fq, and the
argument checks of bn254s_map_to_g1."""
import ctypes as C
import os

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import gen_map_to_g1_constants
from tools import map_to_g1_ref as m2g1
from tools import map_to_g2_ref as m2g
from tools import synth

P = synth.P
SEED = 0x706C6F6E6B7932 + 11
HALF = (P + 1) // 2  # 1/2


def test_constants():
    assert m2g1.TV4 * m2g1.TV4 % P == P - 12
    assert m2g1.TV4 == pow(P - 12, (P + 1) // 4, P) and m2g1.TV4 % 2 == 0
    assert hex(m2g1.TV4).startswith("0x16789af3") and hex(m2g1.TV4).endswith("dffffffa")
    assert 2 * m2g1.NEG_Z_BY_2 % P == P - 1                                  # nz2 = -1/2
    assert 3 * m2g1.TV6 % P == P - 16 and m2g1.TV6 == (P - 4 * m2g1.g(1)) * pow(3, -1, P) % P  # tv6 = -4 gz/3 = -16/3
    assert m2g1.GZ == m2g1.g(1) == 4
    assert pow(P - 3, (P - 1) // 3, P) != 1                                  # -3 is no cube: g(x) is never zero
    assert pow(P - 1, (P - 1) // 2, P) == P - 1                              # -1 is no square: tv1 tv2 = 0 only for u = +-1/2


def test_committed_constants_are_what_the_generator_prints():
    path = os.path.join(os.path.dirname(pk.__file__), "csrc", "map_to_g1_constants.inc")
    assert open(path).read() == gen_map_to_g1_constants.emit()


@pytest.fixture(scope="module")
def seeded():
    us = m2g1.inputs(256, seed=SEED)
    assert len(us) == 256 and all(u < P for u in us) and us == m2g1.inputs(256)  # the default seed is this one
    return us


def check_image(u):
    x1, x2, x3 = m2g1.candidates(u)
    sq = [m2g1.is_square(m2g1.g(x)) for x in (x1, x2, x3)]
    assert sq[2] or sq[0] or sq[1], u          # g(x3) is a square whenever neither other one is
    x, y = m2g1.map_to_g1(u)
    assert 0 < y < P and x < P and y * y % P == (x * x * x + 3) % P, u  # on the curve
    assert y % 2 == u % 2, u                   # parity(y) == parity(u)
    b = m2g1.branch(u)
    assert x == (x1, x2, x3)[b] and b == (0 if sq[0] else 1 if sq[1] else 2), u  # the first candidate with a square g
    return b


def test_python_map_on_the_crafted_inputs():
    assert m2g1.CRAFTED == (0, 1, P - 1, 2, 3, HALF, P - HALF) and (P - 1) // 2 == P - HALF
    branches = [check_image(u) for u in m2g1.CRAFTED]
    assert branches[0] == 0 and branches[1] == 0  # u = 0 and u = 1 take x1
    assert branches[3] == 1                       # u = 2 takes x2
    assert branches[4] == 2                       # u = 3 takes x3
    for u in (HALF, P - HALF):                    # tv1 tv2 = 0: inv(0) = 0, x1 = x2 = -1/2, and g(-1/2) = 23/8 is a square
        x1, x2, _ = m2g1.candidates(u)
        assert x1 == x2 == P - HALF and m2g1.map_to_g1(u)[0] == P - HALF
        assert m2g1.g(P - HALF) == 23 * pow(8, -1, P) % P and m2g1.is_square(m2g1.g(P - HALF))
    for u in range(1, P, P // 7):                 # tv1 tv2 vanishes nowhere else on a spread of inputs
        tv1 = 4 * u * u % P
        assert ((1 - tv1) * (1 + tv1) % P == 0) == (u in (HALF, P - HALF))


def test_python_map_on_the_seeded_inputs(seeded):
    counts = [0, 0, 0]
    for u in seeded:
        counts[check_image(u)] += 1
    assert min(counts) >= 32, counts  # every branch well covered (126 / 63 / 67 for this seed)


def test_front_end_arrays_follow_the_map(seeded):
    us = list(m2g1.CRAFTED) + seeded[:9]
    pts, flags, jobs = m2g1.front_end(us)
    assert pts.shape == (16, 8) and flags.shape == (32,) and jobs.shape == (32, 8) and np.array_equal(jobs, m2g1.fq_exp_jobs(us))
    for k, u in enumerate(us):
        x1, x2, _ = m2g1.candidates(u)
        assert (synth.words_to_int(pts[k, :4]), synth.words_to_int(pts[k, 4:])) == m2g1.map_to_g1(u)
        for i, xc in enumerate((x1, x2)):
            assert synth.words_to_int(jobs[2 * k + i, :4]) == (P - 1) // 2
            assert synth.words_to_int(jobs[2 * k + i, 4:]) == m2g1.g(xc)
            assert flags[2 * k + i] == m2g1.is_square(m2g1.g(xc))


@pytest.mark.parametrize("ln", [0, 1, 7, 8, 9, 20])
def test_hash_to_fq_host_function(ln):
    from plonky2_bn254_amd import lib as L
    lib = L.load_library()
    rng = synth.Xoshiro256ss(5 + ln)
    inp = np.array([rng.next_u64() % m2g.GL_P for _ in range(ln)], dtype=np.uint64)
    out, out2 = np.full(4, 7, np.uint64), np.zeros(8, np.uint64)
    assert lib.bn254s_hash_to_fq(L._ptr(inp) if ln else None, ln, L._ptr(out)) == 0
    assert lib.bn254s_hash_to_fq2(L._ptr(inp) if ln else None, ln, L._ptr(out2)) == 0
    got = synth.words_to_int(out)
    assert got == m2g1.hash_to_fq(inp.tolist()) and got < P
    assert np.array_equal(out, out2[:4])  # hash_to_fq(v) == hash_to_fq2(v).c0
    assert got == m2g.hash_to_fq2(inp.tolist())[0]


def test_hash_to_fq_checks_its_arguments():
    from plonky2_bn254_amd import lib as L
    lib = L.load_library()
    inp, out = np.zeros(3, np.uint64), np.zeros(4, np.uint64)
    assert lib.bn254s_hash_to_fq(None, 3, L._ptr(out)) == -1 and lib.bn254s_hash_to_fq(L._ptr(inp), 3, None) == -1
    assert lib.bn254s_hash_to_fq_batch(None, L._ptr(inp), 1, 3, L._ptr(out)) == -1
    assert lib.bn254s_hash_to_g1_batch(None, L._ptr(inp), 1, 3, L._ptr(np.zeros(8, np.uint64))) == -1


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_map_to_g1_checks_its_arguments():
    lib = pk.load_library()
    u = m2g1.to_words(m2g1.inputs(3))
    pts, flags, jobs = np.zeros((3, 8), np.uint64), np.zeros(6, np.uint8), np.zeros((6, 8), np.uint64)
    params = pk.default_params()
    E_ARG, E_UNSUP = -1, -5

    def front(u=u, n=3, pts=pts, flags=flags, jobs=jobs):
        return lib.bn254s_map_to_g1_batch(None, _vp(u), n, _vp(pts), _vp(flags), _vp(jobs))

    # no context: the front-end needs one, whatever else is passed
    assert front() == E_ARG and front(flags=None, jobs=None) == E_ARG
    assert front(u=None) == E_ARG and front(pts=None) == E_ARG and front(n=0) == E_ARG

    def full(ctx=None, params=params, u=u, n=3, per_proof=16385, pts=pts, flags=flags, jobs=jobs, slots=True):
        outs = (C.c_void_p * 5)(*([1] * 5))
        rc = lib.bn254s_map_to_g1(ctx, C.byref(params) if params is not None else None, _vp(u), n, per_proof, _vp(pts), _vp(flags),
                                  _vp(jobs), outs if slots else None)
        return rc, list(outs)

    # every argument but the context is valid: the shape check answers first (per_proof above 16384), every slot is cleared
    rc, outs = full()
    assert rc == E_UNSUP and outs[0] is None and outs[1] == 1   # 6 jobs: one slot
    rc, outs = full(per_proof=20000)
    assert rc == E_UNSUP and outs[0] is None and outs[1] == 1
    assert full(per_proof=16384)[0] == E_ARG  # a valid shape without a context
    rc, outs = full(per_proof=2)
    assert rc == E_ARG and outs[:3] == [None] * 3 and outs[3] == 1  # 6 jobs of 2 per proof: three slots
    # each invalid argument alone is reported before the shape
    assert full(u=None)[0] == E_ARG
    assert full(pts=None)[0] == E_ARG
    assert full(slots=False)[0] == E_ARG
    assert full(params=None)[0] == E_ARG
    assert full(n=0)[0] == E_ARG
    assert full(n=1 << 31)[0] == E_ARG and full(n=(1 << 32) + 3)[0] == E_ARG  # 2n must stay below 2^32
    assert full(per_proof=0)[0] == E_ARG
    bad = pk.default_params()
    bad.struct_size += 4
    assert full(params=bad)[0] == E_ARG
    assert full(flags=None, jobs=None)[0] == E_UNSUP  # sq_flags and fq_jobs may be NULL
    assert not pts.any() and not flags.any() and not jobs.any()
