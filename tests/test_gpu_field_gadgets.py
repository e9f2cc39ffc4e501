"""The field gadgets on the GPU (csrc/root_front.hip, csrc/field_gadgets.hip; reference src/fields/: is_square, sqrt_with_sgn, inv): the device
front-ends against the big-integer definitions of tools/field_gadgets_ref.py word for word - random inputs at the block boundary,
the crafted inputs that a curve equation never produces (zero, c1 = 0, roots with c0 = 0, both branches on delta) -, against the
fused recovery kernels, the proven forms with their three-valued Legendre linkage, and the error contract."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import field_gadgets_ref as ref
from tools import synth

P = ref.P
SIZES = [1, 63, 64, 65, 200]  # one lane, one short of a block, one block, one over, several blocks with a ragged tail
FIELDS = ["fq", "fq2"]


def _api(ctx, field):
    """(words per element, batch call, proven call, reference, checker, to words)"""
    if field == "fq":
        return 4, ctx.fq_sqrt_batch, ctx.fq_sqrt, ref.fq_sqrt_words, pk.verify_fq_sqrt, ref.fq_words
    return 8, ctx.fq2_sqrt_batch, ctx.fq2_sqrt, ref.fq2_sqrt_words, pk.verify_fq2_sqrt, ref.fq2_words


def _same(got, want):
    """roots, square, root_ok, jobs word for word, naming the first rows that differ."""
    for name, g, w in zip(("roots", "square", "root_ok", "fq_jobs"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        diff = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert diff.size == 0, f"{name} differ at {diff[:4]}"


@pytest.fixture(scope="module")
def random_reference():
    """field -> (xs, sgns, expectation) for the 200 random inputs (every smaller case is a prefix), computed once."""
    out = {}
    for field, vals, to_words, fn in (("fq", ref.random_fq(max(SIZES), 21), ref.fq_words, ref.fq_sqrt_words),
                                      ("fq2", ref.random_fq2(max(SIZES), 22), ref.fq2_words, ref.fq2_sqrt_words)):
        xs, sgns = to_words(vals), ref.random_sgns(max(SIZES), 23)
        sgns[0] = 1  # n = 1 runs the odd sign; the prefix of 63 holds both
        want = fn(xs, sgns)
        assert 0 < int(want[1][:63].sum()) < 63 and 0 < int(sgns[:63].sum()) < 63
        for a in (xs, sgns) + want:
            a.setflags(write=False)
        out[field] = (xs, sgns, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", SIZES)
def test_front_end_matches_the_reference(gpu_ctx, random_reference, field, n):
    xs, sgns, want = random_reference[field]
    batch = _api(gpu_ctx, field)[1]
    got = batch(np.ascontiguousarray(xs[:n]), np.ascontiguousarray(sgns[:n]))
    _same(got, tuple(np.ascontiguousarray(a[:n]) for a in want))
    if n == 65:  # sgns = NULL is all zero
        _same(batch(np.ascontiguousarray(xs[:n])), _api(gpu_ctx, field)[3](xs[:n], np.zeros(n, np.uint8)))


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_crafted_inputs(gpu_ctx, field):
    """Every crafted input with both wanted signs.  Fq: 0, 1, p-1, 4, p-4, the smallest non-residue, ((p-+1)/2)^2, a root with the
    top limb at its maximum.  Fq2: (0,0), (a^2,0), (n,0) and (p-1,0) - roots (0,t), the sign from c1 -, (0,1), (0,c1) of both kinds,
    (t,0)^2, (0,t)^2, non-residue norms, delta a residue and a non-residue."""
    w, batch, _, fn, _, to_words = _api(gpu_ctx, field)
    crafted = ref.crafted_fq() if field == "fq" else ref.crafted_fq2()
    vals, sgns = ref.both_signs(list(crafted.values()))
    xs = to_words(vals)
    roots, square, ok, jobs = batch(xs, sgns)
    want = fn(xs, sgns)
    names = [f"{name} / sgn {s}" for name in crafted for s in (0, 1)]
    for i, name in enumerate(names):
        assert (int(square[i]), int(ok[i])) == (int(want[1][i]), int(want[2][i])), name
        assert np.array_equal(roots[i], want[0][i]), name
        assert np.array_equal(jobs[i], want[3][i]), name
    # the zero: no square, the even root only, zero words either way
    assert square[:2].tolist() == [0, 0] and ok[:2].tolist() == [1, 0] and not roots[:2].any()
    if field == "fq2":
        k = 2 * list(crafted).index("(p-1,0)")
        assert [ref.from_words(roots[k + 1, j:j + 4]) for j in (0, 4)] == [0, 1]      # (0, 1): sgn 1 from c1
        assert [ref.from_words(roots[k, j:j + 4]) for j in (0, 4)] == [0, P - 1]
        k = 2 * list(crafted).index("non-residue norm 0")
        assert not square[k:k + 6].any() and not ok[k:k + 6].any() and not roots[k:k + 6].any()


@pytest.mark.gpu
def test_inverses(gpu_ctx):
    fq = ref.crafted_inv_fq() + ref.random_fq(130, seed=24)
    xs = ref.fq_words(fq)
    got = gpu_ctx.fq_inv_batch(xs)
    assert np.array_equal(got, ref.fq_inv_words(xs))
    assert not got[0].any() and ref.from_words(got[1]) == 1 and ref.from_words(got[2]) == P - 1 and ref.from_words(got[4]) == 2
    fq2 = ref.crafted_inv_fq2() + ref.random_fq2(130, seed=25)
    xs = ref.fq2_words(fq2)
    got = gpu_ctx.fq2_inv_batch(xs)
    assert np.array_equal(got, ref.fq2_inv_words(xs))
    assert not got[0].any() and not got[1, 4:].any() and not got[2, :4].any()  # (0,0); (c,0) -> (1/c, 0); (0,c) -> (0, -1/c)
    for n in (1, 64, 65):
        assert np.array_equal(gpu_ctx.fq2_inv_batch(np.ascontiguousarray(xs[:n])), got[:n])


@pytest.mark.gpu
def test_roots_agree_with_the_fused_recover_kernels(gpu_ctx):
    """g = x^3 + 3 (the base of bn254s_g1_recover_from_x_batch's jobs) through bn254s_fq_sqrt_batch with the sign 0 gives the
    recover call's y, flags and jobs byte for byte; g = x^3 + b', recomputed in Python, likewise for G2 with its signs."""
    xs = synth.g1_recover_inputs(70, seed=31)
    pts, flags, jobs = gpu_ctx.g1_recover_from_x_batch(xs)
    roots, square, ok, fjobs = gpu_ctx.fq_sqrt_batch(np.ascontiguousarray(jobs[:, 4:]))
    assert 0 < int(flags.sum()) < 70
    assert roots.tobytes() == np.ascontiguousarray(pts[:, 4:]).tobytes()
    assert square.tobytes() == flags.tobytes() and ok.tobytes() == flags.tobytes() and fjobs.tobytes() == jobs.tobytes()
    xs2 = ref.fq2_words(ref.random_fq2(70, seed=32))
    sgns = ref.random_sgns(70, seed=33)
    pts, flags, jobs = gpu_ctx.g2_recover_from_x_batch(xs2, sgns)
    g = ref.fq2_words([synth.g2_rhs((ref.from_words(x[:4]), ref.from_words(x[4:]))) for x in xs2])
    roots, square, ok, fjobs = gpu_ctx.fq2_sqrt_batch(g, sgns)
    assert 0 < int(flags.sum()) < 70
    assert roots.tobytes() == np.ascontiguousarray(pts[:, 8:]).tobytes()
    assert square.tobytes() == flags.tobytes() and ok.tobytes() == flags.tobytes() and fjobs.tobytes() == jobs.tobytes()


def _proven_inputs(field):
    """130 inputs for per_proof = 128: x = 0, a square and a non-square in the first slice; the second slice has two places, and
    holds x = 0 and a non-square: the two values of the linkage that the recovery calls never see a zero base for."""
    if field == "fq":
        vals = [0, 4, ref.smallest_non_residue()] + ref.random_fq(125, seed=41) + [0, P - 1]
        return ref.fq_words(vals)
    c = ref.crafted_fq2()
    vals = [(0, 0), c["(a^2,0)"], c["non-residue norm 0"], c["(n,0), n a non-residue"]] + ref.random_fq2(124, seed=42) + \
        [(0, 0), c["non-residue norm 1"]]
    return ref.fq2_words(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_proven_call_two_proofs(gpu_ctx, field):
    w, batch, proven, fn, check, _ = _api(gpu_ctx, field)
    n = 130
    xs = _proven_inputs(field)
    sgns = ref.random_sgns(n, seed=43)
    sgns[0], sgns[128] = 0, 1  # the zero with both wanted signs
    roots, square, ok, jobs, proofs = proven(xs, sgns, per_proof=128)
    assert len(proofs) == 2 and proofs[0].outputs.size == 4 * 128 and proofs[1].outputs.size == 4 * 2
    assert all(p.degree_bits == 16 for p in proofs)
    _same((roots, square, ok, jobs), batch(xs, sgns))
    _same((roots, square, ok, jobs), fn(xs, sgns))
    legs = [synth.words_to_int(o) for p in proofs for o in p.outputs.reshape(-1, 4)]
    assert legs[:3] == [0, 1, P - 1] and legs[128:] == [0, P - 1]
    assert (ok[0], ok[128]) == (1, 0) and not roots[0].any() and not roots[128].any()
    check(xs, sgns, roots, square, ok, jobs, proofs, 128, ctx=gpu_ctx)  # the GPU verifier
    check(xs, sgns, roots, square, ok, jobs, proofs, 128)               # the host verifier
    for flags, pos in ((square, 1), (square, 129), (ok, 0), (ok, 5)):   # one returned flag flipped
        keep = flags[pos]
        flags[pos] ^= 1
        with pytest.raises(pk.VerifyError, match=f"flag {pos} "):
            check(xs, sgns, roots, square, ok, jobs, proofs, 128)
        flags[pos] = keep
    k = int(np.nonzero(ok)[0][-1])                                      # one root word flipped
    roots[k, w - 1] ^= 1
    with pytest.raises(pk.VerifyError, match=f"root {k} "):
        check(xs, sgns, roots, square, ok, jobs, proofs, 128)
    roots[k, w - 1] ^= 1
    roots[128, 0] = 1                                                   # a root where none exists
    with pytest.raises(pk.VerifyError, match="root 128 "):
        check(xs, sgns, roots, square, ok, jobs, proofs, 128)
    # the proofs are those of prove_batch (kind 2) of the returned jobs, word for word
    plain = gpu_ctx.prove_batch(2, np.ascontiguousarray(jobs[:, :4]), np.ascontiguousarray(jobs[:, 4:]), None, per_proof=128)
    assert len(plain) == 2 and all(np.array_equal(a.words, b.words) and np.array_equal(a.outputs, b.outputs) for a, b in zip(proofs, plain))


@pytest.mark.gpu
@pytest.mark.parametrize("field", FIELDS)
def test_errors_with_a_live_context(gpu_ctx, random_reference, field):
    w, batch, proven, fn, _, _ = _api(gpu_ctx, field)
    lib, name = gpu_ctx._lib, f"bn254s_{field}_sqrt"
    xs = random_reference[field][0][:8].copy()
    sgns = np.zeros(8, np.uint8)

    def vp(a):
        return a.ctypes.data_as(C.c_void_p)

    def raw_calls(xs, sgns):
        """The batch and the proven call on sentinel-filled outputs -> the two (return code, error text)."""
        roots, jobs = np.full((8, w), 7, np.uint64), np.full((8, 8), 7, np.uint64)
        square, ok = np.full(8, 7, np.uint8), np.full(8, 7, np.uint8)
        out = []
        rc = getattr(lib, name + "_batch")(gpu_ctx._h, vp(xs), vp(sgns), 8, vp(roots), vp(square), vp(ok), vp(jobs))
        out.append((rc, lib.bn254s_last_error(gpu_ctx._h).decode()))
        slots = (C.c_void_p * 4)(*([1] * 4))
        params = pk.default_params()
        rc = getattr(lib, name)(gpu_ctx._h, C.byref(params), vp(xs), vp(sgns), 8, 2, vp(roots), vp(square), vp(ok), vp(jobs), slots)
        out.append((rc, lib.bn254s_last_error(gpu_ctx._h).decode()))
        assert list(slots) == [None] * 4
        assert (roots == 7).all() and (jobs == 7).all() and (square == 7).all() and (ok == 7).all()  # nothing was written
        return out

    xs[5, w - 4:] = ref.to_words(P)  # the last coordinate of input 5
    coord = "x_5 is not below p" if field == "fq" else "x_5 has c1 not below p"
    for rc, text in raw_calls(xs, sgns):
        assert rc == -1 and coord in text, text
    xs[5, w - 4:] = ref.to_words(2**256 - 1)
    with pytest.raises(RuntimeError, match="failed with -1: .*x_5 "):
        batch(xs, sgns)
    if field == "fq2":
        xs[5, 4:] = ref.to_words(P - 1)
        xs[5, :4] = ref.to_words(P)
        for rc, text in raw_calls(xs, sgns):
            assert rc == -1 and "x_5 has c0 not below p" in text, text
    xs[5] = random_reference[field][0][5]
    sgns[3] = 2
    for rc, text in raw_calls(xs, sgns):
        assert rc == -1 and "sgn_3" in text, text
    sgns[3] = 1
    with pytest.raises(RuntimeError, match="failed with -5: .*per_proof"):
        proven(xs, sgns, per_proof=16385)
    # the context still works, also while a batch is open
    s, x = synth.fq_inputs(128, seed=54)
    want = fn(xs, sgns)
    h = gpu_ctx.prove_batch_begin(2, s, x)
    try:
        _same(batch(xs, sgns), want)
        inv = gpu_ctx.fq_inv_batch(xs) if field == "fq" else gpu_ctx.fq2_inv_batch(xs)
    finally:
        h.end()
    assert np.array_equal(inv, ref.fq_inv_words(xs) if field == "fq" else ref.fq2_inv_words(xs))
