"""Many MSMs as one segmented chain on the GPU (csrc/msm.hip, bn254s_msm_multi_chain / bn254s_msm_multi): every array word for
word against the Python reference (tools/msm_multi_ref.py) at the lane and block boundaries of the segmented scan, on three
levels, with heads that must cut, with supplied points that cannot be proven, with drawn and redrawn points, and proven."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_check_ref as jc
from tools import job_outputs_ref as jr
from tools import msm_multi_ref as mm
from tools import synth

P, R_ORD = synth.P, synth.R_ORDER
CURVES = (0, 1)
PW = jr.POINT_WORDS
SEED = (0x6D6D75, 0xFFFFFFFF00000000, 0, 9)
FIELDS = ("results", "finite", "offsets", "outputs", "R", "attempts", "bad_link", "bad_step")
# G1, 1000 inputs, heads at 0, 1, 2, 255, 256, 258, 512, 513, 769: a one-input MSM at lane 255, heads at lane 0 of a block (256,
# 512), an MSM ending on a block's last lane (258 .. 511), one crossing a boundary by one lane (513 .. 768)
G1_LAYOUTS = ([1, 1, 253, 1, 2, 254, 1, 256, 231], [700, 300], [1] * 300, [1000])
# G2, 300 inputs: the same places around the one boundary; a block without a head; m = n; one MSM
G2_LAYOUTS = ([1, 1, 253, 1, 2, 42], [257, 43], [1] * 300, [300])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def jobs():
    """kind -> (scalars, x, points for R, products): 1000 G1 inputs (those of tests/test_gpu_msm.py), 300 G2 inputs with every other
    x outside the subgroup under a scalar above r.  Computed once, read-only."""
    out = {}
    for kind, n in ((0, 1000), (1, 300)):
        s, x, o = synth.g1_inputs(n, seed=0x6D736D) if kind == 0 else jr.provable_jobs(1, n, seed=0x67326D)
        out[kind] = _frozen(s, x, o) + (mm.products(kind, s, x),)
    return out


def _same(got, want):
    """Every array of the call against the reference's, word for word."""
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(g, w), f"{name}: first differing rows {np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:4]}"


def _check(ctx, kind, s, x, seg, prods, walk=None, **kw):
    """The call against the reference.  walk: the MSMs whose links the Python job check walks (default: the first sixteen of at
    most three inputs); that the other links are provable is what the device's job check says of the returned offsets."""
    n = sum(seg)
    s, x = np.ascontiguousarray(s[:n]), np.ascontiguousarray(x[:n])
    got = ctx.msm_multi_chain(kind, s, x, seg, **kw)
    walk = set([j for j, ln in enumerate(seg) if ln <= 3][:16]) if walk is None else walk
    want = mm.msm_multi(kind, s, x, seg, prods=prods[:n], check=walk, **kw)
    _same(got, want)
    good = np.repeat(got.bad_link == pk.MSM_LINK_NONE, seg)
    if good.any():
        provable, _ = ctx.job_check_batch(kind, *(np.ascontiguousarray(a[good]) for a in (s, x, got.offsets)))
        assert provable.all()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seg", G1_LAYOUTS, ids=lambda v: f"{len(v)}x{v[0]}")
def test_g1_layouts(gpu_ctx, jobs, seg):
    s, x, o, prods = jobs[0]
    m, n = len(seg), sum(seg)
    R = np.ascontiguousarray(o[500:500 + m] if m <= 500 else o[:m])
    got = _check(gpu_ctx, 0, s, x, seg, prods, R=R)
    assert got.finite.all() and (got.attempts == 0).all() and (got.bad_link == pk.MSM_LINK_NONE).all()
    if m == 1:  # one MSM is the chain of g1_msm
        offs, res = gpu_ctx.g1_msm_chain(s, x, R[0])
        assert np.array_equal(got.offsets, offs[:n]) and np.array_equal(got.outputs, offs[1:]) and np.array_equal(got.results[0], res)
    if m == 9:  # the same layout with drawn points: the results do not move, every R_j is the hash of its inputs
        drawn = _check(gpu_ctx, 0, s, x, seg, prods, seed=SEED)
        assert np.array_equal(drawn.results, got.results) and (drawn.attempts == 0).all()
        ins = np.zeros((m, 8), np.uint64)
        ins[:, :4], ins[:, 4], ins[:, 7] = np.array(SEED, np.uint64), np.arange(m, dtype=np.uint64), 0x626D6D00
        assert np.array_equal(drawn.R, gpu_ctx.hash_to_g1_batch(ins))


@pytest.mark.gpu
@pytest.mark.parametrize("seg", G2_LAYOUTS, ids=lambda v: f"{len(v)}x{v[0]}")
def test_g2_layouts(gpu_ctx, jobs, seg):
    s, x, o, prods = jobs[1]
    m, n = len(seg), sum(seg)
    assert synth.words_to_int(s[1]) > R_ORD and not synth.g2_in_subgroup(jr.from_words(1, x[1]))
    R = np.ascontiguousarray(o[:m])
    got = _check(gpu_ctx, 1, s, x, seg, prods, R=R)
    assert got.finite.all() and (got.bad_link == pk.MSM_LINK_NONE).all()
    if m == 1:
        offs, res = gpu_ctx.g2_msm_chain(s, x, R[0])
        assert np.array_equal(got.offsets, offs[:n]) and np.array_equal(got.outputs, offs[1:]) and np.array_equal(got.results[0], res)
    if m == 6:
        drawn = _check(gpu_ctx, 1, s, x, seg, prods, seed=SEED)
        assert np.array_equal(drawn.results, got.results) and (drawn.attempts == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_one_msm_of_257_is_the_chain(gpu_ctx, jobs, kind):
    """One MSM of 257 inputs under a supplied R, one element into a second scan block: the smallest size at which the block-total and
    add-back kernels run, here with head flags (257 products) and in g1_msm_chain / g2_msm_chain without (258 points, R among them).
    Both are the same kernels in their two instantiations and must give the same words.  The inputs are random, so the links are
    provable but for a chance of about 2^-245 (the job check); mm.msm_multi(kind, s, x, [257], R=R, check={0}) walks
    all 257 links of either kind and finds them so.  That the words are right, not only equal, is what the layout tests above
    check against the Python reference."""
    s0, x0, o, _ = jobs[kind]
    n = 257
    s, x, R = np.ascontiguousarray(s0[:n]), np.ascontiguousarray(x0[:n]), np.ascontiguousarray(o[7:8])
    got = gpu_ctx.msm_multi_chain(kind, s, x, [n], R=R)
    offs, res = (gpu_ctx.g1_msm_chain if kind == 0 else gpu_ctx.g2_msm_chain)(s, x, R[0])
    assert offs.shape == (n + 1, PW[kind])
    assert np.array_equal(got.offsets, offs[:n])
    assert np.array_equal(got.outputs, offs[1:n + 1])
    assert np.array_equal(got.results[0], res)
    assert got.finite[0] == 1
    assert got.bad_link[0] == pk.MSM_LINK_NONE


@pytest.mark.gpu
def test_three_levels(gpu_ctx):
    """70 000 inputs x_i = (a + i d) G: more than 256^2 products, so the scan has three levels, and the long MSM spans 258 blocks
    of level 0 and two of level 1."""
    n, a, d, seg = 70000, 0x1234567, 0x9E3779B9, [1, 66000, 255, 3744]
    rng = synth.Xoshiro256ss(70000)
    G = synth.G1_GEN
    dG, cur = synth.g1_mul(d, G), synth.g1_mul(a, G)
    xs, ss = [], []
    for i in range(n):
        xs.append(cur)
        ss.append(rng.next_u256())
        cur = synth.g1_add(cur, dG)
    s = np.array([synth._to_words(v) for v in ss], np.uint64).reshape(n, 4)
    x = synth.g1_points_to_words(xs)
    R = synth.g1_points_to_words([synth.g1_mul(0xC0FFEE + j, G) for j in range(4)])
    got = gpu_ctx.msm_multi_chain(0, s, x, seg, R=R)
    assert (got.bad_link == pk.MSM_LINK_NONE).all() and got.finite.all() and np.array_equal(got.R, R)
    pt = lambda w: jr.from_words(0, w)
    first = np.concatenate([[0], np.cumsum(seg)])
    for j in range(4):
        lo, hi = int(first[j]), int(first[j + 1])
        acc = sum(ss[i] * (a + i * d) for i in range(lo, hi)) % R_ORD
        assert pt(got.results[j]) == synth.g1_mul(acc, G), j
        assert np.array_equal(got.offsets[lo], R[j]) and np.array_equal(got.offsets[lo + 1:hi], got.outputs[lo:hi - 1])
    sample = set(np.random.default_rng(1).choice(n, 64, replace=False).tolist()) | set(first[:-1].tolist()) | set((first[1:] - 1).tolist())
    for i in sorted(sample):
        assert pt(got.outputs[i]) == synth.g1_scalar_mul_offset(ss[i], xs[i], pt(got.offsets[i])), f"link {i}"


def _swords(ss):
    return np.array([synth._to_words(v) for v in ss], np.uint64).reshape(-1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_heads_really_cut(gpu_ctx, jobs, kind):
    s0, x0, o, _ = jobs[kind]
    sv = lambda i: synth.words_to_int(s0[i])
    k = sv(0) % R_ORD
    # even indices: points of order r on both curves, so that (r - k) x = -(k x)
    seg = [3, 2, 2, 2, 3, 2]
    ss = [sv(2), sv(4), k,               # MSM 0 ends with k x_0
          R_ORD - k, sv(6),              # MSM 1 starts with (r - k) x_0: nothing may cancel across the head
          sv(8), k,                      # MSM 2 ends with k x_0
          k, sv(10),                     # MSM 3 starts with the same product: nothing may double across the head
          k, R_ORD - k, sv(12),          # MSM 4: the partial sum returns to infinity, the offset is R again
          k, R_ORD - k]                  # MSM 5: the result is infinity
    xi = [2, 4, 0, 0, 6, 8, 0, 0, 10, 0, 0, 12, 0, 0]
    s, x = _swords(ss), np.ascontiguousarray(x0[xi])
    R = np.ascontiguousarray(o[20:26])
    got = _check(gpu_ctx, kind, s, x, seg, mm.products(kind, s, x), walk=set(range(6)), R=R)
    assert (got.bad_link == pk.MSM_LINK_NONE).all()  # an infinite result is no obstacle under a supplied R
    assert list(got.finite) == [1, 1, 1, 1, 1, 0] and not got.results[5].any()
    assert np.array_equal(got.offsets[11], R[4]) and np.array_equal(got.outputs[10], R[4]) and np.array_equal(got.outputs[13], R[5])
    assert np.array_equal(got.offsets[3], R[1]) and np.array_equal(got.offsets[7], R[3])
    alone = gpu_ctx.msm_multi_chain(kind, np.ascontiguousarray(s[3:5]), np.ascontiguousarray(x[3:5]), [2], R=R[1:2])
    assert np.array_equal(alone.outputs, got.outputs[3:5]) and np.array_equal(alone.results[0], got.results[1])


def _five(kind, jobs):
    """Five MSMs of 3, 2, 4, 5, 2 inputs from indices whose points have order r, their products, and points for R."""
    s0, x0, o, prods = jobs[kind]
    idx = list(range(0, 32, 2))
    return np.ascontiguousarray(s0[idx]), np.ascontiguousarray(x0[idx]), [3, 2, 4, 5, 2], np.ascontiguousarray(o[40:45]), [prods[i] for i in idx]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_supplied_points_that_cannot_be_proven(gpu_ctx, jobs, kind):
    s, x, seg, R, prods = _five(kind, jobs)
    base = _check(gpu_ctx, kind, s, x, seg, prods, walk=set(range(5)), R=R)
    assert (base.bad_link == pk.MSM_LINK_NONE).all()
    _, neg = jr._law(kind)
    R2, x2 = R.copy(), x.copy()
    R2[1] = jr.to_words(kind, neg(prods[3]))  # MSM 1 = inputs 3, 4: R = -(s_3 x_3), the output of link 0 is infinity
    T = mm.chain_one(kind, prods[9:11], None)[2]  # MSM 3 = inputs 9 .. 13: link 2 is input 11
    x2[11] = jr.to_words(kind, mm.crafted_x(kind, jr.from_words(kind, R[3]), T, synth.words_to_int(s[11]), 64))
    prods2 = prods[:11] + mm.products(kind, s[11:12], x2[11:12]) + prods[12:]
    got = _check(gpu_ctx, kind, s, x2, seg, prods2, walk=set(range(5)), R=R2)
    step0 = jc.check_one(kind, synth.words_to_int(s[3]), jr.from_words(kind, x[3]), jr.from_words(kind, R2[1]))[1]
    assert step0 == synth.words_to_int(s[3]).bit_length() - 1
    assert list(got.bad_link) == [pk.MSM_LINK_NONE, 0, pk.MSM_LINK_NONE, 2, pk.MSM_LINK_NONE]
    assert list(got.bad_step) == [pk.JOB_STEP_NONE, step0, pk.JOB_STEP_NONE, 64, pk.JOB_STEP_NONE]
    assert (got.attempts == 0).all() and got.finite.all() and np.array_equal(got.R, R2)
    assert not got.offsets[3:5].any() and not got.outputs[3:5].any() and not got.offsets[9:14].any() and not got.outputs[9:14].any()
    assert np.array_equal(got.results[:3], base.results[:3]) and np.array_equal(got.results[4], base.results[4])
    for lo, hi in ((0, 3), (5, 9), (14, 16)):  # the three good MSMs are what they are without the two
        assert np.array_equal(got.offsets[lo:hi], base.offsets[lo:hi]) and np.array_equal(got.outputs[lo:hi], base.outputs[lo:hi])


def _crafted_against_attempt_0(kind, jobs):
    """_five with input 11 (link 2 of MSM 3) made to hit step 64 under the point drawn for MSM 3 at attempt 0."""
    s, x, seg, _, prods = _five(kind, jobs)
    T = mm.chain_one(kind, prods[9:11], None)[2]
    x2 = x.copy()
    x2[11] = jr.to_words(kind, mm.crafted_x(kind, mm.drawn(kind, SEED, 3, 0), T, synth.words_to_int(s[11]), 64))
    return s, x, x2, seg, prods, prods[:11] + mm.products(kind, s[11:12], x2[11:12]) + prods[12:]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_drawn_points_and_the_redraw(gpu_ctx, jobs, kind):
    s, x, x2, seg, prods, prods2 = _crafted_against_attempt_0(kind, jobs)
    every = set(range(5))
    plain = _check(gpu_ctx, kind, s, x, seg, prods, walk=every, seed=SEED)
    assert (plain.attempts == 0).all()
    for j in range(5):
        assert list(plain.R[j]) == jr.to_words(kind, mm.drawn(kind, SEED, j, 0))
    fixed = _check(gpu_ctx, kind, s, x2, seg, prods2, walk=every, seed=SEED)
    assert list(fixed.attempts) == [0, 0, 0, 1, 0] and (fixed.bad_link == pk.MSM_LINK_NONE).all()
    assert list(fixed.R[3]) == jr.to_words(kind, mm.drawn(kind, SEED, 3, 1)) and np.array_equal(fixed.offsets[9], fixed.R[3])
    for lo, hi in ((0, 9), (14, 16)):  # the neighbours' rows are those of the call without the crafted input, byte for byte
        assert fixed.offsets[lo:hi].tobytes() == plain.offsets[lo:hi].tobytes() and fixed.outputs[lo:hi].tobytes() == plain.outputs[lo:hi].tobytes()
    assert np.array_equal(np.delete(fixed.R, 3, 0), np.delete(plain.R, 3, 0)) and np.array_equal(np.delete(fixed.results, 3, 0), np.delete(plain.results, 3, 0))
    once = _check(gpu_ctx, kind, s, x2, seg, prods2, walk=every, seed=SEED, max_attempts=1)
    assert list(once.attempts) == [0, 0, 0, 1, 0] and int(once.bad_link[3]) == 2 and int(once.bad_step[3]) == 64
    assert not once.offsets[9:14].any() and not once.outputs[9:14].any() and np.array_equal(once.results, fixed.results)
    assert list(once.R[3]) == jr.to_words(kind, mm.drawn(kind, SEED, 3, 0))
    assert once.offsets[:9].tobytes() == plain.offsets[:9].tobytes() and once.offsets[14:].tobytes() == plain.offsets[14:].tobytes()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(kind, m, n):
    """Output buffers pre-filled with 7, in the order of the entry points."""
    pw = PW[kind]
    return (np.full((m, pw), 7, np.uint64), np.full(m, 7, np.uint8), np.full((n, pw), 7, np.uint64), np.full((n, pw), 7, np.uint64),
            np.full((m, pw), 7, np.uint64), np.full(m, 7, np.uint8), np.full(m, 7, np.uint32), np.full(m, 7, np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_point_off_its_curve_is_found_on_the_device(gpu_ctx, jobs, kind):
    s, x, seg, R, _ = _five(kind, jobs)
    lib, segw = gpu_ctx._lib, np.array(seg, np.uintp)
    x2, R2 = x.copy(), R.copy()
    for i in (12, 7):
        x2[i, PW[kind] // 2] += 1  # y (y.c0) + 1: below p still
    R2[2, PW[kind] // 2] += 1
    bufs = _raw(kind, 5, 16)
    call = lambda xx, RR: lib.bn254s_msm_multi_chain(gpu_ctx._h, kind, _vp(s), _vp(xx), _vp(segw), 5, 16, _vp(RR), None, 4, *(_vp(b) for b in bufs))
    assert call(x2, R2) == -1 and lib.bn254s_last_error(gpu_ctx._h).decode().startswith("msm_multi_chain: x_7 is not on the ")  # x before R
    assert call(x, R2) == -1 and lib.bn254s_last_error(gpu_ctx._h).decode().startswith("msm_multi_chain: R_2 is not on the ")
    x2[9, :4] = synth._to_words(P)  # a coordinate that is p is found on the host
    assert call(x2, R) == -1 and lib.bn254s_last_error(gpu_ctx._h).decode().startswith("msm_multi_chain: x_9 has x")
    R2[4, 4:8] = synth._to_words(P)
    assert call(x, R2) == -1 and lib.bn254s_last_error(gpu_ctx._h).decode().startswith("msm_multi_chain: R_4 has ")
    assert all((b == 7).all() for b in bufs)
    assert call(x, R) == 0 and not any((b == 7).all() for b in bufs[:4])  # optional outputs may be NULL
    assert lib.bn254s_msm_multi_chain(gpu_ctx._h, kind, _vp(s), _vp(x), _vp(segw), 5, 16, _vp(R), None, 4, *(_vp(b) for b in bufs[:4]), None,
                                      None, _vp(bufs[6]), None) == 0


@pytest.mark.gpu
def test_proven_g1_with_an_msm_across_the_cut(gpu_ctx, jobs):
    s0, x0, _, prods = jobs[0]
    seg = [3, 1, 130, 60, 62]  # 256 links, two proofs of 128: MSM 2 = links 4 .. 133 straddles the cut
    s, x = np.ascontiguousarray(s0[:256]), np.ascontiguousarray(x0[:256])
    got = gpu_ctx.msm_multi(0, s, x, seg, seed=SEED, per_proof=128)
    _same(got, mm.msm_multi(0, s, x, seg, seed=SEED, prods=prods[:256], check={0, 1}))
    assert len(got.proofs) == 2 and all(p.outputs.size == 128 * 8 for p in got.proofs)
    assert np.array_equal(np.concatenate([p.outputs for p in got.proofs]).reshape(256, 8), got.outputs)
    pk.verify_msm_multi(0, s, x, seg, got.R, got.results, got.finite, got.offsets, got.outputs, got.proofs, 128, ctx=gpu_ctx)
    swapped = got.R.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    with pytest.raises(pk.VerifyError, match=r"offsets\[4\] != R_2"):
        pk.verify_msm_multi(0, s, x, seg, swapped, got.results, got.finite, got.offsets, got.outputs, got.proofs, 128, ctx=gpu_ctx)
    with pytest.raises(RuntimeError, match="failed with -5: msm_multi: per_proof"):
        gpu_ctx.msm_multi(0, s, x, seg, seed=SEED, per_proof=16385)


@pytest.mark.gpu
def test_proven_g2(gpu_ctx, jobs):
    s0, x0, o, prods = jobs[1]
    seg = [2, 1, 5]
    s, x, R = np.ascontiguousarray(s0[:8]), np.ascontiguousarray(x0[:8]), np.ascontiguousarray(o[:3])
    got = gpu_ctx.msm_multi(1, s, x, seg, R=R, per_proof=128)
    _same(got, mm.msm_multi(1, s, x, seg, R=R, prods=prods[:8]))
    assert len(got.proofs) == 1
    pk.verify_msm_multi(1, s, x, seg, R, got.results, got.finite, got.offsets, got.outputs, got.proofs, 128, ctx=gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_an_unprovable_msm_stops_the_proven_call(gpu_ctx, jobs, kind):
    s, x, x2, seg, prods, _ = _crafted_against_attempt_0(kind, jobs)
    lib, segw, seed = gpu_ctx._lib, np.array(seg, np.uintp), np.array(SEED, np.uint64)
    params = pk.default_params()
    bufs = _raw(kind, 5, 16)
    slots = (C.c_void_p * 3)(1, 1, 1)
    rc = lib.bn254s_msm_multi(gpu_ctx._h, kind, C.byref(params), _vp(s), _vp(x2), _vp(segw), 5, 16, None, _vp(seed), 1, 8,
                              *(_vp(b) for b in bufs), slots)
    assert rc == -4 and list(slots) == [None, None, 1] and all((b == 7).all() for b in bufs)
    assert lib.bn254s_last_error(gpu_ctx._h).decode() == ("msm_multi: msm 3 cannot be proven: link 2, sum == -double at step 64 (row 128 of "
                                                          "its frame) with the offset of attempt 0, the last of 1")
    R0 = np.array([jr.to_words(kind, mm.drawn(kind, SEED, j, 0)) for j in range(5)], np.uint64)
    with pytest.raises(RuntimeError, match=r"failed with -4: msm_multi: msm 3 cannot be proven: link 2, sum == -double at step 64 \(row 128 of "
                                           r"its frame\) with the supplied offset"):
        gpu_ctx.msm_multi(kind, s, x2, seg, R=R0, per_proof=8)
    # the same context then proves the same inputs with a second attempt
    got = gpu_ctx.msm_multi(kind, s, x2, seg, seed=SEED, per_proof=8)
    assert list(got.attempts) == [0, 0, 0, 1, 0] and len(got.proofs) == 2
    pk.verify_msm_multi(kind, s, x2, seg, got.R, got.results, got.finite, got.offsets, got.outputs, got.proofs, 8, ctx=gpu_ctx)
