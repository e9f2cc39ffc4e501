"""The statement verifiers on the GPU (csrc/point_sum.hip: bn254s_verify_scalar_mul, bn254s_verify_msm_multi): calls of scalar_mul
and msm_multi, proven once per module, are accepted as they are, and rejected with the exact link codes, proof verdicts and message
once a product, a result, an output, an offset, an input point or a proof word is not what it was.  The Python checker of
msm_multi (plonky2_bn254_amd.lib.verify_msm_multi) agrees on one accepted and one rejected call.  The Python side does point
negations and array surgery only: no scalar multiplication."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import job_outputs_ref as jr
from tools import synth

R_ORD = synth.R_ORDER
CURVES = (0, 1)
PW = jr.POINT_WORDS
SEED = (0x767374, 0xFFFFFFFF00000000, 0, 3)
SEG = [1, 2, 64, 63]  # 130 links at 128 per proof: MSM 3 = links 67 .. 129 lies across the cut
CURVE = {0: "the curve y^2 = x^3 + 3", 1: "the twist curve y^2 = x^3 + b'"}


def _jobs(kind, n, seed):
    """n provable jobs with s = 0 at job 4 and s = r at job 6, both on points of order r: their products are the point at infinity."""
    s, x, o = jr.provable_jobs(kind, n, seed)
    s[4] = 0
    s[6] = synth._to_words(R_ORD)
    return s, x, o


@pytest.fixture(scope="module")
def smul(gpu_ctx):
    """kind -> (scalars, x, products, finite, offsets, outputs, proofs) of 130 jobs in two proofs of 128; key 300: 300 G1 jobs in
    two proofs of 256, of 2^17 and 2^16 rows."""
    out = {}
    for key, kind, n, per in ((0, 0, 130, 128), (1, 1, 130, 128), (300, 0, 300, 256)):
        s, x, _ = _jobs(kind, n, seed=1301 + key)
        prods, finite, offs, outs, _, proofs = gpu_ctx.scalar_mul(kind, s, x, SEED, per_proof=per)
        for a in (s, x, prods, finite, offs, outs):
            a.setflags(write=False)
        out[key] = (s, x, prods, finite, offs, outs, proofs)
    return out


@pytest.fixture(scope="module")
def msm(gpu_ctx):
    """kind -> (scalars, x, spare points, MsmMulti) of the four MSMs of SEG under drawn R."""
    out = {}
    for kind in CURVES:
        s, x, o = jr.provable_jobs(kind, 130, seed=1401 + kind)
        got = gpu_ctx.msm_multi(kind, s, x, SEG, seed=SEED, per_proof=128)
        assert (got.bad_link == pk.MSM_LINK_NONE).all() and got.finite.all() and len(got.proofs) == 2
        out[kind] = (s, x, o, got)
    return out


def _rejected(call):
    with pytest.raises(pk.VerifyError) as e:
        call()
    return str(e.value), [int(v) for v in e.value.link_codes], [int(v) for v in e.value.proof_status]


def _codes(n, **at):
    out = [0] * n
    for i, v in at.items():
        out[int(i[1:])] = v
    return out


# ---- scalar_mul ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", (0, 1, 300))
def test_scalar_mul_accepted(gpu_ctx, smul, key):
    s, x, prods, finite, offs, outs, proofs = smul[key]
    kind, per = (0, 256) if key == 300 else (key, 128)
    assert [i for i in range(len(finite)) if not finite[i]] == [4, 6] and not prods[[4, 6]].any()
    assert len(proofs) == 2 and [p.degree_bits for p in proofs] == ([17, 16] if key == 300 else [16, 16])
    link, status = gpu_ctx.verify_scalar_mul(kind, proofs, per, s, x, prods, finite, offs, outs)
    assert link.shape == (len(finite),) and link.dtype == np.uint8 and not link.any()
    assert status.shape == (2,) and status.dtype == np.int32 and not status.any()
    pairs = [(p.words, p.degree_bits) for p in proofs]  # the other form of `proofs`
    link, status = gpu_ctx.verify_scalar_mul(kind, pairs, per, s, x, prods, finite, offs, outs)
    assert not link.any() and not status.any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_scalar_mul_rejected(gpu_ctx, smul, kind):
    s, x, prods, finite, offs, outs, proofs = smul[kind]
    add, neg = jr._law(kind)

    def verify(**kw):
        a = dict(proofs=proofs, x=x, prods=prods, finite=finite, offs=offs, outs=outs)
        a.update(kw)
        return gpu_ctx.verify_scalar_mul(kind, a["proofs"], 128, s, a["x"], a["prods"], a["finite"], a["offs"], a["outs"])

    # the products of two jobs swapped: both links break, the proofs do not speak of products
    p2 = prods.copy()
    p2[[3, 70]] = p2[[70, 3]]
    assert _rejected(lambda: verify(prods=p2)) == ("verify_scalar_mul: job 3: products + offsets != outputs (x)", _codes(130, i3=6, i70=6),
                                                   [0, 0])
    # an output replaced by its neighbour's: the link breaks and the proof of job 64 fails its cross-table lookup
    o2 = outs.copy()
    o2[64] = o2[65]
    assert _rejected(lambda: verify(outs=o2)) == ("verify_scalar_mul: job 64: products + offsets != outputs (x)", _codes(130, i64=6), [-8, 0])
    verdicts = gpu_ctx.verify_batch(kind, [(p.words, o2[lo:hi]) for p, (lo, hi) in zip(proofs, ((0, 128), (128, 130)))], s, x, offs,
                                    n_jobs=[128, 2], degree_bits=16)
    assert verdicts[0] and "CTL" in verdicts[0] and verdicts[1] is None
    # a product negated: -a + b has the x of a + b only where 2a or 2b is O, so this is code 6 (x) again ...
    p3 = prods.copy()
    p3[9] = jr.to_words(kind, neg(jr.from_words(kind, prods[9])))
    assert _rejected(lambda: verify(prods=p3)) == ("verify_scalar_mul: job 9: products + offsets != outputs (x)", _codes(130, i9=6), [0, 0])
    # ... and code 7 is the negated SUM: the product -(a + 2b) gives -(a + b), with every proof untouched
    a9, b9 = jr.from_words(kind, prods[9]), jr.from_words(kind, offs[9])
    p3[9] = jr.to_words(kind, neg(add(add(a9, b9), b9)))
    assert _rejected(lambda: verify(prods=p3)) == ("verify_scalar_mul: job 9: products + offsets != outputs (y)", _codes(130, i9=7), [0, 0])
    # the output negated says the same of the link, and its proof fails
    o3 = outs.copy()
    o3[129] = jr.to_words(kind, neg(jr.from_words(kind, outs[129])))
    assert _rejected(lambda: verify(outs=o3)) == ("verify_scalar_mul: job 129: products + offsets != outputs (y)", _codes(130, i129=7), [0, -8])
    # one word of the query rounds of proof 1 flipped: the linkage is whole, the message is the proof's
    w1 = proofs[1].words.copy()
    sec = proofs[1].section("query_round_proofs")
    tail = sum(proofs[1].section(name).size for name in ("final_poly", "pow_witness", "init_challenger_state"))  # what follows
    off = w1.size - tail - sec.size
    assert np.array_equal(w1[off:off + sec.size], sec)
    w1[off + 5] ^= np.uint64(1)
    msg, link, status = _rejected(lambda: verify(proofs=[proofs[0], (w1, 16)]))
    assert msg.startswith("proof 1: ") and len(msg) > len("proof 1: ") and link == [0] * 130 and status == [0, -8]
    # an input point moved off its curve
    x2 = x.copy()
    x2[77, PW[kind] // 2] ^= np.uint64(1)
    assert _rejected(lambda: verify(x=x2)) == (f"verify_scalar_mul: job 77: x is not on {CURVE[kind]}", _codes(130, i77=8), [-8, 0])
    # ... which comes before the codes of the same job's relation, and the smallest job is the one named
    p4 = p2.copy()
    x2[3, PW[kind] // 2] ^= np.uint64(1)
    msg, link, status = _rejected(lambda: verify(x=x2, prods=p4))
    assert msg == f"verify_scalar_mul: job 3: x is not on {CURVE[kind]}" and link == _codes(130, i3=8, i70=6, i77=8) and status == [-8, 0]
    # finite cleared with the words left; finite set on zero words
    f2 = finite.copy()
    f2[5], f2[4] = 0, 1
    msg, link, status = _rejected(lambda: verify(finite=f2))
    assert msg == f"verify_scalar_mul: job 4: products is not on {CURVE[kind]}" and link == _codes(130, i4=2, i5=1) and status == [0, 0]
    # and the unmodified call is still accepted by the same context
    link, status = verify()
    assert not link.any() and not status.any()


@pytest.mark.gpu
def test_scalar_mul_arguments_with_a_context(gpu_ctx, smul):
    s, x, prods, finite, offs, outs, proofs = smul[0]
    with pytest.raises(RuntimeError, match="failed with -1"):  # three proofs for 130 jobs of 128
        gpu_ctx.verify_scalar_mul(0, proofs + [proofs[0]], 128, s, x, prods, finite, offs, outs)
    o2 = outs.copy()
    o2[100, 4:8] = synth._to_words(synth.P)
    with pytest.raises(RuntimeError, match="failed with -1: verify_scalar_mul: outputs_100 has y not below p"):
        gpu_ctx.verify_scalar_mul(0, proofs, 128, s, x, prods, finite, offs, o2)
    p2 = prods.copy()
    p2[4] = 2**64 - 1  # a row with finite = 0 is not a point: no range check, code 1
    msg, link, status = _rejected(lambda: gpu_ctx.verify_scalar_mul(0, proofs, 128, s, x, p2, finite, offs, outs))
    assert msg == "verify_scalar_mul: job 4: finite is 0 and products is not zero words" and link == _codes(130, i4=1) and status == [0, 0]


# ---- msm_multi ----------------------------------------------------------------------------------------------------------------
def _verify_msm(ctx, kind, s, x, got, seg=SEG, **kw):
    a = dict(proofs=got.proofs, R=got.R, results=got.results, finite=got.finite, offsets=got.offsets, outputs=got.outputs)
    a.update(kw)
    return ctx.verify_msm_multi(kind, a["proofs"], 128, s, x, seg, a["R"], a["results"], a["finite"], a["offsets"], a["outputs"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_msm_multi_accepted_and_the_python_checker_agrees(gpu_ctx, msm, kind):
    s, x, _, got = msm[kind]
    link, status = _verify_msm(gpu_ctx, kind, s, x, got)
    assert link.shape == (4,) and status.shape == (2,) and not link.any() and not status.any()
    pk.verify_msm_multi(kind, s, x, SEG, got.R, got.results, got.finite, got.offsets, got.outputs, got.proofs, 128, ctx=gpu_ctx)
    r2 = got.results.copy()
    r2[[2, 3]] = r2[[3, 2]]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, results=r2)) == (
        "verify_msm_multi: msm 2: results + R != outputs[66] (x)", [0, 0, 6, 6], [0, 0])
    with pytest.raises(pk.VerifyError, match=r"results\[2\] != outputs\[66\] - R_2"):
        pk.verify_msm_multi(kind, s, x, SEG, got.R, r2, got.finite, got.offsets, got.outputs, got.proofs, 128, ctx=gpu_ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_msm_multi_rejected(gpu_ctx, msm, kind):
    s, x, spare, got = msm[kind]
    # the head of MSM 2 (link 3) replaced by another point of the curve: the proof of link 3 was made for another offset
    o2 = got.offsets.copy()
    o2[3] = spare[0]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, offsets=o2)) == (
        "verify_msm_multi: msm 2: offsets[3] != R_2 (the head)", [0, 0, 9, 0], [-8, 0])
    # ... and so is R_2 itself, which no proof holds
    R2 = got.R.copy()
    R2[2] = spare[0]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, R=R2)) == (
        "verify_msm_multi: msm 2: offsets[3] != R_2 (the head)", [0, 0, 9, 0], [0, 0])
    # an offset inside MSM 2 and one inside MSM 3, past the cut
    o3 = got.offsets.copy()
    o3[40], o3[129] = spare[1], spare[2]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, offsets=o3)) == (
        "verify_msm_multi: msm 2: offsets[40] != outputs[39] (link 36 -> 37)", [0, 0, 10, 10], [-8, -8])
    # finite cleared with the words left
    f2 = got.finite.copy()
    f2[1] = 0
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, finite=f2)) == (
        "verify_msm_multi: msm 1: finite is 0 and results is not zero words", [0, 1, 0, 0], [0, 0])
    # an input point off its curve comes first: MSM 3 with a broken chain too, MSM 0 with a wrong result too
    x2, r2 = x.copy(), got.results.copy()
    x2[128, 0] ^= np.uint64(1)
    x2[0, 0] ^= np.uint64(1)
    r2[0] = spare[3]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x2, got, offsets=o3, results=r2)) == (
        f"verify_msm_multi: msm 0: x_0 is not on {CURVE[kind]}", [8, 0, 10, 8], [-8, -8])
    # the last output replaced: the result no longer follows, and the proof of the last link fails
    out2 = got.outputs.copy()
    out2[129] = spare[4]
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, outputs=out2)) == (
        "verify_msm_multi: msm 3: results + R != outputs[129] (x)", [0, 0, 0, 6], [0, -8])
    link, status = _verify_msm(gpu_ctx, kind, s, x, got)
    assert not link.any() and not status.any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_msm_with_supplied_points_and_an_infinite_result(gpu_ctx, msm, kind):
    """Two MSMs under caller-supplied R: (1, P), (1, -P), whose result is the point at infinity, and three ordinary inputs."""
    s0, x0, spare, _ = msm[kind]
    _, neg = jr._law(kind)
    s, x = s0[:5].copy(), x0[:5].copy()
    s[:2] = 0
    s[:2, 0] = 1
    x[1] = jr.to_words(kind, neg(jr.from_words(kind, x[0])))
    R = np.ascontiguousarray(spare[10:12])
    got = gpu_ctx.msm_multi(kind, s, x, [2, 3], R=R, per_proof=128)
    assert list(got.finite) == [0, 1] and not got.results[0].any() and np.array_equal(got.outputs[1], R[0]) and np.array_equal(got.R, R)
    link, status = _verify_msm(gpu_ctx, kind, s, x, got, seg=[2, 3])
    assert not link.any() and not status.any() and status.shape == (1,)
    f2 = got.finite.copy()
    f2[0] = 1  # zero words are no point of the curve
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, seg=[2, 3], finite=f2)) == (
        f"verify_msm_multi: msm 0: results is not on {CURVE[kind]}", [2, 0], [0])
    r2 = got.results.copy()
    r2[0] = jr.to_words(kind, neg(jr.from_words(kind, R[0])))  # a result that would make the sum infinite
    assert _rejected(lambda: _verify_msm(gpu_ctx, kind, s, x, got, seg=[2, 3], finite=f2, results=r2)) == (
        "verify_msm_multi: msm 0: results == -R: their sum is the point at infinity", [5, 0], [0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", CURVES)
def test_a_single_msm_call_is_one_msm(gpu_ctx, msm, kind):
    """What g1_msm / g2_msm return, fed in as m = 1: offsets[:n] are the offsets, offsets[1:] the outputs."""
    s0, x0, spare, _ = msm[kind]
    s, x, R = np.ascontiguousarray(s0[10:15]), np.ascontiguousarray(x0[10:15]), np.ascontiguousarray(spare[20])
    res, offs, proofs = (gpu_ctx.g1_msm if kind == 0 else gpu_ctx.g2_msm)(s, x, R, per_proof=128)
    args = (kind, proofs, 128, s, x, [5], R[None], res[None], [1], offs[:5])
    link, status = gpu_ctx.verify_msm_multi(*args, offs[1:])
    assert list(link) == [0] and list(status) == [0]
    assert _rejected(lambda: gpu_ctx.verify_msm_multi(*args, offs[:5])) == (  # the outputs one link late
        "verify_msm_multi: msm 0: offsets[1] != outputs[0] (link 0 -> 1)", [10], [-8])
