"""bn254s_verify_batch on the device (csrc/verify_batch.hip: k_vb_merkle, k_vb_fri) against the same query-round functions on the
host and against bn254s_verify_host proof by proof, on the smallest proofs the provers make.  All comparisons are exact."""
import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import synth
from tests import verify_batch_cases as vc

pytestmark = pytest.mark.gpu

# name -> (kind, jobs, num_queries, pow_bits, touched queries); 63 | 64 is the wave edge of the lane-per-(proof, query) mapping
SHAPES = {
    "g1_3": (0, 3, 84, 16, (0, 41, 63, 64, 83)),
    "g1_200_tall": (0, 200, 84, 16, (0, 41, 63, 64, 83)),
    "g2_4": (1, 4, 84, 16, (0, 41, 63, 64, 83)),
    "fq_6": (2, 6, 84, 16, (0, 41, 63, 64, 83)),
    "g1_3_q20": (0, 3, 20, 10, (0, 19)),
}
_made = {}


def shape(ctx, name):
    """One proof of the shape, its honest record, the corrupted copies and what the host says about each: made once."""
    if name in _made:
        return _made[name]
    kind, n, nq, pow_bits, qs = SHAPES[name]
    params = pk.default_params()
    params.num_queries, params.pow_bits = nq, pow_bits
    if kind == 2:
        s, x = synth.fq_inputs(n, seed=31 + n)
        o = None
        pr = ctx.prove_fq_exp(s, x, params=params)
    else:
        s, x, o = (synth.g1_inputs if kind == 0 else synth.g2_inputs)(n, seed=31 + n)
        pr = (ctx.prove_g1 if kind == 0 else ctx.prove_g2)(s, x, o, params=params)
    words, outs, db = pr.words.copy(), pr.outputs.copy(), pr.degree_bits
    lay = vc.layout(kind, db, params)
    rc, rec = pk.verify_front(kind, words, db, params)
    assert rc == 0 and words.size == lay["total"]
    cases = [c for i, q in enumerate(qs) for c in vc.query_cases(lay, rec, q, full=False, rot=i)]
    copies = [words] + [vc.flipped(words, at) for _, at, _, _ in cases]
    expect = np.zeros((len(copies), nq), dtype=np.int32)
    for k, (cname, _, code, _) in enumerate(cases):
        expect[1 + k, int(cname.split()[0][1:])] = code
    host_codes = pk.query_round(kind, copies, db, np.stack([rec] * len(copies)), params=params)
    fronts = [vc.flipped(words, at) for _, at, _ in vc.front_cases(lay)]
    every = copies + fronts
    alone = [vc.verify_host_text(kind, w, db, s, x, o, outs, params) for w in every]
    d = dict(kind=kind, n=n, s=s, x=x, o=o, words=words, outs=outs, db=db, params=params, lay=lay, rec=rec, cases=cases,
             copies=copies, expect=expect, host_codes=host_codes, every=every, alone=alone)
    _made[name] = d
    return d


def tiled(a, k):
    return None if a is None else np.concatenate([a] * k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_query_round_equals_the_host(gpu_ctx, name):
    d = shape(gpu_ctx, name)
    if name == "g1_200_tall":
        assert d["db"] == 17
    # the host functions give the table's code at the touched query and 0 elsewhere ...
    assert np.array_equal(d["host_codes"], d["expect"]), [(c[0], np.nonzero(h)[0], h[h != 0])
                                                          for c, h, e in zip([("untouched",)] + d["cases"], d["host_codes"], d["expect"])
                                                          if not np.array_equal(h, e)]
    # ... and the kernels give what the host functions give, in every code of every proof
    dev = gpu_ctx.query_round(d["kind"], d["copies"], d["db"], np.stack([d["rec"]] * len(d["copies"])), params=d["params"])
    assert np.array_equal(dev, d["host_codes"]), np.argwhere(dev != d["host_codes"])[:10]


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_batch_verdicts_equal_verify_host(gpu_ctx, name):
    d = shape(gpu_ctx, name)
    k = len(d["every"])
    texts = [None] + [c[3] for c in d["cases"]] + [t for _, _, t in vc.front_cases(d["lay"])]
    assert d["alone"] == texts
    got = gpu_ctx.verify_batch(d["kind"], [(w, d["outs"]) for w in d["every"]], tiled(d["s"], k), tiled(d["x"], k), tiled(d["o"], k),
                               params=d["params"], degree_bits=d["db"])
    assert got == d["alone"], [(i, g, a) for i, (g, a) in enumerate(zip(got, d["alone"])) if g != a]
    err = pk.load_library().bn254s_last_error(gpu_ctx._h).decode()
    assert err == "proof 1: " + d["alone"][1]
    assert gpu_ctx.verify_batch(d["kind"], [(d["words"], d["outs"])] * 2, tiled(d["s"], 2), tiled(d["x"], 2), tiled(d["o"], 2),
                                params=d["params"], degree_bits=d["db"]) == [None, None]


def test_crafted_records_on_the_device(gpu_ctx):
    d = shape(gpu_ctx, "g1_3")
    cases = vc.crafted(d["lay"], d["words"], d["rec"], 84)
    assert len(cases) == 5
    dev = gpu_ctx.query_round(0, [c[1] for c in cases], d["db"], np.stack([c[2] for c in cases]))
    for k, (cname, _, _, expect) in enumerate(cases):
        assert np.array_equal(dev[k], expect), (cname, dev[k])
    assert pk.query_text(d["lay"]["L"], 4 + 2 * d["lay"]["L"]) == vc.TEXT_FINAL


@pytest.fixture(scope="module")
def eight(gpu_ctx):
    s, x, o = synth.g1_inputs(24, seed=77)
    proofs = gpu_ctx.prove_batch(0, s, x, o, per_proof=3)
    assert len(proofs) == 8
    return s, x, o, [(p.words.copy(), p.outputs.copy()) for p in proofs], proofs[0].degree_bits


def test_distinct_proofs(gpu_ctx, eight):
    s, x, o, proofs, db = eight
    assert gpu_ctx.verify_batch(0, proofs, s, x, o, degree_bits=db) == [None] * 8
    lay = vc.layout(0, db)
    bad = list(proofs)
    bad[2] = (vc.flipped(proofs[2][0], lay["queries"] + 17 * lay["wpq"] + 9), proofs[2][1])
    bad[5] = (vc.flipped(proofs[5][0], lay["queries"] + 80 * lay["wpq"] + lay["layers"][1][1] + 2), proofs[5][1])
    outs4 = proofs[4][1].copy()
    outs4.reshape(-1, 8)[13 - 12, 2] ^= np.uint64(1)  # job 13 is the second job of proof 4
    bad[4] = (proofs[4][0], outs4)
    got = gpu_ctx.verify_batch(0, bad, s, x, o, degree_bits=db)
    assert [i for i, g in enumerate(got) if g is not None] == [2, 4, 5], got
    assert got[4] == "CTL sum mismatch" and got[2] == vc.TEXT_INITIAL and got[5] == vc.TEXT_LAYER
    for i in (2, 4, 5):
        assert got[i] == vc.verify_host_text(0, bad[i][0], db, s[3 * i:3 * i + 3], x[3 * i:3 * i + 3], o[3 * i:3 * i + 3], bad[i][1])
    assert got == pk.verify_batch_host(0, bad, s, x, o, degree_bits=db)


def test_chunking(gpu_ctx):
    d = shape(gpu_ctx, "g1_3")
    five = d["copies"][:5]
    recs = np.stack([d["rec"]] * 5)
    whole = gpu_ctx.query_round(0, five, d["db"], recs, chunk_proofs=0)
    assert np.array_equal(gpu_ctx.query_round(0, five, d["db"], recs, chunk_proofs=2), whole)
    assert np.array_equal(whole, d["host_codes"][:5]) and whole[1:].any()


def test_inside_an_open_batch(gpu_ctx, eight):
    d = shape(gpu_ctx, "g1_3")
    s, x, o, undisturbed, db = eight
    k = len(d["every"])
    args = (0, [(w, d["outs"]) for w in d["every"]], tiled(d["s"], k), tiled(d["x"], k), tiled(d["o"], k))
    batch = gpu_ctx.prove_batch_begin(0, s, x, o, per_proof=3)
    got = gpu_ctx.verify_batch(*args, degree_bits=d["db"])
    proofs = batch.end()
    assert got == d["alone"]
    assert len(proofs) == 8
    for p, (w, outs) in zip(proofs, undisturbed):
        assert np.array_equal(p.words, w) and np.array_equal(p.outputs, outs)
