"""bn254s_verify_batch without a context (no GPU): the batch verifier's verdicts, the query round (csrc/verify_query.h) pinned
query by query on the host, crafted front records and the refusals, on one proof made by the CPU oracle.  The device form of the
same functions is compared against this one in tests/test_gpu_verify_batch.py.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import synth
from tests import oracle_lib
from tests import verify_batch_cases as vc

KIND, NQ = 2, 84


@pytest.fixture(scope="module")
def fq(oracle):
    s, x = synth.fq_inputs(3, seed=0xA4)
    words, outs, _, degree_bits = oracle_lib.prove(oracle, KIND, s, x)
    lay = vc.layout(KIND, degree_bits)
    rc, rec = pk.verify_front(KIND, words, degree_bits)
    assert rc == 0
    return dict(s=s, x=x, words=words, outs=outs, db=degree_bits, lay=lay, rec=rec)


def test_layout_is_the_documented_one(fq):
    lay = fq["lay"]
    assert fq["words"].size == lay["total"] and lay["queries"] == 2640 and lay["wpq"] == 877 and lay["L"] == 3
    assert lay["trees"] == [(0, 427, 427, 52), (479, 134, 613, 52), (665, 4, 669, 52)]
    assert lay["layers"] == [(721, 753, 36), (789, 821, 20), (841, 873, 4)]


def test_batch_verdicts(fq):
    lay, words, rec, db = fq["lay"], fq["words"], fq["rec"], fq["db"]
    per_q = {name: (at, text) for name, at, _, text in vc.query_cases(lay, rec, 41, full=True)}
    rows = ["q41 tree0 leaf", "q41 tree1 path", "q41 layer1 queried c0", "q41 layer1 other evals", "q41 layer2 path"]
    copies = [("untouched", words, fq["s"], None)]
    copies += [(name, vc.flipped(words, per_q[name][0]), fq["s"], per_q[name][1]) for name in rows]  # one per row of the table
    copies += [(name, vc.flipped(words, at), fq["s"], text) for name, at, text in vc.front_cases(lay)]
    s2 = fq["s"].copy()
    s2[1, 0] ^= np.uint64(2)
    copies.append(("flipped scalar", words, s2, "CTL sum mismatch"))
    copies.append(("local_values", vc.flipped(words, 192 + 7), fq["s"], "Mismatch between evaluation and opening of quotient polynomial"))
    copies.append(("cut short", words[:-1].copy(), fq["s"], "bad proof shape"))
    assert {c[3] for c in copies} >= {None, vc.TEXT_INITIAL, vc.TEXT_CONSISTENCY, vc.TEXT_LAYER, vc.TEXT_POW}

    def run(cs):
        proofs = [(w, fq["outs"]) for _, w, _, _ in cs]
        s = np.concatenate([c[2] for c in cs])
        x = np.concatenate([fq["x"]] * len(cs))
        return pk.verify_batch_host(KIND, proofs, s, x, None, degree_bits=db)

    alone = [vc.verify_host_text(KIND, w, db, s, fq["x"], None, fq["outs"]) for _, w, s, _ in copies]
    assert alone == [c[3] for c in copies], list(zip([c[0] for c in copies], alone))
    got = run(copies)
    assert got == alone, list(zip([c[0] for c in copies], got, alone))
    assert run(copies[::-1]) == alone[::-1]
    assert run([copies[0]] * 3) == [None, None, None]


def _raw_batch(fq, word_arrays, s=None, n_jobs=3, status=True, err_stride=64, kind=KIND, params=None, n_proofs=None, x=True,
               outputs=True, jobs=True, words=True, err=True):
    """bn254s_verify_batch through ctypes with every argument in reach: (return code, status, texts)."""
    lib = pk.load_library()
    params = params or pk.default_params()
    n = len(word_arrays)
    arrs = [np.ascontiguousarray(w, dtype=np.uint64) for w in word_arrays]
    table = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    s = np.ascontiguousarray(np.concatenate([fq["s"]] * n) if s is None else s)
    xs = np.ascontiguousarray(np.concatenate([fq["x"]] * n))
    outs = np.ascontiguousarray(np.concatenate([fq["outs"].reshape(-1)] * n))
    nj = (C.c_size_t * n)(*([n_jobs] * n))
    st = np.full(n, 99, dtype=np.int32)
    buf = C.create_string_buffer(n * max(err_stride, 1))
    vp = C.c_void_p
    rc = lib.bn254s_verify_batch(None, kind, C.byref(params), fq["db"], table if words else None, arrs[0].size,
                                 s.ctypes.data_as(vp), xs.ctypes.data_as(vp) if x else None, None,
                                 outs.ctypes.data_as(vp) if outputs else None, nj if jobs else None, n if n_proofs is None else n_proofs,
                                 st.ctypes.data_as(vp) if status else None, buf if err else None, err_stride)
    texts = [buf.raw[i * err_stride:(i + 1) * err_stride].split(b"\0", 1)[0].decode() for i in range(n)] if err_stride else []
    return rc, st, texts


def test_return_codes_and_status_arrays(fq):
    lay, words = fq["lay"], fq["words"]
    rc, st, texts = _raw_batch(fq, [words, words])
    assert rc == 0 and list(st) == [0, 0] and texts == ["", ""]
    bad = vc.flipped(words, lay["queries"] + 5)
    rc, st, texts = _raw_batch(fq, [words, bad, words])
    assert rc == -8 and list(st) == [0, -8, 0] and texts == ["", vc.TEXT_INITIAL, ""]
    rc, st, _ = _raw_batch(fq, [bad, words], err=False)  # err may be NULL
    assert rc == -8 and list(st) == [-8, 0]
    rc, st, texts = _raw_batch(fq, [bad], err_stride=8)  # a short buffer gets the text cut, NUL-terminated
    assert rc == -8 and texts == [vc.TEXT_INITIAL[:7]]


def test_query_round_on_the_host(fq):
    lay, words, rec, db = fq["lay"], fq["words"], fq["rec"], fq["db"]
    assert not pk.query_round(KIND, [words], db, rec[None]).any()
    cases = [c for q in (0, 41, 83) for c in vc.query_cases(lay, rec, q, full=True)]
    assert len(cases) == 3 * (6 + 3 * 4)
    codes = pk.query_round(KIND, [vc.flipped(words, at) for _, at, _, _ in cases], db, np.stack([rec] * len(cases)))
    for k, (name, at, code, text) in enumerate(cases):
        q = int(name.split()[0][1:])
        expect = np.zeros(NQ, dtype=np.int32)
        expect[q] = code
        assert np.array_equal(codes[k], expect), (name, at, np.nonzero(codes[k])[0], codes[k][codes[k] != 0])
        assert pk.query_text(lay["L"], code) == text
    # the text of the table is what the whole verifier says about such a proof (a sample: one case per code)
    seen = {}
    for name, at, code, text in cases:
        seen.setdefault(code, (name, at, text))
    assert sorted(seen) == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    for code, (name, at, text) in seen.items():
        assert vc.verify_host_text(KIND, vc.flipped(words, at), db, fq["s"], fq["x"], None, fq["outs"]) == text, name


def test_front_cases_never_reach_the_query_round(fq):
    for name, at, text in vc.front_cases(fq["lay"]):
        rc, _ = pk.verify_front(KIND, vc.flipped(fq["words"], at), fq["db"])
        assert rc == -8, name
        assert vc.verify_host_text(KIND, vc.flipped(fq["words"], at), fq["db"], fq["s"], fq["x"], None, fq["outs"]) == text


def test_crafted_records(fq):
    lay, db = fq["lay"], fq["db"]
    cases = vc.crafted(lay, fq["words"], fq["rec"], NQ)
    assert [c[0] for c in cases] == ["final_poly in the words", "fri_betas[1]", "fri_betas[L-1]", "reduced[0]", "query index"]
    codes = pk.query_round(KIND, [c[1] for c in cases], db, np.stack([c[2] for c in cases]))
    for k, (name, _, _, expect) in enumerate(cases):
        assert np.array_equal(codes[k], expect), (name, codes[k])
    assert pk.query_text(lay["L"], 4 + 2 * lay["L"]) == vc.TEXT_FINAL
    assert pk.query_text(lay["L"], 8) == vc.TEXT_CONSISTENCY and pk.query_text(lay["L"], 0) == ""
    assert pk.query_text(lay["L"], 5 + 2 * lay["L"]) is None


def test_query_round_refuses_bad_records(fq):
    rec = fq["rec"].copy()
    rec[vc.REC_HEAD + 3] = np.uint64(1 << (fq["db"] + 1))  # a query index past the domain would address past the caps
    with pytest.raises(RuntimeError, match="-1"):
        pk.query_round(KIND, [fq["words"]], fq["db"], rec[None])
    rec = fq["rec"].copy()
    rec[0] = np.uint64(0xFFFFFFFF00000001)
    with pytest.raises(RuntimeError, match="-1"):
        pk.query_round(KIND, [fq["words"]], fq["db"], rec[None])
    with pytest.raises(RuntimeError, match="-1"):
        pk.query_round(KIND, [fq["words"][:-1]], fq["db"], fq["rec"][None])


def test_refusals(fq):
    w = [fq["words"]]
    assert _raw_batch(fq, w)[0] == 0
    for kw in (dict(words=False), dict(x=False), dict(outputs=False), dict(jobs=False), dict(status=False)):  # a null array
        assert _raw_batch(fq, w, **kw)[0] == -1, kw
    assert _raw_batch(fq, w, n_proofs=0)[0] == -1
    assert _raw_batch(fq, w, err_stride=0)[0] == -1
    assert _raw_batch(fq, w, err_stride=0, err=False)[0] == 0  # no err array: the stride is not looked at
    assert _raw_batch(fq, w, kind=3)[0] == -1 and _raw_batch(fq, w, kind=-1)[0] == -1
    p = pk.default_params()
    p.struct_size += 4
    assert _raw_batch(fq, w, params=p)[0] == -1
    assert _raw_batch(fq, w, n_jobs=0)[0] == -1
