"""Shared by tests/test_verify_batch_cpu.py and tests/test_gpu_verify_batch.py: where the words of a query round sit in a proof
(the layout of include/bn254_stark.h, as make_view of csrc/verify_query.h walks it), one-bit corruptions of them with the code and
the text the verifier must answer, and crafted front records."""
import numpy as np

import plonky2_bn254_amd as pk

REC_HEAD = pk.lib.VERIFY_RECORD_HEAD
REC_REDUCED, REC_BETAS = 2, 18
TEXT_INITIAL = "Invalid Merkle proof (initial tree)"
TEXT_CONSISTENCY = "FRI consistency check failed"
TEXT_LAYER = "Invalid Merkle proof (FRI layer)"
TEXT_FINAL = "Final polynomial evaluation is invalid"
TEXT_POW = "Invalid proof of work witness"


def layout(kind, degree_bits, params=None):
    """Offsets of one proof: queries, wpq, per initial tree (leaf, leaf words, path, path words), per FRI layer (evals, path,
    path words), fri_caps, final_poly, pow."""
    params = params or pk.default_params()
    plan = pk.proof_plan(kind, 1, 0)
    w, a = plan["W"], plan["A"]
    path = degree_bits + params.rate_bits - params.cap_height
    trees, pos = [], 0
    for width in (w, a, 4):
        trees.append((pos, width, pos + width, 4 * path))
        pos += width + 4 * path
    layers, d, bits = [], degree_bits, degree_bits + params.rate_bits
    while d > params.final_poly_bits and d + params.rate_bits - params.arity_bits >= params.cap_height:
        d -= params.arity_bits
        bits -= params.arity_bits
        n_ev = 2 << params.arity_bits
        layers.append((pos, pos + n_ev, 4 * (bits - params.cap_height)))
        pos += n_ev + 4 * (bits - params.cap_height)
    fri_caps = 192 + 4 * w + 4 * a + 4 + 8
    queries = fri_caps + 64 * len(layers)
    final_poly = queries + params.num_queries * pos
    lay = dict(trees=trees, layers=layers, L=len(layers), wpq=pos, fri_caps=fri_caps, queries=queries, final_poly=final_poly,
               pow=final_poly + (2 << d), total=final_poly + (2 << d) + 1 + 12, arity_bits=params.arity_bits)
    assert lay["total"] == pk.proof_words(kind, degree_bits, params)
    return lay


def flipped(words, at, bit=0):
    bad = words.copy()
    bad[at] ^= np.uint64(1 << bit)
    return bad


def query_cases(lay, rec, q, full=True, rot=0):
    """[(name, word, code, text)] for one-bit corruptions inside query q.  full: every row of the table for every tree and layer
    (a leaf and a path word per tree; both words at the queried position, another evals word and a path word per layer);
    otherwise a rotating selection (rot) that still takes one case per tree and the three kinds of one layer."""
    base = lay["queries"] + lay["wpq"] * q
    x_index = int(rec[REC_HEAD + q])
    ab = lay["arity_bits"]
    out = []
    for t, (leaf, leaf_len, path, path_len) in enumerate(lay["trees"]):
        picks = [("leaf", leaf + (7 * q + 3) % leaf_len), ("path", path + (5 * q + 1) % path_len)]
        if not full:
            picks = [picks[(t + rot) % 2]]
        for what, at in picks:
            out.append((f"q{q} tree{t} {what}", base + at, 1 + t, TEXT_INITIAL))
    layers = range(lay["L"]) if full else [rot % lay["L"]]
    for l in layers:
        evals, path, path_len = lay["layers"][l]
        within = (x_index >> (ab * l)) & ((1 << ab) - 1)
        other = (within + 1 + q % ((1 << ab) - 1)) % (1 << ab)
        assert other != within
        comps = (0, 1) if full else ((q + rot) % 2,)
        for comp in comps:
            out.append((f"q{q} layer{l} queried c{comp}", base + evals + 2 * within + comp, 4 + 2 * l, TEXT_CONSISTENCY))
        out.append((f"q{q} layer{l} other evals", base + evals + 2 * other + q % 2, 5 + 2 * l, TEXT_LAYER))
        if path_len:
            out.append((f"q{q} layer{l} path", base + path + (3 * q) % path_len, 5 + 2 * l, TEXT_LAYER))
    return out


def front_cases(lay):
    """Corruptions the front catches at the proof-of-work check (they shift the transcript): never sent to the query round."""
    return [("final_poly", lay["final_poly"] + 3, TEXT_POW), ("fri_caps", lay["fri_caps"] + 70, TEXT_POW),
            ("witness", lay["pow"], TEXT_POW)]


def crafted(lay, words, rec, nq):
    """[(name, words, record, expected codes[nq])]: the honest record of the untouched proof, changed in one place."""
    L = lay["L"]
    out = []
    full = lambda code: np.full(nq, code, dtype=np.int32)
    out.append(("final_poly in the words", flipped(words, lay["final_poly"]), rec, full(4 + 2 * L)))

    def rec_with(at):
        r = rec.copy()
        r[at] ^= np.uint64(1)
        return r
    if L >= 3:
        out.append(("fri_betas[1]", words, rec_with(REC_BETAS + 2 * 1), full(8)))
    out.append(("fri_betas[L-1]", words, rec_with(REC_BETAS + 2 * (L - 1) + 1), full(4 + 2 * L)))
    out.append(("reduced[0]", words, rec_with(REC_REDUCED), full(4)))
    q = nq // 2
    one = np.zeros(nq, dtype=np.int32)
    # a query index with bit 0 flipped is the sibling leaf: the honest leaf no longer hashes to the cap - unless another query
    # already sits there, which changes nothing for query q itself
    one[q] = 1
    out.append(("query index", words, rec_with(REC_HEAD + q), one))
    return out


def verify_host_text(kind, words, degree_bits, s, x, o, outputs, params=None):
    try:
        pk.verify_host(kind, words, degree_bits, s, x, o, outputs, params)
        return None
    except pk.VerifyError as e:
        return str(e)
