"""The contract that the four one-job root front-ends share (bn254s_g1_recover_from_x, bn254s_g2_recover_from_x, bn254s_fq_sqrt,
bn254s_fq2_sqrt and their _batch forms), as one table: which input a call names when coordinates and sign bytes are both at
fault (the first input with either, its coordinates before its sign), the exact error text, that a rejected call writes nothing
and leaves every proof slot NULL, and that the proven call returns what the _batch call returns, word for word.  Every error
case is rejected on the host before any device work."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk
from tools import field_gadgets_ref as ref

P = ref.P
N = 8            # inputs of an error case
SENTINEL = 0x5A  # what every output array holds before a call that must not write

# kind -> (tag of the error text, words of an input, words of an output row, takes signs, has root_ok, Python front-end name)
KINDS = {
    "g1_recover": ("g1_recover_from_x", 4, 8, False, False, "g1_recover_from_x"),
    "g2_recover": ("g2_recover_from_x", 8, 16, True, False, "g2_recover_from_x"),
    "fq_sqrt": ("fq_sqrt", 4, 4, True, True, "fq_sqrt"),
    "fq2_sqrt": ("fq2_sqrt", 8, 8, True, True, "fq2_sqrt"),
}


def _inputs(kind, n):
    """n inputs below p and n sign bytes of both values (None for the kind without signs)."""
    _, w, _, signed, _, _ = KINDS[kind]
    xs = ref.fq_words(ref.random_fq(n, seed=61)) if w == 4 else ref.fq2_words(ref.random_fq2(n, seed=62))
    return xs, (ref.random_sgns(n, seed=63) if signed else None)


def _coord_text(kind, i, k):
    """What coordinate k of input i says when it is not below p."""
    tag, w = KINDS[kind][:2]
    return f"{tag}: x_{i} is not below p" if w == 4 else f"{tag}: x_{i} has c{k} not below p"


def _sgn_text(kind, i, v):
    return f"{KINDS[kind][0]}: sgn_{i} is {v}, neither 0 nor 1"


def _cases(kind):
    """(id, coordinate faults [(input, coordinate)], sign faults [input], the expected text)"""
    _, w, _, signed, _, _ = KINDS[kind]
    out = [(f"x_5.c{k}", [(5, k)], [], _coord_text(kind, 5, k)) for k in range(w // 4)]
    if signed:
        out += [("sgn_5", [], [5], _sgn_text(kind, 5, 2)),
                ("x_5+sgn_5", [(5, w // 4 - 1)], [5], _coord_text(kind, 5, w // 4 - 1)),
                ("sgn_3+x_5", [(5, 0)], [3], _sgn_text(kind, 3, 2)),
                ("x_3+sgn_5", [(3, 0)], [5], _coord_text(kind, 3, 0))]
    return out


ERROR_CASES = [pytest.param(kind, *case[1:], id=f"{kind}-{case[0]}") for kind in KINDS for case in _cases(kind)]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _raw_call(ctx, kind, proven, xs, sgns):
    """One call on sentinel-filled outputs -> (return code, error text, the output arrays, the proof slots or None)."""
    tag, w, ow, signed, has_ok, _ = KINDS[kind]
    n = xs.shape[0]
    name = f"bn254s_{tag}" + ("" if proven else "_batch")
    outs = [np.full((n, ow), SENTINEL, np.uint64), np.full(n, SENTINEL, np.uint8)]
    if has_ok:
        outs.append(np.full(n, SENTINEL, np.uint8))
    outs.append(np.full((n, 8), SENTINEL, np.uint64))
    args = [_vp(xs)] + ([_vp(sgns)] if signed else []) + [n]
    slots = None
    if proven:
        params = pk.default_params()
        slots = (C.c_void_p * 4)(*([1] * 4))  # per_proof = 2: the four slots of 8 jobs, preset to a non-NULL value
        args = [C.byref(params)] + args + [2]
    args += [_vp(a) for a in outs] + ([slots] if proven else [])
    rc = getattr(ctx._lib, name)(ctx._h, *args)
    return rc, ctx._lib.bn254s_last_error(ctx._h).decode(), outs, slots


def _faulty(kind, coord_faults, sgn_faults):
    xs, sgns = _inputs(kind, N)
    xs = xs.copy()
    for i, k in coord_faults:
        xs[i, 4 * k:4 * k + 4] = ref.to_words(P)
    if sgns is not None:
        sgns = sgns.copy()
        for i in sgn_faults:
            sgns[i] = 2
    return xs, sgns


@pytest.mark.gpu
@pytest.mark.parametrize("kind,coord_faults,sgn_faults,text", ERROR_CASES)
def test_batch_call_names_the_first_fault_and_writes_nothing(gpu_ctx, kind, coord_faults, sgn_faults, text):
    xs, sgns = _faulty(kind, coord_faults, sgn_faults)
    rc, got, outs, _ = _raw_call(gpu_ctx, kind, False, xs, sgns)
    assert rc == -1 and got == text, (rc, got)  # BN254S_E_INVALID_ARG
    assert all((a == SENTINEL).all() for a in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_proven_call_rejects_like_the_batch_call(gpu_ctx, kind):
    """The first case of the table through the proven entry point: the same code and text, every slot NULL, nothing written."""
    _, coord_faults, sgn_faults, text = _cases(kind)[0]
    xs, sgns = _faulty(kind, coord_faults, sgn_faults)
    rc, got, outs, slots = _raw_call(gpu_ctx, kind, True, xs, sgns)
    assert rc == -1 and got == text, (rc, got)
    assert list(slots) == [None] * 4
    assert all((a == SENTINEL).all() for a in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_proven_call_returns_what_the_batch_call_returns(gpu_ctx, kind):
    """n = 65: one block and one lane.  Outputs, flags and fq_jobs of the proven call equal the _batch call's word for word."""
    front = KINDS[kind][5]
    xs, sgns = _inputs(kind, 65)
    args = (xs,) if sgns is None else (xs, sgns)
    plain = getattr(gpu_ctx, front + "_batch")(*args)
    *proven, proofs = getattr(gpu_ctx, front)(*args, per_proof=128)
    assert len(proofs) == 1 and len(proven) == len(plain)
    for got, want in zip(proven, plain):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert 0 < int(plain[1].sum()) < 65  # both values of the flag
