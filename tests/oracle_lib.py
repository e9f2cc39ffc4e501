"""ctypes loader for the CPU oracle (oracle/liboracle.so).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "oracle", "liboracle.so")
_lib = None
VP = C.c_void_p


def load():
    global _lib
    if _lib is not None:
        return _lib
    # make checks the dependencies itself: a library older than one of its sources is rebuilt, an up-to-date one costs a stat each
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(PATH)
    lib.orc_last_error.restype = C.c_char_p
    lib.orc_gl_mul.restype = C.c_uint64
    lib.orc_gl_mul.argtypes = [C.c_uint64, C.c_uint64]
    lib.orc_gl_inv.restype = C.c_uint64
    lib.orc_gl_inv.argtypes = [C.c_uint64]
    lib.orc_poseidon_permute.argtypes = [VP]
    lib.orc_hash_or_noop.argtypes = [VP, C.c_size_t, VP]
    lib.orc_two_to_one.argtypes = [VP, VP, VP]
    lib.orc_merkle_cap.argtypes = [VP, C.c_size_t, C.c_size_t, C.c_int, VP]
    lib.orc_challenger_observe_get.argtypes = [VP, C.c_size_t, VP, C.c_size_t]
    lib.orc_ntt.argtypes = [VP, C.c_size_t, C.c_int, C.c_uint64]
    lib.orc_commit_values.argtypes = [VP, C.c_size_t, C.c_size_t, VP, VP, VP]
    lib.orc_fq_mul.argtypes = [VP, VP, VP]
    lib.orc_fq_inv.argtypes = [VP, VP]
    lib.orc_g1_add.argtypes = [VP, VP, VP]
    lib.orc_generate_modulus_zero.argtypes = [VP, VP]
    lib.orc_g1_num_rows.restype = C.c_size_t
    lib.orc_g1_num_rows.argtypes = [C.c_size_t, C.c_int]
    lib.orc_g1_generate_trace.argtypes = [VP, VP, VP, C.c_size_t, C.c_int, VP, VP]
    lib.orc_g1_eval_constraints.argtypes = [VP, VP, VP, C.c_uint64, C.c_uint64, C.c_uint64, VP]
    lib.orc_g1_proof_len.restype = C.c_size_t
    lib.orc_g1_proof_len.argtypes = [C.c_int]
    lib.orc_g1_prove.argtypes = [VP, VP, VP, C.c_size_t, C.c_int, VP, C.c_size_t, VP, VP]
    lib.orc_g1_verify.argtypes = [VP, C.c_size_t, C.c_int, VP, VP, VP, C.c_size_t]
    lib.orc_stark_width.argtypes = [C.c_int]
    lib.orc_proof_len.restype = C.c_size_t
    lib.orc_proof_len.argtypes = [C.c_int, C.c_int]
    lib.orc_generate_trace.argtypes = [C.c_int, VP, VP, VP, C.c_size_t, C.c_int, VP, VP]
    lib.orc_prove.argtypes = [C.c_int, VP, VP, VP, C.c_size_t, C.c_int, VP, C.c_size_t, VP, VP]
    lib.orc_verify.argtypes = [C.c_int, VP, C.c_size_t, C.c_int, VP, VP, VP, C.c_size_t]
    lib.orc_eval_constraints.argtypes = [C.c_int, VP, VP, VP, C.c_uint64, C.c_uint64, C.c_uint64, VP]
    lib.orc_aux_width.argtypes = [C.c_int]
    lib.orc_eval_vanishing_values.argtypes = [C.c_int, VP, VP, VP, VP, VP, VP, C.c_uint64, C.c_uint64, C.c_uint64, VP]
    lib.orc_eval_vanishing_values_at.argtypes = [C.c_int, VP, VP, C.c_size_t, C.c_size_t, VP, VP, VP, VP, VP, VP, VP, VP, C.c_size_t]
    lib.orc_aux_columns.argtypes = [C.c_int, VP, C.c_size_t, VP, VP, VP]
    _lib = lib
    return lib


def ptr(a):
    return a.ctypes.data_as(VP) if a is not None else None


def commit_values(lib, values):
    C_, N = values.shape
    coeffs = np.zeros((C_, N), np.uint64)
    lde = np.zeros((C_, 2 * N), np.uint64)
    cap = np.zeros((16, 4), np.uint64)
    lib.orc_commit_values(ptr(values), C_, N, ptr(coeffs), ptr(lde), ptr(cap))
    return coeffs, lde, cap


def g1_prove(lib, s, x, o, min_rows_log2=16):
    n = s.shape[0]
    rows = lib.orc_g1_num_rows(n, min_rows_log2)
    degree_bits = rows.bit_length() - 1
    plen = lib.orc_g1_proof_len(degree_bits)
    proof = np.zeros(plen, np.uint64)
    outs = np.zeros((n, 8), np.uint64)
    tm = np.zeros(8)
    r = lib.orc_g1_prove(ptr(s), ptr(x), ptr(o), n, min_rows_log2, ptr(proof), plen, ptr(outs), tm.ctypes.data_as(VP))
    if r < 0:
        raise RuntimeError(lib.orc_last_error().decode())
    return proof[:r], outs, tm, degree_bits


def g1_verify(lib, proof, degree_bits, s, x, o):
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    r = lib.orc_g1_verify(ptr(proof), proof.shape[0], degree_bits, ptr(s), ptr(x), ptr(o), s.shape[0])
    return r, lib.orc_last_error().decode()


POINT_WORDS = {0: 8, 1: 16, 2: 4}


def generate_trace(lib, kind, s, x, o=None, min_rows_log2=16):
    n = s.shape[0]
    rows = lib.orc_g1_num_rows(n, min_rows_log2)
    tr = np.zeros((lib.orc_stark_width(kind), rows), np.uint64)
    outs = np.zeros((n, POINT_WORDS[kind]), np.uint64)
    rc = lib.orc_generate_trace(kind, ptr(s), ptr(x), ptr(o), n, min_rows_log2, ptr(tr), ptr(outs))
    if rc != 0:
        raise RuntimeError(lib.orc_last_error().decode())
    return tr, outs


def prove(lib, kind, s, x, o=None, min_rows_log2=16):
    n = s.shape[0]
    rows = lib.orc_g1_num_rows(n, min_rows_log2)
    degree_bits = rows.bit_length() - 1
    plen = lib.orc_proof_len(kind, degree_bits)
    proof = np.zeros(plen, np.uint64)
    outs = np.zeros((n, POINT_WORDS[kind]), np.uint64)
    tm = np.zeros(8)
    r = lib.orc_prove(kind, ptr(s), ptr(x), ptr(o), n, min_rows_log2, ptr(proof), plen, ptr(outs), tm.ctypes.data_as(VP))
    if r < 0:
        raise RuntimeError(lib.orc_last_error().decode())
    return proof[:r], outs, tm, degree_bits


def vanishing_values(lib, kind, local, nxt, aux_local, aux_next, betas, gammas, z_last, lfirst, llast):
    """Every constraint value of one point in emission order (AIR, lookups, CTLs), as Python integers."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint64) for a in (local, nxt, aux_local, aux_next, betas, gammas)]
    out = np.zeros(4096, np.uint64)
    k = lib.orc_eval_vanishing_values(kind, *[ptr(a) for a in arrs], int(z_last), int(lfirst), int(llast), ptr(out))
    return [int(v) for v in out[:k]]


def vanishing_values_at(lib, kind, trace, aux, idx_local, idx_next, betas, gammas, z_last, lfirst, llast):
    """values[n][K] (uint64) for the n points whose local / next rows are the positions idx_local / idx_next of the column-major
    trace[W][stride], aux[A][stride]."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    aux = np.ascontiguousarray(aux, dtype=np.uint64)
    stride = trace.shape[1]
    assert trace.shape[0] == lib.orc_stark_width(kind) and aux.shape == (lib.orc_aux_width(kind), stride)
    v = [np.ascontiguousarray(a, dtype=np.uint64) for a in (idx_local, idx_next, betas, gammas, z_last, lfirst, llast)]
    n = v[0].shape[0]
    assert all(a.shape == (n,) for a in (v[1], v[4], v[5], v[6])) and int(max(v[0].max(), v[1].max())) < stride
    cap = 4096
    out = np.zeros((n, cap), np.uint64)
    k = lib.orc_eval_vanishing_values_at(kind, ptr(trace), ptr(aux), stride, n, *[ptr(a) for a in v], ptr(out), cap)
    assert 0 < k <= cap
    return out[:, :k]


def aux_columns(lib, kind, trace, betas, gammas):
    """out[A][N] of trace[W][N]: the oracle's LogUp columns per challenge, then its CTL Z columns.  RuntimeError with the
    oracle's text on a filter that is not 0 or 1."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    b = np.array([int(v) for v in betas], dtype=np.uint64)
    g = np.array([int(v) for v in gammas], dtype=np.uint64)
    out = np.zeros((lib.orc_aux_width(kind), trace.shape[1]), np.uint64)
    if lib.orc_aux_columns(kind, ptr(trace), trace.shape[1], ptr(b), ptr(g), ptr(out)) != 0:
        raise RuntimeError(lib.orc_last_error().decode())
    return out


def verify(lib, kind, proof, degree_bits, s, x, o=None):
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    r = lib.orc_verify(kind, ptr(proof), proof.shape[0], degree_bits, ptr(s), ptr(x), ptr(o), s.shape[0])
    return r, lib.orc_last_error().decode()
