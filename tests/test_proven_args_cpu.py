"""The argument ladder of the proven entry points (csrc/proven_jobs.h: proven_args) over every full call from one table, without
a GPU and without a context: a valid shape answers BN254S_E_INVALID_ARG (no context), per_proof above 16384 answers
BN254S_E_UNSUPPORTED with the slots of the call cleared and the next one untouched, and each NULL pointer alone answers
BN254S_E_INVALID_ARG before the shape is looked at.  The per-feature tests (test_*_cpu.py: test_entry_points_check_their_arguments,
test_map_to_g1_checks_its_arguments) pin the same order call by call."""
import ctypes as C

import numpy as np
import pytest

import plonky2_bn254_amd as pk

E_ARG, E_UNSUP = -1, -5
N = 3
PARAMS, PER_PROOF, SLOTS = "params", "per_proof", "slots"  # the places of the ladder's own arguments in a call


class Opt:
    """A pointer argument that may be NULL."""

    def __init__(self, a):
        self.a = a


def _u64(*shape):
    return np.zeros(shape, np.uint64)


def _u8(*shape):
    return np.zeros(shape, np.uint8)


def _job_outputs(kind, pw):
    offset = _u64(N, pw) if kind != 2 else Opt(None)  # (not read for Fq exp)
    return ("bn254s_job_outputs", [kind, PARAMS, _u64(N, 4), _u64(N, pw), offset, N, PER_PROOF, _u64(N, pw), SLOTS], N, 16384)


# entry point, arguments after the context, jobs of the call, largest valid per_proof
CALLS = [
    ("bn254s_g1_msm", [PARAMS, _u64(N, 4), _u64(N, 8), _u64(8), N, PER_PROOF, _u64(8), Opt(_u64(N + 1, 8)), SLOTS], N, 16384),
    ("bn254s_g2_msm", [PARAMS, _u64(N, 4), _u64(N, 16), _u64(16), N, PER_PROOF, _u64(16), Opt(_u64(N + 1, 16)), SLOTS], N, 16384),
    ("bn254s_g1_recover_from_x", [PARAMS, _u64(N, 4), N, PER_PROOF, _u64(N, 8), _u8(N), Opt(_u64(N, 8)), SLOTS], N, 16384),
    ("bn254s_g2_recover_from_x", [PARAMS, _u64(N, 8), Opt(_u8(N)), N, PER_PROOF, _u64(N, 16), _u8(N), Opt(_u64(N, 8)), SLOTS], N, 16384),
    ("bn254s_g2_subgroup_check", [PARAMS, _u64(N, 16), _u64(N, 16), N, PER_PROOF, _u8(N), Opt(_u64(N, 20)), SLOTS], N, 16384),
    ("bn254s_g2_clear_cofactor", [PARAMS, _u64(N, 16), _u64(N, 16), N, PER_PROOF, _u64(N, 16), _u8(N), Opt(_u64(N, 20)), SLOTS], N, 16384),
    _job_outputs(0, 8),
    _job_outputs(1, 16),
    _job_outputs(2, 4),
    ("bn254s_map_to_g1", [PARAMS, _u64(N, 4), N, PER_PROOF, _u64(N, 8), Opt(_u8(2 * N)), Opt(_u64(2 * N, 8)), SLOTS], 2 * N, 16384),
]


def _call(lib, name, args, per_proof, null=None, params=None):
    """The entry point without a context and with every slot preset to the marker 1; argument `null` (an index) is passed as NULL.
    -> (return code, slots)."""
    params = params or pk.default_params()
    slots = (C.c_void_p * 8)(*([1] * 8))
    out = []
    for i, a in enumerate(args):
        if isinstance(a, Opt):
            a = a.a
        if i == null:
            out.append(None)
        elif isinstance(a, str):
            out.append({PARAMS: C.byref(params), PER_PROOF: per_proof, SLOTS: slots}[a])
        elif isinstance(a, np.ndarray):
            out.append(a.ctypes.data_as(C.c_void_p))
        else:
            out.append(a)
    return getattr(lib, name)(None, *out), list(slots)


@pytest.mark.parametrize("name,args,n_jobs,largest", CALLS, ids=[f"{c[0]}-{i}" for i, c in enumerate(CALLS)])
def test_argument_ladder(name, args, n_jobs, largest):
    lib = pk.load_library()
    # a valid shape: only the context is missing
    rc, slots = _call(lib, name, args, largest)
    assert rc == E_ARG and slots[0] is None and slots[1] == 1
    rc, slots = _call(lib, name, args, 2)
    count = (n_jobs + 1) // 2
    assert rc == E_ARG and slots[:count] == [None] * count and slots[count] == 1
    # per_proof above the limit: the shape answers before the context; slot 0 is cleared, the slot past the count is not touched
    rc, slots = _call(lib, name, args, 16385)
    assert rc == E_UNSUP and slots[0] is None and slots[1:] == [1] * 7
    # each NULL pointer alone answers before the shape and touches no slot; one that may be NULL changes nothing
    for i, a in enumerate(args):
        if isinstance(a, np.ndarray) or a in (PARAMS, SLOTS):
            rc, slots = _call(lib, name, args, 16385, null=i)
            assert rc == E_ARG and (a is SLOTS or slots == [1] * 8), (name, i)
        elif isinstance(a, Opt):
            assert _call(lib, name, args, 16385, null=i)[0] == E_UNSUP, (name, i)
    # per_proof 0 and parameters of another size likewise
    assert _call(lib, name, args, 0) == (E_ARG, [1] * 8)
    bad = pk.default_params()
    bad.struct_size += 4
    assert _call(lib, name, args, 16385, params=bad) == (E_ARG, [1] * 8)
    for a in args:
        if isinstance(a, np.ndarray):
            assert not a.any()  # nothing was written
