"""ctypes binding of libbn254stark.so (include/bn254_stark.h).  No CPU fallback: if the HIP library is
missing or a call fails, an exception is raised."""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BN254S_LIB: another build of the same library (A/B measurements of compile-time knobs, tools/ubench/ab/); never a fallback
LIB_PATH = os.environ.get("BN254S_LIB") or os.path.join(_HERE, "libbn254stark.so")

U64P = C.POINTER(C.c_uint64)


class LibraryMissing(RuntimeError):
    pass


class VerifyError(RuntimeError):
    """bn254s_verify rejected the proof; the message is the reference verifier's error text."""


class UnprovableJobs(RuntimeError):
    """prove_batch_checked found jobs whose trace meets a + (-a) (-4): `provable` [n] uint8 and `step` [n] uint16 are the answer
    of the job check, step[i] the first hitting step of job i or JOB_STEP_NONE."""

    def __init__(self, msg, provable, step):
        super().__init__(msg)
        self.provable, self.step = provable, step


JOB_STEP_NONE = 0xFFFF  # BN254S_JOB_STEP_NONE
MSM_LINK_NONE = 0xFFFFFFFF  # BN254S_MSM_LINK_NONE
# BN254S_SUM_*: the codes of point_sum_check_batch (0..7) and the link codes of verify_scalar_mul / verify_msm_multi (0..10)
(SUM_OK, SUM_A_NOT_ZERO, SUM_A_OFF_CURVE, SUM_B_OFF_CURVE, SUM_C_OFF_CURVE, SUM_INFINITE, SUM_X, SUM_Y, SUM_X_OFF_CURVE, SUM_HEAD,
 SUM_CHAIN) = range(11)
# `what` of root_links_check_batch, and BN254S_ROOT_*: its codes, which are the link codes of the five root verifiers
ROOT_WHAT = (G1_RECOVER, G2_RECOVER, FQ_SQRT, FQ2_SQRT, MAP_TO_G1) = range(5)
(ROOT_OK, ROOT_JOB_SCALAR, ROOT_JOB_BASE, ROOT_FLAG, ROOT_CARRY, ROOT_NOT_ZERO, ROOT_SQUARE, ROOT_SIGN) = range(8)
_ROOT_IN_WORDS, _ROOT_OUT_WORDS = (4, 8, 4, 8, 4), (8, 16, 4, 8, 8)

# what msm_multi_chain / msm_multi return: results [m,PW], finite [m] uint8, offsets, outputs [n,PW], R [m,PW], attempts [m] uint8,
# bad_link [m] uint32, bad_step [m] uint16, and the proofs (None from msm_multi_chain)
MsmMulti = collections.namedtuple("MsmMulti", "results finite offsets outputs R attempts bad_link bad_step proofs")


class Params(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "struct_size", "security_bits", "num_challenges", "rate_bits", "cap_height", "pow_bits",
        "arity_bits", "final_poly_bits", "num_queries", "min_rows_log2")]


_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the proving path)")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.bn254s_abi_version.restype = C.c_int
    lib.bn254s_params_default.argtypes = [C.POINTER(Params)]
    lib.bn254s_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.bn254s_ctx_destroy.argtypes = [vp]
    lib.bn254s_ctx_trim.argtypes = [vp]
    lib.bn254s_last_error.argtypes = [vp]
    lib.bn254s_last_error.restype = C.c_char_p
    for name in ("bn254s_prove_g1", "bn254s_prove_g2"):
        getattr(lib, name).argtypes = [vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.POINTER(vp)]
    lib.bn254s_prove_fq_exp.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, C.POINTER(vp)]
    lib.bn254s_generate_trace.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
    lib.bn254s_prove_g1_batch.argtypes = [vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    lib.bn254s_prove_batch.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    lib.bn254s_prove_batch_begin.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, C.POINTER(vp),
                                             C.POINTER(vp)]
    lib.bn254s_prove_batch_end.argtypes = [vp]
    lib.bn254s_prove_batch_multi.argtypes = [C.POINTER(vp), C.c_size_t, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t,
                                             C.c_size_t, C.POINTER(vp)]
    lib.bn254s_proof_words.argtypes = [vp, C.POINTER(U64P), C.POINTER(C.c_size_t)]
    lib.bn254s_proof_outputs.argtypes = [vp, C.POINTER(U64P), C.POINTER(C.c_size_t)]
    lib.bn254s_proof_degree_bits.argtypes = [vp]
    lib.bn254s_proof_section.argtypes = [vp, C.c_int, C.POINTER(U64P), C.POINTER(C.c_size_t)]
    lib.bn254s_proof_stage_ms.argtypes = [vp, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t)]
    lib.bn254s_stage_name.argtypes = [C.c_size_t]
    lib.bn254s_stage_name.restype = C.c_char_p
    lib.bn254s_proof_free.argtypes = [vp]
    lib.bn254s_proof_serialize.argtypes = [vp, vp, C.c_size_t]
    lib.bn254s_proof_serialize.restype = C.c_size_t
    lib.bn254s_verify.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t]
    lib.bn254s_verify_host.argtypes = [C.c_int, C.POINTER(Params), C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, C.c_size_t, C.c_char_p,
                                       C.c_size_t]
    if hasattr(lib, "bn254s_verify_batch"):  # (absent from a library built before the batch verifier existed)
        lib.bn254s_verify_batch.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_size_t,
                                            vp, vp, C.c_size_t]
        lib.bn254s_selftest_verify_front.argtypes = [C.c_int, C.POINTER(Params), C.c_uint32, vp, C.c_size_t, vp, C.c_size_t]
        lib.bn254s_selftest_query_round.argtypes = [vp, C.c_int, C.POINTER(Params), C.c_uint32, vp, C.c_size_t, vp, C.c_size_t,
                                                    C.c_size_t, vp]
        lib.bn254s_selftest_verify_batch_ms.argtypes = [vp, vp]
        lib.bn254s_selftest_query_text.argtypes = [C.c_int, C.c_int]
        lib.bn254s_selftest_query_text.restype = C.c_char_p
    lib.bn254s_map_to_g2.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.bn254s_hash_to_fq2.argtypes = [vp, C.c_size_t, vp]
    lib.bn254s_g1_msm_chain.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_g1_msm.argtypes = [vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(vp)]
    lib.bn254s_g2_msm_chain.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_g2_msm.argtypes = [vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(vp)]
    lib.bn254s_g1_recover_from_x_batch.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    lib.bn254s_g1_recover_from_x.argtypes = [vp, C.POINTER(Params), vp, C.c_size_t, C.c_size_t, vp, vp, vp, C.POINTER(vp)]
    lib.bn254s_g2_recover_from_x_batch.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp]
    lib.bn254s_g2_recover_from_x.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, C.POINTER(vp)]
    for name in ("bn254s_fq_sqrt", "bn254s_fq2_sqrt"):
        getattr(lib, name + "_batch").argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
        getattr(lib, name).argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, C.POINTER(vp)]
    lib.bn254s_fq_inv_batch.argtypes = [vp, vp, C.c_size_t, vp]
    lib.bn254s_fq2_inv_batch.argtypes = [vp, vp, C.c_size_t, vp]
    lib.bn254s_g2_subgroup_check_batch.argtypes = [vp, vp, C.c_size_t, vp]
    lib.bn254s_g2_subgroup_check.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(vp)]
    lib.bn254s_g2_clear_cofactor_batch.argtypes = [vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_g2_clear_cofactor.argtypes = [vp, C.POINTER(Params), vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp, C.POINTER(vp)]
    lib.bn254s_map_to_g2_batch.argtypes = [vp, vp, C.c_size_t, vp]
    lib.bn254s_hash_to_g2_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    lib.bn254s_job_outputs_batch.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_job_outputs.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.POINTER(vp)]
    lib.bn254s_job_check_batch.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_prove_batch_checked.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp,
                                               C.POINTER(vp)]
    lib.bn254s_hash_to_fq2_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
    if hasattr(lib, "bn254s_scalar_mul"):   # (as below: an older build in an A/B run has neither of the two)
        lib.bn254s_scalar_mul_batch.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, vp, C.c_int, vp, vp, vp, vp, vp]
        lib.bn254s_scalar_mul.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, C.c_size_t, C.c_size_t, vp, C.c_int, vp, vp, vp, vp,
                                          vp, C.POINTER(vp)]
    if hasattr(lib, "bn254s_msm_multi"):   # (likewise)
        lib.bn254s_msm_multi_chain.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_int] + [vp] * 8
        lib.bn254s_msm_multi.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_int,
                                         C.c_size_t] + [vp] * 8 + [C.POINTER(vp)]
    if hasattr(lib, "bn254s_point_sum_check_batch"):   # (likewise; the three entry points of csrc/point_sum.hip come together)
        lib.bn254s_point_sum_check_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_size_t, vp]
        lib.bn254s_verify_scalar_mul.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t,
                                                 vp, vp, vp, vp, vp, vp]
        lib.bn254s_verify_msm_multi.argtypes = [vp, C.c_int, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp,
                                                C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "bn254s_root_links_check_batch"):   # (likewise; the six entry points of csrc/root_links.hip come together)
        lib.bn254s_root_links_check_batch.argtypes = [vp, C.c_int, vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        head = [vp, C.POINTER(Params), vp, vp, vp, C.c_size_t, C.c_size_t]
        lib.bn254s_verify_g1_recover.argtypes = head + [vp, C.c_size_t, vp, vp, vp, vp, vp]
        lib.bn254s_verify_g2_recover.argtypes = head + [vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
        lib.bn254s_verify_fq_sqrt.argtypes = head + [vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        lib.bn254s_verify_fq2_sqrt.argtypes = head + [vp, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        lib.bn254s_verify_map_to_g1.argtypes = head + [vp, C.c_size_t, vp, vp, vp, vp, vp]
    if hasattr(lib, "bn254s_map_to_g1"):   # (as for bn254s_selftest_logup below: an older build in an A/B run has none of them)
        lib.bn254s_hash_to_fq.argtypes = [vp, C.c_size_t, vp]
        lib.bn254s_hash_to_fq_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        lib.bn254s_map_to_g1_batch.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        lib.bn254s_hash_to_g1_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        lib.bn254s_map_to_g1.argtypes = [vp, C.POINTER(Params), vp, C.c_size_t, C.c_size_t, vp, vp, vp, C.POINTER(vp)]
    lib.bn254s_ctl_values.argtypes = [C.c_int, vp, vp, vp, vp, C.c_size_t, vp, vp]
    lib.bn254s_commit_values.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    lib.bn254s_bench_ntt.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_float)]
    lib.bn254s_bench_ntt_clock.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.bn254s_bench_issue.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.bn254s_poseidon_permute.argtypes = [vp, vp, C.c_size_t]
    lib.bn254s_selftest_field.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.bn254s_selftest_poseidon.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.bn254s_selftest_leaf_hash.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, vp]
    lib.bn254s_selftest_fq_inv.argtypes = [vp, vp, C.c_size_t, vp]
    lib.bn254s_selftest_fq.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
    if hasattr(lib, "bn254s_selftest_logup"):   # (an older build loaded through BN254S_LIB for an A/B run has no such entry)
        lib.bn254s_selftest_logup.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    if hasattr(lib, "bn254s_selftest_fri_fold"):   # (likewise; the five entry points of csrc/fri_selftest.hip come together)
        lib.bn254s_selftest_acc.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
        lib.bn254s_selftest_openings.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
        lib.bn254s_selftest_fri_combine.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, vp, vp, vp, vp]
        lib.bn254s_selftest_fri_fold.argtypes = [vp, vp, C.c_int, C.c_uint64, vp, vp]
        lib.bn254s_selftest_fri_rows.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, C.c_int, vp, vp]
    if hasattr(lib, "bn254s_selftest_transforms"):   # (likewise; the three entry points of csrc/ntt_selftest.hip come together)
        lib.bn254s_selftest_transforms.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        lib.bn254s_selftest_mul_2exp.argtypes = [vp, vp, C.c_size_t, vp]
        lib.bn254s_selftest_outer_dft.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    if hasattr(lib, "bn254s_selftest_quotient"):   # (likewise; the three entry points of csrc/quotient_selftest.hip come together)
        lib.bn254s_selftest_quotient.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp,
                                                 vp, vp, vp, vp, vp, vp, vp, vp]
        lib.bn254s_selftest_point_tables.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp]
        lib.bn254s_selftest_aux.argtypes = [vp, C.c_int, vp, C.c_size_t, vp, vp, vp]
    if hasattr(lib, "bn254s_selftest_proof_plan"):   # (likewise)
        lib.bn254s_selftest_proof_plan.argtypes = [C.c_int, C.c_size_t, C.POINTER(Params), C.c_uint64, C.c_int, C.c_int, C.c_int,
                                                   C.c_int, vp, C.c_char_p, C.c_size_t]
    lib.bn254s_bench_copy.argtypes = [vp, C.c_size_t, C.c_int]
    lib.bn254s_bench_leafhash.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]
    lib.bn254s_g1_generate_trace.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, vp, vp]
    _lib = lib
    return lib


def default_params() -> Params:
    p = Params()
    load_library().bn254s_params_default(C.byref(p))
    return p


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def _slots(n_jobs, per_proof):
    """The NULL proof slots of n_jobs jobs cut into proofs of per_proof: what a proving entry point fills."""
    return (C.c_void_p * ((n_jobs + per_proof - 1) // per_proof))()


def _proofs(lib, slots):
    """The filled slots as Proof objects, which own them from here on."""
    return [Proof(lib, C.c_void_p(h)) for h in slots]


class Proof:
    """Owns a bn254s_proof*; `words` is the canonical u64 layout documented in bn254_stark.h."""

    _stage_names = None

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self._words = self._outputs = None
        self.degree_bits = lib.bn254s_proof_degree_bits(handle)
        ms, k = C.POINTER(C.c_float)(), C.c_size_t()
        lib.bn254s_proof_stage_ms(handle, C.byref(ms), C.byref(k))
        if Proof._stage_names is None or len(Proof._stage_names) != k.value:
            Proof._stage_names = [lib.bn254s_stage_name(i).decode() for i in range(k.value)]
        self.stage_ms = dict(zip(Proof._stage_names, ms[:k.value]))

    # the 1.1 MB of proof words are copied out of the library's buffer on first use (a throughput loop that only needs the caps
    # and the stage times does not pay for eight copies per step)
    def _fetch(self, fn, what):
        if not self._h:
            raise RuntimeError(f"Proof.{what}: the proof was closed before its {what} were read")
        data, n = U64P(), C.c_size_t()
        rc = fn(self._h, C.byref(data), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"bn254s_proof_{what} failed with {rc}")
        return data, n.value

    @property
    def words(self) -> np.ndarray:
        if self._words is None:
            data, n = self._fetch(self._lib.bn254s_proof_words, "words")
            self._words = np.ctypeslib.as_array(data, shape=(n,)).copy()
        return self._words

    @property
    def outputs(self) -> np.ndarray:
        if self._outputs is None:
            data, n = self._fetch(self._lib.bn254s_proof_outputs, "outputs")
            self._outputs = np.ctypeslib.as_array(data, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        return self._outputs

    def caps(self) -> np.ndarray:
        """The three Merkle caps (trace, auxiliary, quotient): the first 192 words of the proof."""
        if self._words is not None:
            return self._words[:192].copy()
        data, n = self._fetch(self._lib.bn254s_proof_words, "words")
        assert n >= 192
        return np.ctypeslib.as_array(data, shape=(192,)).copy()

    SECTIONS = ("trace_cap", "auxiliary_polys_cap", "quotient_polys_cap", "local_values", "next_values", "auxiliary_polys",
                "auxiliary_polys_next", "ctl_zs_first", "quotient_polys", "commit_phase_merkle_caps", "query_round_proofs",
                "final_poly", "pow_witness", "init_challenger_state")

    def section(self, name: str) -> np.ndarray:
        """One field of StarkProofWithMetadata (bn254s_proof_section): a copy of its words."""
        data, n = U64P(), C.c_size_t()
        rc = self._lib.bn254s_proof_section(self._h, self.SECTIONS.index(name), C.byref(data), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"bn254s_proof_section({name}) failed with {rc}")
        return np.ctypeslib.as_array(data, shape=(n.value,)).copy() if n.value else np.zeros(0, np.uint64)

    def serialize(self) -> bytes:
        """Little-endian bytes of the word layout (bn254s_proof_serialize)."""
        need = self._lib.bn254s_proof_serialize(self._h, None, 0)
        buf = C.create_string_buffer(need)
        assert self._lib.bn254s_proof_serialize(self._h, buf, need) == need
        return buf.raw

    def close(self):
        """Frees the library's copy; `words` and `outputs` stay readable (they are copied out first)."""
        if self._h:
            try:
                self.words, self.outputs
            finally:
                self._lib.bn254s_proof_free(self._h)
                self._h = None

    def __del__(self):
        if getattr(self, "_h", None):  # (no copy on garbage collection: nobody can read it afterwards)
            self._lib.bn254s_proof_free(self._h)
            self._h = None


class Context:
    """One context per GPU (bn254s_ctx)."""

    def __init__(self, device: int = 0):
        self._h = None
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.bn254s_ctx_create(device, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"bn254s_ctx_create(device={device}) failed with {rc} (is a GPU visible?)")
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            self._lib.bn254s_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def trim(self):
        """bn254s_ctx_trim: idle slots give their (grow-only) workspaces back to the driver."""
        self._check(self._lib.bn254s_ctx_trim(self._h), "bn254s_ctx_trim")

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with {rc}: {self._lib.bn254s_last_error(self._h).decode()}")

    # ---- proving (mirrors run_once of the reference generators) ----
    def prove_g1(self, scalars, x, offset, params: Optional[Params] = None) -> Proof:
        params = params or default_params()
        n = scalars.shape[0]
        out = C.c_void_p()
        self._check(self._lib.bn254s_prove_g1(self._h, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n,
                                              C.byref(out)), "bn254s_prove_g1")
        return Proof(self._lib, out)

    def prove_g2(self, scalars, x, offset, params: Optional[Params] = None) -> Proof:
        """G2 scalar multiplications (points as 16 words x.c0, x.c1, y.c0, y.c1): run_once of G2StarkProofGenerator."""
        params = params or default_params()
        out = C.c_void_p()
        self._check(self._lib.bn254s_prove_g2(self._h, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset),
                                              scalars.shape[0], C.byref(out)), "bn254s_prove_g2")
        return Proof(self._lib, out)

    def prove_fq_exp(self, scalars, x, params: Optional[Params] = None) -> Proof:
        """Fq exponentiations x^s: run_once of FqStarkProofGenerator (src/generators/fq/stark_proof.rs:135-178)."""
        params = params or default_params()
        out = C.c_void_p()
        self._check(self._lib.bn254s_prove_fq_exp(self._h, C.byref(params), _ptr(scalars), _ptr(x), scalars.shape[0],
                                                  C.byref(out)), "bn254s_prove_fq_exp")
        return Proof(self._lib, out)

    def prove_g1_batch(self, scalars, x, offset, per_proof=128, params: Optional[Params] = None, keep=True):
        params = params or default_params()
        n = scalars.shape[0]
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_prove_g1_batch(self._h, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n,
                                                    per_proof, outs), "bn254s_prove_g1_batch")
        return _proofs(self._lib, outs)

    def prove_batch(self, kind, scalars, x, offset=None, per_proof=128, params: Optional[Params] = None):
        """kind 0 = G1, 1 = G2, 2 = Fq exp: n jobs cut into independent 128-instance proofs, pipelined on the GPU."""
        params = params or default_params()
        n = scalars.shape[0]
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_prove_batch(self._h, kind, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n,
                                                 per_proof, outs), "bn254s_prove_batch")
        return _proofs(self._lib, outs)

    def prove_batch_begin(self, kind, scalars, x, offset=None, per_proof=128, params: Optional[Params] = None):
        """bn254s_prove_batch_begin: queues the batch and returns a handle; `handle.end()` waits and returns the proofs.  Batches
        run in the order they were begun, so beginning the next one before ending the current one keeps the GPU busy."""
        return BatchInFlight(self, kind, scalars, x, offset, per_proof, params or default_params())

    def verify(self, kind, words, degree_bits, scalars, x, offset, outputs, params: Optional[Params] = None):
        """Native `verify` (src/starks/common/verifier.rs:32-98 + CTL check): returns None or raises VerifyError(reason)."""
        params = params or default_params()
        words = np.ascontiguousarray(words, dtype=np.uint64)
        outputs = np.ascontiguousarray(outputs, dtype=np.uint64)
        rc = self._lib.bn254s_verify(self._h, kind, C.byref(params), degree_bits, _ptr(words), words.size, _ptr(scalars), _ptr(x),
                                     _ptr(offset), _ptr(outputs), scalars.shape[0])
        if rc == -8:
            raise VerifyError(self._lib.bn254s_last_error(self._h).decode())
        self._check(rc, "bn254s_verify")

    def verify_batch(self, kind, proofs, scalars, x, offset, n_jobs=None, params: Optional[Params] = None, degree_bits=None):
        """bn254s_verify_batch: many proofs of one kind, parameter set and height at once, the FRI query rounds on the device.
        `proofs`: a list of Proof or of (words, outputs); the job arrays hold the jobs of all proofs in proof order, n_jobs[i] of
        them for proof i (default: as many as proof i has outputs).  Returns a list with None for an accepted proof and the
        reference verifier's text for a rejected one - what verify_host raises for that proof alone."""
        return _verify_batch(self._lib, self._h, kind, proofs, scalars, x, offset, n_jobs, params, degree_bits)

    def verify_batch_ms(self) -> dict:
        """The split of the latest verify_batch of this context in ms: front and ctl are wall times of the host threads, upload,
        k_vb_merkle and k_vb_fri come from device events."""
        ms = (C.c_float * 5)()
        self._check(self._lib.bn254s_selftest_verify_batch_ms(self._h, ms), "bn254s_selftest_verify_batch_ms")
        return dict(zip(("front", "upload", "k_vb_merkle", "k_vb_fri", "ctl"), (float(v) for v in ms)))

    def query_round(self, kind, words, degree_bits, records, chunk_proofs=0, params: Optional[Params] = None) -> np.ndarray:
        """bn254s_selftest_query_round on the device: see the module-level query_round."""
        return query_round(kind, words, degree_bits, records, chunk_proofs, params, _ctx=self)

    def map_to_g2(self, u, offsets, params: Optional[Params] = None):
        """u [n,8], offsets [n,16] -> (points [n,16], fq_jobs [2n,8], g2_jobs [n,20], fq proofs, g2 proofs): the config-5
        pipeline on the device (csrc/map_to_g2.hip)."""
        params = params or default_params()
        n = u.shape[0]
        pts = np.zeros((n, 16), np.uint64)
        fq_jobs = np.zeros((2 * n, 8), np.uint64)
        g2_jobs = np.zeros((n, 20), np.uint64)
        pf, pg = _slots(2 * n, 128), _slots(n, 128)
        self._check(self._lib.bn254s_map_to_g2(self._h, C.byref(params), _ptr(u), _ptr(offsets), n, _ptr(pts), _ptr(fq_jobs),
                                               _ptr(g2_jobs), pf, pg), "bn254s_map_to_g2")
        return pts, fq_jobs, g2_jobs, _proofs(self._lib, pf), _proofs(self._lib, pg)

    def _msm_chain(self, fn, w, scalars, x, offset):
        scalars, x, offset = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x, offset))
        n = scalars.shape[0]
        offs = np.zeros((n + 1, w), np.uint64)
        res = np.zeros(w, np.uint64)
        self._check(getattr(self._lib, fn)(self._h, _ptr(scalars), _ptr(x), _ptr(offset), n, _ptr(offs), _ptr(res)), fn)
        return offs, res

    def _msm(self, fn, w, scalars, x, offset, per_proof, params):
        params = params or default_params()
        scalars, x, offset = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x, offset))
        n = scalars.shape[0]
        offs = np.zeros((n + 1, w), np.uint64)
        res = np.zeros(w, np.uint64)
        outs = _slots(n, per_proof)
        self._check(getattr(self._lib, fn)(self._h, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n, per_proof, _ptr(res),
                                           _ptr(offs), outs), fn)
        return res, offs, _proofs(self._lib, outs)

    def g1_msm_chain(self, scalars, x, offset):
        """scalars [n,4], x [n,8], offset = R [8] -> (offsets [n+1,8], result [8]): the witness chain of g1_msm
        (offsets[i] = R + sum_{j<i} s_j x_j, result = offsets[n] - R) on the device, no proof (bn254s_g1_msm_chain)."""
        return self._msm_chain("bn254s_g1_msm_chain", 8, scalars, x, offset)

    def g1_msm(self, scalars, x, offset, per_proof=128, params: Optional[Params] = None):
        """-> (result [8], offsets [n+1,8], proofs): the chain plus the G1 proofs of its n jobs (s_i, x_i, offsets[i]), cut into
        ceil(n / per_proof) proofs like prove_batch (bn254s_g1_msm).  Check it with verify_g1_msm."""
        return self._msm("bn254s_g1_msm", 8, scalars, x, offset, per_proof, params)

    def g2_msm_chain(self, scalars, x, offset):
        """scalars [n,4], x [n,16], offset = R [16] -> (offsets [n+1,16], result [16]): the witness chain of g2_msm
        (offsets[i] = R + sum_{j<i} s_j x_j with the unreduced 256-bit s_j, result = offsets[n] - R) on the device, no proof
        (bn254s_g2_msm_chain)."""
        return self._msm_chain("bn254s_g2_msm_chain", 16, scalars, x, offset)

    def g2_msm(self, scalars, x, offset, per_proof=128, params: Optional[Params] = None):
        """-> (result [16], offsets [n+1,16], proofs): the chain plus the G2 proofs of its n jobs (s_i, x_i, offsets[i]), cut into
        ceil(n / per_proof) proofs like prove_batch(1, ...) (bn254s_g2_msm).  Check it with verify_g2_msm."""
        return self._msm("bn254s_g2_msm", 16, scalars, x, offset, per_proof, params)

    def g1_recover_from_x_batch(self, xs):
        """xs [n,4] (canonical, below p) -> (points [n,8], flags [n] uint8, fq_jobs [n,8]): flags[i] = 1 iff x_i^3 + 3 is a square,
        points[i] = (x_i, y_i) with y_i even where it is and (x_i, 0) where it is not, fq_jobs[i] = (p-1)/2 | x_i^3 + 3: the
        witness side of is_recoverable_from_x / recover_from_x on the device, no proof (bn254s_g1_recover_from_x_batch)."""
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        n = xs.shape[0]
        pts, flags, jobs = np.zeros((n, 8), np.uint64), np.zeros(n, np.uint8), np.zeros((n, 8), np.uint64)
        self._check(self._lib.bn254s_g1_recover_from_x_batch(self._h, _ptr(xs), n, _ptr(pts), flags.ctypes.data_as(C.c_void_p),
                                                             _ptr(jobs)), "bn254s_g1_recover_from_x_batch")
        return pts, flags, jobs

    def g1_recover_from_x(self, xs, per_proof=128, params: Optional[Params] = None):
        """-> (points [n,8], flags [n], fq_jobs [n,8], proofs): the front-end plus the Fq-exp proofs of the n Legendre jobs, cut
        into ceil(n / per_proof) proofs like prove_batch(2, ...) (bn254s_g1_recover_from_x).  Check it with verify_g1_recover."""
        params = params or default_params()
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        n = xs.shape[0]
        pts, flags, jobs = np.zeros((n, 8), np.uint64), np.zeros(n, np.uint8), np.zeros((n, 8), np.uint64)
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_g1_recover_from_x(self._h, C.byref(params), _ptr(xs), n, per_proof, _ptr(pts),
                                                       flags.ctypes.data_as(C.c_void_p), _ptr(jobs), outs), "bn254s_g1_recover_from_x")
        return pts, flags, jobs, _proofs(self._lib, outs)

    @staticmethod
    def _sgns(sgns, n):
        """sgns (None: all 0) as n contiguous bytes, kept as the caller gave them so that the library sees a value above 1."""
        if sgns is None:
            return None, None
        sgns = np.ascontiguousarray(sgns, dtype=np.uint8).reshape(-1)
        if sgns.shape[0] != n:
            raise ValueError(f"{sgns.shape[0]} sgns for {n} xs")
        return sgns, sgns.ctypes.data_as(C.c_void_p)

    def g2_recover_from_x_batch(self, xs, sgns=None):
        """xs [n,8] (x.c0, x.c1, canonical, below p), sgns [n] in {0, 1} (None: all 0) -> (points [n,16], flags [n] uint8,
        fq_jobs [n,8]): with g = x_i^3 + b' on the twist, flags[i] = 1 iff g is a square in Fq2, points[i] = (x_i, y_i) with
        y_i^2 = g and sgn(y_i) == sgns[i] where it is and (x_i, 0) where it is not, fq_jobs[i] = (p-1)/2 | norm(g): the witness
        side of g_circuit / is_square / sqrt_with_sgn on the device, no proof (bn254s_g2_recover_from_x_batch)."""
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        n = xs.shape[0]
        sgns, sp = self._sgns(sgns, n)
        pts, flags, jobs = np.zeros((n, 16), np.uint64), np.zeros(n, np.uint8), np.zeros((n, 8), np.uint64)
        self._check(self._lib.bn254s_g2_recover_from_x_batch(self._h, _ptr(xs), sp, n, _ptr(pts), flags.ctypes.data_as(C.c_void_p),
                                                             _ptr(jobs)), "bn254s_g2_recover_from_x_batch")
        return pts, flags, jobs

    def g2_recover_from_x(self, xs, sgns=None, per_proof=128, params: Optional[Params] = None):
        """-> (points [n,16], flags [n], fq_jobs [n,8], proofs): the front-end plus the Fq-exp proofs of the n Legendre jobs, cut
        into ceil(n / per_proof) proofs like prove_batch(2, ...) (bn254s_g2_recover_from_x).  Check it with verify_g2_recover."""
        params = params or default_params()
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        n = xs.shape[0]
        sgns, sp = self._sgns(sgns, n)
        pts, flags, jobs = np.zeros((n, 16), np.uint64), np.zeros(n, np.uint8), np.zeros((n, 8), np.uint64)
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_g2_recover_from_x(self._h, C.byref(params), _ptr(xs), sp, n, per_proof, _ptr(pts),
                                                       flags.ctypes.data_as(C.c_void_p), _ptr(jobs), outs), "bn254s_g2_recover_from_x")
        return pts, flags, jobs, _proofs(self._lib, outs)

    def _sqrt(self, fn, w, xs, sgns, per_proof, params):
        """The four root calls: w words per element, per_proof None for the front-end alone."""
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        n = xs.shape[0]
        sgns, sp = self._sgns(sgns, n)
        roots, jobs = np.zeros((n, w), np.uint64), np.zeros((n, 8), np.uint64)
        square, ok = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        sq_p, ok_p = square.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p)
        if per_proof is None:
            self._check(getattr(self._lib, fn)(self._h, _ptr(xs), sp, n, _ptr(roots), sq_p, ok_p, _ptr(jobs)), fn)
            return roots, square, ok, jobs
        params = params or default_params()
        outs = _slots(n, per_proof)
        self._check(getattr(self._lib, fn)(self._h, C.byref(params), _ptr(xs), sp, n, per_proof, _ptr(roots), sq_p, ok_p, _ptr(jobs),
                                           outs), fn)
        return roots, square, ok, jobs, _proofs(self._lib, outs)

    def fq_sqrt_batch(self, xs, sgns=None):
        """xs [n,4] (canonical, below p), sgns [n] in {0, 1} (None: all 0) -> (roots [n,4], square [n] uint8, root_ok [n] uint8,
        fq_jobs [n,8]): square[i] = 1 iff x_i^((p-1)/2) == 1 (0 for x_i = 0), root_ok[i] = 1 iff a y with y^2 = x_i and the parity
        sgns[i] exists (for x_i = 0: iff sgns[i] == 0), roots[i] that y or zeros, fq_jobs[i] = (p-1)/2 | x_i: the witness side of
        FqTarget::is_square / sqrt_with_sgn on the device, no proof (bn254s_fq_sqrt_batch)."""
        return self._sqrt("bn254s_fq_sqrt_batch", 4, xs, sgns, None, None)

    def fq2_sqrt_batch(self, xs, sgns=None):
        """xs [n,8] (c0, c1), sgns [n] -> (roots [n,8], square [n], root_ok [n], fq_jobs [n,8]): the same for Fq2, the Legendre
        symbol taken of norm(x_i) = c0^2 + c1^2 (fq_jobs[i] = (p-1)/2 | norm(x_i)) and the sign the parity of the root's c0, or of
        its c1 when c0 is zero: the witness side of Fq2Target::is_square / sqrt_with_sgn (bn254s_fq2_sqrt_batch)."""
        return self._sqrt("bn254s_fq2_sqrt_batch", 8, xs, sgns, None, None)

    def fq_sqrt(self, xs, sgns=None, per_proof=128, params: Optional[Params] = None):
        """-> (roots, square, root_ok, fq_jobs, proofs): the front-end plus the Fq-exp proofs of the n Legendre jobs, cut into
        ceil(n / per_proof) proofs like prove_batch(2, ...) (bn254s_fq_sqrt).  Check it with verify_fq_sqrt."""
        return self._sqrt("bn254s_fq_sqrt", 4, xs, sgns, per_proof, params)

    def fq2_sqrt(self, xs, sgns=None, per_proof=128, params: Optional[Params] = None):
        """-> (roots, square, root_ok, fq_jobs, proofs): the Fq2 twin of fq_sqrt (bn254s_fq2_sqrt).  Check it with
        verify_fq2_sqrt."""
        return self._sqrt("bn254s_fq2_sqrt", 8, xs, sgns, per_proof, params)

    def _inv(self, fn, xs):
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        out = np.zeros_like(xs)
        self._check(getattr(self._lib, fn)(self._h, _ptr(xs), xs.shape[0], _ptr(out)), fn)
        return out

    def fq_inv_batch(self, xs):
        """xs [n,4] (canonical, below p) -> [n,4]: x_i^-1, zeros for x_i = 0: FqTarget::inv on the device (bn254s_fq_inv_batch)."""
        return self._inv("bn254s_fq_inv_batch", xs)

    def fq2_inv_batch(self, xs):
        """xs [n,8] (c0, c1) -> [n,8]: (c0, -c1) / norm, zeros for x_i = 0: Fq2Target::inv on the device (bn254s_fq2_inv_batch)."""
        return self._inv("bn254s_fq2_inv_batch", xs)

    def g2_subgroup_check_batch(self, points):
        """points [n,16] (x.c0, x.c1, y.c0, y.c1, canonical, below p, on the twist curve) -> flags [n] uint8: flags[i] = 1 iff
        [r] P_i is the point at infinity, by the endomorphism criterion on the device, no proof (bn254s_g2_subgroup_check_batch).
        A coordinate >= p or a point off the curve raises (-1, the message names the first such point)."""
        points = np.ascontiguousarray(points, dtype=np.uint64)
        n = points.shape[0]
        flags = np.zeros(n, np.uint8)
        self._check(self._lib.bn254s_g2_subgroup_check_batch(self._h, _ptr(points), n, flags.ctypes.data_as(C.c_void_p)),
                    "bn254s_g2_subgroup_check_batch")
        return flags

    def g2_subgroup_check(self, points, offsets, per_proof=128, params: Optional[Params] = None):
        """points [n,16], offsets [n,16] (R_i: random subgroup points, set_random_g2) -> (flags [n], g2_jobs [n,20] = r | P_i,
        proofs): the front-end plus the G2 proofs of the n jobs (r, P_i, R_i), cut into ceil(n / per_proof) proofs like
        prove_batch(1, ...); output i is R_i + [r]P_i, R_i exactly where flags[i] is 1 (bn254s_g2_subgroup_check).  Check it with
        verify_g2_subgroup."""
        params = params or default_params()
        points, offsets = (np.ascontiguousarray(a, dtype=np.uint64) for a in (points, offsets))
        n = points.shape[0]
        if offsets.shape != (n, 16):
            raise ValueError(f"offsets {offsets.shape} for {n} points")
        flags, jobs = np.zeros(n, np.uint8), np.zeros((n, 20), np.uint64)
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_g2_subgroup_check(self._h, C.byref(params), _ptr(points), _ptr(offsets), n, per_proof,
                                                       flags.ctypes.data_as(C.c_void_p), _ptr(jobs), outs), "bn254s_g2_subgroup_check")
        return flags, jobs, _proofs(self._lib, outs)

    def g2_clear_cofactor_batch(self, points):
        """points [n,16] (x.c0, x.c1, y.c0, y.c1, canonical, below p, on the twist curve) -> (images [n,16], finite [n] uint8):
        images[i] = [h] P_i for the cofactor h = 2p - r, a member of the r-torsion subgroup, zeros where finite[i] is 0 ([h] P_i is
        the point at infinity), by the endomorphism form on the device, no proof (bn254s_g2_clear_cofactor_batch).  A coordinate
        >= p or a point off the curve raises (-1, the message names the first such point)."""
        points = np.ascontiguousarray(points, dtype=np.uint64)
        n = points.shape[0]
        images, finite = np.zeros((n, 16), np.uint64), np.zeros(n, np.uint8)
        self._check(self._lib.bn254s_g2_clear_cofactor_batch(self._h, _ptr(points), n, _ptr(images), finite.ctypes.data_as(C.c_void_p)),
                    "bn254s_g2_clear_cofactor_batch")
        return images, finite

    def g2_clear_cofactor(self, points, offsets, per_proof=128, params: Optional[Params] = None):
        """points [n,16], offsets [n,16] (R_i: random subgroup points, set_random_g2) -> (images [n,16], finite [n], g2_jobs [n,20]
        = h | P_i, proofs): the front-end plus the G2 proofs of the n jobs (h, P_i, R_i), cut into ceil(n / per_proof) proofs like
        prove_batch(1, ...); output i is R_i + [h]P_i = R_i + images[i], R_i exactly where finite[i] is 0
        (bn254s_g2_clear_cofactor).  Check it with verify_g2_clear_cofactor."""
        params = params or default_params()
        points, offsets = (np.ascontiguousarray(a, dtype=np.uint64) for a in (points, offsets))
        n = points.shape[0]
        if offsets.shape != (n, 16):
            raise ValueError(f"offsets {offsets.shape} for {n} points")
        images, finite, jobs = np.zeros((n, 16), np.uint64), np.zeros(n, np.uint8), np.zeros((n, 20), np.uint64)
        outs = _slots(n, per_proof)
        self._check(self._lib.bn254s_g2_clear_cofactor(self._h, C.byref(params), _ptr(points), _ptr(offsets), n, per_proof,
                                                       _ptr(images), finite.ctypes.data_as(C.c_void_p), _ptr(jobs), outs),
                    "bn254s_g2_clear_cofactor")
        return images, finite, jobs, _proofs(self._lib, outs)

    def map_to_g2_batch(self, u):
        """u [n,8] (c0, c1, canonical, below p) -> points [n,16]: the reference's native map_to_g2 (hash_to_g2.rs:113-148) on the
        device, no proof - the points map_to_g2 returns for the same u (bn254s_map_to_g2_batch)."""
        u = np.ascontiguousarray(u, dtype=np.uint64)
        n = u.shape[0]
        pts = np.zeros((n, 16), np.uint64)
        self._check(self._lib.bn254s_map_to_g2_batch(self._h, _ptr(u), n, _ptr(pts)), "bn254s_map_to_g2_batch")
        return pts

    def hash_to_g2_batch(self, inputs):
        """inputs [n, len] Goldilocks elements -> points [n,16]: hash_to_g2 (hash_to_g2.rs:40-43), hash_to_fq2 of every row and
        map_to_g2 of the result without leaving the device, no proof (bn254s_hash_to_g2_batch)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        n, ln = inputs.shape
        pts = np.zeros((n, 16), np.uint64)
        self._check(self._lib.bn254s_hash_to_g2_batch(self._h, _ptr(inputs) if ln else None, n, ln, _ptr(pts)), "bn254s_hash_to_g2_batch")
        return pts

    def hash_to_fq2_batch(self, inputs: np.ndarray) -> np.ndarray:
        """inputs [n, len] Goldilocks elements -> u [n, 8]: hash_to_fq2 (hash_to_g2.rs:76-87) of every row, on the device."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        n, ln = inputs.shape
        out = np.zeros((n, 8), np.uint64)
        self._check(self._lib.bn254s_hash_to_fq2_batch(self._h, _ptr(inputs) if ln else None, n, ln, _ptr(out)), "bn254s_hash_to_fq2_batch")
        return out

    def hash_to_fq_batch(self, inputs: np.ndarray) -> np.ndarray:
        """inputs [n, len] Goldilocks elements -> u [n, 4]: hash_to_fq, the first coordinate of hash_to_fq2 (hash_to_g2.rs:76-87),
        of every row, on the device (bn254s_hash_to_fq_batch)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        n, ln = inputs.shape
        out = np.zeros((n, 4), np.uint64)
        self._check(self._lib.bn254s_hash_to_fq_batch(self._h, _ptr(inputs) if ln else None, n, ln, _ptr(out)), "bn254s_hash_to_fq_batch")
        return out

    def map_to_g1_batch(self, u):
        """u [n,4] (canonical, below p) -> (points [n,8], sq_flags [2n] uint8, fq_jobs [2n,8]): the Shallue-van de Woestijne map
        onto y^2 = x^3 + 3 (the reference's map_to_g2, hash_to_g2.rs:113-148, read over Fq) on the device, no proof.
        sq_flags[2i + j] = 1 iff g(x_{j+1}) of input i is a square, fq_jobs[2i + j] = (p-1)/2 | g(x_{j+1}), points[i] = (x, y) for
        the first candidate with a square g, y of the parity of u_i (bn254s_map_to_g1_batch)."""
        u = np.ascontiguousarray(u, dtype=np.uint64)
        n = u.shape[0]
        pts, flags, jobs = np.zeros((n, 8), np.uint64), np.zeros(2 * n, np.uint8), np.zeros((2 * n, 8), np.uint64)
        self._check(self._lib.bn254s_map_to_g1_batch(self._h, _ptr(u), n, _ptr(pts), flags.ctypes.data_as(C.c_void_p), _ptr(jobs)),
                    "bn254s_map_to_g1_batch")
        return pts, flags, jobs

    def hash_to_g1_batch(self, inputs):
        """inputs [n, len] Goldilocks elements -> points [n,8]: hash_to_fq of every row and map_to_g1 of the result without
        leaving the device, no proof (bn254s_hash_to_g1_batch)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
        n, ln = inputs.shape
        pts = np.zeros((n, 8), np.uint64)
        self._check(self._lib.bn254s_hash_to_g1_batch(self._h, _ptr(inputs) if ln else None, n, ln, _ptr(pts)), "bn254s_hash_to_g1_batch")
        return pts

    def map_to_g1(self, u, per_proof=128, params: Optional[Params] = None):
        """-> (points [n,8], sq_flags [2n], fq_jobs [2n,8], proofs): the front-end plus the Fq-exp proofs of the 2n Legendre jobs,
        cut into ceil(2n / per_proof) proofs like prove_batch(2, ...) (bn254s_map_to_g1).  Check it with verify_map_to_g1."""
        params = params or default_params()
        u = np.ascontiguousarray(u, dtype=np.uint64)
        n = u.shape[0]
        pts, flags, jobs = np.zeros((n, 8), np.uint64), np.zeros(2 * n, np.uint8), np.zeros((2 * n, 8), np.uint64)
        outs = _slots(2 * n, per_proof)
        self._check(self._lib.bn254s_map_to_g1(self._h, C.byref(params), _ptr(u), n, per_proof, _ptr(pts),
                                               flags.ctypes.data_as(C.c_void_p), _ptr(jobs), outs), "bn254s_map_to_g1")
        return pts, flags, jobs, _proofs(self._lib, outs)

    def _job_arrays(self, kind, scalars, x, offset):
        scalars, x = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x))
        # a kind outside 0..2 goes on to the library, which answers BN254S_E_INVALID_ARG before it reads an array
        pw = {0: 8, 1: 16, 2: 4}.get(kind, x.shape[-1] if x.ndim == 2 else 0)
        offset = None if kind == 2 or offset is None else np.ascontiguousarray(offset, dtype=np.uint64)
        n = scalars.shape[0]
        if scalars.shape != (n, 4) or x.shape != (n, pw) or (offset is not None and offset.shape != (n, pw)):
            raise ValueError(f"job_outputs: scalars {scalars.shape}, x {x.shape}, offset {None if offset is None else offset.shape}")
        return pw, n, scalars, x, offset

    def job_outputs_batch(self, kind, scalars, x, offset=None):
        """kind 0 = G1, 1 = G2, 2 = Fq exp (no offset); scalars [n,4], x and offset [n, 8 | 16 | 4] -> (outputs [n, 8 | 16 | 4],
        finite [n] uint8): outputs[i] = s_i x_i + offset_i, or x_i^s_i, for n independent jobs on the device, no proof
        (bn254s_job_outputs_batch) - what the reference's SingleGenerators compute.  Scalars are the full 256-bit values.  Where
        finite[i] is 0 the output is the point at infinity and outputs[i] is zeros.  A coordinate >= p or a point off its curve
        raises (-1, the message names the argument and the first such job)."""
        pw, n, scalars, x, offset = self._job_arrays(kind, scalars, x, offset)
        outs, finite = np.zeros((n, pw), np.uint64), np.zeros(n, np.uint8)
        self._check(self._lib.bn254s_job_outputs_batch(self._h, kind, _ptr(scalars), _ptr(x), _ptr(offset), n, _ptr(outs),
                                                       finite.ctypes.data_as(C.c_void_p)), "bn254s_job_outputs_batch")
        return outs, finite

    def job_outputs(self, kind, scalars, x, offset=None, per_proof=128, params: Optional[Params] = None):
        """-> (outputs [n, 8 | 16 | 4], proofs): the front-end plus prove_batch(kind, ...) of the same jobs, the outputs of the
        proofs checked word for word against the front-end's (bn254s_job_outputs).  A job whose output is the point at infinity
        raises (-4, the message names it).  Check the result with verify_job_outputs."""
        params = params or default_params()
        pw, n, scalars, x, offset = self._job_arrays(kind, scalars, x, offset)
        outs = np.zeros((n, pw), np.uint64)
        slots = _slots(n, per_proof)
        self._check(self._lib.bn254s_job_outputs(self._h, kind, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n, per_proof,
                                                 _ptr(outs), slots), "bn254s_job_outputs")
        return outs, _proofs(self._lib, slots)

    def job_check_batch(self, kind, scalars, x, offset=None):
        """kind, scalars, x, offset as for job_outputs_batch -> (provable [n] uint8, step [n] uint16): whether the trace of job i
        can be proven, and the first step k at which its running sum meets minus its doubling (row 2k of its 512-row frame), or
        JOB_STEP_NONE (bn254s_job_check_batch).  Every Fq-exp job is provable.  A coordinate >= p or a point off its curve
        raises (-1, the message names the argument and the first such job)."""
        _, n, scalars, x, offset = self._job_arrays(kind, scalars, x, offset)
        provable, step = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
        self._check(self._lib.bn254s_job_check_batch(self._h, kind, _ptr(scalars), _ptr(x), _ptr(offset), n,
                                                     provable.ctypes.data_as(C.c_void_p), step.ctypes.data_as(C.c_void_p)),
                    "bn254s_job_check_batch")
        return provable, step

    def prove_batch_checked(self, kind, scalars, x, offset=None, per_proof=128, params: Optional[Params] = None):
        """-> (proofs, provable, step): job_check_batch, then prove_batch(kind, ...) of the same jobs if every one is provable
        (bn254s_prove_batch_checked); the proofs are those of prove_batch.  Otherwise nothing is proven and UnprovableJobs (-4, the
        message names the first such job and its step) carries provable and step."""
        params = params or default_params()
        _, n, scalars, x, offset = self._job_arrays(kind, scalars, x, offset)
        provable, step = np.zeros(n, np.uint8), np.zeros(n, np.uint16)
        slots = _slots(n, per_proof)
        rc = self._lib.bn254s_prove_batch_checked(self._h, kind, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n, per_proof,
                                                  provable.ctypes.data_as(C.c_void_p), step.ctypes.data_as(C.c_void_p), slots)
        if rc == -4 and not provable.all():
            raise UnprovableJobs(f"bn254s_prove_batch_checked failed with -4: {self._lib.bn254s_last_error(self._h).decode()}",
                                 provable, step)
        self._check(rc, "bn254s_prove_batch_checked")
        return _proofs(self._lib, slots), provable, step

    def _scalar_mul_arrays(self, kind, scalars, x, seed):
        pw, n, scalars, x, _ = self._job_arrays(kind, scalars, x, None)
        seed = np.ascontiguousarray(seed, dtype=np.uint64)
        if seed.shape != (4,):
            raise ValueError(f"scalar_mul: seed {seed.shape}, four Goldilocks elements expected")
        out = (np.zeros((n, pw), np.uint64), np.zeros(n, np.uint8), np.zeros((n, pw), np.uint64), np.zeros((n, pw), np.uint64),
               np.zeros(n, np.uint8))
        return n, scalars, x, seed, out

    def scalar_mul_batch(self, kind, scalars, x, seed, max_attempts=4):
        """kind 0 = G1, 1 = G2; scalars [n,4], x [n, 8 | 16], seed [4] canonical Goldilocks elements -> (products [n, 8 | 16],
        finite [n] uint8, offsets, outputs [n, 8 | 16], attempts [n] uint8): products[i] = s_i x_i with the offsets drawn from the
        seed, checked against the jobs and redrawn where a job could not be proven, on the device, no proof
        (bn254s_scalar_mul_batch).  offsets[i] = hash_to_g1 | hash_to_g2 of (seed, i mod 2^32, i >> 32, attempts[i],
        0x62736D00 + kind), outputs[i] = s_i x_i + offsets[i].  Where finite[i] is 0 the product is the point at infinity and
        products[i] is zeros.  A job that no attempt below max_attempts can prove raises (-4, the message names it, its step and
        row)."""
        n, scalars, x, seed, (prods, finite, offs, outs, att) = self._scalar_mul_arrays(kind, scalars, x, seed)
        u8 = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.bn254s_scalar_mul_batch(self._h, kind, _ptr(scalars), _ptr(x), n, _ptr(seed), max_attempts, _ptr(prods),
                                                      u8(finite), _ptr(offs), _ptr(outs), u8(att)), "bn254s_scalar_mul_batch")
        return prods, finite, offs, outs, att

    def scalar_mul(self, kind, scalars, x, seed, max_attempts=4, per_proof=128, params: Optional[Params] = None):
        """-> (products, finite, offsets, outputs, attempts, proofs): the front-end plus prove_batch(kind, scalars, x, offsets) of
        the same jobs, the outputs of the proofs checked word for word against the front-end's (bn254s_scalar_mul).  scalars, x,
        offsets, outputs and the proofs are what verify / verify_batch take."""
        params = params or default_params()
        n, scalars, x, seed, (prods, finite, offs, outs, att) = self._scalar_mul_arrays(kind, scalars, x, seed)
        u8 = lambda a: a.ctypes.data_as(C.c_void_p)
        slots = _slots(n, per_proof)
        self._check(self._lib.bn254s_scalar_mul(self._h, kind, C.byref(params), _ptr(scalars), _ptr(x), n, per_proof, _ptr(seed),
                                                max_attempts, _ptr(prods), u8(finite), _ptr(offs), _ptr(outs), u8(att), slots),
                    "bn254s_scalar_mul")
        return prods, finite, offs, outs, att, _proofs(self._lib, slots)

    def _msm_multi_arrays(self, kind, scalars, x, seg_len, R, seed):
        pw, n, scalars, x, _ = self._job_arrays(kind, scalars, x, None)
        seg = np.ascontiguousarray(seg_len, dtype=np.uintp).reshape(-1)
        m = seg.shape[0]
        R = None if R is None else np.ascontiguousarray(R, dtype=np.uint64)
        seed = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint64)
        if (R is not None and R.shape != (m, pw)) or (seed is not None and seed.shape != (4,)):
            raise ValueError(f"msm_multi: R {None if R is None else R.shape} for {m} MSMs, seed {None if seed is None else seed.shape}")
        out = (np.zeros((m, pw), np.uint64), np.zeros(m, np.uint8), np.zeros((n, pw), np.uint64), np.zeros((n, pw), np.uint64),
               np.zeros((m, pw), np.uint64), np.zeros(m, np.uint8), np.zeros(m, np.uint32), np.zeros(m, np.uint16))
        return n, m, scalars, x, seg, R, seed, out

    def msm_multi_chain(self, kind, scalars, x, seg_len, R=None, seed=None, max_attempts=4):
        """kind 0 = G1, 1 = G2; m MSMs stored one after the other, MSM j with seg_len[j] of the n inputs scalars [n,4], x [n, 8 | 16];
        R [m, 8 | 16] supplied points, or None for points drawn from seed [4] (canonical Goldilocks elements) and redrawn, up to
        max_attempts times, for the MSMs that cannot be proven -> MsmMulti without proofs (bn254s_msm_multi_chain, on the device):
        offsets[i] = R_j + (the sum of MSM j before input i), outputs[i] = offsets[i] + s_i x_i, results[j] = the sum of MSM j
        (zeros and finite[j] = 0 where it is the point at infinity), R[j] the point used, attempts[j] the attempt that gave it.
        An MSM that cannot be proven is a result: bad_link[j] / bad_step[j] name its first hitting link and step (MSM_LINK_NONE /
        JOB_STEP_NONE otherwise), its rows of offsets and outputs are zeros, attempts[j] = max_attempts for drawn points."""
        n, m, scalars, x, seg, R, seed, out = self._msm_multi_arrays(kind, scalars, x, seg_len, R, seed)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.bn254s_msm_multi_chain(self._h, kind, vp(scalars), vp(x), vp(seg), m, n, vp(R), vp(seed), max_attempts,
                                                     *(vp(a) for a in out)), "bn254s_msm_multi_chain")
        return MsmMulti(*out, None)

    def msm_multi(self, kind, scalars, x, seg_len, R=None, seed=None, max_attempts=4, per_proof=128, params: Optional[Params] = None):
        """-> MsmMulti with proofs: the front-end plus prove_batch(kind, scalars, x, offsets) of the n links, cut by per_proof
        regardless of MSM boundaries, the outputs of the proofs checked word for word against the chain's (bn254s_msm_multi).  An
        MSM that cannot be proven raises (-4, the message names it, its link, step and row) before any proof.  Check the result
        with verify_msm_multi."""
        params = params or default_params()
        n, m, scalars, x, seg, R, seed, out = self._msm_multi_arrays(kind, scalars, x, seg_len, R, seed)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        slots = _slots(n, per_proof)
        self._check(self._lib.bn254s_msm_multi(self._h, kind, C.byref(params), vp(scalars), vp(x), vp(seg), m, n, vp(R), vp(seed),
                                               max_attempts, per_proof, *(vp(a) for a in out), slots), "bn254s_msm_multi")
        return MsmMulti(*out, _proofs(self._lib, slots))

    def point_sum_check_batch(self, kind, a, a_finite, b, c):
        """kind 0 = G1, 1 = G2; a, b, c [n, 8 | 16], a_finite [n] -> codes [n] uint8: is c_i == a_i + b_i, with a_i the point at
        infinity where a_finite[i] is 0 (zero words), on the device without an inversion (bn254s_point_sum_check_batch).  SUM_OK,
        or the first of SUM_A_NOT_ZERO .. SUM_Y that applies.  A coordinate >= p raises (-1, the message names the array and the
        first such row)."""
        pw = {0: 8, 1: 16}.get(kind, 8)
        a, b, c = (np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, pw) for v in (a, b, c))
        fin = np.ascontiguousarray(a_finite, dtype=np.uint8).reshape(-1)
        n = a.shape[0]
        if b.shape != a.shape or c.shape != a.shape or fin.shape != (n,):
            raise ValueError(f"point_sum_check: a {a.shape}, a_finite {fin.shape}, b {b.shape}, c {c.shape}")
        codes = np.zeros(n, np.uint8)
        self._check(self._lib.bn254s_point_sum_check_batch(self._h, kind, _ptr(a), fin.ctypes.data_as(C.c_void_p), _ptr(b), _ptr(c), n,
                                                           codes.ctypes.data_as(C.c_void_p)), "bn254s_point_sum_check_batch")
        return codes

    def _verify_statement(self, what, call, kind, proofs, n_links, params):
        """The part the statement verifiers share: the proof table, the call, and what its code means."""
        params = params or default_params()
        pairs = [pr if isinstance(pr, (tuple, list)) else (pr.words, pr.degree_bits) for pr in proofs]
        arrs, table = _word_arrays([w for w, _ in pairs])
        n_words = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        bits = (C.c_uint32 * len(arrs))(*[int(d) for _, d in pairs])
        link, status = np.zeros(n_links, np.uint8), np.zeros(len(arrs), np.int32)
        rc = call(params, table, n_words, bits, len(arrs), link.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p))
        if rc == -8:
            e = VerifyError(self._lib.bn254s_last_error(self._h).decode())
            e.link_codes, e.proof_status = link, status
            raise e
        self._check(rc, what)
        return link, status

    def verify_scalar_mul(self, kind, proofs, per_proof, scalars, x, products, finite, offsets, outputs, params: Optional[Params] = None):
        """The statement products[i] == s_i x_i of a scalar_mul call (bn254s_verify_scalar_mul): every x_i on its curve,
        products[i] + offsets[i] == outputs[i] on the device, and every proof accepted for its jobs (s_i, x_i, offsets[i],
        outputs[i]) by verify_batch.  `proofs`: objects with `words` and `degree_bits`, or (words, degree_bits) pairs, proof k for
        jobs k per_proof ...  Where the offsets come from (the seed, the attempts) is not checked: the statement does not depend
        on it.  -> (link_codes [n] uint8, proof_status [n_proofs] int32), all zero; a rejection raises VerifyError with the
        message of the first broken link, or of the first rejected proof where every link holds, and both arrays as its
        `link_codes` and `proof_status`."""
        pw, n, scalars, x, _ = self._job_arrays(kind, scalars, x, None)
        products, offsets, outputs = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, pw) for a in (products, offsets, outputs))
        finite = np.ascontiguousarray(finite, dtype=np.uint8).reshape(-1)
        if not (products.shape == offsets.shape == outputs.shape == (n, pw)) or finite.shape != (n,):
            raise ValueError(f"verify_scalar_mul: products {products.shape}, finite {finite.shape}, offsets {offsets.shape}, "
                             f"outputs {outputs.shape} for {n} jobs")
        call = lambda params, table, n_words, bits, k, link, status: self._lib.bn254s_verify_scalar_mul(
            self._h, kind, C.byref(params), table, n_words, bits, k, per_proof, _ptr(scalars), _ptr(x), n, _ptr(products),
            finite.ctypes.data_as(C.c_void_p), _ptr(offsets), _ptr(outputs), link, status)
        return self._verify_statement("bn254s_verify_scalar_mul", call, kind, proofs, n, params)

    def verify_msm_multi(self, kind, proofs, per_proof, scalars, x, seg_len, R, results, finite, offsets, outputs,
                         params: Optional[Params] = None):
        """The statement results[j] == the sum of s x over MSM j of a msm_multi call (bn254s_verify_msm_multi): per MSM every x on
        its curve, the offset of its first link R_j and the offset of every later link the output before it, word for word,
        results[j] + R_j == the last output on the device, and every proof accepted for its links.  Arguments and the return value
        as for verify_scalar_mul, with link_codes [m] per MSM: SUM_X_OFF_CURVE, SUM_HEAD, SUM_CHAIN, then the relation's code."""
        pw, n, scalars, x, _ = self._job_arrays(kind, scalars, x, None)
        seg = np.ascontiguousarray(seg_len, dtype=np.uintp).reshape(-1)
        m = seg.shape[0]
        offsets, outputs = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, pw) for a in (offsets, outputs))
        R, results = (np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, pw) for a in (R, results))
        finite = np.ascontiguousarray(finite, dtype=np.uint8).reshape(-1)
        if not (offsets.shape == outputs.shape == (n, pw)) or not (R.shape == results.shape == (m, pw)) or finite.shape != (m,):
            raise ValueError(f"verify_msm_multi: R {R.shape}, results {results.shape}, finite {finite.shape}, offsets {offsets.shape}, "
                             f"outputs {outputs.shape} for {m} MSMs of {n} inputs")
        call = lambda params, table, n_words, bits, k, link, status: self._lib.bn254s_verify_msm_multi(
            self._h, kind, C.byref(params), table, n_words, bits, k, per_proof, _ptr(scalars), _ptr(x), seg.ctypes.data_as(C.c_void_p),
            m, n, _ptr(R), _ptr(results), finite.ctypes.data_as(C.c_void_p), _ptr(offsets), _ptr(outputs), link, status)
        return self._verify_statement("bn254s_verify_msm_multi", call, kind, proofs, m, params)

    def _root_arrays(self, what, tag, xs, sgns, out, flags, root_ok, fq_jobs):
        """The arrays of a root-link call as the library takes them: (n, xs, sgns, out, flags, root_ok, fq_jobs), each contiguous
        or None; the bytes are kept as the caller gave them so that the library sees a value above 1."""
        if what not in ROOT_WHAT:
            raise ValueError(f"{tag}: what {what!r} is none of 0..4")
        xs = np.ascontiguousarray(xs, dtype=np.uint64).reshape(-1, _ROOT_IN_WORDS[what])
        n = xs.shape[0]
        nj = 2 * n if what == MAP_TO_G1 else n
        out = np.ascontiguousarray(out, dtype=np.uint64).reshape(-1, _ROOT_OUT_WORDS[what])
        flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        sgns = None if sgns is None or what in (G1_RECOVER, MAP_TO_G1) else np.ascontiguousarray(sgns, dtype=np.uint8).reshape(-1)
        root_ok = np.ascontiguousarray(root_ok, dtype=np.uint8).reshape(-1) if what in (FQ_SQRT, FQ2_SQRT) else None
        fq_jobs = None if fq_jobs is None else np.ascontiguousarray(fq_jobs, dtype=np.uint64).reshape(-1, 8)
        if out.shape[0] != n or flags.shape != (nj,) or (sgns is not None and sgns.shape != (n,)) or \
                (root_ok is not None and root_ok.shape != (n,)) or (fq_jobs is not None and fq_jobs.shape != (nj, 8)):
            raise ValueError(f"{tag}: {n} inputs with out {out.shape}, flags {flags.shape}, "
                             f"sgns {None if sgns is None else sgns.shape}, root_ok {None if root_ok is None else root_ok.shape}, "
                             f"fq_jobs {None if fq_jobs is None else fq_jobs.shape}")
        return n, xs, sgns, out, flags, root_ok, fq_jobs

    def root_links_check_batch(self, what, xs, out, flags, sgns=None, root_ok=None, fq_jobs=None):
        """The field linkage of a Legendre-proven front-end on the device (bn254s_root_links_check_batch).  what: G1_RECOVER,
        G2_RECOVER, FQ_SQRT, FQ2_SQRT or MAP_TO_G1; xs [n, 4 | 8] the inputs (u for MAP_TO_G1); out the points [n, 8 | 16] or roots
        [n, 4 | 8]; flags [n] (sq_flags [2n] for MAP_TO_G1; `square` for the roots); sgns [n] (None: all 0; not read for G1_RECOVER,
        MAP_TO_G1); root_ok [n] for the roots; fq_jobs [n | 2n, 8] or None -> (codes [n] uint8, bases [n | 2n, 4]): ROOT_OK or
        the first of ROOT_JOB_SCALAR .. ROOT_SIGN that applies, and the canonical base of every job as computed on the device.
        A coordinate >= p that would be read as a field element raises (-1, the message names the array and the row)."""
        tag = "root_links_check"
        n, xs, sgns, out, flags, root_ok, fq_jobs = self._root_arrays(what, tag, xs, sgns, out, flags, root_ok, fq_jobs)
        codes, bases = np.zeros(n, np.uint8), np.zeros((flags.shape[0], 4), np.uint64)
        bp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._lib.bn254s_root_links_check_batch(self._h, what, _ptr(xs), bp(sgns), n, _ptr(out), bp(flags), bp(root_ok),
                                                            bp(fq_jobs), bp(codes), _ptr(bases)), "bn254s_root_links_check_batch")
        return codes, bases

    def _verify_roots(self, what, fn, proofs, per_proof, xs, sgns, out, flags, root_ok, fq_jobs, params):
        """The five root verifiers: the arrays, the call in the argument order of its `what`, _verify_statement."""
        n, xs, sgns, out, flags, root_ok, fq_jobs = self._root_arrays(what, fn[len("bn254s_"):], xs, sgns, out, flags, root_ok, fq_jobs)
        bp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        mid = ([_ptr(xs)] + ([] if what in (G1_RECOVER, MAP_TO_G1) else [bp(sgns)]) + [n, _ptr(out), bp(flags)] +
               ([bp(root_ok)] if what in (FQ_SQRT, FQ2_SQRT) else []) + [bp(fq_jobs)])
        call = lambda params, table, n_words, bits, k, link, status: getattr(self._lib, fn)(
            self._h, C.byref(params), table, n_words, bits, k, per_proof, *mid, link, status)
        return self._verify_statement(fn, call, 2, proofs, n, params)

    def verify_g1_recover(self, proofs, per_proof, xs, points, flags, fq_jobs=None, params: Optional[Params] = None):
        """The statement of a g1_recover_from_x call (bn254s_verify_g1_recover): flags[i] says whether x_i^3 + 3 is a square, and
        points[i] is (x_i, y_i) with y_i its even root where it is and (x_i, 0) where it is not.  The linkage is checked on the
        device, and every Fq-exp proof by verify_batch against jobs computed here: (p-1)/2, x_i^3 + 3, and 1 or p - 1 as the flag
        says - so fq_jobs is only compared and may be None.  `proofs`: objects with `words` and `degree_bits`, or (words,
        degree_bits) pairs, proof k for jobs k per_proof ...  -> (link_codes [n] uint8, proof_status [n_proofs] int32), all
        zero; a rejection raises VerifyError with the message of the smallest failing input, or of the first rejected proof
        where every link holds, and both arrays as its `link_codes` (ROOT_*) and `proof_status`."""
        return self._verify_roots(G1_RECOVER, "bn254s_verify_g1_recover", proofs, per_proof, xs, None, points, flags, None, fq_jobs, params)

    def verify_g2_recover(self, proofs, per_proof, xs, sgns, points, flags, fq_jobs=None, params: Optional[Params] = None):
        """The statement of a g2_recover_from_x call (bn254s_verify_g2_recover): flags[i] says whether g = x_i^3 + b' is a square
        of Fq2 (the proven symbol is that of norm(g)), and points[i] is (x_i, y_i) with y_i^2 = g and sgn(y_i) == sgns[i] (None:
        all 0) where it is and (x_i, 0) where it is not.  Otherwise as verify_g1_recover."""
        return self._verify_roots(G2_RECOVER, "bn254s_verify_g2_recover", proofs, per_proof, xs, sgns, points, flags, None, fq_jobs, params)

    def verify_fq_sqrt(self, proofs, per_proof, xs, sgns, roots, square, root_ok, fq_jobs=None, params: Optional[Params] = None):
        """The statement of an fq_sqrt call (bn254s_verify_fq_sqrt): square[i] says whether the Legendre symbol of x_i is 1 (the
        proofs are judged against 1, p - 1, or 0 for x_i = 0), root_ok[i] whether a root with the parity sgns[i] exists, and
        roots[i] is that root or zero.  Otherwise as verify_g1_recover."""
        return self._verify_roots(FQ_SQRT, "bn254s_verify_fq_sqrt", proofs, per_proof, xs, sgns, roots, square, root_ok, fq_jobs, params)

    def verify_fq2_sqrt(self, proofs, per_proof, xs, sgns, roots, square, root_ok, fq_jobs=None, params: Optional[Params] = None):
        """The Fq2 twin of verify_fq_sqrt (bn254s_verify_fq2_sqrt): the symbol of norm(x_i), the square in Fq2, the sign of
        sgn.rs:20-27."""
        return self._verify_roots(FQ2_SQRT, "bn254s_verify_fq2_sqrt", proofs, per_proof, xs, sgns, roots, square, root_ok, fq_jobs, params)

    def verify_map_to_g1(self, proofs, per_proof, u, points, sq_flags, fq_jobs=None, params: Optional[Params] = None):
        """The statement of a map_to_g1 call (bn254s_verify_map_to_g1): sq_flags[2i], sq_flags[2i + 1] say whether g(x1), g(x2) of
        the candidates of u_i are squares (2n jobs: len(proofs) == ceil(2n / per_proof)), and points[i] is the candidate that they
        select with the root of g of the parity of u_i.  link_codes is [n], per input.  Otherwise as verify_g1_recover."""
        return self._verify_roots(MAP_TO_G1, "bn254s_verify_map_to_g1", proofs, per_proof, u, None, points, sq_flags, None, fq_jobs, params)

    def ctl_values(self, kind, scalars, x, offset, outputs):
        """(input rows [n, 81|145|33], output rows [n, 33|65|17]): the extra looking values of the two CTLs."""
        n = scalars.shape[0]
        pl = {0: 32, 1: 64, 2: 16}[kind]
        rows_in = np.zeros((n, (pl if kind == 2 else 2 * pl) + 17), np.uint64)
        rows_out = np.zeros((n, pl + 1), np.uint64)
        outputs = np.ascontiguousarray(outputs, dtype=np.uint64)
        self._check(self._lib.bn254s_ctl_values(kind, _ptr(scalars), _ptr(x), _ptr(offset), _ptr(outputs), n, _ptr(rows_in),
                                                _ptr(rows_out)), "bn254s_ctl_values")
        return rows_in, rows_out

    # ---- kernel-level entry points ----
    def commit_values(self, values: np.ndarray, want_coeffs=True, want_lde=True):
        ncols, n = values.shape
        assert n == 65536
        coeffs = np.zeros((ncols, n), np.uint64) if want_coeffs else None
        lde = np.zeros((ncols, 2 * n), np.uint64) if want_lde else None
        cap = np.zeros((16, 4), np.uint64)
        self._check(self._lib.bn254s_commit_values(self._h, _ptr(values), ncols, _ptr(coeffs), _ptr(lde), _ptr(cap)),
                    "bn254s_commit_values")
        return coeffs, lde, cap

    def bench_ntt(self, ncols: int, iters: int = 10) -> float:
        ms = C.c_float()
        self._check(self._lib.bn254s_bench_ntt(self._h, ncols, iters, C.byref(ms)), "bn254s_bench_ntt")
        return ms.value

    def bench_ntt_clock(self, ncols: int, iters: int = 10):
        """(ms per stage, mean shader MHz, slowest-interval MHz) of the NTT/LDE stage alone on the GPU."""
        ms, mhz, mn = C.c_float(), C.c_float(), C.c_float()
        self._check(self._lib.bn254s_bench_ntt_clock(self._h, ncols, iters, C.byref(ms), C.byref(mhz), C.byref(mn)), "bn254s_bench_ntt_clock")
        return ms.value, mhz.value, mn.value

    def bench_issue(self):
        """(ns per wave-instruction and SIMD of the half-rate vector class at 8 waves per SIMD, shader MHz meanwhile)."""
        ns, mhz = C.c_float(), C.c_float()
        self._check(self._lib.bn254s_bench_issue(self._h, C.byref(ns), C.byref(mhz)), "bn254s_bench_issue")
        return ns.value, mhz.value

    def bench_copy(self, words: int, iters: int = 3):
        self._check(self._lib.bn254s_bench_copy(self._h, words, iters), "bn254s_bench_copy")

    def bench_leafhash(self, ncols: int, log_leaves: int = 17, iters: int = 5) -> float:
        ms = C.c_float()
        self._check(self._lib.bn254s_bench_leafhash(self._h, ncols, log_leaves, iters, C.byref(ms)), "bn254s_bench_leafhash")
        return ms.value

    def selftest_field(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """Debug: the hand-written field sequences (csrc/gl_asm.h) on operand pairs; returns out[n][17]."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        out = np.zeros((a.shape[0], 17), np.uint64)
        self._check(self._lib.bn254s_selftest_field(self._h, _ptr(a), _ptr(b), a.shape[0], _ptr(out)), "bn254s_selftest_field")
        return out

    def selftest_poseidon(self, variant: int, states: np.ndarray) -> np.ndarray:
        """Debug: states[n][12] through one implementation of the permutation: 0 the hand-scheduled statement, 1 the compiler's
        code, 2 the cooperative code (bn254s_selftest_poseidon)."""
        st = np.ascontiguousarray(states, dtype=np.uint64).copy()
        assert st.ndim == 2 and st.shape[1] == 12
        self._check(self._lib.bn254s_selftest_poseidon(self._h, variant, _ptr(st), st.shape[0]), "bn254s_selftest_poseidon")
        return st

    def selftest_leaf_hash(self, data: np.ndarray, kernel: int, chunk_cols: int = 0) -> np.ndarray:
        """Debug: leaf digests [2^k][4] of column-major data[ncols][2^k] by one leaf-hash kernel: 0 what the latency mode picks,
        1 k_leaf_hash, 2 k_leaf_hash_coop, 3 k_leaf_absorb fed chunk_cols columns per call (bn254s_selftest_leaf_hash)."""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        ncols, n = data.shape
        assert n > 0 and n & (n - 1) == 0, "the number of leaves must be a power of two"
        out = np.zeros((n, 4), np.uint64)
        self._check(self._lib.bn254s_selftest_leaf_hash(self._h, _ptr(data), ncols, n.bit_length() - 1, kernel, chunk_cols, _ptr(out)),
                    "bn254s_selftest_leaf_hash")
        return out

    def selftest_fq_inv(self, x: np.ndarray) -> np.ndarray:
        """Debug: x[n][4] canonical words -> out[n][8] = x^-1 mod p by divsteps and by Fermat (bn254s_selftest_fq_inv)."""
        x = np.ascontiguousarray(x, dtype=np.uint64)
        out = np.zeros((x.shape[0], 8), np.uint64)
        self._check(self._lib.bn254s_selftest_fq_inv(self._h, _ptr(x), x.shape[0], _ptr(out)), "bn254s_selftest_fq_inv")
        return out

    SELFTEST_FQ_WORDS = ((16, 68), (16, 60), (32, 92), (72, 74))   # (in, out) words per row, by group

    def selftest_fq(self, group: int, rows: np.ndarray) -> np.ndarray:
        """Debug: the Fq / Fq2 device arithmetic on raw residues, rows[n][W_in] words -> out[n][W_out]; group 0 Fq, 1 Fq2,
        2 the cooperative products and combine, 3 the Jacobian curve code (bn254s_selftest_fq)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if not 0 <= group < len(self.SELFTEST_FQ_WORDS):
            raise ValueError(f"selftest_fq: unknown group {group}")
        wi, wo = self.SELFTEST_FQ_WORDS[group]
        assert rows.ndim == 2 and rows.shape[1] == wi, (rows.shape, wi)
        out = np.zeros((rows.shape[0], wo), np.uint64)
        self._check(self._lib.bn254s_selftest_fq(self._h, group, _ptr(rows), rows.shape[0], _ptr(out)), "bn254s_selftest_fq")
        return out

    def selftest_logup(self, trace: np.ndarray, rc_begin: int, n_rc: int, table_col: int, freq_col: int, betas) -> np.ndarray:
        """Debug: the LogUp columns of trace[ncols][rows] through the provers' aux_build: out[2 (m + 1)][rows], per challenge the
        m = ceil(n_rc / 2) helper columns and Z (bn254s_selftest_logup)."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        assert trace.ndim == 2
        ncols, rows = trace.shape
        b = np.array([int(betas[0]), int(betas[1])], dtype=np.uint64)
        out = np.zeros((2 * ((n_rc + 1) // 2 + 1), rows), np.uint64)
        self._check(self._lib.bn254s_selftest_logup(self._h, _ptr(trace), rows, ncols, rc_begin, n_rc, table_col, freq_col, _ptr(b),
                                                    _ptr(out)), "bn254s_selftest_logup")
        return out

    # The quotient kernels and the auxiliary columns of a STARK kind on caller data (csrc/quotient_selftest.hip; include/bn254_stark.h
    # has the layouts).
    STARK_SHAPES = {0: (781, 456, 1111, 1573), 1: (1295, 906, 1693, 2605), 2: (427, 134, 770, 910)}   # kind: W, A, AIR constraints, K
    QS_MAX_PARTS = 7
    QS_N_PARTS = {0: 6, 1: 7, 2: 2}

    def selftest_quotient(self, kind: int, log_n: int, trace: np.ndarray, aux: np.ndarray, alphas, betas, gammas, raw: bool = False,
                          window=None, tables=None, fill: int = 0):
        """Debug: the quotient kernels of `kind` on trace[W][stride], aux[A][stride] (bn254s_selftest_quotient).  window = None: the
        whole domain in leaf order, stride = 2^(log_n + 1); window = (h, k0, count): the rows k0 .. k0 + count of coset h in natural
        order.  tables = (x, lfirst, llast) or None for the library's own.  raw: no division by Z_H, z_last = x.  Returns
        (out[2][2][N], part[7][2][stride]); both start out filled with the word `fill`."""
        w, a, _, _ = self.STARK_SHAPES[kind]
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        aux = np.ascontiguousarray(aux, dtype=np.uint64)
        stride = trace.shape[1]
        assert trace.shape == (w, stride) and aux.shape == (a, stride), (trace.shape, aux.shape)
        n = 1 << log_n
        flags = (2 if raw else 0) | (1 if window is not None else 0)
        h, k0, count = window if window is not None else (0, 0, 0)
        if window is None:
            assert stride == 2 * n, (stride, n)
        ch = [np.array([int(v[0]), int(v[1])], dtype=np.uint64) for v in (alphas, betas, gammas)]
        tabs = [None, None, None] if tables is None else [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
        if tables is not None:
            want = count if window is not None else 2 * n
            assert all(t.shape == (want,) for t in tabs), [t.shape for t in tabs]
        out = np.full((2, 2, n), fill, np.uint64)
        part = np.full((self.QS_MAX_PARTS, 2, stride), fill, np.uint64)
        self._check(self._lib.bn254s_selftest_quotient(self._h, kind, log_n, flags, h, k0, count, stride if window is not None else 0,
                                                       _ptr(trace), _ptr(aux), _ptr(ch[0]), _ptr(ch[1]), _ptr(ch[2]), _ptr(tabs[0]),
                                                       _ptr(tabs[1]), _ptr(tabs[2]), _ptr(out), _ptr(part)), "bn254s_selftest_quotient")
        return out, part

    def selftest_point_tables(self, log_n: int, window=None) -> np.ndarray:
        """Debug: out[3][n] = x, L_first, L_last of the quotient kernels' point tables: the whole domain in leaf order (n = 2^(log_n + 1))
        or, window = (h, k0, count), the rows k0 .. of coset h in natural order (bn254s_selftest_point_tables)."""
        h, k0, count = window if window is not None else (0, 0, 2 << log_n)
        out = np.zeros((3, count), np.uint64)
        self._check(self._lib.bn254s_selftest_point_tables(self._h, log_n, int(window is not None), h, k0, count, _ptr(out)),
                    "bn254s_selftest_point_tables")
        return out

    def selftest_aux(self, kind: int, trace: np.ndarray, betas, gammas) -> np.ndarray:
        """Debug: all auxiliary columns out[A][rows] of trace[W][rows] through the provers' aux_build with the kind's shape, CTL Z
        columns included (bn254s_selftest_aux)."""
        w, a, _, _ = self.STARK_SHAPES[kind]
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        assert trace.ndim == 2 and trace.shape[0] == w, trace.shape
        rows = trace.shape[1]
        b = np.array([int(betas[0]), int(betas[1])], dtype=np.uint64)
        g = np.array([int(gammas[0]), int(gammas[1])], dtype=np.uint64)
        out = np.zeros((a, rows), np.uint64)
        self._check(self._lib.bn254s_selftest_aux(self._h, kind, _ptr(trace), rows, _ptr(b), _ptr(g), _ptr(out)), "bn254s_selftest_aux")
        return out

    # The openings / FRI kernels and the un-reduced accumulators on caller data (csrc/fri_selftest.hip; include/bn254_stark.h has
    # the layouts).  Extension elements are (c0, c1) pairs of Python integers or two-word arrays.
    def selftest_acc(self, values: np.ndarray, weights: np.ndarray) -> np.ndarray:
        """Debug: values[rows][T], weights[T] -> out[rows][2] = sum_t values[r][t] weights[t] mod p by Acc and by Acc3, one
        accumulator per row (bn254s_selftest_acc)."""
        values = np.ascontiguousarray(values, dtype=np.uint64)
        weights = np.ascontiguousarray(weights, dtype=np.uint64)
        rows, t = values.shape
        assert weights.shape == (t,)
        out = np.zeros((rows, 2), np.uint64)
        self._check(self._lib.bn254s_selftest_acc(self._h, _ptr(values), _ptr(weights), t, rows, _ptr(out)), "bn254s_selftest_acc")
        return out

    def selftest_openings(self, coeffs: np.ndarray, log_r: int, zeta, zeta_next) -> np.ndarray:
        """Debug: coeffs[npolys][2^(16 + log_r)] in the provers' transposed layout -> the partial evaluations
        out[npolys][2^log_r][5] of fri_openings at (zeta, zeta_next) (bn254s_selftest_openings)."""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
        npolys, n = coeffs.shape
        assert n == 1 << (16 + log_r), (n, log_r)
        z0 = np.array([int(v) for v in zeta], dtype=np.uint64)
        z1 = np.array([int(v) for v in zeta_next], dtype=np.uint64)
        out = np.zeros((npolys, 1 << log_r, 5), np.uint64)
        self._check(self._lib.bn254s_selftest_openings(self._h, _ptr(coeffs), npolys, log_r, _ptr(z0), _ptr(z1), _ptr(out)),
                    "bn254s_selftest_openings")
        return out

    def selftest_fri_combine_coeffs(self, cols: np.ndarray, w: int, n_rc: int, n_ctl: int, weights: np.ndarray) -> np.ndarray:
        """Debug: cols[W + A + 4][n] (trace | auxiliary | quotient), weights[W + A + 4][2] -> comb[6][n] of fri_combine_coeffs
        (bn254s_selftest_fri_combine, mode 0)."""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        weights = np.ascontiguousarray(weights, dtype=np.uint64)
        n_polys, n = cols.shape
        assert n_polys == w + 2 * ((n_rc + 1) // 2 + 1) + 2 * n_ctl + 4 and weights.shape == (n_polys, 2), (cols.shape, weights.shape)
        out = np.zeros((6, n), np.uint64)
        self._check(self._lib.bn254s_selftest_fri_combine(self._h, 0, w, n_rc, n_ctl, n, _ptr(cols), _ptr(weights), None, _ptr(out)),
                    "bn254s_selftest_fri_combine")
        return out

    def selftest_fri_combine_final(self, cl: np.ndarray, xs: np.ndarray, w: int, n_rc: int, n_ctl: int, zeta, zeta_next, r0, r1, r2,
                                   alpha) -> np.ndarray:
        """Debug: cl[6][m], xs[m] -> out[m][2], the point-wise part of the batched quotient by fri_combine_final
        (bn254s_selftest_fri_combine, mode 1)."""
        cl = np.ascontiguousarray(cl, dtype=np.uint64)
        xs = np.ascontiguousarray(xs, dtype=np.uint64)
        m = xs.shape[0]
        assert cl.shape == (6, m)
        pts = np.array([int(v) for e in (zeta, zeta_next, r0, r1, r2, alpha) for v in e], dtype=np.uint64)
        out = np.zeros((m, 2), np.uint64)
        self._check(self._lib.bn254s_selftest_fri_combine(self._h, 1, w, n_rc, n_ctl, m, _ptr(cl), _ptr(xs), _ptr(pts), _ptr(out)),
                    "bn254s_selftest_fri_combine")
        return out

    def selftest_fri_fold(self, vals: np.ndarray, shift: int, beta) -> np.ndarray:
        """Debug: vals[2^log_m][2] (bit-reversed order on shift <w>) -> the arity-16 fold at beta, out[2^(log_m - 4)][2]
        (bn254s_selftest_fri_fold)."""
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        m = vals.shape[0]
        assert vals.shape == (m, 2) and m >= 16 and m & (m - 1) == 0
        b = np.array([int(beta[0]), int(beta[1])], dtype=np.uint64)
        out = np.zeros((m >> 4, 2), np.uint64)
        self._check(self._lib.bn254s_selftest_fri_fold(self._h, _ptr(vals), m.bit_length() - 1, int(shift), _ptr(b), _ptr(out)),
                    "bn254s_selftest_fri_fold")
        return out

    def selftest_fri_rows(self, lde: np.ndarray, h: int, k0: int, rows: int, indices):
        """Debug: lde[ncols][2 N] in leaf order -> (window[ncols][rows] of coset h from row k0 on, wrapping at N;
        gathered[ncols][nq] = lde[:, indices]) by fri_extract_window and fri_gather_rows (bn254s_selftest_fri_rows)."""
        lde = np.ascontiguousarray(lde, dtype=np.uint64)
        ncols, m2 = lde.shape
        assert m2 >= 4 and m2 & (m2 - 1) == 0
        idx = np.ascontiguousarray(indices, dtype=np.uint32)
        win = np.zeros((ncols, rows), np.uint64)
        gat = np.zeros((ncols, idx.shape[0]), np.uint64)
        self._check(self._lib.bn254s_selftest_fri_rows(self._h, _ptr(lde), ncols, m2.bit_length() - 2, h, k0, rows,
                                                       idx.ctypes.data_as(C.c_void_p), idx.shape[0], _ptr(win), _ptr(gat)),
                    "bn254s_selftest_fri_rows")
        return win, gat

    # The NTT / LDE stage at every height on caller data (csrc/ntt_selftest.hip; include/bn254_stark.h has the layouts).
    TRANSFORM_SPLIT, TRANSFORM_COMPACT = 1, 2   # flags of selftest_transforms

    def selftest_transforms(self, op: int, log_n: int, flags: int, data: np.ndarray, coset_mask: int = 3):
        """Debug: the provers' transform dispatch for a proof of 2^log_n rows on data[ncols][2^log_n]: op 0 values -> (coeffs, lde),
        1 coeffs -> lde, 2 coeffs -> lde of the cosets in coset_mask (the rest stays 2^64 - 1), 3 qv[4][N] -> ab[4][N]
        (bn254s_selftest_transforms)."""
        data = np.ascontiguousarray(data, dtype=np.uint64)
        ncols, n = data.shape
        assert n == 1 << log_n, (n, log_n)
        out0 = np.zeros((ncols, n if op in (0, 3) else 2 * n), np.uint64)
        out1 = np.zeros((ncols, 2 * n), np.uint64) if op == 0 else None
        self._check(self._lib.bn254s_selftest_transforms(self._h, op, log_n, flags, ncols, coset_mask, _ptr(data), _ptr(out0),
                                                         _ptr(out1)), "bn254s_selftest_transforms")
        return (out0, out1) if op == 0 else out0

    def selftest_mul_2exp(self, x: np.ndarray) -> np.ndarray:
        """Debug: x[n] -> out[n][64], out[i][e] = x[i] 2^(3 e) mod p by the shift table of the outer NTT passes
        (bn254s_selftest_mul_2exp)."""
        x = np.ascontiguousarray(x, dtype=np.uint64)
        out = np.zeros((x.shape[0], 64), np.uint64)
        self._check(self._lib.bn254s_selftest_mul_2exp(self._h, _ptr(x), x.shape[0], _ptr(out)), "bn254s_selftest_mul_2exp")
        return out

    def selftest_outer_dft(self, log_r: int, inverse: bool, rows: np.ndarray) -> np.ndarray:
        """Debug: rows[n][2^log_r] -> the registers of the outer passes' R-point DFT on each row, in register order
        (bn254s_selftest_outer_dft)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        assert rows.ndim == 2 and rows.shape[1] == 1 << log_r, (rows.shape, log_r)
        out = np.zeros_like(rows)
        self._check(self._lib.bn254s_selftest_outer_dft(self._h, log_r, int(inverse), _ptr(rows), rows.shape[0], _ptr(out)),
                    "bn254s_selftest_outer_dft")
        return out

    def poseidon_permute(self, states: np.ndarray) -> np.ndarray:
        st = np.ascontiguousarray(states, dtype=np.uint64).copy()
        self._check(self._lib.bn254s_poseidon_permute(self._h, _ptr(st), st.shape[0]), "bn254s_poseidon_permute")
        return st

    def generate_trace(self, kind, scalars, x, offset=None, min_rows_log2=16):
        """kind 0 = G1, 1 = G2, 2 = Fq exp.  Returns (trace[W, rows], outputs[n, 8|16|4])."""
        width, pw = {0: (781, 8), 1: (1295, 16), 2: (427, 4)}[kind]
        n = scalars.shape[0]
        rows = max(1 << min_rows_log2, 512 * n)
        rows = 1 << (rows - 1).bit_length()
        trace = np.zeros((width, rows), np.uint64)
        outs = np.zeros((n, pw), np.uint64)
        self._check(self._lib.bn254s_generate_trace(self._h, kind, _ptr(scalars), _ptr(x), _ptr(offset), n, min_rows_log2,
                                                    _ptr(trace), _ptr(outs)), "bn254s_generate_trace")
        return trace, outs

    def g1_generate_trace(self, scalars, x, offset, min_rows_log2=16, width=781):
        n = scalars.shape[0]
        rows = max(1 << min_rows_log2, 512 * n)
        rows = 1 << (rows - 1).bit_length()
        trace = np.zeros((width, rows), np.uint64)
        outs = np.zeros((n, 8), np.uint64)
        self._check(self._lib.bn254s_g1_generate_trace(self._h, _ptr(scalars), _ptr(x), _ptr(offset), n, min_rows_log2,
                                                       _ptr(trace), _ptr(outs)), "bn254s_g1_generate_trace")
        return trace, outs


def verify_host(kind, words, degree_bits, scalars, x, offset, outputs, params: Optional[Params] = None):
    """bn254s_verify_host: the native verifier without a context or a GPU (the AIR is evaluated on the host over the quadratic
    extension).  Returns None or raises VerifyError(reason)."""
    lib = load_library()
    params = params or default_params()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    outputs = np.ascontiguousarray(outputs, dtype=np.uint64)
    buf = C.create_string_buffer(256)
    rc = lib.bn254s_verify_host(kind, C.byref(params), degree_bits, _ptr(words), words.size, _ptr(scalars), _ptr(x), _ptr(offset),
                                _ptr(outputs), scalars.shape[0], buf, 256)
    if rc == -8:
        raise VerifyError(buf.value.decode())
    if rc != 0:
        raise RuntimeError(f"bn254s_verify_host failed with {rc}: {buf.value.decode()}")


_POINT_WORDS = (8, 16, 4)
VERIFY_RECORD_HEAD = 34  # BN254S_VERIFY_RECORD_HEAD: words of a front record before the query indices


def proof_words(kind, degree_bits, params: Optional[Params] = None) -> int:
    """Words of a proof of 2^degree_bits rows in the layout of include/bn254_stark.h (make_view of csrc/verify_query.h)."""
    params = params or default_params()
    plan = proof_plan(kind, 1, 0)
    w, a = plan["W"], plan["A"]
    log_m2 = degree_bits + params.rate_bits
    path = log_m2 - params.cap_height
    wpq = w + a + 4 + 12 * path
    d, bits, layers = degree_bits, log_m2, 0
    while d > params.final_poly_bits and d + params.rate_bits - params.arity_bits >= params.cap_height:
        d -= params.arity_bits
        bits -= params.arity_bits
        layers += 1
        wpq += (2 << params.arity_bits) + 4 * (bits - params.cap_height)
    return 192 + 4 * w + 4 * a + 4 + 8 + 64 * layers + params.num_queries * wpq + (2 << d) + 1 + 12


def _word_arrays(word_list):
    """Contiguous uint64 arrays (kept alive by the caller) and the pointer table the batch entry points take."""
    arrs = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in word_list]
    table = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    return arrs, table


def _verify_batch(lib, handle, kind, proofs, scalars, x, offset, n_jobs, params, degree_bits):
    params = params or default_params()
    pw = _POINT_WORDS[kind]
    words, outs = [], []
    for pr in proofs:
        if isinstance(pr, (tuple, list)):
            w, o = pr
        else:
            w, o = pr.words, pr.outputs
            degree_bits = pr.degree_bits if degree_bits is None else degree_bits
        words.append(np.ascontiguousarray(w, dtype=np.uint64).reshape(-1))
        outs.append(np.ascontiguousarray(o, dtype=np.uint64).reshape(-1))
    n = len(words)
    if n == 0:
        raise ValueError("verify_batch: no proofs")
    if degree_bits is None:  # the height whose proof has as many words as one of these
        sizes = {proof_words(kind, d, params): d for d in range(7, 31)}
        degree_bits = next((sizes[w.size] for w in words if w.size in sizes), None)
        if degree_bits is None:
            raise ValueError("verify_batch: cannot tell degree_bits from the proof sizes, pass it")
    if n_jobs is None:
        n_jobs = [o.size // pw for o in outs]
    n_jobs = [int(k) for k in n_jobs]
    lo = np.concatenate(([0], np.cumsum(n_jobs)))
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, pw)
    offset = None if offset is None else np.ascontiguousarray(offset, dtype=np.uint64).reshape(-1, pw)
    verdicts = [None] * n
    # one size per call in the C interface: proofs of different sizes (a truncated one beside whole ones) go in one call per size
    groups = {}
    for i, w in enumerate(words):
        groups.setdefault(w.size, []).append(i)
    for n_words, idx in groups.items():
        rows = np.concatenate([np.arange(lo[i], lo[i + 1]) for i in idx]).astype(np.int64)
        whole = len(groups) == 1
        s_, x_ = (scalars, x) if whole else (np.ascontiguousarray(scalars[rows]), np.ascontiguousarray(x[rows]))
        o_ = offset if whole or offset is None else np.ascontiguousarray(offset[rows])
        outputs = np.ascontiguousarray(np.concatenate([outs[i] for i in idx]))
        arrs, table = _word_arrays([words[i] for i in idx])
        m = len(idx)
        nj = (C.c_size_t * m)(*[n_jobs[i] for i in idx])
        status = np.zeros(m, dtype=np.int32)
        stride = 128
        err = C.create_string_buffer(m * stride)
        rc = lib.bn254s_verify_batch(handle, kind, C.byref(params), degree_bits, table, n_words, _ptr(s_), _ptr(x_), _ptr(o_),
                                     _ptr(outputs), nj, m, status.ctypes.data_as(C.c_void_p), err, stride)
        if rc not in (0, -8):
            why = lib.bn254s_last_error(handle).decode() if handle else ""
            raise RuntimeError(f"bn254s_verify_batch failed with {rc}: {why}")
        for k, i in enumerate(idx):
            if status[k] != 0:
                verdicts[i] = err.raw[k * stride:(k + 1) * stride].split(b"\0", 1)[0].decode()
    return verdicts


def verify_batch_host(kind, proofs, scalars, x, offset, n_jobs=None, params: Optional[Params] = None, degree_bits=None):
    """bn254s_verify_batch without a context: the same verdicts as Context.verify_batch, every part on host threads, no GPU."""
    return _verify_batch(load_library(), None, kind, proofs, scalars, x, offset, n_jobs, params, degree_bits)


def verify_front(kind, words, degree_bits, params: Optional[Params] = None):
    """bn254s_selftest_verify_front: (status, record) of one proof - the host part of the verifier up to and including the proof of
    work, and the front record the query rounds read (layout: include/bn254_stark.h).  Host only."""
    lib = load_library()
    params = params or default_params()
    words = np.ascontiguousarray(words, dtype=np.uint64)
    rec = np.zeros(VERIFY_RECORD_HEAD + params.num_queries, dtype=np.uint64)
    rc = lib.bn254s_selftest_verify_front(kind, C.byref(params), degree_bits, _ptr(words), words.size, _ptr(rec), rec.size)
    return rc, rec


def query_round(kind, words, degree_bits, records, chunk_proofs=0, params: Optional[Params] = None, _ctx=None) -> np.ndarray:
    """bn254s_selftest_query_round on the host: the code of every query of every proof, [n_proofs, num_queries] int32, for the
    proofs `words` (a list of word arrays of one size) and their front records [n_proofs, record words]."""
    lib = load_library()
    params = params or default_params()
    arrs, table = _word_arrays(words)
    records = np.ascontiguousarray(records, dtype=np.uint64).reshape(len(arrs), -1)
    if records.shape[1] != VERIFY_RECORD_HEAD + params.num_queries:
        raise ValueError("query_round: records of the wrong length")
    codes = np.full((len(arrs), params.num_queries), -1, dtype=np.int32)
    rc = lib.bn254s_selftest_query_round(_ctx._h if _ctx is not None else None, kind, C.byref(params), degree_bits, table,
                                         arrs[0].size, _ptr(records), len(arrs), chunk_proofs, codes.ctypes.data_as(C.c_void_p))
    if rc != 0:
        why = lib.bn254s_last_error(_ctx._h).decode() if _ctx is not None else ""
        raise RuntimeError(f"bn254s_selftest_query_round failed with {rc}: {why}")
    return codes


def query_text(n_layers, code):
    """bn254s_selftest_query_text: the verifier's text of a query code ("" for 0, None for a code that does not exist)."""
    t = load_library().bn254s_selftest_query_text(n_layers, code)
    return None if t is None else t.decode()


PLAN_BUFFERS = ("in", "tvals", "tcoef", "hist", "tmp", "ldechunk", "sponge", "comb", "tlde", "trees", "avals", "acoef", "alde",
                "scratch", "quot", "tabs", "open", "fri", "fritrees", "qout", "win")
_PLAN_HEAD = ("kind", "n", "W", "A", "K", "point_words", "N", "log_n", "log_s", "log_r", "R", "NH", "NSPL", "stream", "lowmem",
              "log_bk", "BK", "WROWS", "L")
_PLAN_TAIL = ("wpq", "tree_words", "fri_words", "fri_tree_words", "in_words")


def proof_plan(kind, n, dev_total_bytes, force_split=False, force_lowmem=False, force_stream=False, stream_win_log=None,
               params: Optional[Params] = None) -> dict:
    """bn254s_selftest_proof_plan: what the prover decides before it touches memory, without a context or a GPU.  The scalar fields
    by name, "arities" (a list of L), "words" (a dict over PLAN_BUFFERS; 0 = no buffer of that name) and "pinned_bytes".  The
    keyword arguments stand for the BN254S_FORCE_* / BN254S_STREAM_WIN_LOG overrides.  Raises RuntimeError(code and reason)."""
    lib = load_library()
    params = params or default_params()
    out = np.zeros(54, np.uint64)
    buf = C.create_string_buffer(256)
    rc = lib.bn254s_selftest_proof_plan(kind, n, C.byref(params), dev_total_bytes, int(force_split), int(force_lowmem), int(force_stream),
                                        -1 if stream_win_log is None else stream_win_log, _ptr(out), buf, 256)
    if rc != 0:
        raise RuntimeError(f"bn254s_selftest_proof_plan failed with {rc}: {buf.value.decode()}")
    v = [int(w) for w in out]
    plan = dict(zip(_PLAN_HEAD, v[:19]))
    plan["arities"] = v[19:19 + plan["L"]]
    plan.update(zip(_PLAN_TAIL, v[27:32]))
    plan["words"] = dict(zip(PLAN_BUFFERS, v[32:53]))
    plan["pinned_bytes"] = v[53]
    return plan


def _proof_slices(tag, proofs, n, per_proof, w):
    """Checks the number of proofs for n jobs at once, then yields (k, proof, lo, hi, outs) for proof k of jobs lo .. hi - 1, outs
    [hi - lo, w] its outputs, after checking that it has one per job."""
    if len(proofs) != (n + per_proof - 1) // per_proof:
        raise VerifyError(f"{tag}: {len(proofs)} proofs for {n} jobs of {per_proof} per proof")

    def walk():
        for k, pr in enumerate(proofs):
            lo, hi = k * per_proof, min(n, (k + 1) * per_proof)
            outs = np.asarray(pr.outputs, dtype=np.uint64).reshape(-1, w)
            if outs.shape[0] != hi - lo:
                raise VerifyError(f"{tag}: proof {k} has {outs.shape[0]} outputs for jobs {lo}..{hi - 1}")
            yield k, pr, lo, hi, outs
    return walk()


def _verify_slice(tag, kind, k, pr, lo, hi, scalars, x, offset, ctx, params):
    """Proof k against its jobs lo .. hi - 1 of the job arrays: Context.verify with a context, else verify_host."""
    s_, x_, o_ = (None if a is None else np.ascontiguousarray(a[lo:hi]) for a in (scalars, x, offset))
    try:
        if ctx is not None:
            ctx.verify(kind, pr.words, pr.degree_bits, s_, x_, o_, pr.outputs, params)
        else:
            verify_host(kind, pr.words, pr.degree_bits, s_, x_, o_, pr.outputs, params)
    except VerifyError as e:
        raise VerifyError(f"{tag}: proof {k} (jobs {lo}..{hi - 1}) rejected: {e}") from None


def _check_legendre(tag, p, k, lo, hi, outs, flags, note=lambda j: ("", "")):
    """The proven Legendre symbols of the jobs lo .. hi - 1 of proof k: each is 1 or p - 1 and agrees with its flag.  note(j): what
    the two messages add after "proof k" and after "flag j"."""
    from tools import synth

    for j in range(lo, hi):
        leg = synth.words_to_int(outs[j - lo])
        if leg not in (1, p - 1):
            raise VerifyError(f"{tag}: output {j} of proof {k}{note(j)[0]} is neither 1 nor p - 1")
        if (leg == 1) != bool(flags[j]):
            raise VerifyError(f"{tag}: flag {j}{note(j)[1]} is {int(flags[j])}, the proven Legendre symbol of job {j} is "
                              f"{'1' if leg == 1 else 'p - 1'}")


def _verify_msm(tag, kind, w, pt, neg, add, scalars, x, R, result, offsets, proofs, per_proof, ctx, params):
    """The checks of verify_g1_msm / verify_g2_msm for points of w words: pt(words) -> affine point, neg / add the group law."""
    scalars, x, R, result, offsets = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x, R, result, offsets))
    n = scalars.shape[0]
    offsets = offsets.reshape(-1, w)
    if x.shape != (n, w) or offsets.shape != (n + 1, w) or R.size != w or result.size != w:
        raise VerifyError(f"{tag}: shapes: scalars {scalars.shape}, x {x.shape}, offsets {offsets.shape}, R {R.shape}, result {result.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, w)
    if not np.array_equal(offsets[0], R.reshape(w)):
        raise VerifyError(f"{tag}: offsets[0] != R")
    for i, pr, lo, hi, outs in slices:
        bad = np.nonzero(np.any(outs != offsets[lo + 1:hi + 1], axis=1))[0]
        if bad.size:
            j = lo + int(bad[0])
            raise VerifyError(f"{tag}: output {j} of proof {i} != offsets[{j + 1}] (link s_{j} x_{j} + offset_{j})")
    try:
        want = add(pt(offsets[n]), neg(pt(R.reshape(w))))
    except ValueError:
        raise VerifyError(f"{tag}: offsets[n] == R, the result would be the point at infinity") from None
    if pt(result.reshape(w)) != want:
        raise VerifyError(f"{tag}: result != offsets[n] - R")
    for i, pr, lo, hi, _ in _proof_slices(tag, proofs, n, per_proof, w):
        _verify_slice(tag, kind, i, pr, lo, hi, scalars, x, offsets, ctx, params)


def verify_g1_msm(scalars, x, R, result, offsets, proofs, per_proof, ctx: Optional[Context] = None, params: Optional[Params] = None):
    """Checks a g1_msm: the linkage (offsets[0] == R, the outputs of proof i are offsets[lo + 1 .. hi] for its jobs lo .. hi - 1,
    result == offsets[n] - R in Python integer arithmetic, tools/synth.py) and every proof (Context.verify with a context, else
    verify_host) against its jobs (s_i, x_i, offsets[i]).  `proofs`: objects with `words`, `degree_bits` and `outputs`, such as
    Proof.  Returns None or raises VerifyError naming the first broken link or the rejected proof."""
    from tools import synth

    def pt(w):
        return (synth.words_to_int(w[:4]), synth.words_to_int(w[4:]))

    _verify_msm("g1_msm", 0, 8, pt, lambda p: (p[0], (-p[1]) % synth.P), synth.g1_add, scalars, x, R, result, offsets, proofs,
                per_proof, ctx, params)


def verify_g2_msm(scalars, x, R, result, offsets, proofs, per_proof, ctx: Optional[Context] = None, params: Optional[Params] = None):
    """Checks a g2_msm like verify_g1_msm checks a g1_msm: the linkage, result == offsets[n] - R in Python integer arithmetic over
    Fq2 (tools/synth.py) and every G2 proof (kind 1) against its jobs.  Returns None or raises VerifyError ("g2_msm: ...")."""
    from tools import synth

    def neg(p):
        return (p[0], ((-p[1][0]) % synth.P, (-p[1][1]) % synth.P))

    _verify_msm("g2_msm", 1, 16, synth.g2_from_words, neg, synth.g2_add, scalars, x, R, result, offsets, proofs, per_proof, ctx,
                params)


def verify_msm_multi(kind, scalars, x, seg_len, R, results, finite, offsets, outputs, proofs, per_proof, ctx: Optional[Context] = None,
                     params: Optional[Params] = None):
    """Checks a msm_multi (kind 0 = G1, 1 = G2): the outputs of proof k are outputs[lo .. hi - 1] for its jobs; offsets at the head
    of MSM j is R_j and offsets[i + 1] == outputs[i] inside an MSM; results[j] == outputs[last_j] - R_j in Python integer
    arithmetic (tools/synth.py) - a second route to the result, which the device takes from the scan - with finite[j] == 0 and
    zero words exactly where the two are equal; and every proof (Context.verify with a context, else verify_host) against its
    jobs (s_i, x_i, offsets[i]).  Returns None or raises VerifyError naming the first broken link, MSM or rejected proof."""
    from tools import job_outputs_ref as jr

    tag, w = "msm_multi", {0: 8, 1: 16}[kind]
    scalars, x, R, results, offsets, outputs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x, R, results, offsets, outputs))
    seg = [int(v) for v in np.asarray(seg_len).reshape(-1)]
    finite = np.asarray(finite).reshape(-1)
    n, m = scalars.shape[0], len(seg)
    if (x.shape != (n, w) or offsets.shape != (n, w) or outputs.shape != (n, w) or R.shape != (m, w) or results.shape != (m, w) or
            finite.shape != (m,) or min(seg, default=0) < 1 or sum(seg) != n):
        raise VerifyError(f"{tag}: shapes: scalars {scalars.shape}, x {x.shape}, offsets {offsets.shape}, outputs {outputs.shape}, "
                          f"R {R.shape}, results {results.shape}, finite {finite.shape}, seg_len sums to {sum(seg)}")
    for k, pr, lo, hi, outs in _proof_slices(tag, proofs, n, per_proof, w):
        bad = np.nonzero(np.any(outs != outputs[lo:hi], axis=1))[0]
        if bad.size:
            raise VerifyError(f"{tag}: output {lo + int(bad[0])} of proof {k} != outputs[{lo + int(bad[0])}]")
    add, neg = jr._law(kind)
    first = 0
    for j, ln in enumerate(seg):
        last = first + ln - 1
        if not np.array_equal(offsets[first], R[j]):
            raise VerifyError(f"{tag}: offsets[{first}] != R_{j} (the head of msm {j})")
        bad = np.nonzero(np.any(offsets[first + 1:last + 1] != outputs[first:last], axis=1))[0]
        if bad.size:
            t = int(bad[0])
            raise VerifyError(f"{tag}: offsets[{first + t + 1}] != outputs[{first + t}] (link {t} -> {t + 1} of msm {j})")
        want = add(jr.from_words(kind, outputs[last]), neg(jr.from_words(kind, R[j])))
        if bool(finite[j]) != (want is not None):
            raise VerifyError(f"{tag}: finite[{j}] is {int(finite[j])}, outputs[{last}] - R_{j} is "
                              f"{'finite' if want is not None else 'the point at infinity'}")
        if [int(v) for v in results[j]] != jr.to_words(kind, want):
            raise VerifyError(f"{tag}: results[{j}] != outputs[{last}] - R_{j}")
        first += ln
    for k, pr, lo, hi, _ in _proof_slices(tag, proofs, n, per_proof, w):
        _verify_slice(tag, kind, k, pr, lo, hi, scalars, x, offsets, ctx, params)


def verify_g1_recover(xs, points, flags, fq_jobs, proofs, per_proof, ctx: Optional[Context] = None, params: Optional[Params] = None):
    """Checks a g1_recover_from_x: job i is ((p-1)/2, x_i^3 + 3) in Python integer arithmetic (tools/synth.py), every Fq-exp proof
    verifies against its jobs (Context.verify with a context, else verify_host), the proven Legendre symbol of job i is 1 or p - 1
    and agrees with flags[i], and points[i] is (x_i, y_i) with y_i < p, y_i even and y_i^2 = x_i^3 + 3 where the flag is set and
    (x_i, 0) where it is not.  `proofs`: objects with `words`, `degree_bits` and `outputs`, such as Proof.  Returns None or raises
    VerifyError naming the first input or proof that fails."""
    from tools import synth

    tag, p = "g1_recover", synth.P
    xs, points, fq_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (xs, points, fq_jobs))
    flags = np.asarray(flags).reshape(-1)
    n = xs.shape[0]
    if xs.shape != (n, 4) or points.shape != (n, 8) or fq_jobs.shape != (n, 8) or flags.shape != (n,):
        raise VerifyError(f"{tag}: shapes: xs {xs.shape}, points {points.shape}, flags {flags.shape}, fq_jobs {fq_jobs.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, 4)
    g = []
    for i in range(n):
        x = synth.words_to_int(xs[i])
        if x >= p:
            raise VerifyError(f"{tag}: x_{i} is not below p")
        g.append((x * x * x + 3) % p)
        if synth.words_to_int(fq_jobs[i, :4]) != (p - 1) // 2:
            raise VerifyError(f"{tag}: scalar of job {i} != (p - 1)/2")
        if synth.words_to_int(fq_jobs[i, 4:]) != g[i]:
            raise VerifyError(f"{tag}: x of job {i} != x_{i}^3 + 3")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 2, k, pr, lo, hi, fq_jobs[:, :4], fq_jobs[:, 4:], None, ctx, params)
        _check_legendre(tag, p, k, lo, hi, outs, flags)
    for i in range(n):
        px, py = synth.words_to_int(points[i, :4]), synth.words_to_int(points[i, 4:])
        if px != synth.words_to_int(xs[i]):
            raise VerifyError(f"{tag}: point {i} does not carry x_{i}")
        if flags[i]:
            if py >= p or py & 1 or py * py % p != g[i]:
                raise VerifyError(f"{tag}: y of point {i} is not the even root of x_{i}^3 + 3 below p")
        elif py != 0:
            raise VerifyError(f"{tag}: point {i} is not (x_{i}, 0) although its flag is clear")


def verify_map_to_g1(u, points, sq_flags, fq_jobs, proofs, per_proof, ctx: Optional[Context] = None, params: Optional[Params] = None):
    """Checks a map_to_g1: jobs 2i and 2i + 1 are ((p-1)/2, g(x1)) and ((p-1)/2, g(x2)) for the candidates of u_i in Python integer
    arithmetic (tools/map_to_g1_ref.py), every Fq-exp proof verifies against its jobs (Context.verify with a context, else
    verify_host), the proven Legendre symbol of job k is 1 or p - 1 and agrees with sq_flags[k], and points[i] is the point that
    the flags select: the first candidate with a square g(x), y its root with the parity of u_i.  `proofs`: objects with `words`,
    `degree_bits` and `outputs`, such as Proof.  Returns None or raises VerifyError naming the first input or proof that fails."""
    from tools import map_to_g1_ref as ref
    from tools import synth

    tag, p = "map_to_g1", synth.P
    u, points, fq_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (u, points, fq_jobs))
    sq_flags = np.asarray(sq_flags).reshape(-1)
    n = u.shape[0]
    if u.shape != (n, 4) or points.shape != (n, 8) or fq_jobs.shape != (2 * n, 8) or sq_flags.shape != (2 * n,):
        raise VerifyError(f"{tag}: shapes: u {u.shape}, points {points.shape}, sq_flags {sq_flags.shape}, fq_jobs {fq_jobs.shape}")
    slices = _proof_slices(tag, proofs, 2 * n, per_proof, 4)
    us = []
    for i in range(n):
        ui = synth.words_to_int(u[i])
        if ui >= p:
            raise VerifyError(f"{tag}: u_{i} is not below p")
        us.append(ui)
        for j, xc in enumerate(ref.candidates(ui)[:2]):
            if synth.words_to_int(fq_jobs[2 * i + j, :4]) != (p - 1) // 2:
                raise VerifyError(f"{tag}: scalar of job {2 * i + j} (input {i}) != (p - 1)/2")
            if synth.words_to_int(fq_jobs[2 * i + j, 4:]) != ref.g(xc):
                raise VerifyError(f"{tag}: x of job {2 * i + j} != g(x{j + 1}) of input {i}")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 2, k, pr, lo, hi, fq_jobs[:, :4], fq_jobs[:, 4:], None, ctx, params)
        _check_legendre(tag, p, k, lo, hi, outs, sq_flags, lambda j: (f" (input {j // 2})", f" (g(x{j % 2 + 1}) of input {j // 2})"))
    for i in range(n):
        try:
            want = ref.select_point(us[i], bool(sq_flags[2 * i]), bool(sq_flags[2 * i + 1]))
        except ValueError:
            raise VerifyError(f"{tag}: g of the candidate that the flags of input {i} select is not a square") from None
        if (synth.words_to_int(points[i, :4]), synth.words_to_int(points[i, 4:])) != want:
            raise VerifyError(f"{tag}: point {i} is not the image of input {i}: the first candidate with a square g(x) and the root "
                              "of the parity of u")


def verify_g2_recover(xs, sgns, points, flags, fq_jobs, proofs, per_proof, ctx: Optional[Context] = None,
                      params: Optional[Params] = None):
    """Checks a g2_recover_from_x: job i is ((p-1)/2, norm(x_i^3 + b')) in Python integer arithmetic (tools/synth.py), every Fq-exp
    proof verifies against its jobs (Context.verify with a context, else verify_host), the proven Legendre symbol of job i is 1 or
    p - 1 and agrees with flags[i], and points[i] is (x_i, y_i) with both coordinates of y_i below p, y_i^2 = x_i^3 + b' and
    sgn(y_i) == sgns[i] (src/fields/sgn.rs:20-27; sgns None: all 0) where the flag is set and (x_i, 0) where it is not.  `proofs`:
    objects with `words`, `degree_bits` and `outputs`, such as Proof.  Returns None or raises VerifyError naming the first input
    or proof that fails."""
    from tools import synth

    tag, p = "g2_recover", synth.P
    xs, points, fq_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (xs, points, fq_jobs))
    flags = np.asarray(flags).reshape(-1)
    n = xs.shape[0]
    sgns = np.zeros(n, np.uint8) if sgns is None else np.asarray(sgns).reshape(-1)
    if xs.shape != (n, 8) or points.shape != (n, 16) or fq_jobs.shape != (n, 8) or flags.shape != (n,) or sgns.shape != (n,):
        raise VerifyError(f"{tag}: shapes: xs {xs.shape}, sgns {sgns.shape}, points {points.shape}, flags {flags.shape}, "
                          f"fq_jobs {fq_jobs.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, 4)
    g = []
    for i in range(n):
        x = (synth.words_to_int(xs[i, :4]), synth.words_to_int(xs[i, 4:]))
        if x[0] >= p or x[1] >= p:
            raise VerifyError(f"{tag}: x_{i} is not below p")
        if int(sgns[i]) not in (0, 1):
            raise VerifyError(f"{tag}: sign {i} is {int(sgns[i])}, neither 0 nor 1")
        g.append(synth.g2_rhs(x))
        if synth.words_to_int(fq_jobs[i, :4]) != (p - 1) // 2:
            raise VerifyError(f"{tag}: scalar of job {i} != (p - 1)/2")
        if synth.words_to_int(fq_jobs[i, 4:]) != (g[i][0] * g[i][0] + g[i][1] * g[i][1]) % p:
            raise VerifyError(f"{tag}: x of job {i} != norm(x_{i}^3 + b')")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 2, k, pr, lo, hi, fq_jobs[:, :4], fq_jobs[:, 4:], None, ctx, params)
        _check_legendre(tag, p, k, lo, hi, outs, flags)
    for i in range(n):
        if not np.array_equal(points[i, :8], xs[i]):
            raise VerifyError(f"{tag}: point {i} does not carry x_{i}")
        y = (synth.words_to_int(points[i, 8:12]), synth.words_to_int(points[i, 12:]))
        if flags[i]:
            if y[0] >= p or y[1] >= p or synth.f2_mul(y, y) != g[i]:
                raise VerifyError(f"{tag}: y of point {i} is not a root of x_{i}^3 + b' below p")
            if synth.f2_sgn(y) != bool(sgns[i]):
                raise VerifyError(f"{tag}: sign {i} is {int(sgns[i])}, y of point {i} has the other one")
        elif y != (0, 0):
            raise VerifyError(f"{tag}: point {i} is not (x_{i}, 0) although its flag is clear")


def _verify_sqrt(tag, w, xs, sgns, roots, square, root_ok, fq_jobs, proofs, per_proof, ctx, params):
    """The checks of verify_fq_sqrt / verify_fq2_sqrt for elements of w words (4: Fq, 8: Fq2)."""
    from tools import synth

    p = synth.P
    xs, roots, fq_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (xs, roots, fq_jobs))
    square, root_ok = np.asarray(square).reshape(-1), np.asarray(root_ok).reshape(-1)
    n = xs.shape[0]
    sgns = np.zeros(n, np.uint8) if sgns is None else np.asarray(sgns).reshape(-1)
    if xs.shape != (n, w) or roots.shape != (n, w) or fq_jobs.shape != (n, 8) or square.shape != (n,) or root_ok.shape != (n,) or \
            sgns.shape != (n,):
        raise VerifyError(f"{tag}: shapes: xs {xs.shape}, sgns {sgns.shape}, roots {roots.shape}, square {square.shape}, "
                          f"root_ok {root_ok.shape}, fq_jobs {fq_jobs.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, 4)

    def elem(row):
        return tuple(synth.words_to_int(row[4 * k:4 * k + 4]) for k in range(w // 4))

    x, base = [], []
    for i in range(n):
        x.append(elem(xs[i]))
        if max(x[i]) >= p:
            raise VerifyError(f"{tag}: x_{i} is not below p")
        if int(sgns[i]) not in (0, 1):
            raise VerifyError(f"{tag}: sign {i} is {int(sgns[i])}, neither 0 nor 1")
        base.append(sum(c * c for c in x[i]) % p if w == 8 else x[i][0])
        if synth.words_to_int(fq_jobs[i, :4]) != (p - 1) // 2:
            raise VerifyError(f"{tag}: scalar of job {i} != (p - 1)/2")
        if synth.words_to_int(fq_jobs[i, 4:]) != base[i]:
            raise VerifyError(f"{tag}: x of job {i} != {'norm(x_%d)' % i if w == 8 else 'x_%d' % i}")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 2, k, pr, lo, hi, fq_jobs[:, :4], fq_jobs[:, 4:], None, ctx, params)
        for j in range(lo, hi):  # the three-valued linkage: 1 for a square, p - 1 for a non-square, 0 for a zero base
            leg = synth.words_to_int(outs[j - lo])
            want = 0 if base[j] == 0 else 1 if square[j] else p - 1
            if leg not in (0, 1, p - 1) or (leg == 0) != (base[j] == 0):
                raise VerifyError(f"{tag}: output {j} of proof {k} is not a Legendre symbol of the base of job {j}")
            if leg != want or int(square[j]) not in (0, 1) or (square[j] and base[j] == 0):
                raise VerifyError(f"{tag}: flag {j} (square) is {int(square[j])}, the proven Legendre symbol of job {j} is "
                                  f"{'0' if leg == 0 else '1' if leg == 1 else 'p - 1'}")
    for i in range(n):
        has = bool(square[i]) if base[i] else int(sgns[i]) == 0  # the one root of zero has the sign 0
        if int(root_ok[i]) != int(has):
            raise VerifyError(f"{tag}: flag {i} (root_ok) is {int(root_ok[i])}, a root of x_{i} with the sign {int(sgns[i])} "
                              f"{'exists' if has else 'does not exist'}")
        y = elem(roots[i])
        if not has:
            if any(y):
                raise VerifyError(f"{tag}: root {i} is not zero although root_ok is clear")
            continue
        if max(y) >= p or (synth.f2_mul(y, y) if w == 8 else (y[0] * y[0] % p,)) != x[i]:
            raise VerifyError(f"{tag}: root {i} is not a root of x_{i} below p")
        if (synth.f2_sgn(y) if w == 8 else bool(y[0] & 1)) != bool(sgns[i]):
            raise VerifyError(f"{tag}: sign {i} is {int(sgns[i])}, root {i} has the other one")


def verify_fq_sqrt(xs, sgns, roots, square, root_ok, fq_jobs, proofs, per_proof, ctx: Optional[Context] = None,
                   params: Optional[Params] = None):
    """Checks an fq_sqrt: job i is ((p-1)/2, x_i), every Fq-exp proof verifies against its jobs (Context.verify with a context, else
    verify_host), the proven Legendre symbol of job i is 1 where square[i] is set, p - 1 where it is clear and x_i != 0, and 0 for
    x_i = 0 (where square[i] must be clear); root_ok[i] is square[i] for x_i != 0 and sgns[i] == 0 for x_i = 0; roots[i] is below p,
    squares to x_i and has the parity sgns[i] (None: all 0) where root_ok[i] is set, and is zero where it is not.  `proofs`: objects
    with `words`, `degree_bits` and `outputs`, such as Proof.  Returns None or raises VerifyError naming the first input or proof
    that fails."""
    _verify_sqrt("fq_sqrt", 4, xs, sgns, roots, square, root_ok, fq_jobs, proofs, per_proof, ctx, params)


def verify_fq2_sqrt(xs, sgns, roots, square, root_ok, fq_jobs, proofs, per_proof, ctx: Optional[Context] = None,
                    params: Optional[Params] = None):
    """Checks an fq2_sqrt like verify_fq_sqrt, with job i ((p-1)/2, norm(x_i)), norm = c0^2 + c1^2 (zero only for x_i = 0), the
    square taken in Fq2 and the sign rule of src/fields/sgn.rs:20-27: the parity of the root's c0, or of its c1 when c0 is zero."""
    _verify_sqrt("fq2_sqrt", 8, xs, sgns, roots, square, root_ok, fq_jobs, proofs, per_proof, ctx, params)


def verify_g2_subgroup(points, offsets, flags, g2_jobs, proofs, per_proof, ctx: Optional[Context] = None,
                       params: Optional[Params] = None):
    """Checks a g2_subgroup_check: job i is r | P_i (r from tools/synth.py), every coordinate of P_i is below p and P_i is on
    the twist curve in Python integer arithmetic, every G2 proof (kind 1) verifies against its jobs (r, P_i, offsets[i])
    (Context.verify with a context, else verify_host), and the proven output of job i, offsets[i] + [r]P_i, equals offsets[i]
    word for word iff flags[i].  `proofs`: objects with `words`, `degree_bits` and `outputs`, such as Proof.  Returns None or
    raises VerifyError naming the first point, job, flag or proof that fails."""
    from tools import synth

    tag, p = "g2_subgroup", synth.P
    points, offsets, g2_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (points, offsets, g2_jobs))
    flags = np.asarray(flags).reshape(-1)
    n = points.shape[0]
    if points.shape != (n, 16) or offsets.shape != (n, 16) or g2_jobs.shape != (n, 20) or flags.shape != (n,):
        raise VerifyError(f"{tag}: shapes: points {points.shape}, offsets {offsets.shape}, flags {flags.shape}, g2_jobs {g2_jobs.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, 16)
    r_words = np.array(synth._to_words(synth.R_ORDER), np.uint64)
    for i in range(n):
        pt = synth.g2_from_words(points[i])
        if max(pt[0] + pt[1]) >= p:
            raise VerifyError(f"{tag}: point {i} has a coordinate that is not below p")
        if not synth.g2_on_curve(pt):
            raise VerifyError(f"{tag}: point {i} is not on the twist curve")
        if not np.array_equal(g2_jobs[i, :4], r_words):
            raise VerifyError(f"{tag}: scalar of job {i} != r")
        if not np.array_equal(g2_jobs[i, 4:], points[i]):
            raise VerifyError(f"{tag}: x of job {i} != point {i}")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 1, k, pr, lo, hi, g2_jobs[:, :4], points, offsets, ctx, params)
        for i in range(lo, hi):
            back = np.array_equal(outs[i - lo], offsets[i])
            if back != bool(flags[i]):
                raise VerifyError(f"{tag}: flag {i} is {int(flags[i])}, the proven offset_{i} + [r] point_{i} "
                                  f"{'equals' if back else 'differs from'} offset_{i}")


def verify_g2_clear_cofactor(points, offsets, images, finite, g2_jobs, proofs, per_proof, ctx: Optional[Context] = None,
                             params: Optional[Params] = None):
    """Checks a g2_clear_cofactor: job i is h | P_i (h = 2p - r from tools/synth.py), every coordinate of P_i is below p and P_i
    is on the twist curve in Python integer arithmetic, every G2 proof (kind 1) verifies against its jobs (h, P_i, offsets[i])
    (Context.verify with a context, else verify_host), and the proven output of job i equals offsets[i] + images[i] in Python
    integer arithmetic where finite[i] is 1 and offsets[i] word for word where it is 0 (where images[i] must be zeros).
    `proofs`: objects with `words`, `degree_bits` and `outputs`, such as Proof.  Returns None or raises VerifyError naming the
    first point, job, image or proof that fails."""
    from tools import synth

    tag, p = "g2_clear_cofactor", synth.P
    points, offsets, images, g2_jobs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (points, offsets, images, g2_jobs))
    finite = np.asarray(finite).reshape(-1)
    n = points.shape[0]
    if points.shape != (n, 16) or offsets.shape != (n, 16) or images.shape != (n, 16) or g2_jobs.shape != (n, 20) or finite.shape != (n,):
        raise VerifyError(f"{tag}: shapes: points {points.shape}, offsets {offsets.shape}, images {images.shape}, finite {finite.shape}, "
                          f"g2_jobs {g2_jobs.shape}")
    slices = _proof_slices(tag, proofs, n, per_proof, 16)
    h_words = np.array(synth._to_words(synth.G2_COFACTOR), np.uint64)
    for i in range(n):
        pt = synth.g2_from_words(points[i])
        if max(pt[0] + pt[1]) >= p:
            raise VerifyError(f"{tag}: point {i} has a coordinate that is not below p")
        if not synth.g2_on_curve(pt):
            raise VerifyError(f"{tag}: point {i} is not on the twist curve")
        if not np.array_equal(g2_jobs[i, :4], h_words):
            raise VerifyError(f"{tag}: scalar of job {i} != h")
        if not np.array_equal(g2_jobs[i, 4:], points[i]):
            raise VerifyError(f"{tag}: x of job {i} != point {i}")
    for k, pr, lo, hi, outs in slices:
        _verify_slice(tag, 1, k, pr, lo, hi, g2_jobs[:, :4], points, offsets, ctx, params)
        for i in range(lo, hi):
            if finite[i]:
                img = synth.g2_from_words(images[i])
                if max(img[0] + img[1]) >= p or not synth.g2_on_curve(img):
                    raise VerifyError(f"{tag}: image {i} is not a point of the twist curve with coordinates below p")
                want = synth.g2_add_complete(synth.g2_from_words(offsets[i]), img)
                if want is None or not np.array_equal(outs[i - lo], synth.g2_points_to_words([want])[0]):
                    raise VerifyError(f"{tag}: image {i}: the proven offset_{i} + [h] point_{i} != offset_{i} + image_{i}")
            else:
                if images[i].any():
                    raise VerifyError(f"{tag}: image {i} is not zeros although finite[{i}] is 0")
                if not np.array_equal(outs[i - lo], offsets[i]):
                    raise VerifyError(f"{tag}: image {i}: finite[{i}] is 0, the proven offset_{i} + [h] point_{i} differs from offset_{i}")


def verify_job_outputs(kind, scalars, x, offset, outputs, proofs, per_proof, ctx: Optional[Context] = None,
                       params: Optional[Params] = None):
    """Checks a job_outputs: the outputs of proof k are outputs[lo .. hi - 1] word for word for its jobs lo .. hi - 1, and every
    proof verifies against its jobs (s_i, x_i, offset_i) and those outputs (Context.verify with a context, else verify_host).
    kind 0 = G1, 1 = G2, 2 = Fq exp (offset None).  `proofs`: objects with `words`, `degree_bits` and `outputs`, such as Proof.
    Returns None or raises VerifyError naming the first output or proof that fails."""
    if kind not in (0, 1, 2):
        raise ValueError(f"job_outputs: kind {kind} (0 = G1, 1 = G2, 2 = Fq exp)")
    tag, pw = "job_outputs", {0: 8, 1: 16, 2: 4}[kind]
    scalars, x, outputs = (np.ascontiguousarray(a, dtype=np.uint64) for a in (scalars, x, outputs))
    offset = None if kind == 2 or offset is None else np.ascontiguousarray(offset, dtype=np.uint64)
    n = scalars.shape[0]
    if (scalars.shape != (n, 4) or x.shape != (n, pw) or outputs.shape != (n, pw) or (kind != 2 and offset is None) or
            (offset is not None and offset.shape != (n, pw))):
        raise VerifyError(f"{tag}: shapes: scalars {scalars.shape}, x {x.shape}, offset {None if offset is None else offset.shape}, "
                          f"outputs {outputs.shape}")
    for k, pr, lo, hi, outs in _proof_slices(tag, proofs, n, per_proof, pw):
        bad = np.nonzero(np.any(outs != outputs[lo:hi], axis=1))[0]
        if bad.size:
            raise VerifyError(f"{tag}: output {lo + int(bad[0])} is not the proven output of proof {k}")
    for k, pr, lo, hi, _ in _proof_slices(tag, proofs, n, per_proof, pw):
        _verify_slice(tag, kind, k, pr, lo, hi, scalars, x, offset, ctx, params)


class BatchInFlight:
    """A batch between bn254s_prove_batch_begin and bn254s_prove_batch_end (keeps the input arrays alive meanwhile)."""

    def __init__(self, ctx, kind, scalars, x, offset, per_proof, params):
        self._ctx = ctx
        self._keep = (scalars, x, offset, params)
        n = scalars.shape[0]
        self._outs = _slots(n, per_proof)
        self._h = C.c_void_p()
        ctx._check(ctx._lib.bn254s_prove_batch_begin(ctx._h, kind, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n, per_proof,
                                                     self._outs, C.byref(self._h)), "bn254s_prove_batch_begin")

    def end(self):
        if self._h is None:
            raise RuntimeError("batch already ended")
        h, self._h = self._h, None
        self._ctx._check(self._ctx._lib.bn254s_prove_batch_end(h), "bn254s_prove_batch_end")
        self._keep = None
        return _proofs(self._ctx._lib, self._outs)

    def __del__(self):
        if getattr(self, "_h", None) is not None:  # never leave a batch running into freed inputs
            try:
                self.end()
            except Exception:
                pass


def prove_batch_multi(contexts, kind, scalars, x, offset=None, per_proof=128, params: Optional[Params] = None):
    """bn254s_prove_batch_multi: proof i on contexts[i % len(contexts)] (one Context per GPU), one process."""
    params = params or default_params()
    lib = contexts[0]._lib
    n = scalars.shape[0]
    handles = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    outs = _slots(n, per_proof)
    rc = lib.bn254s_prove_batch_multi(handles, len(contexts), kind, C.byref(params), _ptr(scalars), _ptr(x), _ptr(offset), n, per_proof,
                                      outs)
    if rc != 0:
        raise RuntimeError(f"bn254s_prove_batch_multi failed with {rc}: " + "; ".join(c._lib.bn254s_last_error(c._h).decode()
                                                                                     for c in contexts))
    return _proofs(lib, outs)
