"""The FRI batch polynomial formed on the coefficient vectors (csrc/fri.hip: k_fri_combine_coeffs, the LDE of its six sum columns,
k_fri_combine_final) is the path of every workspace kind: whole proofs through the normal entry points, word for word against
the CPU oracle, compared with the helper of tests/test_gpu_prove.py.

A proof has at least 2^16 rows (bn254s_params.min_rows_log2; shorter traces are BN254S_E_UNSUPPORTED, test_gpu_prove.py::
test_argument_errors), so the one-instance G1 proof (512 live rows) is padded to 2^16 like every small proof; the 128-instance
proof fills 2^16 rows.  The compact and the streaming workspace exist above 2^16 rows only: they are forced at 2^17 rows on an
Fq-exp proof (the narrowest trace) next to the plain workspace of the same proof, one oracle proof for the three."""
import numpy as np
import pytest

from tools import synth
from tests import oracle_lib
from tests.test_gpu_prove import first_mismatch

pytestmark = pytest.mark.gpu


def assert_same_words(got, ref):
    assert got.shape == ref.shape
    assert first_mismatch(got, ref) is None


@pytest.mark.parametrize("n", [1, 128])
def test_g1_proof_matches_oracle(gpu_ctx, oracle, n):
    """n = 1: one instance, 512 live rows padded to 2^16; n = 128: all 2^16 rows live."""
    s, x, o = synth.g1_inputs(n, seed=90 + n)
    ref, ref_out, _, degree_bits = oracle_lib.prove(oracle, 0, s, x, o)
    pr = gpu_ctx.prove_g1(s, x, o)
    assert pr.degree_bits == degree_bits == 16
    assert_same_words(pr.words, ref)
    assert np.array_equal(pr.outputs.reshape(ref_out.shape), ref_out)


def test_fq_exp_smallest_proof_matches_oracle(gpu_ctx, oracle):
    s, x = synth.fq_inputs(1, seed=93)
    ref, ref_out, _, degree_bits = oracle_lib.prove(oracle, 2, s, x)
    pr = gpu_ctx.prove_fq_exp(s, x)
    assert pr.degree_bits == degree_bits == 16
    assert_same_words(pr.words, ref)
    assert np.array_equal(pr.outputs.reshape(ref_out.shape), ref_out)


@pytest.fixture(scope="module")
def tall_fq(oracle):
    s, x = synth.fq_inputs(130, seed=94)      # 66560 rows -> 2^17
    ref, _, _, degree_bits = oracle_lib.prove(oracle, 2, s, x)
    assert degree_bits == 17
    return s, x, ref


@pytest.mark.parametrize("env", [{}, {"BN254S_FORCE_LOWMEM": "1"}, {"BN254S_FORCE_STREAM": "1", "BN254S_STREAM_WIN_LOG": "16"}],
                         ids=["plain", "compact", "streaming"])
def test_workspace_kinds_share_the_coefficient_path(gpu_ctx, tall_fq, monkeypatch, env):
    s, x, ref = tall_fq
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pr = gpu_ctx.prove_fq_exp(s, x)
    for k in env:
        monkeypatch.delenv(k)
    assert pr.degree_bits == 17
    assert_same_words(pr.words, ref)
