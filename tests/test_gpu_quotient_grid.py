"""GPU parity for the G1 quotient stage run as one grid: `k_quotient_g1_parts` evaluates the six independent parts of the
constraint stream (the five eval_modulus_zero blocks of eval_g1_add and the schedule) in one launch, blockIdx.y selecting the
part, `k_quotient_finish` adds their partial sums.  Every proof word must stay what the oracle computes.

Shapes: the library proves no trace below 2^16 rows (the range-check table needs all 2^16 values: `min_rows_log2 < 16` is
BN254S_E_UNSUPPORTED, tests/test_gpu_prove.py::test_argument_errors), so one and five instances are both padded to 2^16 rows
= 2^17 LDE points = 512 workgroups in x for each of the 6 parts; all but 512 / 2560 of the rows are padding rows (filter = 0)
that pass through every part's filters.  The G2 and Fq-exp kinds keep one launch per part (their merged grids need scratch
memory) and stay covered by tests/test_gpu_g2_fq.py.
"""
import numpy as np
import pytest

from tools import synth
from tests import oracle_lib
from tests.test_gpu_prove import first_mismatch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,seed", [(1, 91), (5, 92)])
def test_g1_proof_word_for_word_vs_oracle(gpu_ctx, oracle, n, seed):
    s, x, o = synth.g1_inputs(n, seed=seed)
    ref, ref_out, _, degree_bits = oracle_lib.g1_prove(oracle, s, x, o)
    pr = gpu_ctx.prove_g1(s, x, o)
    assert pr.degree_bits == degree_bits == 16 and pr.words.shape == ref.shape
    assert first_mismatch(pr.words, ref) is None
    assert np.array_equal(pr.outputs.reshape(-1, 8), ref_out)
    rc, msg = oracle_lib.g1_verify(oracle, pr.words, degree_bits, s, x, o)
    assert rc == 0, msg


def test_streaming_windows_go_through_the_part_grid(gpu_ctx, monkeypatch):
    """Window mode of QArgs (natural order, column stride, next row = j + 1) through the same grid: the streaming workspace
    forced at 2^17 rows with windows of 2^15 rows (the smallest that tests/test_gpu_tall.py forces: four windows per coset)
    against the resident path, every word of the proof."""
    s, x, o = synth.g1_inputs(150, seed=93)
    resident = gpu_ctx.prove_batch(0, s, x, o, per_proof=150)[0]
    assert resident.degree_bits == 17
    monkeypatch.setenv("BN254S_FORCE_STREAM", "1")
    monkeypatch.setenv("BN254S_STREAM_WIN_LOG", "15")
    streamed = gpu_ctx.prove_batch(0, s, x, o, per_proof=150)[0]
    monkeypatch.delenv("BN254S_FORCE_STREAM")
    monkeypatch.delenv("BN254S_STREAM_WIN_LOG")
    assert streamed.degree_bits == 17 and streamed.words.shape == resident.words.shape
    bad = np.flatnonzero(streamed.words != resident.words)
    assert bad.size == 0, f"first differing words {bad[:5]} of {resident.words.size}"
    assert np.array_equal(streamed.outputs, resident.outputs)
    back = gpu_ctx.prove_batch(0, s, x, o, per_proof=150)[0]     # back to the resident layout in the same slot
    assert np.array_equal(back.words, resident.words)
