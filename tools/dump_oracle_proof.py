"""Writes one CPU-oracle proof and its inputs as the raw dump tools/verify_batch_asan.cpp reads (no GPU):
little-endian u64 words kind, degree_bits, n_jobs, n_words, words, scalars, x, offset (not for Fq exp), outputs.
usage: python tools/dump_oracle_proof.py out.raw [kind=2] [jobs=3]"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from tools import synth
from tests import oracle_lib

out = sys.argv[1]
kind = int(sys.argv[2]) if len(sys.argv) > 2 else 2
n = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if kind == 2:
    s, x = synth.fq_inputs(n, seed=0xA4)
    o = None
else:
    s, x, o = (synth.g1_inputs if kind == 0 else synth.g2_inputs)(n, seed=0xA4)
words, outs, _, degree_bits = oracle_lib.prove(oracle_lib.load(), kind, s, x, o)
parts = [np.array([kind, degree_bits, n, words.size], dtype=np.uint64), words, s, x] + ([] if o is None else [o]) + [outs]
np.concatenate([np.ascontiguousarray(p, dtype=np.uint64).reshape(-1) for p in parts]).astype("<u8").tofile(out)
print(f"{out}: kind {kind}, {n} jobs, 2^{degree_bits} rows, {words.size} words")
