"""map_to_g1 on ONE GPU: the device front-end alone (bn254s_map_to_g1_batch: one inversion and three ladders g^((p+1)/4) per
input) beside the G1 recover front-end (bn254s_g1_recover_from_x_batch: one ladder per input) at the same sizes, on the same
box in the same run; hash_to_g1 (bn254s_hash_to_g1_batch, inputs of 8 elements) at the same sizes; then the full call
(bn254s_map_to_g1: front-end + Fq-exp proofs of the 2n Legendre jobs + linkage check) at 16 384 inputs against
bn254s_prove_batch (kind 2) of the same 32 768 jobs.
usage: python tools/run_map_to_g1.py [reps=5]
Inputs: uniform u below p (about half take x1, a quarter each x2 and x3).  Every figure is synchronised (the calls return after
their device work and the copies of their results to the host) and taken warm; the median of `reps` runs is reported, the
largest shape fewer times."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 5
SIZES = (128, 16384, 1 << 20)
ctx = pk.Context(0)
rng = np.random.default_rng(11)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)
GL_P = 0xFFFFFFFF00000001


def below_p(n):
    """n x 4 words, uniform below p: 256-bit values with the top word reduced below p's top word."""
    x = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    x[:, 3] %= P_WORDS[3]
    return x


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


print("map_to_g1 front-end only (bn254s_map_to_g1_batch: candidates with one inversion, three ladders, flags, points, 2n jobs) "
      "beside the G1 recover front-end (bn254s_g1_recover_from_x_batch: one ladder), ms", flush=True)
for n in SIZES:
    k = reps if n < (1 << 20) else 3
    u = below_p(n)
    med, lo, hi = median_ms(lambda: ctx.map_to_g1_batch(u), k)
    _, flags, _ = ctx.map_to_g1_batch(u)
    x1, x2 = int(flags[0::2].sum()), int(((flags[0::2] == 0) & (flags[1::2] == 1)).sum())
    rmed, rlo, rhi = median_ms(lambda: ctx.g1_recover_from_x_batch(u), k)
    print(f"  n = {n:8d}: map_to_g1 {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} inputs/s; x1 / x2 / x3 taken "
          f"{x1} / {x2} / {n - x1 - x2}), recover {rmed:9.2f} ms  (min {rlo:.2f}, max {rhi:.2f}): {med / rmed:.2f} of it", flush=True)

print("hash_to_g1 (bn254s_hash_to_g1_batch: hash_to_fq of 8 elements per input, then the map, u staying on the device), ms", flush=True)
for n in SIZES:
    inp = rng.integers(0, GL_P, size=(n, 8), dtype=np.uint64)
    med, lo, hi = median_ms(lambda: ctx.hash_to_g1_batch(inp), reps if n < (1 << 20) else 3)
    print(f"  n = {n:8d}: {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} inputs/s)", flush=True)

print("map_to_g1 (front-end + Fq-exp proofs of the 2n Legendre jobs + linkage check) vs prove_batch of the same jobs, ms", flush=True)
n, per_proof = 16384, 128
u = below_p(n)
_, _, jobs = ctx.map_to_g1_batch(u)
js, jx = np.ascontiguousarray(jobs[:, :4]), np.ascontiguousarray(jobs[:, 4:])
m_med, m_lo, _ = median_ms(lambda: ctx.map_to_g1(u, per_proof=per_proof), 2)
b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(2, js, jx, None, per_proof=per_proof), 2)
print(f"  n = {n:6d} inputs, {2 * n} jobs, per_proof {per_proof:5d}: map_to_g1 {m_med:9.1f} ms (min {m_lo:.1f}), prove_batch {b_med:9.1f} ms "
      f"(min {b_lo:.1f}): the front-end and the linkage check add {m_med - b_med:+.1f} ms; {n / m_med * 1e3:,.0f} proven images/s", flush=True)
ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
ctx.close()
