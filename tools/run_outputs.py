"""Proof-free job outputs on ONE GPU (reference src/generators/{g1,g2,fq}/single.rs:48-52): the device front-end alone
(bn254s_job_outputs_batch, copies included) for each kind at n = 128, 16 384 and 2^20, beside bn254s_g1_msm_chain /
bn254s_g2_msm_chain on the same scalars and points in the same process - the chain was the one way to get the products s_i x_i
on the device without a proof - and, for 16 384 jobs, the front-end plus the proofs (bn254s_job_outputs) against
bn254s_prove_batch of the same jobs.
usage: python tools/run_outputs.py [reps=5]
Inputs: random 256-bit scalars; 4096 distinct points tiled (G1: random; G2: an arithmetic progression, as tools/run_msm.py),
offsets the same points rolled by one; uniform x below p for Fq exp.  Every figure is synchronised (the calls return after their
device work and the copies of their results to the host) and taken warm; the median of `reps` runs is reported (of 3 at n = 2^20),
beside the fastest and the slowest of them."""
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
NAMES = {0: "G1", 1: "G2", 2: "Fq exp"}
ctx = pk.Context(0)
rng = np.random.default_rng(7)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)

_, g1_pts, _ = synth.g1_inputs(4096, seed=0x6D736D)
step, cur = synth.g2_mul(0x9E3779B9, synth.G2_GEN), synth.g2_mul(0x1234567, synth.G2_GEN)
pts = []
for _ in range(4096):
    pts.append(cur)
    cur = synth.g2_add(cur, step)
BASE = {0: g1_pts, 1: synth.g2_points_to_words(pts)}


def scalars(n):
    return rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)


def jobs(kind, n):
    s = scalars(n)
    if kind == 2:
        x = scalars(n)
        x[:, 3] %= P_WORDS[3]  # uniform below p
        return s, x, None
    x = np.tile(BASE[kind], ((n + 4095) // 4096, 1))[:n].copy()
    return s, x, np.tile(np.roll(BASE[kind], 1, axis=0), ((n + 4095) // 4096, 1))[:n].copy()


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


print("job outputs, front-end only (bn254s_job_outputs_batch: on-curve tests, window ladder over the job's own scalar, + offset, one "
      "inversion; copies included) beside the msm chain (bn254s_g1_msm_chain / bn254s_g2_msm_chain) of the same scalars and points, ms",
      flush=True)
for kind in (0, 1, 2):
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        s, x, o = jobs(kind, n)
        med, lo, hi = median_ms(lambda: ctx.job_outputs_batch(kind, s, x, o), k)
        line = f"  {NAMES[kind]:6s} n = {n:8d}: job outputs {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} jobs/s)"
        if kind != 2:
            chain = ctx.g1_msm_chain if kind == 0 else ctx.g2_msm_chain
            R0 = np.ascontiguousarray(o[0])
            cmed, clo, chi = median_ms(lambda: chain(s, x, R0), k)
            line += f", msm chain {cmed:9.2f} ms  (min {clo:.2f}, max {chi:.2f}): {med / cmed:.2f} of it"
        print(line, flush=True)

print("job_outputs (front-end + proofs + linkage check) vs prove_batch of the same jobs, ms", flush=True)
n, per_proof = 16384, 128
for kind in (0, 1, 2):
    s, x, o = jobs(kind, n)
    f_med, f_lo, f_hi = median_ms(lambda: ctx.job_outputs(kind, s, x, o, per_proof=per_proof), reps)
    b_med, b_lo, b_hi = median_ms(lambda: ctx.prove_batch(kind, s, x, o, per_proof=per_proof), reps)
    print(f"  {NAMES[kind]:6s} n = {n:6d}, per_proof {per_proof:5d}: job_outputs {f_med:9.1f} ms (min {f_lo:.1f}, max {f_hi:.1f}), prove_batch "
          f"{b_med:9.1f} ms (min {b_lo:.1f}, max {b_hi:.1f}; spread {b_hi - b_lo:.1f}): the front-end and the linkage check add "
          f"{f_med - b_med:+.1f} ms", flush=True)
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
ctx.close()
