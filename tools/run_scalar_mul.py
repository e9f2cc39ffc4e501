"""Scalar multiplication without an offset argument on ONE GPU: the device front-end (bn254s_scalar_mul_batch, copies included) for
both curve kinds at n = 128, 16 384 and 2^20 beside the three calls it replaces on the same jobs in the same process -
bn254s_hash_to_g1_batch / bn254s_hash_to_g2_batch of the defined inputs, bn254s_job_check_batch and bn254s_job_outputs_batch with
the drawn offsets - and, for 16 384 jobs of each kind, bn254s_scalar_mul against bn254s_prove_batch of the same jobs with the same
offsets.
usage: python tools/run_scalar_mul.py [reps=5] [--out=profiles/scalar_mul_times.txt]
Inputs as tools/run_job_check.py: random 256-bit scalars; 4096 distinct points tiled (G1: random; G2: an arithmetic progression).
Every figure is synchronised (the calls return after their device work and the copies of their results to the host) and taken
warm; the median of `reps` runs is reported (of 3 at n = 2^20), beside the fastest and the slowest of them.  The lines are printed
as they come and written to the file at the end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or
            [__file__.rsplit("/tools/", 1)[0] + "/profiles/scalar_mul_times.txt"])[0]
reps = int(args[0]) if args else 5
SIZES = (128, 16384, 1 << 20)
NAMES = {0: "G1", 1: "G2"}
SEED = (0x74696D65, 1, 2, 3)
ctx = pk.Context(0)
rng = np.random.default_rng(7)
lines = []

_, g1_pts, _ = synth.g1_inputs(4096, seed=0x6D736D)
step, cur = synth.g2_mul(0x9E3779B9, synth.G2_GEN), synth.g2_mul(0x1234567, synth.G2_GEN)
pts = []
for _ in range(4096):
    pts.append(cur)
    cur = synth.g2_add(cur, step)
BASE = {0: g1_pts, 1: synth.g2_points_to_words(pts)}


def say(line):
    print(line, flush=True)
    lines.append(line)


def jobs(kind, n):
    s = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    return s, np.tile(BASE[kind], ((n + 4095) // 4096, 1))[:n].copy()


def hash_inputs(kind, n):
    a = np.zeros((n, 8), np.uint64)
    a[:, :4] = np.array(SEED, np.uint64)
    a[:, 4] = np.arange(n, dtype=np.uint64)
    a[:, 7] = 0x62736D00 + kind
    return a


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


say("scalar_mul_batch (draw, check, ladder, subtract on the device; copies included) beside the three front-ends it replaces on the "
    "same jobs (hash_to_g1 | hash_to_g2 of the offsets' inputs, job_check_batch, job_outputs_batch), ms")
for kind in (0, 1):
    hash_fn = ctx.hash_to_g1_batch if kind == 0 else ctx.hash_to_g2_batch
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        s, x = jobs(kind, n)
        ins = hash_inputs(kind, n)
        prods, finite, offs, outs, att = ctx.scalar_mul_batch(kind, s, x, SEED)
        assert np.array_equal(offs, hash_fn(ins)) and (att == 0).all() and finite.all()
        med, lo, hi = median_ms(lambda: ctx.scalar_mul_batch(kind, s, x, SEED), k)
        h = median_ms(lambda: hash_fn(ins), k)
        c = median_ms(lambda: ctx.job_check_batch(kind, s, x, offs), k)
        o = median_ms(lambda: ctx.job_outputs_batch(kind, s, x, offs), k)
        total = h[0] + c[0] + o[0]
        say(f"  {NAMES[kind]:3s} n = {n:8d}: scalar_mul_batch {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} jobs/s); "
            f"hash {h[0]:.2f} + check {c[0]:.2f} + outputs {o[0]:.2f} = {total:.2f} ms: {med / total:.2f} of the sum")

say("scalar_mul (front-end + proofs) vs prove_batch of the same jobs with the same offsets, ms")
n, per_proof = 16384, 128
for kind in (0, 1):
    s, x = jobs(kind, n)
    offs = ctx.scalar_mul_batch(kind, s, x, SEED)[2]
    f_med, f_lo, f_hi = median_ms(lambda: ctx.scalar_mul(kind, s, x, SEED, per_proof=per_proof), reps)
    b_med, b_lo, b_hi = median_ms(lambda: ctx.prove_batch(kind, s, x, offs, per_proof=per_proof), reps)
    say(f"  {NAMES[kind]:3s} n = {n:6d}, per_proof {per_proof:5d}: scalar_mul {f_med:9.1f} ms (min {f_lo:.1f}, max {f_hi:.1f}), "
        f"prove_batch {b_med:9.1f} ms (min {b_lo:.1f}, max {b_hi:.1f}; spread {b_hi - b_lo:.1f}): the front-end adds {f_med - b_med:+.1f} ms")
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
say(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
