"""The job check on ONE GPU: the device front-end alone (bn254s_job_check_batch, copies included) for both curve kinds at
n = 128, 16 384 and 2^20 beside bn254s_job_outputs_batch on the same inputs in the same process - the ladder of the outputs is
the nearest thing the library has to the 256-step walk of the check - and, for 16 384 jobs of each kind, bn254s_prove_batch_checked
against bn254s_prove_batch of the same jobs.
usage: python tools/run_job_check.py [reps=5] [--out=profiles/job_check_times.txt]
Inputs as tools/run_outputs.py: random 256-bit scalars; 4096 distinct points tiled (G1: random; G2: an arithmetic progression),
offsets the same points rolled by one; uniform x below p for Fq exp.  Every figure is synchronised (the calls return after their
device work and the copies of their results to the host) and taken warm; the median of `reps` runs is reported (of 3 at n = 2^20),
beside the fastest and the slowest of them.  The lines are printed as they come and written to the file at the end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or
            [__file__.rsplit("/tools/", 1)[0] + "/profiles/job_check_times.txt"])[0]
reps = int(args[0]) if args else 5
SIZES = (128, 16384, 1 << 20)
NAMES = {0: "G1", 1: "G2", 2: "Fq exp"}
ctx = pk.Context(0)
rng = np.random.default_rng(7)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)
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


say("job check, front-end only (bn254s_job_check_batch: on-curve tests, 256 steps of one addition and one doubling in Jacobian "
    "coordinates, no inversion; copies included) beside the job outputs (bn254s_job_outputs_batch) of the same jobs, ms")
for kind in (0, 1):
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        s, x, o = jobs(kind, n)
        prov, _ = ctx.job_check_batch(kind, s, x, o)
        assert prov.all()
        med, lo, hi = median_ms(lambda: ctx.job_check_batch(kind, s, x, o), k)
        omed, olo, ohi = median_ms(lambda: ctx.job_outputs_batch(kind, s, x, o), k)
        say(f"  {NAMES[kind]:6s} n = {n:8d}: job check {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} jobs/s), "
            f"job outputs {omed:9.2f} ms  (min {olo:.2f}, max {ohi:.2f}): {med / omed:.2f} of it")

say("prove_batch_checked (check + proofs) vs prove_batch of the same jobs, ms")
n, per_proof = 16384, 128
for kind in (0, 1, 2):
    s, x, o = jobs(kind, n)
    c_med, c_lo, c_hi = median_ms(lambda: ctx.prove_batch_checked(kind, s, x, o, per_proof=per_proof), reps)
    b_med, b_lo, b_hi = median_ms(lambda: ctx.prove_batch(kind, s, x, o, per_proof=per_proof), reps)
    say(f"  {NAMES[kind]:6s} n = {n:6d}, per_proof {per_proof:5d}: prove_batch_checked {c_med:9.1f} ms (min {c_lo:.1f}, max {c_hi:.1f}), "
        f"prove_batch {b_med:9.1f} ms (min {b_lo:.1f}, max {b_hi:.1f}; spread {b_hi - b_lo:.1f}): the check adds {c_med - b_med:+.1f} ms")
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
say(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
