"""The statement verifiers on ONE GPU: the point-sum check (bn254s_point_sum_check_batch, copies included) for both curve kinds at
n = 128, 16 384 and 2^20 relations beside bn254s_scalar_mul_batch of the same size, which made them, in the same process; and, for
16 384 jobs of each kind in 128 proofs, bn254s_verify_scalar_mul and bn254s_verify_msm_multi (128 MSMs of 128) beside
bn254s_verify_batch of the same proofs alone, and the Python checker plonky2_bn254_amd.lib.verify_msm_multi on the same call.
usage: python tools/run_verify_statements.py [reps=5] [--out=profiles/verify_statements_times.txt]
Inputs as tools/run_scalar_mul.py: random 256-bit scalars; 4096 distinct points tiled (G1: random; G2: an arithmetic progression).
Every figure is synchronised (the calls return after their device work and the copies of their results to the host) and taken
warm; the median of `reps` runs is reported (of 3 at n = 2^20; the Python checker runs once), beside the fastest and the slowest of
them.  The lines are printed as they come and written to the file at the end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or
            [__file__.rsplit("/tools/", 1)[0] + "/profiles/verify_statements_times.txt"])[0]
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


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


say("point_sum_check_batch (three point arrays up, one kernel, the codes down) beside scalar_mul_batch of the same jobs, ms")
for kind in (0, 1):
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        s, x = jobs(kind, n)
        prods, finite, offs, outs, _ = ctx.scalar_mul_batch(kind, s, x, SEED)
        assert not ctx.point_sum_check_batch(kind, prods, finite, offs, outs).any()
        med, lo, hi = median_ms(lambda: ctx.point_sum_check_batch(kind, prods, finite, offs, outs), k)
        f = median_ms(lambda: ctx.scalar_mul_batch(kind, s, x, SEED), k)
        say(f"  {NAMES[kind]:3s} n = {n:8d}: point_sum_check_batch {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} relations/s); "
            f"scalar_mul_batch {f[0]:.2f} ms: {med / f[0]:.3f} of it")

say("the verifiers for 16384 jobs in 128 proofs of 128 beside verify_batch of the same proofs alone, ms")
n, per_proof, seg = 16384, 128, [128] * 128
for kind in (0, 1):
    s, x = jobs(kind, n)
    prods, finite, offs, outs, _, proofs = ctx.scalar_mul(kind, s, x, SEED, per_proof=per_proof)
    pairs = [(p.words, p.outputs) for p in proofs]
    assert not any(ctx.verify_batch(kind, pairs, s, x, offs))
    v = median_ms(lambda: ctx.verify_scalar_mul(kind, proofs, per_proof, s, x, prods, finite, offs, outs), reps)
    b = median_ms(lambda: ctx.verify_batch(kind, pairs, s, x, offs), reps)
    say(f"  {NAMES[kind]:3s} verify_scalar_mul {v[0]:9.1f} ms (min {v[1]:.1f}, max {v[2]:.1f}), verify_batch {b[0]:9.1f} ms "
        f"(min {b[1]:.1f}, max {b[2]:.1f}): the linkage adds {v[0] - b[0]:+.1f} ms")
    del proofs, pairs
    got = ctx.msm_multi(kind, s, x, seg, seed=SEED, per_proof=per_proof)
    pairs = [(p.words, p.outputs) for p in got.proofs]
    call = (got.R, got.results, got.finite, got.offsets, got.outputs)
    v = median_ms(lambda: ctx.verify_msm_multi(kind, got.proofs, per_proof, s, x, seg, *call), reps)
    b = median_ms(lambda: ctx.verify_batch(kind, pairs, s, x, got.offsets), reps)
    t0 = time.perf_counter()
    pk.verify_msm_multi(kind, s, x, seg, *call, got.proofs, per_proof, ctx=ctx)
    py = (time.perf_counter() - t0) * 1e3
    say(f"  {NAMES[kind]:3s} verify_msm_multi  {v[0]:9.1f} ms (min {v[1]:.1f}, max {v[2]:.1f}), verify_batch {b[0]:9.1f} ms "
        f"(min {b[1]:.1f}, max {b[2]:.1f}): the linkage adds {v[0] - b[0]:+.1f} ms; the Python checker (one run, ctx.verify per proof) "
        f"{py:.0f} ms")
    del got, pairs
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
say(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
