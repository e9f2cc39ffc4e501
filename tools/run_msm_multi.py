"""Many MSMs as one segmented chain on ONE GPU: the device front-end (bn254s_msm_multi_chain, copies included) for both curve kinds
at m x len = 128 x 128, 16 384 x 1, 1 x 16 384 and 1024 x 1024, with drawn and with supplied points, beside, in the same process:
one msm chain of the same n (bn254s_g1_msm_chain | bn254s_g2_msm_chain), bn254s_job_check_batch of the same n links, at 128 x 128
the loop over m chain calls that the one call replaces, and bn254s_msm_multi against bn254s_prove_batch of the same jobs with the
same offsets (128 x 128, per_proof 128).
usage: python tools/run_msm_multi.py [reps=5] [--out=profiles/msm_multi_times.txt]
Inputs: random 256-bit scalars; 4096 distinct points of an arithmetic progression (a + i d) G tiled, the supplied R_j from the
same progression.  Every figure is synchronised (the calls return after their device work and the copies of their results to the
host) and taken warm; the median of `reps` runs is reported (of 3 at 1024 x 1024), beside the fastest and the slowest of them.
The lines are printed as they come and written to the file at the end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or
            [__file__.rsplit("/tools/", 1)[0] + "/profiles/msm_multi_times.txt"])[0]
reps = int(args[0]) if args else 5
SHAPES = ((128, 128), (16384, 1), (1, 16384), (1024, 1024))
NAMES = {0: "G1", 1: "G2"}
SEED = (0x74696D65, 1, 2, 3)
ctx = pk.Context(0)
rng = np.random.default_rng(7)
lines = []


def progression(mul, add, gen, to_words):
    step, cur, pts = mul(0x9E3779B9, gen), mul(0x1234567, gen), []
    for _ in range(4096):
        pts.append(cur)
        cur = add(cur, step)
    return to_words(pts)


BASE = {0: progression(synth.g1_mul, synth.g1_add, synth.G1_GEN, synth.g1_points_to_words),
        1: progression(synth.g2_mul, synth.g2_add, synth.G2_GEN, synth.g2_points_to_words)}


def say(line):
    print(line, flush=True)
    lines.append(line)


def jobs(kind, m, ln):
    n = m * ln
    s = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    x = np.tile(BASE[kind], ((n + 4095) // 4096, 1))[:n].copy()
    R = np.ascontiguousarray(BASE[kind][(np.arange(m) * 7 + 13) % 4096])
    return s, x, R, [ln] * m


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


say("msm_multi_chain (products, segmented scan, per round: draw, link, inversion, job check, minimum; copies included) beside one "
    "msm chain of the same n and job_check_batch of the same links, ms")
for kind in (0, 1):
    chain = ctx.g1_msm_chain if kind == 0 else ctx.g2_msm_chain
    for m, ln in SHAPES:
        n, k = m * ln, reps if m * ln < (1 << 20) else 3
        s, x, R, seg = jobs(kind, m, ln)
        drawn = ctx.msm_multi_chain(kind, s, x, seg, seed=SEED)
        given = ctx.msm_multi_chain(kind, s, x, seg, R=R)
        assert (drawn.attempts == 0).all() and (drawn.bad_link == pk.MSM_LINK_NONE).all() and np.array_equal(drawn.results, given.results)
        bad = int((given.bad_link != pk.MSM_LINK_NONE).sum())
        d = median_ms(lambda: ctx.msm_multi_chain(kind, s, x, seg, seed=SEED), k)
        g = median_ms(lambda: ctx.msm_multi_chain(kind, s, x, seg, R=R), k)
        c = median_ms(lambda: chain(s, x, R[0]), k)
        j = median_ms(lambda: ctx.job_check_batch(kind, s, x, drawn.offsets), k)
        say(f"  {NAMES[kind]:3s} {m:5d} x {ln:5d}: drawn {d[0]:9.2f} ms  (min {d[1]:.2f}, max {d[2]:.2f}; {n / d[0] * 1e3:,.0f} links/s), "
            f"supplied {g[0]:9.2f} ms  (min {g[1]:.2f}, max {g[2]:.2f}; {bad} MSMs unprovable); one chain of n {c[0]:.2f} ms, "
            f"job_check_batch {j[0]:.2f} ms")
        if (m, ln) == (128, 128):
            def loop():
                for i in range(m):
                    chain(s[i * ln:(i + 1) * ln], x[i * ln:(i + 1) * ln], R[i])
            lp = median_ms(loop, k)
            say(f"      the loop over {m} chain calls of {ln}: {lp[0]:9.2f} ms  (min {lp[1]:.2f}, max {lp[2]:.2f}): {lp[0] / g[0]:.1f} x the one call")

say("msm_multi (front-end + proofs) vs prove_batch of the same jobs with the same offsets, 128 x 128, ms")
per_proof = 128
for kind in (0, 1):
    s, x, R, seg = jobs(kind, 128, 128)
    offs = ctx.msm_multi_chain(kind, s, x, seg, seed=SEED).offsets
    f_med, f_lo, f_hi = median_ms(lambda: ctx.msm_multi(kind, s, x, seg, seed=SEED, per_proof=per_proof), reps)
    b_med, b_lo, b_hi = median_ms(lambda: ctx.prove_batch(kind, s, x, offs, per_proof=per_proof), reps)
    say(f"  {NAMES[kind]:3s} n = {128 * 128:6d}, per_proof {per_proof:5d}: msm_multi {f_med:9.1f} ms (min {f_lo:.1f}, max {f_hi:.1f}), "
        f"prove_batch {b_med:9.1f} ms (min {b_lo:.1f}, max {b_hi:.1f}; spread {b_hi - b_lo:.1f}): the front-end adds {f_med - b_med:+.1f} ms")
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
say(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
