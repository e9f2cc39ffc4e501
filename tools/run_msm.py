"""g1_msm on ONE GPU (reference src/utils/g1_msm.rs:22-36): the device witness chain alone, and the chain plus its proofs
(bn254s_g1_msm) against bn254s_prove_batch of the same jobs.  With --g2 the same for g2_msm (bn254s_g2_msm_chain,
bn254s_g2_msm against bn254s_prove_batch kind 1).
usage: python tools/run_msm.py [--g2] [reps=5]
Inputs: 4096 distinct random points tiled (python G1 arithmetic is slow; repeated x_i change nothing for the timing; for G2 the
points (a + i d) G2 of an arithmetic progression, one affine addition each) and random 256-bit scalars.  Every figure is
synchronised (the calls return after their device work) and taken warm; the median of `reps` runs is reported, the largest
shapes fewer times."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
g2 = "--g2" in sys.argv[1:]
reps = int(args[0]) if args else 5
ctx = pk.Context(0)
if g2:
    step, cur = synth.g2_mul(0x9E3779B9, synth.G2_GEN), synth.g2_mul(0x1234567, synth.G2_GEN)
    pts = []
    for _ in range(4096):
        pts.append(cur)
        cur = synth.g2_add(cur, step)
    base_x, base_r = synth.g2_points_to_words(pts), synth.g2_points_to_words([synth.g2_mul(0xC0FFEE, synth.G2_GEN)])
else:
    _, base_x, base_r = synth.g1_inputs(4096, seed=0x6D736D)
rng = np.random.default_rng(7)
chain, msm, kind, tag = (ctx.g2_msm_chain, ctx.g2_msm, 1, "g2_msm") if g2 else (ctx.g1_msm_chain, ctx.g1_msm, 0, "g1_msm")


def jobs(n):
    s = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    x = np.tile(base_x, ((n + 4095) // 4096, 1))[:n].copy()
    return s, x, np.ascontiguousarray(base_r[0])


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


print(f"chain only (bn254s_{tag}_chain: products, scan, affine normalisation, result), ms", flush=True)
for n in (128, 1024, 16384, 1 << 20):
    s, x, R = jobs(n)
    med, lo, hi = median_ms(lambda: chain(s, x, R), reps if n < (1 << 20) else 3)
    print(f"  n = {n:8d}: {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} links/s)", flush=True)

print(f"{tag} (chain + proofs + linkage check) vs prove_batch of the same jobs, ms", flush=True)
# G2: 16 384 jobs in proofs of 128 (the 16 384-job proof, 2^23 rows in the streaming workspace, about 8 s, is left out)
for n, per_proof, k in ((1024, 128, reps), (16384, 128, 2) if g2 else (16384, 16384, 2)):
    s, x, R = jobs(n)
    offs, _ = chain(s, x, R)
    o = np.ascontiguousarray(offs[:n])
    m_med, m_lo, _ = median_ms(lambda: msm(s, x, R, per_proof=per_proof), k)
    b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(kind, s, x, o, per_proof=per_proof), k)
    print(f"  n = {n:6d}, per_proof {per_proof:5d}: {tag} {m_med:9.1f} ms (min {m_lo:.1f}), prove_batch {b_med:9.1f} ms "
          f"(min {b_lo:.1f}): the chain adds {m_med - b_med:+.1f} ms", flush=True)
ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
ctx.close()
