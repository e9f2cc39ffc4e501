"""The field gadgets on ONE GPU (reference src/fields/: is_square, sqrt_with_sgn, inv): the device front-ends alone
(bn254s_fq_sqrt_batch, bn254s_fq2_sqrt_batch, bn254s_fq_inv_batch, bn254s_fq2_inv_batch) beside the G1 / G2 recover front-ends of the
same run at the same sizes, then the proven calls (bn254s_fq_sqrt, bn254s_fq2_sqrt) on 16 384 inputs beside bn254s_prove_batch of
the same jobs.
usage: python tools/run_field_gadgets.py [reps=5]
Inputs: uniform values below p (about half of them squares), for Fq2 two such coordinates, and a random sign.  Every figure is
synchronised (the calls return after their device work and the copies of their results to the host) and taken warm; the median of
`reps` runs is reported, the largest shape fewer times.
What to expect, not a gate: bn254s_fq_sqrt_batch is one ladder, about the G1 recover front-end (which adds x^3 + 3 and copies twice
the words back); bn254s_fq2_sqrt_batch is two ladders and an inversion, about the G2 recover front-end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SIZES = (128, 16384, 1 << 20)
ctx = pk.Context(0)
rng = np.random.default_rng(7)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)


def xs_below_p(n):
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


print("front-ends only, ms (expectation, not a gate: fq_sqrt about g1_recover, fq2_sqrt about g2_recover)", flush=True)
for n in SIZES:
    k = reps if n < (1 << 20) else 3
    x1, x2 = xs_below_p(n), np.concatenate([xs_below_p(n), xs_below_p(n)], axis=1)
    sgns = rng.integers(0, 2, size=n, dtype=np.uint8)
    rows = [("fq_sqrt_batch", lambda: ctx.fq_sqrt_batch(x1, sgns)), ("g1_recover_from_x_batch", lambda: ctx.g1_recover_from_x_batch(x1)),
            ("fq2_sqrt_batch", lambda: ctx.fq2_sqrt_batch(x2, sgns)), ("g2_recover_from_x_batch", lambda: ctx.g2_recover_from_x_batch(x2, sgns)),
            ("fq_inv_batch", lambda: ctx.fq_inv_batch(x1)), ("fq2_inv_batch", lambda: ctx.fq2_inv_batch(x2))]
    med = {}
    for name, fn in rows:
        med[name], lo, hi = median_ms(fn, k)
        print(f"  n = {n:8d}: {name:24s} {med[name]:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med[name] * 1e3:,.0f} elements/s)", flush=True)
    print(f"  n = {n:8d}: fq_sqrt is {med['fq_sqrt_batch'] / med['g1_recover_from_x_batch']:.2f} of g1_recover, fq2_sqrt "
          f"{med['fq2_sqrt_batch'] / med['g2_recover_from_x_batch']:.2f} of g2_recover; {int(ctx.fq_sqrt_batch(x1, sgns)[1].sum())} Fq and "
          f"{int(ctx.fq2_sqrt_batch(x2, sgns)[1].sum())} Fq2 squares", flush=True)

print("proven calls (front-end + Fq-exp proofs + linkage check) vs prove_batch of the same jobs, ms", flush=True)
n, per_proof = 16384, 128
for tag, xs, batch, full in (("fq_sqrt", xs_below_p(n), ctx.fq_sqrt_batch, ctx.fq_sqrt),
                             ("fq2_sqrt", np.concatenate([xs_below_p(n), xs_below_p(n)], axis=1), ctx.fq2_sqrt_batch, ctx.fq2_sqrt)):
    sgns = rng.integers(0, 2, size=n, dtype=np.uint8)
    jobs = batch(xs, sgns)[3]
    js, jx = np.ascontiguousarray(jobs[:, :4]), np.ascontiguousarray(jobs[:, 4:])
    r_med, r_lo, _ = median_ms(lambda: full(xs, sgns, per_proof=per_proof), 2)
    b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(2, js, jx, None, per_proof=per_proof), 2)
    print(f"  n = {n:6d}, per_proof {per_proof:5d}: {tag:8s} {r_med:9.1f} ms (min {r_lo:.1f}), prove_batch {b_med:9.1f} ms (min {b_lo:.1f}): "
          f"the front-end and the linkage check add {r_med - b_med:+.1f} ms; {n / r_med * 1e3:,.0f} proven roots/s", flush=True)
ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
ctx.close()
