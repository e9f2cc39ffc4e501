"""The root statement verifiers on ONE GPU: the link check (bn254s_root_links_check_batch, copies included) for the five front-ends
at n = 128, 16 384 and 2^20 inputs beside the front-end (*_batch) of the same size, which made the inputs, in the same process; and,
for 16 384 inputs of each front-end at 128 jobs per proof (128 proofs; 256 for map_to_g1, whose jobs number 2n), the verifier
beside bn254s_verify_batch of the same proofs and jobs alone, and the Python checker of plonky2_bn254_amd.lib on the same call.
usage: python tools/run_verify_roots.py [reps=5] [--out=profiles/verify_roots_times.txt]
Inputs: uniform values below p (about half of them squares), for Fq2 two such coordinates, and a random sign.  Every figure is
synchronised (the calls return after their device work and the copies of their results to the host) and taken warm; the median of
`reps` runs is reported (of 3 at n = 2^20; the Python checker runs once), beside the fastest and the slowest of them.
What to expect, not a gate: a verifier is verify_batch plus the link check, the difference inside the run-to-run spread of
verify_batch in this run - as it was for verify_scalar_mul.  The lines are printed as they come and written to the file at the end."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import root_links_ref as rl
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or
            [__file__.rsplit("/tools/", 1)[0] + "/profiles/verify_roots_times.txt"])[0]
reps = int(args[0]) if args else 5
SIZES = (128, 16384, 1 << 20)
NAMES = ("g1_recover", "g2_recover", "fq_sqrt", "fq2_sqrt", "map_to_g1")
ctx = pk.Context(0)
rng = np.random.default_rng(7)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def inputs(what, n):
    """(xs [n, 4 | 8] uniform below p: 256-bit values with the top word reduced below p's top word, sgns [n])"""
    w = rl.IN_WORDS[what]
    x = rng.integers(0, 2**63, size=(n, w), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, w), dtype=np.uint64)
    x[:, 3::4] %= P_WORDS[3]
    return x, rng.integers(0, 2, size=n, dtype=np.uint8)


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def check(what, r, jobs=True):
    return ctx.root_links_check_batch(what, r.xs, r.out, r.flags, sgns=r.sgns, root_ok=r.root_ok, fq_jobs=r.jobs if jobs else None)


def verify(what, proofs, per, r):
    if what == rl.G1_RECOVER:
        return ctx.verify_g1_recover(proofs, per, r.xs, r.out, r.flags, r.jobs)
    if what == rl.G2_RECOVER:
        return ctx.verify_g2_recover(proofs, per, r.xs, r.sgns, r.out, r.flags, r.jobs)
    if what == rl.MAP_TO_G1:
        return ctx.verify_map_to_g1(proofs, per, r.xs, r.out, r.flags, r.jobs)
    return (ctx.verify_fq_sqrt if what == rl.FQ_SQRT else ctx.verify_fq2_sqrt)(proofs, per, r.xs, r.sgns, r.out, r.flags, r.root_ok, r.jobs)


def python_checker(what, proofs, per, r):
    if what == rl.G1_RECOVER:
        return pk.verify_g1_recover(r.xs, r.out, r.flags, r.jobs, proofs, per, ctx=ctx)
    if what == rl.G2_RECOVER:
        return pk.verify_g2_recover(r.xs, r.sgns, r.out, r.flags, r.jobs, proofs, per, ctx=ctx)
    if what == rl.MAP_TO_G1:
        return pk.verify_map_to_g1(r.xs, r.out, r.flags, r.jobs, proofs, per, ctx=ctx)
    return (pk.verify_fq_sqrt if what == rl.FQ_SQRT else pk.verify_fq2_sqrt)(r.xs, r.sgns, r.out, r.flags, r.root_ok, r.jobs, proofs, per, ctx=ctx)


say("root_links_check_batch (inputs, points / roots, flags and jobs up, one kernel, codes and bases down) beside the front-end "
    "that made them, ms")
for what in rl.WHATS:
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        xs, sgns = inputs(what, n)
        r, _ = rl.device_rows(ctx, what, xs, sgns)
        assert not check(what, r)[0].any()
        med, lo, hi = median_ms(lambda: check(what, r), k)
        f = median_ms(lambda: rl.device_rows(ctx, what, xs, sgns), k)
        say(f"  {NAMES[what]:10s} n = {n:8d}: root_links_check_batch {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} inputs/s); "
            f"{NAMES[what]}_batch {f[0]:.2f} ms: {med / f[0]:.3f} of it")

say("the verifiers for 16384 inputs at 128 jobs per proof beside verify_batch of the same proofs and jobs alone, ms")
n, per_proof = 16384, 128
for what in rl.WHATS:
    xs, sgns = inputs(what, n)
    r, proofs = rl.device_rows(ctx, what, xs, sgns, per_proof=per_proof)
    pairs = [(p.words, p.outputs) for p in proofs]
    js, jx = np.ascontiguousarray(r.jobs[:, :4]), np.ascontiguousarray(r.jobs[:, 4:])
    assert not any(ctx.verify_batch(2, pairs, js, jx, None))
    v = median_ms(lambda: verify(what, proofs, per_proof, r), reps)
    b = median_ms(lambda: ctx.verify_batch(2, pairs, js, jx, None), reps)
    c = median_ms(lambda: check(what, r), reps)
    t0 = time.perf_counter()
    python_checker(what, proofs, per_proof, r)
    py = (time.perf_counter() - t0) * 1e3
    say(f"  {NAMES[what]:10s} {len(proofs):3d} proofs: verify_{NAMES[what]} {v[0]:9.1f} ms (min {v[1]:.1f}, max {v[2]:.1f}), verify_batch {b[0]:9.1f} ms "
        f"(min {b[1]:.1f}, max {b[2]:.1f}), the link check alone {c[0]:.2f} ms: the verifier adds {v[0] - b[0]:+.1f} ms to verify_batch, whose "
        f"spread is {b[2] - b[1]:.1f} ms; the Python checker (one run, ctx.verify per proof) {py:.0f} ms")
    del proofs, pairs
_, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
say(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us")
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
