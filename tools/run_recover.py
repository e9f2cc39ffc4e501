"""G1 point recovery from x on ONE GPU (reference src/curves/g1.rs:76-95): the device front-end alone
(bn254s_g1_recover_from_x_batch) and the front-end plus the Fq-exp proofs of its Legendre jobs (bn254s_g1_recover_from_x)
against bn254s_prove_batch of the same jobs; and, in the same process, bn254s_g1_msm_chain at the same sizes: the chain folds
the points that recovery produces, so it is the yardstick for the front-end.
With --g2 the G2 twin (reference src/curves/g2.rs:42-54, src/fields/fq2.rs:209-241): the front-end times of
bn254s_g2_recover_from_x_batch beside the G1 ones and beside bn254s_g2_msm_chain at the same sizes, then bn254s_g2_recover_from_x
against bn254s_prove_batch of its jobs.
With --subgroup the G2 subgroup check that sits between recovery and g2_msm: the front-end times of
bn254s_g2_subgroup_check_batch beside those of bn254s_g2_recover_from_x_batch at the same sizes, then bn254s_g2_subgroup_check
against bn254s_prove_batch (kind 1) of its jobs (r, P_i, R_i).  Its inputs are points of the twist curve made by the recovery
front-end from uniform x (non-members), every other one replaced by a member (an arithmetic progression of 1024 tiled).
With --cofactor the G2 cofactor clearing that turns a recovered point into a member: the front-end times of
bn254s_g2_clear_cofactor_batch beside those of bn254s_g2_subgroup_check_batch on the same points, bn254s_map_to_g2_batch on 4096
inputs beside bn254s_map_to_g2 (2 Fq-exp jobs and 1 G2 job proven per input) of the same inputs, then bn254s_g2_clear_cofactor
against bn254s_prove_batch (kind 1) of its jobs (h, P_i, R_i).
usage: python tools/run_recover.py [--g2 | --subgroup | --cofactor] [reps=5]
Inputs: uniform x below p (about half of them recoverable), for G2 two such coordinates and a random sign; for the chain 4096
distinct points tiled (G1: random; G2: an arithmetic progression) and random 256-bit scalars, as tools/run_msm.py.  Every figure
is synchronised (the calls return after their device work and the copies of their results to the host) and taken warm; the
median of `reps` runs is reported, the largest shape fewer times."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
g2 = "--g2" in sys.argv[1:]
subgroup = "--subgroup" in sys.argv[1:]
cofactor = "--cofactor" in sys.argv[1:]
reps = int(args[0]) if args else 5
SIZES = (128, 16384, 1 << 20)
ctx = pk.Context(0)
rng = np.random.default_rng(7)
if g2:
    step, cur = synth.g2_mul(0x9E3779B9, synth.G2_GEN), synth.g2_mul(0x1234567, synth.G2_GEN)
    pts = []
    for _ in range(4096):
        pts.append(cur)
        cur = synth.g2_add(cur, step)
    base_x, base_r = synth.g2_points_to_words(pts), synth.g2_points_to_words([synth.g2_mul(0xC0FFEE, synth.G2_GEN)])
elif not subgroup and not cofactor:
    _, base_x, base_r = synth.g1_inputs(4096, seed=0x6D736D)
P_WORDS = np.array(synth._to_words(synth.P), np.uint64)


def xs_below_p(n):
    """n x 4 words, uniform below p: 256-bit values with the top word reduced below p's top word."""
    x = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    x[:, 3] %= P_WORDS[3]
    return x


def xs2_below_p(n):
    """n x 8 words (x.c0, x.c1 uniform below p) and n sign bytes."""
    return np.concatenate([xs_below_p(n), xs_below_p(n)], axis=1), rng.integers(0, 2, size=n, dtype=np.uint8)


def chain_jobs(n):
    s = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    return s, np.tile(base_x, ((n + 4095) // 4096, 1))[:n].copy(), np.ascontiguousarray(base_r[0])


def median_ms(fn, k):
    fn()  # warm: buffers, code objects
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def member_points():
    """1024 members of the subgroup in ABI words: an arithmetic progression."""
    step, cur = synth.g2_mul(0x9E3779B9, synth.G2_GEN), synth.g2_mul(0x1234567, synth.G2_GEN)
    members = []
    for _ in range(1024):
        members.append(cur)
        cur = synth.g2_add(cur, step)
    return synth.g2_points_to_words(members)


def twist_points(n, members):
    """n points of the twist curve: recovered from uniform x (about half of them are the x of a point), members at the even
    indices."""
    xs, sgns = xs2_below_p(2 * n + 4096)
    pts, flags, _ = ctx.g2_recover_from_x_batch(xs, sgns)
    pts = np.ascontiguousarray(pts[flags == 1][:n])
    assert pts.shape[0] == n
    pts[::2] = np.tile(members, ((n + 2047) // 2048, 1))[:pts[::2].shape[0]]
    return pts


def subgroup_run():
    members = member_points()
    print("G2 subgroup check, front-end only (bn254s_g2_subgroup_check_batch: on-curve test, [x0]P, three psi, three additions) "
          "beside the G2 recover front-end (bn254s_g2_recover_from_x_batch), ms", flush=True)
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        pts = twist_points(n, members)
        med, lo, hi = median_ms(lambda: ctx.g2_subgroup_check_batch(pts), k)
        flags = ctx.g2_subgroup_check_batch(pts)
        xs, sgns = xs2_below_p(n)
        rmed, rlo, rhi = median_ms(lambda: ctx.g2_recover_from_x_batch(xs, sgns), k)
        print(f"  n = {n:8d}: subgroup check {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} points/s; "
              f"{int(flags.sum())} members), recover {rmed:9.2f} ms  (min {rlo:.2f}, max {rhi:.2f}): {med / rmed:.2f} of it", flush=True)
    print("g2_subgroup_check (front-end + G2 proofs of (r, P_i, R_i) + linkage check) vs prove_batch of the same jobs, ms", flush=True)
    n, per_proof = 16384, 128
    pts = twist_points(n, members)
    offs = np.tile(np.roll(members, 1, axis=0), (n // 1024, 1))
    r = np.tile(np.array(synth._to_words(synth.R_ORDER), np.uint64), (n, 1))
    c_med, c_lo, _ = median_ms(lambda: ctx.g2_subgroup_check(pts, offs, per_proof=per_proof), 2)
    b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(1, r, pts, offs, per_proof=per_proof), 2)
    print(f"  n = {n:6d}, per_proof {per_proof:5d}: g2_subgroup_check {c_med:9.1f} ms (min {c_lo:.1f}), prove_batch {b_med:9.1f} ms "
          f"(min {b_lo:.1f}): the front-end and the linkage check add {c_med - b_med:+.1f} ms; {n / c_med * 1e3:,.0f} proven checks/s",
          flush=True)
    ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)
    print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
    ctx.close()


def cofactor_run():
    members = member_points()
    print("G2 cofactor clearing, front-end only (bn254s_g2_clear_cofactor_batch: on-curve test, [x0]P, [6 x0]Q, three psi, three "
          "additions, two inversions) beside the G2 subgroup check (bn254s_g2_subgroup_check_batch) on the same points, ms", flush=True)
    for n in SIZES:
        k = reps if n < (1 << 20) else 3
        pts = twist_points(n, members)
        med, lo, hi = median_ms(lambda: ctx.g2_clear_cofactor_batch(pts), k)
        _, finite = ctx.g2_clear_cofactor_batch(pts)
        smed, slo, shi = median_ms(lambda: ctx.g2_subgroup_check_batch(pts), k)
        print(f"  n = {n:8d}: clear cofactor {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} points/s; "
              f"{int(finite.sum())} finite), subgroup check {smed:9.2f} ms  (min {slo:.2f}, max {shi:.2f}): {med / smed:.2f} of it", flush=True)
    print("map_to_g2_batch (candidates, three norm ladders, root, cofactor kernel; no proof) vs map_to_g2 (2 Fq-exp jobs + 1 G2 job "
          "proven per input) of the same inputs, ms", flush=True)
    n = 4096
    u = np.concatenate([xs_below_p(n), xs_below_p(n)], axis=1)
    offs = np.tile(np.roll(members, 1, axis=0), (n // 1024, 1))
    m_med, m_lo, m_hi = median_ms(lambda: ctx.map_to_g2_batch(u), reps)
    p_med, p_lo, _ = median_ms(lambda: ctx.map_to_g2(u, offs), 2)
    assert np.array_equal(ctx.map_to_g2_batch(u), ctx.map_to_g2(u, offs)[0])
    print(f"  n = {n:6d}: map_to_g2_batch {m_med:9.2f} ms (min {m_lo:.2f}, max {m_hi:.2f}; {n / m_med * 1e3:,.0f} inputs/s), map_to_g2 "
          f"{p_med:9.1f} ms (min {p_lo:.1f}): the same points {p_med / m_med:,.0f} times faster without the proofs", flush=True)
    print("g2_clear_cofactor (front-end + G2 proofs of (h, P_i, R_i) + linkage check) vs prove_batch of the same jobs, ms", flush=True)
    n, per_proof = 16384, 128
    pts = twist_points(n, members)
    offs = np.tile(np.roll(members, 1, axis=0), (n // 1024, 1))
    h = np.tile(np.array(synth._to_words(synth.G2_COFACTOR), np.uint64), (n, 1))
    c_med, c_lo, _ = median_ms(lambda: ctx.g2_clear_cofactor(pts, offs, per_proof=per_proof), 2)
    b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(1, h, pts, offs, per_proof=per_proof), 2)
    print(f"  n = {n:6d}, per_proof {per_proof:5d}: g2_clear_cofactor {c_med:9.1f} ms (min {c_lo:.1f}), prove_batch {b_med:9.1f} ms "
          f"(min {b_lo:.1f}): the front-end and the linkage check add {c_med - b_med:+.1f} ms; {n / c_med * 1e3:,.0f} proven images/s",
          flush=True)
    ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)
    print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
    ctx.close()


if subgroup:
    subgroup_run()
    sys.exit(0)
if cofactor:
    cofactor_run()
    sys.exit(0)

front = {}
print("G1 front-end only (bn254s_g1_recover_from_x_batch: g = x^3 + 3, g^((p+1)/4), flags, points, jobs), ms", flush=True)
for n in SIZES:
    xs = xs_below_p(n)
    med, lo, hi = median_ms(lambda: ctx.g1_recover_from_x_batch(xs), reps if n < (1 << 20) else 3)
    front[n] = med
    _, flags, _ = ctx.g1_recover_from_x_batch(xs)
    print(f"  n = {n:8d}: {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} inputs/s; {int(flags.sum())} recoverable)",
          flush=True)

if g2:
    front2 = {}
    print("G2 front-end only (bn254s_g2_recover_from_x_batch: g = x^3 + b', two exponentiations, one inversion), ms", flush=True)
    for n in SIZES:
        xs, sgns = xs2_below_p(n)
        med, lo, hi = median_ms(lambda: ctx.g2_recover_from_x_batch(xs, sgns), reps if n < (1 << 20) else 3)
        front2[n] = med
        _, flags, _ = ctx.g2_recover_from_x_batch(xs, sgns)
        print(f"  n = {n:8d}: {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}; {n / med * 1e3:,.0f} inputs/s; {int(flags.sum())} recoverable): "
              f"{med / front[n]:.2f} of the G1 front-end", flush=True)
    front, chain, tag = front2, ctx.g2_msm_chain, "g2"
else:
    chain, tag = ctx.g1_msm_chain, "g1"

print(f"chain only (bn254s_{tag}_msm_chain) at the same sizes, ms", flush=True)
for n in SIZES:
    s, x, R = chain_jobs(n)
    med, lo, hi = median_ms(lambda: chain(s, x, R), reps if n < (1 << 20) else 3)
    print(f"  n = {n:8d}: {med:9.2f} ms  (min {lo:.2f}, max {hi:.2f}): the {tag} recover front-end takes {front[n] / med:.2f} of it",
          flush=True)

print(f"{tag}_recover_from_x (front-end + Fq-exp proofs + linkage check) vs prove_batch of the same jobs, ms", flush=True)
n, per_proof = 16384, 128
if g2:
    xs, sgns = xs2_below_p(n)
    _, _, jobs = ctx.g2_recover_from_x_batch(xs, sgns)
    full = lambda: ctx.g2_recover_from_x(xs, sgns, per_proof=per_proof)
else:
    xs = xs_below_p(n)
    _, _, jobs = ctx.g1_recover_from_x_batch(xs)
    full = lambda: ctx.g1_recover_from_x(xs, per_proof=per_proof)
js, jx = np.ascontiguousarray(jobs[:, :4]), np.ascontiguousarray(jobs[:, 4:])
r_med, r_lo, _ = median_ms(full, 2)
b_med, b_lo, _ = median_ms(lambda: ctx.prove_batch(2, js, jx, None, per_proof=per_proof), 2)
print(f"  n = {n:6d}, per_proof {per_proof:5d}: {tag}_recover_from_x {r_med:9.1f} ms (min {r_lo:.1f}), prove_batch {b_med:9.1f} ms "
      f"(min {b_lo:.1f}): the front-end adds {r_med - b_med:+.1f} ms; {n / r_med * 1e3:,.0f} proven recoveries/s", flush=True)
ms, mhz, mhz_min = ctx.bench_ntt_clock(781 + 456, 5)  # the G1 proof's columns (W + A), as bench.py
print(f"shader clock right after, under the NTT/LDE stage: {mhz:.0f} MHz mean, {mhz_min:.0f} MHz slowest 10 us", flush=True)
ctx.close()
