"""Checking proofs on ONE GPU: bn254s_verify_batch against the two ways there were to check many proofs, in the same process -
the loop over bn254s_verify_host (one host thread, no GPU) and the loop over bn254s_verify (host, the AIR at zeta through the
quotient kernels) - for 1, 8, 128 and 1024 proofs of one kind, beside bn254s_prove_batch of the same jobs.
usage: python tools/run_verify.py [kind=0] [reps=5] [out=profiles/verify_batch_times.txt]
Proofs: 128 distinct proofs of 128 jobs each (2^16 rows), proven once; 1024 = those eight times over.  Inputs as tools/run_outputs.py
draws them (random 256-bit scalars, 4096 distinct points tiled).  Per size the three ways alternate `reps` times in this order and
the median is reported with the fastest and the slowest; the two loops at 1024 proofs run ONCE (they take as long as all the rest
together) and say so.  Every figure is a wall time around calls that return after their device work.  The split of
bn254s_verify_batch (front and CTL: wall time of the host threads; upload, k_vb_merkle, k_vb_fri: device events) is that of
the last run."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import plonky2_bn254_amd as pk
from tools import synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kind = int(args[0]) if len(args) > 0 else 0
reps = int(args[1]) if len(args) > 1 else 5
out_path = args[2] if len(args) > 2 else __file__.rsplit("/tools/", 1)[0] + "/profiles/verify_batch_times.txt"
NAMES = {0: "G1", 1: "G2", 2: "Fq exp"}
PER_PROOF, DISTINCT, SIZES = 128, 128, (1, 8, 128, 1024)
rng = np.random.default_rng(11)
n_jobs = PER_PROOF * DISTINCT


def scalars(n):
    return rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)


s = scalars(n_jobs)
if kind == 2:
    x = scalars(n_jobs)
    x[:, 3] %= np.array(synth._to_words(synth.P), np.uint64)[3]
    o = None
else:
    _, base, _ = (synth.g1_inputs if kind == 0 else synth.g2_inputs)(4096, seed=0x6D736D)
    x = np.tile(base, (n_jobs // 4096, 1)).copy()
    o = np.tile(np.roll(base, 1, axis=0), (n_jobs // 4096, 1)).copy()

ctx = pk.Context(0)
ctx.prove_batch(kind, s[:4 * PER_PROOF], x[:4 * PER_PROOF], None if o is None else o[:4 * PER_PROOF], per_proof=PER_PROOF)  # warm
prove_ms = []
for _ in range(3):
    t0 = time.perf_counter()
    made = ctx.prove_batch(kind, s, x, o, per_proof=PER_PROOF)
    prove_ms.append((time.perf_counter() - t0) * 1e3)
degree_bits = made[0].degree_bits
proofs = [(p.words.copy(), p.outputs.copy()) for p in made]
del made
jobs_of = lambda i: slice(PER_PROOF * (i % DISTINCT), PER_PROOF * (i % DISTINCT + 1))
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


say(f"{NAMES[kind]}: {DISTINCT} distinct proofs of {PER_PROOF} jobs, 2^{degree_bits} rows, {proofs[0][0].size} words each")
say(f"bn254s_prove_batch of the {n_jobs} jobs ({DISTINCT} proofs): median {statistics.median(prove_ms):.1f} ms of 3 "
    f"({statistics.median(prove_ms) / DISTINCT:.2f} ms per proof)")
say()
say("%7s  %-24s %12s %12s %12s %14s" % ("proofs", "way", "median ms", "min ms", "max ms", "ms per proof"))
for n in SIZES:
    batch = [proofs[i % DISTINCT] for i in range(n)]
    tile = lambda a: None if a is None else np.concatenate([a[jobs_of(i)] for i in range(n)])
    bs, bx, bo = tile(s), tile(x), tile(o)

    def loop_host():
        for i, (w, outs) in enumerate(batch):
            j = jobs_of(i)
            pk.verify_host(kind, w, degree_bits, s[j], x[j], None if o is None else o[j], outs)

    def loop_ctx():
        for i, (w, outs) in enumerate(batch):
            j = jobs_of(i)
            ctx.verify(kind, w, degree_bits, s[j], x[j], None if o is None else o[j], outs)

    def batch_call():
        verdicts = ctx.verify_batch(kind, batch, bs, bx, bo, degree_bits=degree_bits)
        assert verdicts == [None] * n

    ways = (("loop bn254s_verify_host", loop_host), ("loop bn254s_verify", loop_ctx), ("bn254s_verify_batch", batch_call))
    once = n > 128
    times = {name: [] for name, _ in ways}
    batch_call()  # warm
    for r in range(reps):
        for name, fn in ways:
            if once and fn is not batch_call and r > 0:
                continue
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    split = ctx.verify_batch_ms()
    for name, _ in ways:
        t = times[name]
        med = statistics.median(t)
        note = "  (one run)" if len(t) == 1 else ""
        say("%7d  %-24s %12.2f %12.2f %12.2f %14.3f%s" % (n, name, med, min(t), max(t), med / n, note))
    b = statistics.median(times["bn254s_verify_batch"])
    say("%7s  ratio to the batch call: loop bn254s_verify_host %.1fx, loop bn254s_verify %.1fx"
        % ("", statistics.median(times["loop bn254s_verify_host"]) / b, statistics.median(times["loop bn254s_verify"]) / b))
    say("%7s  split of the last batch call, ms: " % "" + "  ".join(f"{k} {v:.2f}" for k, v in split.items())
        + f"  (sum {sum(split.values()):.2f})")
    say()
ctx.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
