"""The rare reduction paths of the Poseidon kernels, forced by crafted inputs (tests/golden/poseidon_adversarial.json, written and
verified in the interpreter by tools/gen_poseidon_adversarial.py).

The fast code of the hand-scheduled statements is wrong for some digit patterns; a sticky product flag (about 2^-33 per product,
derived, not measured: no random test reaches it) and the fold check (about one wave-permutation in 100) make the whole wave
repeat the permutation with the exact code.  Each fixture case raises the product flag at one known instruction; here it sits in
one lane of a wave of companions for which the interpreter reports no repeat, so that on the hardware 63 correct lanes repeat
because of one, with the carry pairs as 64-lane masks, and in the sponge statement from the operands parked in LDS with the next
chunk's staged loads in flight.  The same states drive the `lo < hi_hi` borrow of gl_mul_lazy in the compiler's and the
cooperative permutation; the "lazy" cases aim at its `r < t1` wrap and at the `sum < x` branch of the lazy MDS fold.

Every comparison is exact and against the CPU oracle (orc_poseidon_permute, orc_hash_or_noop); expected values are computed once
per input and shared by the kernels that take it."""
import json
import os

import numpy as np
import pytest

from tests import oracle_lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "poseidon_adversarial.json")))
VARIANTS = [0, 1, 2]      # the hand-scheduled statement, poseidon_permute_plain, poseidon_permute_coop
TRIGGER_LANES = (0, 31, 63)
CRAFTED_AT = (0, 63, 64, 255, 256, 300, 511)
N_LEAVES = 512            # two workgroups of k_leaf_hash: the second block's LDS slots and digest offsets
LENS = (8, 9, 16, 17, 21, 24)
LEAF_KERNELS = [(1, 0), (2, 0), (3, 8), (3, 16)]      # (kernel, chunk_cols): k_leaf_hash, k_leaf_hash_coop, k_leaf_absorb


def words(hexes):
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64)


QUIET = np.stack([words(s) for s in FIX["quiet_states"]])
QUIET_LEAVES = np.stack([words(s) for s in FIX["quiet_leaves"]])
PERMUTE_CASES = [words(c["state"]) for c in FIX["permute_cases"]]
LAZY_CASES = [words(c["state"]) for c in FIX["lazy_cases"]]
_expected = {}


def companions(n, shift=0):
    return QUIET[(np.arange(n) + shift) % len(QUIET)].copy()


def one_per_wave(cases):
    """Every case as one lane (0, 31, 63 in turn) of its own 64-state wave of quiet companions."""
    st = companions(64 * len(cases))
    for k, c in enumerate(cases):
        st[64 * k + TRIGGER_LANES[k % 3]] = c
    return st


def state_sets():
    two = companions(64, 5)
    sites = [c["site"] for c in FIX["permute_cases"]]
    other = next(k for k, s in enumerate(sites) if s != sites[0] and FIX["permute_cases"][k]["round"] >= 4)
    two[7], two[50] = PERMUTE_CASES[0], PERMUTE_CASES[other]       # a full-round site and a partial-round site in one wave
    partial = companions(64 * 2 + 5, 9)
    partial[-1] = PERMUTE_CASES[3]                                 # the last active lane of a partial wave
    return {
        "one_per_wave": one_per_wave(PERMUTE_CASES),
        "all_64_lanes": np.stack([PERMUTE_CASES[(7 * k) % len(PERMUTE_CASES)] for k in range(64)]),
        "two_sites_in_one_wave": two,
        "partial_wave": partial,
        "single_state": PERMUTE_CASES[1][None, :].copy(),
        "lazy_branches": one_per_wave(LAZY_CASES),
    }


STATE_SETS = state_sets()


def expected_states(oracle, name, states):
    if name not in _expected:
        exp = states.copy()
        for row in exp:
            oracle.orc_poseidon_permute(oracle_lib.ptr(row))
        exp.setflags(write=False)
        _expected[name] = exp
    return _expected[name]


def expected_digests(oracle, name, data):
    if name not in _expected:
        leaves = np.ascontiguousarray(data.T)
        dig = np.zeros((leaves.shape[0], 4), np.uint64)
        for j in range(leaves.shape[0]):
            oracle.orc_hash_or_noop(oracle_lib.ptr(leaves[j]), leaves.shape[1], oracle_lib.ptr(dig[j]))
        dig.setflags(write=False)
        _expected[name] = dig
    return _expected[name]


def assert_rows_equal(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d wrong, first at %s" % (what, bad.size, exp.shape[0], bad[:8].tolist())


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(STATE_SETS))
def test_crafted_states(gpu_ctx, oracle, name, variant):
    states = STATE_SETS[name]
    got = gpu_ctx.selftest_poseidon(variant, states)
    assert_rows_equal(got, expected_states(oracle, name, states), "%s, variant %d" % (name, variant))


def test_variant_0_is_the_kernel_of_poseidon_permute(gpu_ctx):
    states = STATE_SETS["two_sites_in_one_wave"]
    assert np.array_equal(gpu_ctx.selftest_poseidon(0, states), gpu_ctx.poseidon_permute(states))


@pytest.mark.parametrize("variant", VARIANTS)
def test_fold_check_repeat_from_a_fixed_seed(gpu_ctx, oracle, variant):
    """4096 random states: the fold check's repeat, which every proof takes thousands of times.  The interpreter must predict it for
    the recorded state of this seed; if the seed stopped producing a repeat the test would fail instead of testing nothing."""
    from tools import gen_poseidon_adversarial as adv
    stat = FIX["stat"]
    states = adv.stat_states(stat["seed"], stat["n"])
    assert len(states) == 4096
    assert adv.fold_repeat(states[stat["fold_repeat_at"]]), "the interpreter predicts no fold-check repeat for this seed any more"
    st = np.array(states, dtype=np.uint64)
    assert_rows_equal(gpu_ctx.selftest_poseidon(variant, st), expected_states(oracle, "stat", st), "variant %d" % variant)


def leaf_batches(length):
    """Per batch: column-major data [length][512] with a crafted leaf at each of the seven indices of CRAFTED_AT (every other leaf
    is a quiet one), and which case of the length sits at which index.  The cases are taken in turn until each has been placed
    and the last batch is full, so every batch has crafted leaves in both workgroups."""
    cases = [words(c["leaf"]) for c in FIX["sponge_cases"] if c["len"] == length]
    assert cases
    out = []
    for b in range(-(-len(cases) // len(CRAFTED_AT))):
        leaves = QUIET_LEAVES[(np.arange(N_LEAVES) + b) % len(QUIET_LEAVES), :length].copy()
        placed = {at: (len(CRAFTED_AT) * b + k) % len(cases) for k, at in enumerate(CRAFTED_AT)}
        for at, k in placed.items():
            leaves[at] = cases[k]
        out.append((np.ascontiguousarray(leaves.T), placed))
    return out, cases


@pytest.mark.parametrize("kernel,chunk_cols", LEAF_KERNELS)
@pytest.mark.parametrize("length", LENS)
def test_crafted_leaves(gpu_ctx, oracle, length, kernel, chunk_cols):
    batches, cases = leaf_batches(length)
    run = set()
    for b, (data, placed) in enumerate(batches):
        assert sorted(placed) == [0, 63, 64, 255, 256, 300, 511]      # all seven indices of every batch hold a crafted leaf
        for at, k in placed.items():
            assert np.array_equal(data[:, at], cases[k])
        run.update(placed.values())
        exp = expected_digests(oracle, "leaves %d %d" % (length, b), data)
        got = gpu_ctx.selftest_leaf_hash(data, kernel, chunk_cols)
        assert_rows_equal(got, exp, "length %d, batch %d, kernel %d, chunk_cols %d" % (length, b, kernel, chunk_cols))
    assert run == set(range(len(cases)))      # and every case of this length was run


def test_sixteen_leaves_through_the_latency_mode_choice(gpu_ctx, oracle):
    leaves = QUIET_LEAVES[:16, :17].copy()
    cases = [words(c["leaf"]) for c in FIX["sponge_cases"] if c["len"] == 17]
    for at, leaf in zip((0, 5, 15), cases[::4]):
        leaves[at] = leaf
    data = np.ascontiguousarray(leaves.T)
    assert_rows_equal(gpu_ctx.selftest_leaf_hash(data, 0), expected_digests(oracle, "sixteen", data), "kernel 0")


def test_shapes_the_prover_never_launches_are_refused(gpu_ctx):
    small = np.zeros((8, 16), np.uint64)
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_leaf_hash(small, 1)                           # k_leaf_hash: whole workgroups of 256 leaves
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_leaf_hash(np.zeros((4, 512), np.uint64), 1)   # leaves of <= 4 elements are not hashed
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_leaf_hash(np.zeros((4, 512), np.uint64), 2)
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_leaf_hash(np.zeros((24, 512), np.uint64), 3, 12)   # a streamed chunk is a multiple of the rate
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_leaf_hash(np.zeros((24, 512), np.uint64), 4)
    with pytest.raises(RuntimeError):
        gpu_ctx.selftest_poseidon(3, QUIET[:1])
