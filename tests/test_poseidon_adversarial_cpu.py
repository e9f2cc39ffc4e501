"""The crafted Poseidon inputs (tools/gen_poseidon_adversarial.py -> tests/golden/poseidon_adversarial.json), without a GPU.

The generator verifies every case in the one-lane interpreter of tools/gen_poseidon_asm.py before it writes it: the statement gives
the textbook result, with exactly one repeat raised at the intended product, and the fast code alone is wrong.  Here it runs once
into a temporary directory and the committed fixture must be what it writes; the flag sites the fixture reaches are set against an
enumeration made here from the instruction lists; a sample of the cases is executed again; and the crafted inputs go through the
host's permutation (sparse partial rounds, PoseidonDot, gl_reduce128) by way of bn254s_hash_to_fq2."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tools import gen_poseidon_adversarial as adv
from tools import map_to_g2_ref as m2g
from tools import synth
from tools.derive_poseidon_constants import KATS, P, permute

gen = adv.G      # tools/gen_poseidon_asm.py as the generator of the cases sees it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "poseidon_adversarial.json")
FIX = json.load(open(FIXTURE))


def ints(hexes):
    return [int(h, 16) for h in hexes]


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    out = tmp_path_factory.mktemp("poseidon_adv") / "poseidon_adversarial.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_poseidon_adversarial.py"), str(out)], capture_output=True, text=True)
    return out, r


def test_committed_fixture_is_the_generators(generated):
    out, r = generated
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == open(FIXTURE, "rb").read()
    assert os.path.getsize(FIXTURE) < 1 << 20
    m = re.search(r"flag sites covered \(products 1 and 2\): (\d+) of the bare statement, (\d+) of the sponge", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (44, 24), r.stdout


def product_sites(ins):
    """Enumerated here, not taken from the generator: the fast code ORs the borrow of a product into the sticky flag from the
    stream's first carry pair; a stream runs its S-boxes one after the other, four products each, so the n-th such instruction
    that names a carry pair is product n mod 4 + 1.  -> {product: set of instruction indices}, the full-round body's apart."""
    out = {p: set() for p in (1, 2, 3, 4)}
    full = {p: set() for p in (1, 2, 3, 4)}
    seen, in_full = {}, False
    for k, t in enumerate(ins):
        if t[0] == "flagcheck":
            break
        if t[0] == "label" and t[1] == "full":
            in_full = True
        if t[0] == "loop" and t[2] == "full":
            in_full = False
        if t[0] == "s_or" and t[1] == gen.sp(gen.S_FLAG):
            pair = t[3]
            product = seen.get(pair, 0) % 4 + 1
            seen[pair] = seen.get(pair, 0) + 1
            out[product].add(k)
            if in_full:
                full[product].add(k)
    assert all(n % 4 == 0 for n in seen.values()) and len(seen) == gen.N_STREAMS
    return out, full


def test_fixture_reaches_every_product_1_and_2_flag_site(capsys):
    every, _ = product_sites(adv.PERM)
    want = every[1] | every[2]
    # 12 S-boxes in the full-round body, 3 x 3 in the static copies of the merged block, 1 in the single partial round
    assert len(every[1]) == len(every[2]) == 12 + 9 + 1
    got = {c["site"] for c in FIX["permute_cases"]}
    assert got == want
    for p in (1, 2):
        assert {c["site"] for c in FIX["permute_cases"] if c["product"] == p} == every[p]
    # each of them also by a case in which the fold check's min / max stayed in range: the product flag alone made the wave repeat
    assert {c["site"] for c in FIX["permute_cases"] if c["isolated"]} == want
    # bodies that run as loops: first and last iteration
    rounds = {c["round"] for c in FIX["permute_cases"]}
    assert {0, 3, 26, 29, 25} <= rounds and set(range(4, 25)) <= rounds
    # the sponge statement: rounds 0 and 1 of a chunk's permutation are all that can be steered, i.e. the full-round body
    _, full = product_sites(adv.SPONGE)
    assert {c["site"] for c in FIX["sponge_cases"]} == full[1] | full[2] and len(full[1] | full[2]) == 24
    classes = set()
    for c in FIX["sponge_cases"]:
        classes |= adv.chunk_classes(c["len"], c["chunk"])
    assert classes == {"only", "first", "middle", "before_ragged", "ragged", "last"}
    with capsys.disabled():
        print("\nproduct-1/2 flag sites covered: %d of %d (bare statement), %d of %d (sponge statement, full-round body)" %
              (len(got), len(want), len(full[1] | full[2]), 24))


def test_cases_not_isolated_are_the_ones_that_cannot_be():
    """Product 1 needs x = 0 mod 2^32; where x comes out of a fast fold that makes the fold check fire too (the generator, FOLD_FED)."""
    for c in FIX["permute_cases"] + FIX["sponge_cases"]:
        assert c["isolated"] == (not (c["product"] == 1 and c["round"] in adv.FOLD_FED)), c
        x = int(c["x"], 16)
        if c["product"] == 1:
            assert x % (1 << 48) == 0 and x >> 48
        else:
            assert (x * x % P) % (1 << 48) == 0 and x * x % P >= 1 << 48


def test_round_inverses_against_the_known_answers():
    for inp, want in KATS:
        s, trail = list(inp), []
        for r in range(30):
            trail.append(s)
            s = adv.round_fwd(s, r)
        assert " ".join("%016x" % x for x in s) == want and s == permute(inp, adv.RC)
        for r in range(29, -1, -1):
            s = adv.round_inv(s, r)
            assert s == trail[r], r
        assert s == list(inp)
        for r in (0, 1, 3, 4, 14, 25, 26, 29):          # full and partial
            assert adv.state_of(r, adv.sbox_inputs(inp, r)) == list(inp)
            lane = 0 if not adv.is_full(r) else (5 * r) % 12
            st = adv.state_for(r, lane, 0x123456789ABCDEF, inp)
            vec, ref = adv.sbox_inputs(st, r), adv.sbox_inputs(inp, r)
            assert vec[lane] == 0x123456789ABCDEF and vec[:lane] + vec[lane + 1:] == ref[:lane] + ref[lane + 1:]
    assert [sum(adv.M[i][k] * adv.MINV[k][j] for k in range(12)) % P for i in range(12) for j in range(12)] == \
        [int(i == j) for i in range(12) for j in range(12)]


@pytest.mark.parametrize("k", range(0, 140, 9))
def test_permute_case_in_the_interpreter(k):
    c = FIX["permute_cases"][k]
    state = ints(c["state"])
    assert adv.sbox_inputs(state, c["round"])[c["lane"]] == int(c["x"], 16)
    assert adv.permute_case_ok(state, c["site"], c["isolated"])          # right, one repeat at the site, fast code alone wrong
    assert adv.flag_sites(adv.PERM)[c["site"]] == adv.site_name(c["round"], c["lane"], c["product"])


@pytest.mark.parametrize("k", range(0, 56, 5))
def test_sponge_case_in_the_interpreter(k):
    c = FIX["sponge_cases"][k]
    assert len(c["leaf"]) == c["len"]
    assert adv.sponge_case_ok(ints(c["leaf"]), c["chunk"], c["site"], c["isolated"])


def test_companions_are_quiet():
    assert len(FIX["quiet_states"]) == len(FIX["quiet_leaves"]) == adv.POOL
    for s in FIX["quiet_states"][::8]:
        assert adv.quiet_state(ints(s))
    assert adv.quiet_leaf(ints(FIX["quiet_leaves"][3]))


def test_lazy_cases_take_their_branches():
    kinds = set()
    for c in FIX["lazy_cases"]:
        state, x = ints(c["state"]), int(c["x"], 16)
        vec = adv.sbox_inputs(state, c["round"])
        assert vec[c["lane"]] == x
        kinds.add(c["kind"])
        if c["kind"] == "fold_wrap":
            assert c["lane"] in adv.mds_fold_wraps([pow(v, 7, P) for v in vec])
        else:
            r, borrow, wrap = adv.mul_lazy(x, x)
            assert r % P == x * x % P
            assert (borrow, wrap) == {"wrap_max_t1": (False, True), "borrow_and_wrap": (True, True), "wrap_to_small": (True, True),
                                      "no_wrap_at_top": (False, False)}[c["kind"]]
    assert kinds == {"fold_wrap", "wrap_max_t1", "borrow_and_wrap", "wrap_to_small", "no_wrap_at_top"}
    # the product-flag cases are borrow cases of gl_mul_lazy as well
    for c in FIX["permute_cases"][::10]:
        if c["product"] == 1:
            assert adv.mul_lazy(int(c["x"], 16), int(c["x"], 16))[1]


def test_fixed_seed_holds_a_fold_check_repeat():
    stat = FIX["stat"]
    assert (stat["seed"], stat["n"], stat["fold_repeat_at"]) == (adv.STAT_SEED, adv.STAT_N, adv.STAT_INDEX) and stat["n"] == 4096
    assert adv.fold_repeat(adv.stat_states(stat["seed"], stat["n"])[stat["fold_repeat_at"]])


def test_host_permutation_on_crafted_inputs():
    """poseidon_permute_host through bn254s_hash_to_fq2 (host only): its first permutation input is input[0:8] and zeros, like the
    sponge statement's first chunk, so the crafted leaves put their S-box inputs into rounds 0 and 1 of the host code too."""
    from plonky2_bn254_amd import lib as L
    lib = L.load_library()
    inputs = [ints(c["leaf"]) for c in FIX["sponge_cases"]] + [ints(s) for s in FIX["quiet_leaves"][:4]]
    inputs += [ints(c["state"])[:8] for c in FIX["permute_cases"][::12]]
    n_first = 0
    for inp in inputs:
        a = np.array(inp, dtype=np.uint64)
        out = np.zeros(8, np.uint64)
        assert lib.bn254s_hash_to_fq2(L._ptr(a), a.size, L._ptr(out)) == 0
        assert (synth.words_to_int(out[:4]), synth.words_to_int(out[4:])) == m2g.hash_to_fq2(inp)
    for c in FIX["sponge_cases"]:
        if c["chunk"] == 0:
            st = ints(c["leaf"])[:8] + [0] * 4
            assert adv.sbox_inputs(st, c["round"])[c["lane"]] == int(c["x"], 16)
            n_first += 1
    assert n_first >= 20
