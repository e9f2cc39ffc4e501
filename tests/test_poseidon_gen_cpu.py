"""The generator of the hand-scheduled Poseidon statements (tools/gen_poseidon_asm.py) and the files it writes.

The generator executes its own instruction lists in a one-lane interpreter before it prints them: every leaf length 1..25, 456
and 781, with the fast code alone, with the exact repeat on every chunk and on single chunks of every class, and with the lanes
a trimmed last round skips marked undefined.  It exits non-zero if any of that fails.  Here it runs once into a temporary
directory; the committed files must be what it writes, and the bare permutation statement (the Merkle level kernels, the
streaming absorb, the proof-of-work kernel) must be the one from before the sponge's last round was trimmed."""
import hashlib
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "plonky2_bn254_amd", "csrc")
FILES = ("poseidon_asm.inc", "poseidon_init.inc", "poseidon_blocks.inc")
# SHA-256 of the text of the macro POSEIDON_ASM_PERMUTE (from its #define line to its closing "" line) before the change
PERMUTE_SHA256 = "eb597159a02ff58e5ebe2aedcff2132cc23e158997a674072564a5f9c529d220"


def macro_text(path, name):
    src = open(path).read()
    m = re.search(r'^#define %s \\\n(?:  ".*\\n" \\\n)*  ""\n' % name, src, re.M)
    assert m, name
    return m.group(0)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    out = tmp_path_factory.mktemp("poseidon_gen")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_poseidon_asm.py"), str(out)], capture_output=True, text=True)
    return out, r


def test_generator_checks_pass(generated):
    _, r = generated
    assert r.returncode == 0, r.stdout + r.stderr
    assert "interpreter ok" in r.stdout and "sponge statement ok" in r.stdout
    # the dynamic counts the counter measurements are set against are printed for both headline widths
    assert {int(n) for n in re.findall(r"sponge statement, len = (\d+), fast path: \d+ VALU instructions per lane", r.stdout)} == {781, 456}


@pytest.mark.parametrize("name", FILES)
def test_committed_files_are_the_generators(generated, name):
    out, r = generated
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(os.path.join(str(out), name), "rb").read() == open(os.path.join(CSRC, name), "rb").read()


def test_bare_permutation_statement_unchanged(generated):
    out, r = generated
    assert r.returncode == 0, r.stdout + r.stderr
    for path in (os.path.join(str(out), FILES[0]), os.path.join(CSRC, FILES[0])):
        assert hashlib.sha256(macro_text(path, "POSEIDON_ASM_PERMUTE").encode()).hexdigest() == PERMUTE_SHA256
