"""CPU: the k_rdx counter-set rule (csrc/xcd_ctr_plan.h) over every FMCW_XCD_MEMSET knob sequence.

process_onepass asks xcd_ctr_plan which of the context's two counter sets a launch counts in,
which one it zeroes for the next launch, and which one comes next.  tests/native/xcd_ctr_plan.cpp
models the two sets as clean / dirty and runs every knob sequence up to length 10 from every
start state: each launch must count in a set that is clean when it starts and leave it dirty.
The same program run with --parent checks the rule this one replaced (a memset launch always in
set 0, zeroing nothing, not toggling) and must report it broken: from set 0, knob 1 then 0 counts
the second launch in set 0, which the memset launch before it left dirty.  The GPU side of the same sequences is
tests/test_gpu_call_sequences.py::test_xcd_memset_knob_switched_between_launches.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "xcd_ctr_plan.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs the host C++ compiler")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xcd_ctr_plan") / "xcd_ctr_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_every_knob_sequence_counts_in_a_clean_set(binary):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok (current rule)"), r.stdout


def test_the_check_rejects_the_parent_rule(binary):
    r = subprocess.run([binary, "--parent"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "FAIL (parent rule)" in r.stdout and "counts in a dirty set" in r.stdout, r.stdout
