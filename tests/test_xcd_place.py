"""CPU: the place map of k_rdx's one in-place hand-off slot (csrc/xcd_place.h).

tests/native/xcd_place.cpp prints xcd_place(j, r, w) for 6 team steps; the checks here model the kernel's
use of it (kernels_xcd.hip): reading frame j, wave v of member k loads row v of the places of chunks (k, m),
m = 0..31; writing frame j, wave v of member w stores row v of the places of chunks (g, w), g = 0..31.

  - the map is a bijection onto 0..1023 at every step;
  - the rows a wave stores at step j + 1 are exactly the rows it loaded at step j (so a wave overwrites only
    what it has itself read: the one slot needs no write-after-read protection between members);
  - no row is read by two waves, and every row read at step j was written at step j by exactly one wave, the
    one that holds its chirp (member m, wave v for chirp 8 m + v of chunk (k, m));
  - the places fill the 2 MiB slot at the 2 KiB pitch, 8 rows of 256 bytes each.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "xcd_place.cpp")
STEPS, NK, NW = 6, 32, 8

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs the host C++ compiler")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xcd_place") / "xcd_place")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, str(STEPS)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    P = np.full((STEPS, NK, NK), -1, np.int64)
    pitch = None
    for ln in lines:
        t = ln.split()
        if t and t[0] == "pitch":
            pitch = (int(t[1]), int(t[2]))
        elif t:
            j, rr, w, p = map(int, t)
            P[j, rr, w] = p
    assert (P >= 0).all() and pitch is not None
    return P, pitch


def loads(P, j, k, v):
    """The (place, row) pairs wave v of member k loads when it reads frame j."""
    return {(int(P[j, k, m]), v) for m in range(NK)}


def stores(P, j, w, v):
    """The (place, row) pairs wave v of member w stores when it writes frame j."""
    return {(int(P[j, g, w]), v) for g in range(NK)}


def test_bijection_at_every_step(table):
    P, pitch = table
    for j in range(STEPS):
        assert sorted(P[j].ravel().tolist()) == list(range(NK * NK)), j
    assert pitch == (2048, 256) and NK * NK * pitch[0] == 2 << 20 and NW * pitch[1] == pitch[0]


def test_even_steps_are_group_chirp_order(table):
    P, _ = table
    for j in range(0, STEPS, 2):
        for r in range(NK):
            assert P[j, r].tolist() == list(range(32 * r, 32 * r + 32))      # [group][chirp][32] at 2 KiB per 8 chirps


def test_a_wave_stores_exactly_the_rows_it_loaded(table):
    P, _ = table
    for j in range(STEPS - 1):
        for k in range(NK):
            for v in range(NW):
                assert stores(P, j + 1, k, v) == loads(P, j, k, v), (j, k, v)


def test_every_row_read_was_written_once_by_its_chirps_wave(table):
    P, _ = table
    for j in range(STEPS):
        writer = {}
        for w in range(NK):
            for v in range(NW):
                for row in stores(P, j, w, v):
                    assert row not in writer, (j, row)                       # written once
                    writer[row] = (w, v)
        assert len(writer) == NK * NK * NW                                     # the whole slot
        reader = {}
        for k in range(NK):
            for v in range(NW):
                for m in range(NK):
                    row = (int(P[j, k, m]), v)
                    assert row not in reader, (j, row)                       # read by one wave only
                    reader[row] = (k, v)
                    assert writer[row] == (m, v), (j, k, v, m)              # chirp 8 m + v: member m, wave v
        assert len(reader) == NK * NK * NW
