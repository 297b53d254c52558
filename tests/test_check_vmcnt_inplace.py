"""tools/check_vmcnt.py, second obligation: k_rdx's slot stores stay behind the wave's own group loads.

k_rdx rewrites its one hand-off slot in place: the rows a wave stores for frame j + 1 are the rows it loaded
(``buffer_load ... sc1``) of frame j, and no other wave reads them (csrc/xcd_place.h).  The Makefile refuses
to link libfmcw when a slot store (a ``buffer_store`` without a cache-policy flag) can be reached on some
control-flow path with a group load that no ``s_waitcnt vmcnt(N)`` on the way has covered: at least N
vector-memory operations issued between the load and the wait.  These CPU tests feed check_inplace
hand-written gfx950 assembly: covered, uncovered (no wait, a count too loose), a branch around the wait, a
loop whose back edge carries the loads, the loads that are not group loads, and a 16-byte slot store
with an SGPR offset; then the code the Makefile
built, when it is there.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_vmcnt as cv  # noqa: E402

HEAD = "_ZN4fmcw5k_rdxILb1ELb0ELb1EEEvNS_11OnePassArgsE:\n"
TAIL = ".Lfunc_end0:\n"


def _run(body: str) -> bool:
    fns = cv.functions(HEAD + body + TAIL, r"k_rdx")
    assert len(fns) == 1
    (name, lines), = fns.items()
    return bool(cv.check_inplace(name, lines, quiet=True))


def test_drained_loads_pass():
    assert _run("""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    buffer_load_dwordx4 v[4:7], v8, s[0:3], s5 offen sc1
    s_waitcnt vmcnt(0)
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    buffer_store_dwordx4 v[14:17], v9, s[0:3], 0 offen offset:2048
    s_endpgm
""")


def test_counted_wait_passes():
    # two vector-memory operations issued after the last group load: vmcnt(2) means it has returned
    assert _run("""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    global_load_dwordx4 v[20:23], v[24:25], off nt
    buffer_store_dwordx2 v[26:27], v28, s[4:7], 0 offen nt
    s_waitcnt vmcnt(2)
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_no_wait_fails():
    assert not _run("""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    s_waitcnt lgkmcnt(0)
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_count_one_too_loose_fails():
    # the second group load is the wave's youngest operation at the wait: vmcnt(1) may leave it in flight
    assert not _run("""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    buffer_load_dwordx4 v[4:7], v8, s[0:3], s5 offen sc1
    s_waitcnt vmcnt(1)
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_wait_before_the_load_does_not_count():
    assert not _run("""
    s_waitcnt vmcnt(0)
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


@pytest.mark.parametrize("marker", ["", "; %bb.1:\n"])
def test_branch_around_the_wait_fails(marker):
    # one path waits, the other jumps straight to the slot store
    assert not _run(f"""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    s_cbranch_scc1 .LBB0_2
{marker}    s_waitcnt vmcnt(0)
.LBB0_2:
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_wait_on_both_branches_passes():
    assert _run("""
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    s_cbranch_scc1 .LBB0_2
    s_waitcnt vmcnt(0)
    s_branch .LBB0_3
.LBB0_2:
    global_load_dword v20, v[24:25], off
    s_waitcnt vmcnt(1)
.LBB0_3:
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_loads_around_a_loop_back_edge():
    # the steady loop: loads and stores in one body; the first store is covered, and a store reached from the
    # previous iteration's loads passes that iteration's wait on the way
    body = """
.LBB0_1:
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    {wait}
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    buffer_store_dwordx2 v[26:27], v28, s[4:7], 0 offen nt
    s_cbranch_scc1 .LBB0_1
    s_endpgm
"""
    assert _run(body.format(wait="s_waitcnt vmcnt(0)"))
    assert not _run(body.format(wait="s_nop 0"))


def test_first_step_without_group_loads_passes():
    # step 0 stores a slot nobody has read: the path reaches the entry with no group load on it
    assert _run("""
    global_load_dwordx4 v[20:23], v[24:25], off nt
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    s_endpgm
""")


def test_other_loads_and_policy_stores_are_not_held():
    # chirp loads (global, nt) are not group loads; RD rows (stores with a cache policy) are not slot stores
    assert _run("""
    global_load_dwordx4 v[20:23], v[24:25], off nt
    buffer_load_dwordx4 v[0:3], v8, s[0:3], 0 offen
    buffer_store_dwordx4 v[10:13], v9, s[0:3], 0 offen
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    buffer_store_dwordx2 v[26:27], v28, s[4:7], 0 offen nt
    buffer_store_dwordx2 v[26:27], v28, s[4:7], 0 offen sc1
    s_endpgm
""")


def test_wide_slot_store_with_an_sgpr_offset_fails():
    # no wait state is padded behind such a store before its data registers are rewritten (r_end)
    body = """
    buffer_load_dwordx4 v[0:3], v8, s[0:3], s4 offen sc1
    s_waitcnt vmcnt(0)
    buffer_store_dword{width} v[10:13], v9, s[0:3], {soff} offen
    s_endpgm
"""
    assert not _run(body.format(width="x4", soff="s17"))
    assert not _run(body.format(width="x3", soff="s17"))
    assert _run(body.format(width="x4", soff="0"))
    assert _run(body.format(width="x2", soff="s17"))                            # 8 bytes: no hazard


def test_built_kernel_passes_and_reports_both_proofs():
    s = os.path.join(ROOT, "fmcw_radar_processing_amd", "csrc", "build", "kernels_xcd.s")
    if not os.path.exists(s):
        pytest.skip("libfmcw not built here (build() writes build/kernels_xcd.s)")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_vmcnt.py"), s], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "uncovered" not in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if "behind their group loads" in ln]
    assert len(lines) == 8 and all(ln.endswith("OK") for ln in lines), r.stdout      # every k_rdx instantiation
    assert all(int(ln.split(": ")[1].split()[0]) > 0 for ln in lines), r.stdout        # and it found slot stores in each
