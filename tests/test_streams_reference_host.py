"""Host tests of tests/streams_reference.py: the storage-emulating chain is the oracle where nothing is
stored as fp16, and the cases of tests/test_gpu_streams_grid.py meet the conditions its bars rest on.
No GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import streams_reference as SR
from tests.streams_reference import C32H, C64, STORAGE

IDS = SR.case_id
# the conditions are checked on every case; the two largest only for the input dtypes the grid runs them with
GRID = [(g, dt) for g in SR.STORAGE_CASES for dt in (C64, C32H)]


def test_coverage_of_the_grid():
    nr = [g[2] for g in SR.SIZE_CASES]
    nd = [g[3] for g in SR.SIZE_CASES]
    assert set(nr) == set(SR.ALL_NR) and set(nd) == set(SR.ALL_ND)
    # each size no test ran before is run at least twice: by the size cases and by the storage or pair grid
    runs = SR.SIZE_CASES + SR.STORAGE_CASES + SR.PAIR_CASES
    assert all([g[2] for g in runs].count(n) >= 2 for n in SR.NEW_NR)
    assert all([g[3] for g in runs].count(n) >= 2 for n in SR.NEW_ND)
    assert {g[3] for g in SR.PAIR_CASES} == {2, 8, 16, 128, 1024} and 16 in {g[2] for g in SR.PAIR_CASES}
    assert any(g[0] % 2 and g[0] < g[2] for g in SR.SIZE_CASES)                  # odd S
    assert any(g[1] % 2 for g in SR.SIZE_CASES)                                   # odd pn


def test_k1_cases_take_every_profile_path():
    """At NR 16 and at NR 2048: the plain store, the equal parts, the atomicMax, and a last workgroup
    with invalid tail teams."""
    for nr in (16, 2048):
        seen = set()
        for g in SR.K1_CASES:
            if g[2] == nr:
                for cpt in SR.K1_CPT:
                    seen |= SR.k1_profile_paths(g, cpt)
        assert seen == {"store", "parts", "atomic", "tail"}, (nr, seen)
    assert {g[2] for g in SR.K1_CASES} == {16, 64, 256, 2048}


@pytest.mark.parametrize("g", SR.SIZE_CASES[:9] + SR.STORAGE_CASES[3:4], ids=IDS)
def test_all_c64_is_the_oracle_bit_for_bit(g):
    r = SR.ref(g, C64, "noise" if g in SR.SIZE_CASES[:9] else "storage")
    e = r.emu(C64, C64)
    for k in ("profile", "cube", "rd", "slow_mag", "tgt_count", "tgt_range_idx", "tgt_range_mag", "tgt_doppler_idx", "probe"):
        np.testing.assert_array_equal(e[k], r.plain[k], err_msg=k)
    np.testing.assert_array_equal(e["profile_k1"], r.plain["profile"])
    assert all(np.all(v == 0) for v in e["e_ref"].values())


def test_fp16_round_is_the_c32h_store():
    z = np.array([1.0 + 2.0j, 1000.1 - 0.3333j, 3e-6 + 70000j])
    got = SR.fp16_round(z, 1.0 / 16)
    want_re = (z.real / 16).astype(np.float16).astype(np.float64) * 16
    np.testing.assert_array_equal(got.real, want_re)
    assert got[0] == z[0] and got[1] != z[1]


@pytest.mark.parametrize("g,dt", GRID, ids=[f"{IDS(g)}-in{dt}" for g, dt in GRID])
def test_storage_cases_meet_their_conditions(g, dt):
    r = SR.ref(g, dt, "storage")
    pl = r.plain
    has = pl["tgt_count"] > 0
    assert has.any() and (~has).any()
    assert not SR.near_ties(r).any()
    assert r.emu()["cube_peak"] < 100.0                     # X / Nr far inside the fp16 range
    left_out = 0
    for st in STORAGE:
        e = r.emu(*st)
        for k, v in e["e_ref"].items():
            assert np.max(v) <= SR.E_REF_MAX, (st, k, v)
            if st == (C64, C64) or (st[0] == C64 and k != "rd"):
                assert np.all(v == 0), (st, k)              # no fp16 store upstream of this output
        # the fp16 stores change no decision of the peak rule
        np.testing.assert_array_equal(e["tgt_count"], pl["tgt_count"])
        np.testing.assert_array_equal(e["tgt_range_idx"], pl["tgt_range_idx"])
        m = r.doppler_mask(*st)
        for f in np.nonzero(has)[0]:
            peak = np.abs(pl["rd"][f, pl["tgt_range_idx"][f, 0] - 1]).max()
            assert abs(peak - r.p["doppler_thr"]) > 0.05 * r.p["doppler_thr"]
            if not m[f, 0]:
                # no exact index here: the index is held to the near-maximum set, which must be small
                near = SR.near_max_bins(pl, f, 0) | SR.near_max_bins(e, f, 0)
                assert len(near) <= 9 and max(near) - min(near) + 1 == len(near), (st, f, near)
                left_out += g[1] >= g[3]
    # where the transform is not oversampled (pn >= nd) at most 10 % of the target frames may miss the exact check
    assert left_out <= 0.10 * 4 * has.sum()


@pytest.mark.parametrize("g", SR.SIZE_CASES, ids=IDS)
def test_size_cases_meet_their_conditions(g):
    r = SR.ref(g, C64, "noise")
    has = r.plain["tgt_count"][:-1] > 0
    assert has.any() and (~has).any()
    assert not SR.near_ties(r).any()                        # the white frame included
    assert r.noise == r.F - 1 and r.F == g[4] + 1


@pytest.mark.parametrize("g", [c for c in SR.PAIR_CASES if c not in SR.SIZE_CASES] + SR.K1_CASES, ids=IDS)
def test_pair_and_k1_cases_meet_their_conditions(g):
    r = SR.ref(g, C64, "synth")
    has = r.plain["tgt_count"] > 0
    assert has.any() and (~has).any()
    assert not SR.near_ties(r).any()
    if g in SR.K1_CASES:
        for dt in (C64, C32H):
            e = SR.ref(g, dt, "synth").emu(C32H, C64)
            assert np.max(e["e_ref"]["cube"]) <= SR.E_REF_MAX
            assert e["cube_peak"] < 100.0


def test_frame_ids_hold_one_empty_frame():
    g = SR.SIZE_CASES[0]
    cfg, p, *_ = SR.build_case(g)
    ids = SR.frame_ids(g, p)
    A = [O.synth_frame_params(f, g[2], g[3], p["dist_per_bin"])["A"] for f in ids]
    assert len(ids) == g[4] and sum(a == 0 for a in A) == 1 and ids == sorted(ids)
