"""CPU: the host-side half of the signature stage (include/fmcw.h, fmcw_sig_params) -- the argument
rules of fmcw_sig_check and SigConfig -- and a self-check that pins the float64 reference the GPU
tests compare against (tests/sig_reference.py)."""
import ctypes as ct

import numpy as np
import pytest

from fmcw_radar_processing_amd import _lib
from fmcw_radar_processing_amd import params as P
from tests import sig_reference as R


def _q(**over):
    d = dict(r_lo=0, r_hi=0, track_half=0, dc_half=-1, flags=0, floor_db=-80.0)
    d.update(over)
    return _lib.SigParams(*[d[k] for k, _ in _lib.SigParams._fields_])


# every violation fmcw_sig_check must name (shared with tests/test_gpu_sig.py): (params, nr, nd)
REJECTED = {
    "gate_reversed": (dict(r_lo=9, r_hi=8), 256, 16),
    "gate_below_1": (dict(r_lo=0, r_hi=8), 256, 16),
    "gate_above_nr": (dict(r_lo=3, r_hi=257), 256, 16),
    "track_half_negative": (dict(track_half=-1), 256, 16),
    "track_half_65": (dict(track_half=65), 256, 16),
    "dc_band_is_the_whole_axis": (dict(dc_half=8), 256, 16),        # 2 * 8 + 1 = 17 >= 16
    "dc_band_leaves_nothing_at_nd_4": (dict(dc_half=2), 256, 4),    # 5 >= 4
    "dc_half_below_minus_1": (dict(dc_half=-2), 256, 16),
    "floor_db_zero": (dict(floor_db=0.0), 256, 16),
    "floor_db_positive": (dict(floor_db=3.0), 256, 16),
    "floor_db_inf": (dict(floor_db=float("-inf")), 256, 16),
    "floor_db_nan": (dict(floor_db=float("nan")), 256, 16),
    "unknown_flag": (dict(flags=2), 256, 16),
    "nr_not_a_power_of_two": (dict(), 100, 16),
    "nr_too_small": (dict(), 8, 16),
    "nr_too_large": (dict(), 4096, 16),
    "nd_not_a_power_of_two": (dict(), 256, 24),
    "nd_too_small": (dict(), 256, 2),
    "nd_too_large": (dict(), 256, 2048),
}
# the same violations as SigConfig fields (flags has no SigConfig counterpart: db is a bool)
_FIELDS = {"r_lo", "r_hi", "track_half", "dc_half", "floor_db"}


def test_check_and_config_accept_the_defaults():
    lib = _lib.load()
    for nr, nd in ((16, 4), (256, 16), (1024, 256), (2048, 1024)):
        q = P.SigConfig().abi()
        assert lib.fmcw_sig_check(ct.byref(q), nr, nd) == _lib.FMCW_OK
        P.SigConfig().validate(nr, nd)
    q = _q(r_lo=1, r_hi=256, track_half=64, dc_half=7, flags=_lib.FMCW_SIG_DB, floor_db=-0.5)
    assert lib.fmcw_sig_check(ct.byref(q), 256, 16) == _lib.FMCW_OK            # 2 * 7 + 1 = 15 < 16
    P.SigConfig(1, 256, 64, 7, True, -0.5).validate(256, 16)
    assert lib.fmcw_sig_check(None, 256, 16) == _lib.FMCW_E_ARG
    a = P.SigConfig(3, 9, 2, 1, True, -40.0).abi()
    assert (a.r_lo, a.r_hi, a.track_half, a.dc_half, a.flags, a.floor_db) == (3, 9, 2, 1, _lib.FMCW_SIG_DB, -40.0)


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_check_rejects(name):
    lib = _lib.load()
    over, nr, nd = REJECTED[name]
    q = _q(**over)
    assert lib.fmcw_sig_check(ct.byref(q), nr, nd) == _lib.FMCW_E_ARG
    assert lib.fmcw_last_error().startswith(b"sig:") and len(lib.fmcw_last_error()) > 8
    if set(over) <= _FIELDS:
        with pytest.raises(ValueError, match="sig:"):
            P.SigConfig(**over).validate(nr, nd)


def test_null_context_is_an_argument_error():
    lib = _lib.load()
    q = _q()
    assert lib.fmcw_sig(None, ct.byref(q), None, 0, 1, 256, 16, None, 1, *([None] * 4)) == _lib.FMCW_E_ARG
    assert lib.fmcw_sig_device(None, ct.byref(q), None, 0, 1, 256, 16, None, 1, *([None] * 5)) == _lib.FMCW_E_ARG
    assert lib.fmcw_sig_db_device(None, None, 1, None, -80.0, None, None) == _lib.FMCW_E_ARG


def test_reference_self_check():
    """The reference against a direct double loop over the definition on one tiny map, in both storage
    forms, with a gate, a dc band, and centres that clip, miss and are invalid."""
    rng = np.random.default_rng(5)
    F, nr, nd = 5, 16, 8
    x = (rng.standard_normal((F, nr, nd)) + 1j * rng.standard_normal((F, nr, nd))).astype(np.complex64)
    h = (np.stack([x.real, x.imag], -1) / np.float32(nr * nd)).astype(np.float16)
    centers = np.array([4, 99, 0, 99, 1, 99, 16, 99, 17, 99], np.int32)        # stride 2, slots between: garbage
    for rd in (x, h):
        v = R.as_complex(rd)
        for (lo, hi), dc, ctr, th in (((0, 0), -1, None, 0), ((3, 14), 1, None, 0), ((2, 15), 0, centers, 2)):
            ref = R.sig_reference(rd, lo, hi, dc, ctr, 2, th)
            for f in range(F):
                g0, g1 = (0, nr - 1) if (lo, hi) == (0, 0) else (lo - 1, hi - 1)
                rows = list(range(g0, g1 + 1))
                if ctr is not None:
                    c = int(ctr[2 * f])
                    rows = [r for r in range(c - 1 - th, c + th) if g0 <= r <= g1] if 1 <= c <= nr else []
                assert ref["n_dt"][f] == len(rows)
                for d in range(nd):
                    want = sum(abs(v[f, r, d]) ** 2 for r in rows)
                    assert ref["doppler_time"][f, d] == pytest.approx(want, rel=1e-12, abs=0)
                bins = [d for d in range(nd) if min(abs(d - nd // 2), nd - abs(d - nd // 2)) > dc]
                assert ref["n_rt"] == len(bins)
                for r in range(nr):
                    want = sum(abs(v[f, r, d]) ** 2 for d in bins) if r in rows else 0.0
                    assert ref["range_time"][f, r] == pytest.approx(want, rel=1e-12, abs=0)
            assert ref["dt_max"] == ref["doppler_time"].max() and ref["rt_max"] == ref["range_time"].max()
    # the tracked frames: centre 4 -> rows 1..5, centre 0 none, centre 1 -> rows 1..2 (the gate cuts row 0),
    # centre 16 -> rows 13..14 (the gate cuts row 15), centre 17 is outside 0..nr: none
    assert R.sig_reference(x, 2, 15, 0, centers, 2, 2)["n_dt"].tolist() == [5, 0, 2, 2, 0]
    assert R.frame_rows(16, 0, 0, 16, 64) == (0, 16) and R.frame_rows(16, 5, 6, 9, 2) == (0, 0)
    assert R.kept_bins(8, 1).tolist() == [True, True, True, False, False, False, True, True]
    # dB: zeros and a zero maximum give the floor; the clamp holds
    lin = np.array([0.0, 1.0, 1e-9, 0.5])
    np.testing.assert_allclose(R.db_reference(lin, 1.0, -60.0), [-60.0, 0.0, -60.0, 10 * np.log10(0.5)])
    assert R.db_reference(lin, 0.0, -60.0).tolist() == [-60.0] * 4


def test_assert_matches_rejects_what_it_should():
    """The comparison the GPU tests use: accepts float32 roundings of the reference, rejects an output
    off by more than (N + 8) 2^-24, a non-zero where the reference is 0, and a maximum that is not the
    map's."""
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((2, 16, 8)) + 1j * rng.standard_normal((2, 16, 8))).astype(np.complex64)
    ref = R.sig_reference(x, 3, 14, 0)
    good = dict(doppler_time=ref["doppler_time"].astype(np.float32), range_time=ref["range_time"].astype(np.float32))
    good["dt_max"], good["rt_max"] = good["doppler_time"].max(), good["range_time"].max()
    R.assert_matches(good, ref)
    for k, idx, factor in (("doppler_time", (1, 3), 1 + 30 * R.U), ("range_time", (0, 5), 1 - 20 * R.U)):
        bad = {n: np.array(v) for n, v in good.items()}
        bad[k][idx] *= np.float32(factor)                # 12 rows + 8 = 20 < 30; 7 bins + 8 = 15 < 20
        with pytest.raises(AssertionError, match=k):
            R.assert_matches(bad, ref)
    bad = {n: np.array(v) for n, v in good.items()}
    bad["range_time"][0, 0] = 1e-30                      # a row outside the gate
    with pytest.raises(AssertionError, match="exactly 0"):
        R.assert_matches(bad, ref)
    with pytest.raises(AssertionError, match="dt_max"):
        R.assert_matches(dict(good, dt_max=np.float32(0)), ref)
    R.assert_matches(dict(good, dt_max=np.float32(0)), ref, maps=("range_time",))
