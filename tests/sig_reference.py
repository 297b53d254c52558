"""float64 reference of the Doppler-time and range-time signatures (include/fmcw.h, fmcw_sig_params),
written from their definition; test-side code (the library's kernels are csrc/kernels_sig.hip).

All indices in here are 0-based except the arguments the library takes 1-based (the gate, the centres).

  P[r][d] = re^2 + im^2 of the stored value (fp16 storage: times (nr nd)^2);
  rows of frame f: the gate r_lo..r_hi (0, 0 = all rows), or with a centre c (1-based; 0, or outside
  0..nr: no rows) the rows c-1-h .. c-1+h intersected with the gate;
  doppler_time[f][d] = sum of P[r][d] over the frame's rows                       (N = rows)
  range_time[f][r]   = sum of P[r][d] over the bins with |d - nd/2| > dc_half     (N = bins kept),
                       0 for every row that is not one of the frame's.
"""
from __future__ import annotations

import numpy as np

from tests.cfar_reference import U, as_complex


def frame_rows(nr, r_lo=0, r_hi=0, center=None, track_half=0):
    """0-based [ra, rb) of one frame; ra == rb: no rows."""
    g0, g1 = (0, nr - 1) if (r_lo, r_hi) == (0, 0) else (r_lo - 1, r_hi - 1)
    if center is None:
        return g0, g1 + 1
    c = int(center)
    if c < 1 or c > nr:
        return 0, 0
    ra, rb = max(c - 1 - track_half, g0), min(c - 1 + track_half, g1) + 1
    return (ra, rb) if ra < rb else (0, 0)


def kept_bins(nd, dc_half):
    d = np.arange(nd)
    dist = np.abs(d - nd // 2)
    return np.minimum(dist, nd - dist) > dc_half


def sig_reference(rd, r_lo=0, r_hi=0, dc_half=-1, center=None, center_stride=1, track_half=0) -> dict:
    """rd [F][nr][nd] (complex, or the float16 pairs).  center: None or a flat int array read at
    f * center_stride.  Returns doppler_time [F][nd], range_time [F][nr] float64, their maxima, and
    the number of cells summed into every output: n_dt [F] (rows), n_rt (bins kept)."""
    x = as_complex(rd)
    F, nr, nd = x.shape
    P = x.real ** 2 + x.imag ** 2
    keep = kept_bins(nd, dc_half)
    dt = np.zeros((F, nd))
    rt = np.zeros((F, nr))
    n_dt = np.zeros(F, np.int64)
    flat = None if center is None else np.asarray(center).reshape(-1)
    for f in range(F):
        ra, rb = frame_rows(nr, r_lo, r_hi, None if flat is None else flat[f * center_stride], track_half)
        n_dt[f] = rb - ra
        dt[f] = P[f, ra:rb].sum(axis=0)
        rt[f, ra:rb] = P[f, ra:rb][:, keep].sum(axis=1)
    return dict(doppler_time=dt, range_time=rt, dt_max=dt.max(initial=0.0), rt_max=rt.max(initial=0.0), n_dt=n_dt,
                n_rt=int(keep.sum()))


def _close(got, want, n, name):
    assert got.dtype == np.float32 and got.shape == want.shape, name
    zero = want == 0
    assert np.all(got[zero] == 0), f"{name}: outputs whose reference is 0 must be exactly 0"
    err = np.abs(got.astype(np.float64) - want)
    bound = (n + 8) * U * want
    bad = err > bound
    assert not bad.any(), f"{name}: {int(bad.sum())} outputs off, worst {float((err / np.maximum(want, 1e-300))[bad].max()):.3e}"


def assert_matches(got, ref, maps=("doppler_time", "range_time")) -> None:
    """The library's linear outputs against the reference: every output within (N + 8) 2^-24 relative,
    exact zeros where the reference is 0, the maxima equal to the maximum of the returned map."""
    if "doppler_time" in maps:
        _close(got["doppler_time"], ref["doppler_time"], ref["n_dt"][:, None], "doppler_time")
        assert np.float32(got["dt_max"]) == got["doppler_time"].max(initial=np.float32(0)), "dt_max"
    if "range_time" in maps:
        _close(got["range_time"], ref["range_time"], ref["n_rt"], "range_time")
        assert np.float32(got["rt_max"]) == got["range_time"].max(initial=np.float32(0)), "rt_max"


def db_reference(lin, mx, floor_db):
    """max(10 log10(lin / mx), floor_db) in float64; floor_db where lin or mx is 0."""
    lin = np.asarray(lin, np.float64)
    out = np.full(lin.shape, float(floor_db))
    if float(mx) > 0:
        nz = lin > 0
        out[nz] = np.maximum(10.0 * np.log10(lin[nz] / float(mx)), float(floor_db))
    return out


def db_tolerance(floor_db):
    """dB: the divide and log10f at a few ulp each, and the rounding of a result up to |floor_db|."""
    return (10.0 / np.log(10.0)) * 8 * U + 8 * U * abs(floor_db)
