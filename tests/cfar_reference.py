"""float64 reference of the 2-D CA-CFAR detector (include/fmcw.h, fmcw_cfar_params), written from its
definition; test-side code (the library's kernel is csrc/kernels_cfar.hip).

All indices in here are 0-based; the library's outputs are 1-based.

  training set of (r, d): (r + dr, (d + dd) mod nd) with |dr| <= Wr, |dd| <= Wd, not (|dr| <= guard_r
  and |dd| <= guard_d), 0 <= r + dr < nr;  N(r) cells, S their power sum;
  detection iff gated and P > alpha * S / N;  LOCAL_MAX: also P > the four 3 x 3 neighbours before it in
  raster order and P >= the four after it (circular in Doppler, clipped in range).

`exempt` marks the cells whose outcome float32 arithmetic may legitimately flip:
  gated cells with |P - T| <= (N + 8) 2^-24 T, T = alpha S / N (N - 1 roundings of the sum, the rest for
  re^2 + im^2, the scale and the divide), and, with LOCAL_MAX, threshold crossings whose P is within
  8 2^-24 P of a neighbour's.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
MAX_EXEMPT_SHARE = 1e-4            # a test may exempt at most 1 in 10^4 of its gated cells


def as_complex(rd) -> np.ndarray:
    """The values the device is given, exactly, as complex128 [F][nr][nd]: complex64 as is, float16
    [F][nr][nd][2] (D / (nr nd)) times nr nd."""
    rd = np.asarray(rd)
    if rd.dtype == np.float16:
        nr, nd = rd.shape[1:3]
        v = rd.astype(np.float64) * (nr * nd)
        return v[..., 0] + 1j * v[..., 1]
    return rd.astype(np.complex128)


def _shift_rows(a, dr):
    """b[r] = a[r + dr] where that row exists, else 0."""
    b = np.zeros_like(a)
    nr = a.shape[0]
    if dr >= 0:
        b[: nr - dr] = a[dr:]
    else:
        b[-dr:] = a[: nr + dr]
    return b


def cfar_reference(rd, guard, train, alpha, r_lo=0, r_hi=0, local_max=False) -> dict:
    """rd [F][nr][nd] (complex, or the float16 pairs); guard / train = (range, doppler) half-widths;
    alpha the float32 the device is given; r_lo..r_hi the 1-based inclusive gate (0, 0 = all rows).
    Returns det, exempt [F][nr][nd] bool, P, noise [F][nr][nd] float64, N [nr] int, gated [nr] bool."""
    x = as_complex(rd)
    F, nr, nd = x.shape
    gr, gd = guard
    tr, td = train
    Wr, Wd = gr + tr, gd + td
    assert tr + td >= 1 and 2 * Wr + 1 <= nr and 2 * Wd + 1 <= nd
    alpha = float(np.float32(alpha))
    P = x.real ** 2 + x.imag ** 2
    rows = np.arange(nr)
    gated = np.ones(nr, bool) if (r_lo, r_hi) == (0, 0) else (rows >= r_lo - 1) & (rows <= r_hi - 1)
    # N(r): rows inside the guard rows carry 2 train_d cells, the others 2 Wd + 1
    N = np.zeros(nr, np.int64)
    for dr in range(-Wr, Wr + 1):
        ok = (rows + dr >= 0) & (rows + dr < nr)
        N += ok * (2 * td if abs(dr) <= gr else 2 * Wd + 1)
    det = np.zeros((F, nr, nd), bool)
    exempt = np.zeros((F, nr, nd), bool)
    noise = np.zeros((F, nr, nd))
    for f in range(F):
        p = P[f]
        h_full = np.zeros_like(p)
        h_side = np.zeros_like(p)
        for dd in range(-Wd, Wd + 1):
            s = np.roll(p, -dd, axis=1)              # s[r][d] = p[r][(d + dd) mod nd]
            h_full += s
            if abs(dd) > gd:
                h_side += s
        S = np.zeros_like(p)
        for dr in range(-Wr, Wr + 1):
            S += _shift_rows(h_side if abs(dr) <= gr else h_full, dr)
        nz = S / N[:, None]
        T = alpha * nz
        d = (p > T) & gated[:, None]
        ex = (np.abs(p - T) <= (N[:, None] + 8) * U * T) & gated[:, None]
        if local_max:
            top = np.ones_like(d)
            near = np.zeros_like(d)
            for dr in (-1, 0, 1):
                for dd in (-1, 0, 1):
                    if (dr, dd) == (0, 0):
                        continue
                    nb = _shift_rows(np.roll(p, -dd, axis=1), dr)
                    exists = ((rows + dr >= 0) & (rows + dr < nr))[:, None]
                    before = (dr, dd) < (0, 0)
                    top &= ~exists | ((p > nb) if before else (p >= nb))
                    near |= exists & (np.abs(p - nb) <= 8 * U * p)
            ex |= d & near
            d &= top
        det[f], exempt[f], noise[f] = d, ex, nz
    return dict(det=det, exempt=exempt, P=P, noise=noise, N=N, gated=gated)


def check_exempt(ref) -> int:
    """Fail (never skip) when the reference exempts more than 1 in 10^4 of the gated cells."""
    F, nr, nd = ref["det"].shape
    n_gated = int(ref["gated"].sum()) * nd * F
    n_ex = int(ref["exempt"].sum())
    assert n_ex <= MAX_EXEMPT_SHARE * n_gated, f"the reference exempts {n_ex} of {n_gated} gated cells"
    return n_ex


def lists(ref, max_det) -> dict:
    """The library's per-frame outputs from the reference: counts, the first max_det detections in
    (range, doppler) order with 1-based indices, power and noise; 0 where unused."""
    det = ref["det"]
    F = det.shape[0]
    K = max_det
    out = dict(det_count=np.zeros(F, np.int32), det_range_idx=np.zeros((F, K), np.int32),
               det_doppler_idx=np.zeros((F, K), np.int32), det_power=np.zeros((F, K)), det_noise=np.zeros((F, K)),
               det_n=np.zeros((F, K), np.int64))
    for f in range(F):
        r, d = np.nonzero(det[f])                    # row-major: ascending (range, doppler)
        out["det_count"][f] = len(r)
        r, d = r[:K], d[:K]
        n = len(r)
        out["det_range_idx"][f, :n] = r + 1
        out["det_doppler_idx"][f, :n] = d + 1
        out["det_power"][f, :n] = ref["P"][f, r, d]
        out["det_noise"][f, :n] = ref["noise"][f, r, d]
        out["det_n"][f, :n] = ref["N"][r]
    return out


def assert_matches(got, ref, max_det, mask=None) -> None:
    """The library's outputs against the reference: counts, both index lists and the mask equal,
    det_power at rtol 8 2^-24, det_noise at rtol (N + 8) 2^-24, unused entries 0.  With exempt cells
    (at most 1 in 10^4, check_exempt) the comparison leaves those cells' outcome open."""
    n_ex = check_exempt(ref)
    want = lists(ref, max_det)
    if n_ex:                                         # take the device's decision on the exempt cells
        assert mask is not None, "exempt cells need the mask to be compared"
        ex = ref["exempt"]
        np.testing.assert_array_equal(mask.astype(bool)[~ex], ref["det"][~ex])
        ref = dict(ref, det=np.where(ex, mask.astype(bool), ref["det"]))
        want = lists(ref, max_det)
    elif mask is not None:
        np.testing.assert_array_equal(mask, ref["det"].astype(np.uint8))
    np.testing.assert_array_equal(got["det_count"], want["det_count"])
    np.testing.assert_array_equal(got["det_range_idx"], want["det_range_idx"])
    np.testing.assert_array_equal(got["det_doppler_idx"], want["det_doppler_idx"])
    used = want["det_range_idx"] > 0
    for k in ("det_power", "det_noise"):
        assert got[k].dtype == np.float32 and np.all(got[k][~used] == 0), k
    dp = np.abs(got["det_power"][used] - want["det_power"][used])
    assert np.all(dp <= 8 * U * want["det_power"][used]), float((dp / want["det_power"][used]).max())
    dn = np.abs(got["det_noise"][used] - want["det_noise"][used])
    assert np.all(dn <= (want["det_n"][used] + 8) * U * want["det_noise"][used]), \
        float((dn / want["det_noise"][used]).max())
