"""Reference of the angle-of-arrival stage (include/fmcw.h, fmcw_aoa_params), written from its
definition; test-side code (the library's kernel is csrc/kernels_aoa.hip).

Two evaluations, both on exactly the bytes the device is given (complex64 as is; float16 storage
widened, which is exact):

* float32 (aoa_reference): every intermediate is a numpy float32, so every operation is rounded on
  its own, in the order the header writes them; a target's sums run one cell after the other in
  ascending list position.  Every integer output, every z / e0 / e1, tgt_coh and every *_sin (from the
  phase the device returned) must equal it BIT FOR BIT, with no exempt cases.
* float64 (aoa_reference with ftype=np.float64): the same formulas from the same stored values and float32 weights,
  for the bounds.

The float32 sums against the float64 ones.  u = 2^-24.  A component of v = x w is computed as
fl(fl(a) - fl(b)) with |a| + |b| <= |x| |w| = |v|, so it is off by at most (2u + u^2) |v|.  A term
q.re p.re + q.im p.im formed from such components is off by at most 2 (2 (2u) + ..) |p| |q| = 8u |p||q|
from the components plus 2u |p| |q| from its own two products and one add: 10u |p| |q| to first
order (the same for the zi term and, with q = p, for the energies).  Adding N such terms one after the
other from 0 costs at most (N - 1) u of the sum of their magnitudes (0 + t is exact).  Together

    |Z32 - Z64| <= (N + 9) 2^-24 (1 + O(u)) * sum |terms|,     |terms| = |p| |q|  (|p|^2, |q|^2)

and the bound the tests hold the sums to, (N + 8) 2^-23 * sum |terms| = (2N + 16) 2^-24 .., covers it
for every N >= 0.  N is the number of added terms: (A - 1) per cell, times the target's cells.

The phase.  atan2f is a library function on both sides, so *_phase cannot be compared bit for bit.
It is held against float64 arctan2 of the RETURNED (zim, zre).  The bound is measured on numpy's own
float32 arctan2 over the same values: E = its largest error in ulps of the (float32) result; the
device is allowed 2 E + 1 ulps -- a device library is typically a few-ulp function where the host's is
a one-to-two-ulp one, and one ulp is the final rounding.  Where zre = zim = 0 the phase must be 0.
E is taken over all the values a test compares (a test that makes several calls pools them: a
handful of values says little about a function's largest error).  phase_check prints E, the bound
and the device's largest error before it asserts.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
DET_KEYS = ("det_zre", "det_zim", "det_phase", "det_sin")
TGT_KEYS = ("tgt_zre", "tgt_zim", "tgt_e0", "tgt_e1", "tgt_phase", "tgt_sin", "tgt_coh", "tgt_cells")
OUT_KEYS = DET_KEYS + TGT_KEYS


def stored(rd):
    """(re, im) float32 [F][nr][nd]: the stored values the device reads, widened exactly (the view of
    fp16 storage of cfar_reference.as_complex, without its scale)."""
    rd = np.asarray(rd)
    if rd.dtype == np.float16:
        assert rd.ndim == 4 and rd.shape[-1] == 2
        v = rd.astype(F32)
        return np.ascontiguousarray(v[..., 0]), np.ascontiguousarray(v[..., 1])
    assert rd.dtype == np.complex64 and rd.ndim == 3
    return np.ascontiguousarray(rd.real), np.ascontiguousarray(rd.imag)


def scale2_of(rd) -> np.float32:
    """((float) nr (float) nd)^2 for fp16 storage, else 1: a power of two."""
    rd = np.asarray(rd)
    if rd.dtype != np.float16:
        return F32(1)
    nr, nd = rd.shape[1:3]
    s = F32(nr) * F32(nd)
    return F32(s * s)


def _valid(det_count, ridx, didx, nr, nd):
    """[F][K] bool: list position i < n = clamp(det_count, 0, K) with 1 <= r <= nr and 1 <= d <= nd."""
    F, K = ridx.shape
    n = np.clip(np.asarray(det_count, np.int64), 0, K)
    r, d = np.asarray(ridx, np.int64), np.asarray(didx, np.int64)
    return (np.arange(K)[None, :] < n[:, None]) & (r >= 1) & (r <= nr) & (d >= 1) & (d <= nd)


def _cells(rds, valid, ridx, didx, w, ftype):
    """(zr, zi, e0, e1, terms) [F][K] in ftype from the stored values, 0 where not valid; `terms`
    holds (sum |p||q|, sum |p|^2, sum |q|^2) in float64 for the bounds."""
    F, K = ridx.shape
    ff, ii = np.nonzero(valid)
    r = np.asarray(ridx, np.int64)[ff, ii] - 1
    d = np.asarray(didx, np.int64)[ff, ii] - 1
    w = np.asarray(w, F32)
    v = []
    for a, rd in enumerate(rds):
        re, im = stored(rd)
        xr, xi = re[ff, r, d].astype(ftype), im[ff, r, d].astype(ftype)
        wr, wi = ftype(w[a, 0]), ftype(w[a, 1])
        v.append((xr * wr - xi * wi, xr * wi + xi * wr))
    zr = np.zeros(len(ff), ftype)
    zi, e0, e1 = zr.copy(), zr.copy(), zr.copy()
    tz, t0, t1 = np.zeros(len(ff)), np.zeros(len(ff)), np.zeros(len(ff))
    for a in range(len(rds) - 1):
        (pr, pi), (qr, qi) = v[a], v[a + 1]
        zr = zr + (qr * pr + qi * pi)
        zi = zi + (qi * pr - qr * pi)
        e0 = e0 + (pr * pr + pi * pi)
        e1 = e1 + (qr * qr + qi * qi)
        p2 = pr.astype(np.float64) ** 2 + pi.astype(np.float64) ** 2
        q2 = qr.astype(np.float64) ** 2 + qi.astype(np.float64) ** 2
        tz, t0, t1 = tz + np.sqrt(p2 * q2), t0 + p2, t1 + q2
    out = []
    for x in (zr, zi, e0, e1):
        full = np.zeros((F, K), ftype)
        full[ff, ii] = x
        out.append(full)
    terms = np.zeros((3, F, K))
    terms[:, ff, ii] = (tz, t0, t1)
    return out[0], out[1], out[2], out[3], terms


def _member(valid, labels, max_tgt):
    """[F][K] int64: the target 1..max_tgt of a valid cell, 0 for none."""
    if labels is None or max_tgt == 0:
        return np.zeros(valid.shape, np.int64)
    lab = np.asarray(labels, np.int64)
    return np.where(valid & (lab >= 1) & (lab <= max_tgt), lab, 0)


def _seq_sum(x, ftype):
    """0 + x[0] + x[1] + ..., one after the other (cumsum adds sequentially; np.sum would add pairwise)."""
    return np.cumsum(np.concatenate([np.zeros(1, ftype), x.astype(ftype)]), dtype=ftype)[-1]


def phase_of(zr, zi):
    """float32 arctan2, 0 where both are 0 (the reference's own phase; the device's is compared
    against float64, see the module docstring)."""
    zr, zi = np.asarray(zr), np.asarray(zi)
    return np.where((zr == 0) & (zi == 0), zr.dtype.type(0), np.arctan2(zi, zr)).astype(zr.dtype)


def sin_of(phase, kinv):
    """clamp(phase * kinv, -1, 1) in float32."""
    return np.clip(np.asarray(phase, F32) * F32(kinv), F32(-1), F32(1)).astype(F32)


def coh_of(zr, zi, e0, e1):
    """(raw, clamped) float32 coherence: sqrt(zr zr + zi zi) / (sqrt(e0) sqrt(e1)), 0 when e0 or e1
    is 0; numpy's float32 sqrt and divide are correctly rounded."""
    zr, zi, e0, e1 = (np.asarray(x, F32) for x in (zr, zi, e0, e1))
    ok = (e0 != 0) & (e1 != 0)
    den = np.where(ok, np.sqrt(e0) * np.sqrt(e1), F32(1)).astype(F32)
    raw = np.where(ok, np.sqrt(zr * zr + zi * zi) / den, F32(0)).astype(F32)
    return raw, np.minimum(F32(1), raw)


def aoa_reference(rds, det_count, ridx, didx, labels, w, kinv, max_tgt, ftype=F32) -> dict:
    """The library's outputs from the definition, in ftype (float32: the bits the device must give,
    but for the phases; float64: for the bounds).  z / e0 / e1 are returned times scale2; the
    unscaled per-target sums are under raw_*.  Also valid [F][K], member [F][K], terms_det
    [3][F][K] and terms_tgt [3][F][M] (sums of |p||q|, |p|^2, |q|^2) and tgt_terms_n [F][M], the
    number of added terms."""
    ridx, didx = np.asarray(ridx), np.asarray(didx)
    F, K = ridx.shape
    nr, nd = np.asarray(rds[0]).shape[1:3]
    A, M = len(rds), int(max_tgt)
    valid = _valid(det_count, ridx, didx, nr, nd)
    zr, zi, e0, e1, terms = _cells(rds, valid, ridx, didx, w, ftype)
    s2 = ftype(scale2_of(rds[0]))
    out = dict(valid=valid, terms_det=terms, det_zre=zr * s2, det_zim=zi * s2)
    out["det_phase"] = phase_of(zr, zi)
    out["det_sin"] = sin_of(out["det_phase"], kinv) if ftype is F32 else np.clip(out["det_phase"] * float(kinv), -1, 1)
    member = _member(valid, labels, M)
    out["member"] = member
    Z = np.zeros((4, F, M), ftype)
    tt = np.zeros((3, F, M))
    cells = np.zeros((F, M), np.int32)
    for f in range(F):
        for t in np.unique(member[f]):
            if t == 0:
                continue
            mem = np.nonzero(member[f] == t)[0]               # ascending list position
            for k, x in enumerate((zr, zi, e0, e1)):
                Z[k, f, t - 1] = _seq_sum(x[f, mem], ftype)
            tt[:, f, t - 1] = terms[:, f, mem].sum(axis=1)
            cells[f, t - 1] = len(mem)
    for k, name in enumerate(("zre", "zim", "e0", "e1")):
        out["raw_" + name] = Z[k]
        out["tgt_" + name] = Z[k] * s2
    out["tgt_phase"] = phase_of(Z[0], Z[1])
    if ftype is F32:
        out["tgt_sin"] = sin_of(out["tgt_phase"], kinv)
        out["tgt_coh_raw"], out["tgt_coh"] = coh_of(*Z)
    else:
        out["tgt_sin"] = np.clip(out["tgt_phase"] * float(kinv), -1, 1)
        ok = (Z[2] != 0) & (Z[3] != 0)
        out["tgt_coh_raw"] = np.where(ok, np.hypot(Z[0], Z[1]) / np.sqrt(np.where(ok, Z[2] * Z[3], 1.0)), 0.0)
        out["tgt_coh"] = np.minimum(1.0, out["tgt_coh_raw"])
    out["tgt_cells"] = cells
    out["terms_tgt"] = tt
    out["tgt_terms_n"] = cells.astype(np.int64) * (A - 1)
    return out


def reference_of(rds, det: dict, q, labels=None, ftype=F32) -> dict:
    """The reference on the dict of detection lists for an AoaConfig (params.py)."""
    return aoa_reference(rds, det["det_count"], det["det_range_idx"], det["det_doppler_idx"], labels, q.weights_f32(),
                         q.kinv, q.max_tgt if labels is not None else 0, ftype)


def ulps_off(phase, zre, zim):
    """|phase - arctan2(zim, zre)| in ulps of the float32 result, float64 arctan2 of the float32
    inputs as the truth; entries with zre = zim = 0 are left out (their phase is 0 by rule)."""
    phase, zre, zim = (np.asarray(x, F32).ravel() for x in (phase, zre, zim))
    sel = (zre != 0) | (zim != 0)
    truth = np.arctan2(zim[sel].astype(np.float64), zre[sel].astype(np.float64))
    ulp = np.spacing(np.abs(truth).astype(F32)).astype(np.float64)
    return np.abs(phase[sel].astype(np.float64) - truth) / ulp


def phase_check(got_phase, zre, zim, what=""):
    """The device's phases against float64 arctan2 of the returned (zim, zre), within twice numpy
    float32's own largest error over the same values plus one ulp.  Returns (device, numpy, bound)
    in ulps, printed before the assertion."""
    got_phase, zre, zim = (np.asarray(x, F32) for x in (got_phase, zre, zim))
    assert np.all(np.isfinite(zre)) and np.all(np.isfinite(zim)), what
    zero = (zre == 0) & (zim == 0)
    own = ulps_off(np.arctan2(zim, zre), zre, zim)
    dev = ulps_off(got_phase, zre, zim)
    e_np = float(own.max()) if own.size else 0.0
    e_dev = float(dev.max()) if dev.size else 0.0
    bound = 2.0 * e_np + 1.0
    print(f"aoa phase {what}: device {e_dev:.3f} ulp, numpy float32 {e_np:.3f} ulp, bound {bound:.3f} ulp "
          f"over {dev.size} values")
    assert np.all(got_phase[zero] == 0) and not np.signbit(got_phase[zero]).any(), what
    assert np.all(np.abs(got_phase) <= F32(np.pi)), what
    assert e_dev <= bound, (what, e_dev, bound)
    return e_dev, e_np, bound


def phase_check_pool(pool, what=""):
    """phase_check over everything a test's assert_matches calls collected in `pool`."""
    assert pool, what
    return phase_check(*[np.concatenate([np.asarray(p[i], F32).ravel() for p in pool]) for i in range(3)], what)


def assert_matches(got: dict, ref: dict, kinv, keys=None, pool=None) -> None:
    """The library's outputs against the float32 reference (the module's docstring has the rules).
    `keys`: the outputs to compare (default: all of OUT_KEYS that `got` holds).  `pool`: a list; the
    phases are then appended to it as (phase, zre, zim), for one phase_check_pool over all the inputs
    of a test, instead of being checked over this call's alone."""
    have = [k for k in OUT_KEYS if k in got and got[k] is not None]
    for k in have if keys is None else keys:
        g = np.asarray(got[k])
        if k == "tgt_cells":
            assert g.dtype == np.int32, k
            np.testing.assert_array_equal(g, ref[k], err_msg=k)
        elif k.endswith("_phase"):
            assert g.dtype == F32, k
            pre = k[:3]
            # z of the device equals the reference's bit for bit (checked under its own key when
            # present), so the reference's z are the returned ones
            if pool is None:
                phase_check(g, ref[pre + "_zre"], ref[pre + "_zim"], k)
            else:
                pool.append((g, ref[pre + "_zre"], ref[pre + "_zim"]))
        elif k.endswith("_sin"):
            assert g.dtype == F32, k
            ph = got.get(k[:3] + "_phase")
            assert ph is not None, k + " is checked from the returned phase"
            assert g.tobytes() == sin_of(ph, kinv).tobytes(), k
        else:
            assert g.dtype == F32, k
            assert g.tobytes() == np.asarray(ref[k], F32).tobytes(), (k, np.argwhere(g != ref[k])[:4].tolist())
