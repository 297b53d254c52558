"""Reference of the two detection decisions (radar_processing.m:211 f_search_peak, :227-239 the
Doppler index), written from their definition; test-side numpy code, no GPU.  The library's
kernels are select_peaks / detect_frame (csrc/frame_ops.h), k_detect_1p (csrc/kernels_detect.hip)
and k_rdx's candidate keys (csrc/kernels_xcd.hip).

Two uses:

  self-consistent   peaks() on the float32 profile a call RETURNED gives the count, indices and
                    magnitudes the same call must return, bit for bit: every compare of the rule
                    is a float32 compare, exact when widened to double, and the gate is computed
                    from the float32 parameters of the C-ABI as the kernels compute it
                    (abi_params, gate_bins).  doppler_choice() on a returned RD row gives the
                    index, or the set of indices where float32 rounding of the magnitudes may
                    decide (band 2^-21, below).  No frame has to be left out.
  oracle            the float64 oracle (oracle/oracle.py) given the abi_params values; frames and
                    rows where rounding may legitimately decide are found on the oracle alone
                    (frame_ambiguous, row_ambiguous) and are capped at 10 % of a batch.

The band of doppler_choice is derived, not measured: the kernels form sqrtf(x*x + y*y) * unscale
in float32 (unscale a power of two), with or without FMA contraction: two products and a sum
(<= 1.5 ulp of the sum), the square root (halves the relative error, adds 0.5 ulp): within a few
ulp (2^-24 each) of the true magnitude.  2^-21 is 8 ulp.

The scene builder makes one-frame scenes: the calibration tone, complex noise of sigma 1e-3 from
a seeded generator, and tones (A, range_bin, doppler_bin, phase, am_depth, am_bin).
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

BAND = 2.0 ** -21
MAX_AMBIGUOUS_SHARE = 0.10         # of a batch's frames, and of its Doppler rows


# --------------------------------------------------------------------------
# the parameters and the gate as the kernels see them
# --------------------------------------------------------------------------
def abi_params(cfg) -> dict:
    """range_thr, doppler_thr, min_d, max_d, dist_per_bin as the float32 the C-ABI carries
    (fmcw_params), widened to double."""
    f = np.float32
    return {k: float(f(getattr(cfg, k))) for k in ("range_thr", "doppler_thr", "min_d", "max_d", "dist_per_bin")}


def oracle_params(p: dict, cfg, M: int) -> dict:
    """The oracle's parameter dict with the abi_params values and max_targets M."""
    q = dict(p)
    q.update(abi_params(cfg))
    q["max_targets"] = int(M)
    q["doppler_fallback_idx"] = cfg.doppler_fallback_idx
    return q


def gate_bins(cfg) -> np.ndarray:
    """0-based bins the rule admits: 1 <= i <= nr - 2 and i * dist_per_bin in [min_d, max_d], the
    product in double from the float32 parameters (double rng = i * (double)float_dpb)."""
    a = abi_params(cfg)
    out = []
    for i in range(1, cfg.nr - 1):
        rng = float(i) * a["dist_per_bin"]
        if a["min_d"] <= rng <= a["max_d"]:
            out.append(i)
    return np.asarray(out, np.int64)


def xcd_group(r: int) -> int:
    """fmcw_internal.h xcd_group: the range-bin group (k_rdx team member) that holds bin r."""
    return ((r >> 2) & 1) | (((r >> 3) & 1) << 1) | ((r >> 7) << 2)


# --------------------------------------------------------------------------
# :211 the peak rule on float32 profile values, exactly
# --------------------------------------------------------------------------
def peaks(profile_f32, prm: dict, M: int):
    """search_peak restated on one float32 profile [nr].  Returns (count, idx[M] 1-based int32,
    mag[M] float32), unused slots 0: candidates i (0-based, 1..nr-2, inside the gate) with
    p[i] > range_thr, p[i] >= p[i-1], p[i] > p[i+1]; the M largest, descending, ties to the
    lower index."""
    p32 = np.asarray(profile_f32)
    assert p32.dtype == np.float32 and p32.ndim == 1
    p = p32.astype(np.float64)
    nr = len(p)
    cands = []
    for i in range(1, nr - 1):
        rng = float(i) * prm["dist_per_bin"]
        if rng < prm["min_d"] or rng > prm["max_d"]:
            continue
        if p[i] > prm["range_thr"] and p[i] >= p[i - 1] and p[i] > p[i + 1]:
            cands.append((-p[i], i))
    cands.sort()
    sel = cands[:M]
    idx = np.zeros(M, np.int32)
    mag = np.zeros(M, np.float32)
    for j, (_, i) in enumerate(sel):
        idx[j] = i + 1
        mag[j] = p32[i]
    return len(sel), idx, mag


def group_keys(profile, prm: dict, group: int, ncand: int = 2):
    """The bins k_rdx keeps as slow-time candidates of one range-bin group: the ncand largest
    in-gate bins above range_thr (no local-maximum test), ties to the lower bin."""
    p = np.asarray(profile, np.float64)
    ks = []
    for i in range(1, len(p) - 1):
        rng = float(i) * prm["dist_per_bin"]
        if xcd_group(i) == group and prm["min_d"] <= rng <= prm["max_d"] and p[i] > prm["range_thr"]:
            ks.append((-p[i], i))
    ks.sort()
    return [i for _, i in ks[:ncand]]


# --------------------------------------------------------------------------
# :227-239 the Doppler index of one RD row
# --------------------------------------------------------------------------
def doppler_choice(rd_row_complex, thr: float, fallback: int) -> dict:
    """rd_row_complex: the row's values as the device holds them (complex64, or the fp16 pairs
    times Nr Nd), any complex dtype.  Returns idx (the reference's 1-based index: first maximum of
    the float64 magnitudes, kept when max >= thr and idx != fallback, else fallback), allowed (the
    set of indices a float32 evaluation may return) and ambiguous (more than one bin within 2^-21
    of the maximum, or the maximum within 2^-21 of thr).  The band is relative, so a row that is
    exactly zero leaves nothing open: every float32 magnitude is exactly 0, the first maximum is bin 0
    and 0 >= thr is decided exactly."""
    mag = np.abs(np.asarray(rd_row_complex, np.complex128))
    d0 = int(np.argmax(mag))
    mx = float(mag[d0])
    near = np.nonzero(mag >= mx * (1.0 - BAND))[0] if mx > 0.0 else np.array([0])
    thr_amb = mx > 0.0 and abs(mx - thr) <= BAND * max(abs(thr), mx)

    def rule(d, passes):
        return d + 1 if (passes and d + 1 != fallback) else fallback

    idx = rule(d0, mx >= thr)
    allowed = set()
    for d in near:
        if thr_amb:
            allowed.update((rule(int(d), True), rule(int(d), False)))
        else:
            allowed.add(rule(int(d), mx >= thr))
    return dict(idx=idx, allowed=allowed, ambiguous=bool(len(near) > 1 or thr_amb), max=mx)


# --------------------------------------------------------------------------
# where the float64 oracle and a float32 evaluation may legitimately differ
# --------------------------------------------------------------------------
def frame_ambiguous(profile, prm: dict, M: int, tol: float) -> bool:
    """On the oracle's profile: two of the M + 1 strongest candidates within a relative tol of each
    other, or one of them within tol of range_thr.  A candidate here is a bin that passes the rule
    with every compare relaxed by tol, so the partner of a plateau (p[i] within tol of p[i+1], either
    of which a rounding may make the peak) and a bin just below the threshold count.  Weaker
    candidates near the threshold are not looked at: with M + 1 candidates clear of it and of each
    other, they can change neither the count nor the M strongest."""
    p = np.asarray(profile, np.float64)
    v = []
    s = 1.0 - tol
    for i in range(1, len(p) - 1):
        rng = float(i) * prm["dist_per_bin"]
        if rng < prm["min_d"] or rng > prm["max_d"]:
            continue
        if p[i] > prm["range_thr"] * s and p[i] >= p[i - 1] * s and p[i] > p[i + 1] * s:
            v.append(p[i])
    top = np.sort(np.asarray(v))[::-1][: M + 1]
    if np.any(np.abs(top - prm["range_thr"]) <= tol * prm["range_thr"]):
        return True
    return bool(np.any(top[:-1] - top[1:] <= tol * top[:-1])) if len(top) > 1 else False


def row_ambiguous(rd_row, thr: float, tol: float, pre: float = 0.0) -> bool:
    """On the oracle's RD row: the two largest magnitudes within a relative tol, or the largest
    within tol of doppler_thr; or, with pre = sqrt(nd sum |X w|^2) of the row before the mean
    removal of :218, both the largest and doppler_thr at or below tol * pre: the row of a static
    target cancels to the rounding residue of the uncancelled data (helpers.rd_rel_err), which a
    threshold that low does not separate from a signal."""
    mag = np.sort(np.abs(np.asarray(rd_row)))[::-1]
    if mag[0] <= 0.0 or (mag[0] <= tol * pre and thr <= tol * pre):
        return True
    return bool(mag[0] - mag[1] <= tol * mag[0] or abs(mag[0] - thr) <= tol * max(thr, mag[0]))


# --------------------------------------------------------------------------
# scene builder
# --------------------------------------------------------------------------
def tone(A, r, d=0, phase=0.0, am_depth=0.0, am_bin=0):
    return (float(A), float(r), int(d), float(phase), float(am_depth), int(am_bin))


def build_frame(tones, noisy: bool, S: int, C: int, nr: int, nd: int, seed: int, fidx: int,
                sigma: float = 1e-3) -> np.ndarray:
    """x[k, n] = cal[n] + sum A (1 + am_depth cos(2 pi k am_bin / nd)) exp(2 pi j (n r / nr + k d / nd + phase))
    + CN(0, sigma^2), complex64 [C][S]; phase in cycles.  noisy: False, True (the generator is seeded with
    (seed, fidx)) or an integer used in place of fidx."""
    cal = O.synth_cal(S)
    n = np.arange(S, dtype=np.float64)[None, :]
    k = np.arange(C, dtype=np.float64)[:, None]
    x = np.broadcast_to(cal[None, :], (C, S)).astype(np.complex128)
    for (A, r, d, ph, amd, amb) in tones:
        cyc = ((n * r / nr) % 1.0 + (k * (d % nd) / nd) % 1.0 + ph) % 1.0
        x = x + A * (1.0 + amd * np.cos(2 * np.pi * ((k * amb / nd) % 1.0))) * np.exp(2j * np.pi * cyc)
    if noisy is not False:
        g = np.random.default_rng([seed, fidx if noisy is True else int(noisy)])
        x = x + (sigma / np.sqrt(2.0)) * (g.standard_normal((C, S)) + 1j * g.standard_normal((C, S)))
    return x.astype(np.complex64)


def build_frames(scenes, S: int, C: int, nr: int, nd: int, seed: int, sigma: float = 1e-3) -> np.ndarray:
    """scenes: a list of (tones, noisy), one per frame -> complex64 [F][C][S] (build_frame)."""
    return np.stack([build_frame(t, noisy, S, C, nr, nd, seed, f, sigma) for f, (t, noisy) in enumerate(scenes)])


# --------------------------------------------------------------------------
# the float64 oracle over a batch, computed once; decisions per parameter set
# --------------------------------------------------------------------------
def oracle_batch(iq, cal, p: dict, wr, wd) -> dict:
    """The oracle's arithmetic over iq [F][C][S] (anything process_frames accepts): profile [F][nr],
    rd [F][nr][nd] complex128 (every row), absx [F][C][nr] = |cube|, rd_den [F] (the denominator of
    helpers.rd_rel_err), row_pre [F][nr] = sqrt(nd sum_k |X[r, k] wd[k]|^2) over the transformed chirps.  The
    decisions follow from these by decide()."""
    from tests.helpers import rd_rel_err
    F = iq.shape[0]
    nr, nd = p["nr"], p["nd"]
    out = dict(profile=np.zeros((F, nr)), rd=np.zeros((F, nr, nd), np.complex128),
               absx=np.zeros((F, iq.shape[1], nr)), rd_den=np.zeros(F), row_pre=np.zeros((F, nr)))
    kf = min(iq.shape[1], nd)
    for f in range(F):
        X = O.fast_time(iq[f].astype(np.complex128).T, cal, p["if_scale"], wr, nr)
        rd = O.doppler_all_rows(X, wd, nd)
        out["profile"][f] = O.range_profile(X)
        out["rd"][f] = rd
        out["absx"][f] = np.abs(X.T)
        out["row_pre"][f] = np.sqrt(nd * np.sum(np.abs(X[:, :kf] * np.asarray(wd)[None, :kf]) ** 2, axis=1))
        # rd_rel_err(0, ref) = ||ref|| / den  ->  den, the normalisation the RD bar uses
        ratio = rd_rel_err(np.zeros((1, nr, nd)), rd[None], X.T[None], wd, nd)[0]
        out["rd_den"][f] = np.sqrt(np.sum(np.abs(rd) ** 2)) / max(ratio, 1e-300)
    return out


def decide(ob: dict, q: dict) -> dict:
    """oracle.search_peak and oracle.doppler_index over a batch, with the parameters q
    (oracle_params)."""
    F, nr = ob["profile"].shape
    M = q["max_targets"]
    out = dict(tgt_count=np.zeros(F, np.int32), tgt_range_idx=np.zeros((F, M), np.int32),
               tgt_range_mag=np.zeros((F, M)), tgt_doppler_idx=np.zeros((F, M), np.int32))
    for f in range(F):
        ridx, rmag = O.search_peak(ob["profile"][f], nr, q["range_thr"], M, q["min_d"], q["max_d"], q["dist_per_bin"])
        didx = O.doppler_index(ob["rd"][f], ridx, q["doppler_thr"], q["doppler_fallback_idx"])
        n = len(ridx)
        out["tgt_count"][f] = n
        out["tgt_range_idx"][f, :n] = ridx
        out["tgt_range_mag"][f, :n] = rmag
        out["tgt_doppler_idx"][f, :n] = didx
    return out


def ambiguity(ob: dict, dec: dict, q: dict, tol: float):
    """(frames [F] bool, rows [F][M] bool) the oracle comparison leaves out: frame_ambiguous, and
    for every detected row of the other frames row_ambiguous."""
    F, M = dec["tgt_range_idx"].shape
    fa = np.zeros(F, bool)
    ra = np.zeros((F, M), bool)
    for f in range(F):
        fa[f] = frame_ambiguous(ob["profile"][f], q, M, tol)
        for j in range(int(dec["tgt_count"][f])):
            r = dec["tgt_range_idx"][f, j] - 1
            ra[f, j] = row_ambiguous(ob["rd"][f, r], q["doppler_thr"], tol, ob["row_pre"][f, r])
    return fa, ra


def check_caps(fa, ra, dec) -> None:
    """Fail (never skip) when more than 10 % of a batch's frames, or of its Doppler rows, are left
    out of the exact comparison."""
    F = len(fa)
    assert fa.sum() <= MAX_AMBIGUOUS_SHARE * F, f"{int(fa.sum())} of {F} frames are ambiguous"
    used = (np.arange(ra.shape[1])[None, :] < dec["tgt_count"][:, None]) & ~np.asarray(fa)[:, None]
    rows = int(used.sum())
    assert (ra & used).sum() <= MAX_AMBIGUOUS_SHARE * max(rows, 1), f"{int((ra & used).sum())} of {rows} rows are ambiguous"


# --------------------------------------------------------------------------
# the scenes (S1-S11 of the detection tests), one frame each
# --------------------------------------------------------------------------
class Batch:
    """Frames of one geometry with their names; oracle() computes the float64 arithmetic once."""

    def __init__(self, cfg, p, wr, wd, cal, iq, names):
        self.cfg, self.p, self.wr, self.wd, self.cal, self.iq, self.names = cfg, p, wr, wd, cal, iq, list(names)
        self._ob = {}

    def frames(self, prefix):
        """Frames whose name is prefix or prefix and a suffix ('S6' finds S6in and S6out, 'S1' not S10)."""
        return [i for i, n in enumerate(self.names) if n.startswith(prefix) and not n[len(prefix):][:1].isdigit()]

    def iq16(self):
        """The frames as c32h (float16 pairs) and the complex64 values those hold."""
        h = np.stack([self.iq.real, self.iq.imag], -1).astype(np.float16)
        return h, h.astype(np.float32).view(np.complex64)[..., 0]

    def oracle(self, fp16_input=False):
        if fp16_input not in self._ob:
            x = self.iq16()[1] if fp16_input else self.iq
            self._ob[fp16_input] = oracle_batch(x, self.cal, self.p, self.wr, self.wd)
        return self._ob[fp16_input]


def _profile_peak(cfg, p, wr, cal, x_cs):
    X = O.fast_time(x_cs.astype(np.complex128).T, cal, p["if_scale"], wr, cfg.nr)
    return O.range_profile(X)


def threshold_tone(cfg, p, wr, cal, r, d, phase, ratio, seed, fidx, noisy=True):
    """S7: the amplitude at which the oracle's own profile peak at bin r is ratio * range_thr for
    this frame's noise (three secant steps from A = 0.01; the noise makes the peak not quite linear
    in A)."""
    thr = abi_params(cfg)["range_thr"]
    A = 0.01
    for _ in range(4):
        x = _one(cfg, [tone(A, r, d, phase)], noisy, seed, fidx)
        pk = _profile_peak(cfg, p, wr, cal, x)[r]
        A *= ratio * thr / pk
    return A


def _one(cfg, tones, noisy, seed, fidx):
    return build_frame(tones, noisy, cfg.nts, cfg.pn, cfg.nr, cfg.nd, seed, fidx)


def main_scenes(cfg, p, wr, cal, seed: int, full: bool = True):
    """S1-S10 for cfg's geometry as (names, scenes).  Bins come from gate_bins(cfg); u, the tone
    spacing unit, is nr / nts rounded up (a tone's main lobe is 3 nr / nts bins either side).
    full False: S1-S7 only (geometries the single-pass schedule does not serve)."""
    g = gate_bins(cfg)
    g0, g1 = int(g[0]), int(g[-1])
    u = -(-cfg.nr // cfg.nts)
    nd = cfg.nd
    ph = np.random.default_rng(seed)
    nt = min(10, (g1 - g0 - 1) // (3 * u) + 1)
    mid = (g0 + g1) // 2
    names, sc = [], []

    def add(name, tones, noisy=True):
        names.append(name)
        sc.append((tones, noisy))

    def dop(i):                                   # a nonzero Doppler bin in -nd/2+1 .. nd/2-1
        return (1 + (5 * i) % (nd // 2 - 1)) * (1 if i % 2 else -1)

    for v in range(8 if full else 5):             # S1: nt tones, >= 3 u apart, distinct amplitudes
        perm = ph.permutation(nt)
        add("S1", [tone(0.02 * 1.25 ** int(perm[i]), g0 + 1 + 3 * u * i, dop(i + v), ph.random()) for i in range(nt)])
    for v in range(7 if full else 4):             # S2: two tones only
        add("S2", [tone(0.05 + 0.01 * v, g0 + 2 * u + v, dop(v), ph.random()),
                   tone(0.03 + 0.01 * v, mid + 2 * u + v, dop(v + 3), ph.random())])
    for v in range(2):                            # S3: equal amplitudes, noise-free, r and r + 8 u
        # A 0.0305: a peak of about 1384, just below 1448 = 2^10.5, where sqrtf maps the most float32
        # values of |X|^2 onto one profile value, so that the near tie is an exact float32 tie the more often
        add("S3", [tone(0.0305, g0 + 3 + v, 5, 0.0), tone(0.0305, g0 + 3 + v + 8 * u, 5, 0.0)], noisy=False)
    # S4: half-bin tone, a plateau.  Noise-free: bins r and r + 1 are equal to rounding (the window is
    # symmetric about (nts - 1) / 2, not nts / 2, which splits the pair by up to 1e-6 at low bins: mid-gate
    # and above, at a peak near 1400 as for S3, both schedules return an exact float32 plateau)
    add("S4", [tone(0.035, mid + 0.5, 3, 0.25)], noisy=False)
    add("S4", [tone(0.035, mid + 7 * u + 0.5, 3, 0.0)], noisy=False)
    # with noise, at an amplitude where the noise splits the plateau by more than the fp16-storage band
    # (noise realisation 19: the split is 5.7e-3 and 4.7e-3 at the full geometry, found on the oracle)
    add("S4", [tone(0.0055, g0 + 6 + 0.5, 40 % (nd // 2), 0.3)], noisy=19)
    add("S4", [tone(0.0055, g0 + 15 + 0.5, 40 % (nd // 2), 0.3)], noisy=19)
    for v, gap in enumerate((1, 2, 1, 2)):        # S5: adjacent tones one and two bins apart
        r = g0 + 5 + 3 * v
        add("S5", [tone(0.06, r, dop(v), ph.random()), tone(0.045, r + gap, dop(v + 1), ph.random())])
    for A in (0.05, 0.011):                       # S6: both edge bins and the bin outside each
        for r in (g0, g1, g0 - 1, g1 + 1):
            add("S6in" if g0 <= r <= g1 else "S6out", [tone(A, r, dop(r), ph.random())])
    for v, ratio in enumerate((1.02, 0.98, 1.02, 0.98)):          # S7: peak = range_thr (1 +- 0.02)
        r, d, f0 = mid - 3 + 2 * v, dop(v + 2), ph.random()
        A = threshold_tone(cfg, p, wr, cal, r, d, f0, ratio, seed, len(sc))
        add("S7hi" if ratio > 1 else "S7lo", [tone(A, r, d, f0)])
    if full:
        for v in range(2):                        # S8: weak target beside a strong out-of-gate tone
            add("S8", [tone(0.2, g1 + 1, dop(v), ph.random()), tone(0.01, 17, dop(v + 4), ph.random())])
        # C1: the target stronger than the second of those bins: it is its group's candidate 1
        add("C1", [tone(0.2, g1 + 1, dop(2), ph.random()), tone(0.05, 17, dop(6), ph.random())])
        for v in range(3):                        # S9: AM static target, lines at +-9 (the first noise-free)
            add("S9", [tone(0.04 + 0.02 * v, g0 + 6 + 5 * v, 0, ph.random(), 0.5, 9)], noisy=v > 0)
        for v in range(5):                        # S10: moving targets of three strengths
            add("S10", [tone(0.02, g0 + 3 + v, dop(v), ph.random()), tone(0.06, g0 + 12 + v, dop(v + 2), ph.random()),
                        tone(0.18, g0 + 22 + v, dop(v + 5), ph.random())])
    return names, sc


# --------------------------------------------------------------------------
# the batches of the detection tests (built once per process)
# --------------------------------------------------------------------------
FULL = (1024, 256, 1024, 256)      # nts, pn, nr, nd: the single-pass schedule's geometry
# S11: noise seeds whose frame is unambiguous (frame_ambiguous, M = 8, range_thr 5, max_d 700) at 1e-5 and,
# for the fp16-rounded frame, at 3e-3 -- the first twelve of seeds 100..499, found on the oracle alone
NOISE_SEEDS = (106, 107, 108, 116, 117, 118, 128, 137, 146, 165, 170, 176)
_cache = {}


def _case(nts, pn, nr, nd, mode, **over):
    import dataclasses

    from tests.helpers import case
    cfg, p, wr, wd, cal = case(nts, pn, nr, nd, mode)
    cfg = dataclasses.replace(cfg, **over)
    p = dict(p, bw=cfg.bw, r_max=cfg.r_max, dist_per_bin=cfg.dist_per_bin,
             array_bin_range=np.arange(nr) * cfg.dist_per_bin)
    return cfg, p, wr, wd, cal


def with_params(cfg, M: int, **over):
    """A copy of cfg with max_targets M and the given detection parameters."""
    import dataclasses
    return dataclasses.replace(cfg, max_targets=int(M), **over)


def batch_main(geom=FULL, mode="throughput", seed=11) -> Batch:
    """S1-S10 (S1-S7 away from the full geometry) under the default parameters."""
    key = ("main", geom, mode, seed)
    if key not in _cache:
        cfg, p, wr, wd, cal = _case(*geom, mode)
        names, sc = main_scenes(cfg, p, wr, cal, seed, full=(geom == FULL))
        _cache[key] = Batch(cfg, p, wr, wd, cal, build_frames(sc, geom[0], geom[1], geom[2], geom[3], seed), names)
    return _cache[key]


def batch_noise() -> Batch:
    """S11: noise-only frames, for range_thr 5.0, max_d 700, M = 8."""
    if "noise" not in _cache:
        cfg, p, wr, wd, cal = _case(*FULL, "throughput", range_thr=5.0, max_d=700.0)
        sc = [([], s) for s in NOISE_SEEDS]
        _cache["noise"] = Batch(cfg, p, wr, wd, cal, build_frames(sc, *FULL, 11), ["S11"] * len(sc))
    return _cache["noise"]


def median_row_peak(ob: dict, dec: dict) -> float:
    """Set 3's doppler_thr: the median over the detected rows of the oracle's row peak."""
    pk = [np.abs(ob["rd"][f, dec["tgt_range_idx"][f, j] - 1]).max()
          for f in range(len(dec["tgt_count"])) for j in range(int(dec["tgt_count"][f]))]
    return float(np.median(pk))


def s10_threshold(b: Batch, ob: dict) -> float:
    """S10's doppler_thr: the geometric mean of the row peaks of the two weaker tones of the first
    S10 frame (amplitudes 0.02 and 0.06), so the weakest falls back and the others do not."""
    f = b.frames("S10")[0]
    g0 = int(gate_bins(b.cfg)[0])
    lo, hi = (np.abs(ob["rd"][f, r]).max() for r in (g0 + 3, g0 + 12))
    return float(np.sqrt(lo * hi))


def batch_gate(which: str) -> Batch:
    """Set 4, a gate limit on a bin with dist_per_bin inexact in binary: 'max' is bw 250 MHz
    (dist_per_bin 0.6) with max_d = 41 dist_per_bin, 'min' is bw 180 MHz with min_d = 3 dist_per_bin.
    Tones on both edge bins of the float32 gate and on the bin outside each; one of the outside bins is
    the one the double-precision gate admits.  'exact' is the default bw (dist_per_bin 0.75, exact) with
    both limits on a bin, 2.25 and 22.5: the two gates agree, and rng == min_d and rng == max_d are taken."""
    key = ("gate", which)
    if key not in _cache:
        cfg, p, wr, wd, cal = _case(*FULL, "throughput", bw={"max": 250e6, "min": 180e6, "exact": 200e6}[which])
        if which == "max":
            cfg.max_d = 41 * cfg.dist_per_bin
        elif which == "min":
            cfg.min_d = 3 * cfg.dist_per_bin
        else:
            cfg.min_d, cfg.max_d = 3 * cfg.dist_per_bin, 30 * cfg.dist_per_bin
        g = gate_bins(cfg)
        g0, g1 = int(g[0]), int(g[-1])
        ph = np.random.default_rng(5)
        names, sc = [], []
        for A in (0.05, 0.02):
            for r in (g0, g1, g0 - 1, g1 + 1):
                names.append("in" if g0 <= r <= g1 else "out")
                sc.append(([tone(A, r, 7 + r, ph.random())], True))
        _cache[key] = Batch(cfg, p, wr, wd, cal, build_frames(sc, *FULL, 12), names)
    return _cache[key]


def double_gate(cfg) -> np.ndarray:
    """The gate from the Python doubles, as oracle.search_peak computes it (0-based bins)."""
    i = np.arange(1, cfg.nr - 1)
    d = i * cfg.dist_per_bin
    return i[(d >= cfg.min_d) & (d <= cfg.max_d)]


# set 5: gates under fp16 storage, by name -> detection parameters.  '200': blocks 0-2 stay fp32; 'all':
# every block (the mask is empty); '95' and '97': the gate ends at bin 126 / starts at bin 130, within the
# two bins of margin of the block boundary at 128, so the block on the other side stays fp32 only by the
# margin (fmcw_api.cpp host_s16mask)
WIDE_GATES = {"200": dict(max_d=200.0), "all": dict(min_d=0.0, max_d=1e6), "95": dict(max_d=95.0),
              "97": dict(min_d=97.0, max_d=200.0)}


def batch_wide() -> Batch:
    """Set 5: single tones at bins 150, 260 and 20 (each the strongest of its frame), and around the
    block boundary at bin 128: exact-bin tones at 126 and 130, tones at 127.3 and 128.7 (just outside the
    gates '95' and '97') whose main lobes lie across it."""
    if "wide" not in _cache:
        cfg, p, wr, wd, cal = _case(*FULL, "throughput")
        ph = np.random.default_rng(6)
        names, sc = [], []
        for A in (0.05, 0.12):
            for r in (150, 260, 20):
                names.append(f"bin{r}")
                sc.append(([tone(A, r, 11 + r % 50, ph.random())], True))
        for r in (126, 127.3, 130, 128.7):
            names.append(f"bin{r}")
            sc.append(([tone(0.08, r, 21, ph.random())], True))
        _cache["wide"] = Batch(cfg, p, wr, wd, cal, build_frames(sc, *FULL, 13), names)
    return _cache["wide"]


def batch_zero() -> Batch:
    """A static, noise-free, exact-bin tone among moving ones, for doppler_thr 0.  Every chirp of the static
    frame is the same samples, so on the single-pass schedule (k_rdx subtracts the frame's chirp 0 before the
    range FFT) its RD row is exactly zero: the Doppler index is the first of 256 equal maxima, bin 0, and
    0 >= doppler_thr holds with equality."""
    if "zero" not in _cache:
        cfg, p, wr, wd, cal = _case(*FULL, "throughput", doppler_thr=0.0)
        ph = np.random.default_rng(8)
        names = ["static"] + ["moving"] * 11
        sc = [([tone(0.05, 12, 0, 0.1)], False)]
        sc += [([tone(0.03 + 0.01 * v, 4 + 2 * v, 3 + 9 * v, ph.random())], True) for v in range(11)]
        _cache["zero"] = Batch(cfg, p, wr, wd, cal, build_frames(sc, *FULL, 14), names)
    return _cache["zero"]
