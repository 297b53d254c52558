"""The references of the range-angle stage, written from the definition in include/fmcw.h
(fmcw_ra_params); test-side code (the library's kernels are csrc/kernels_ra.hip).

  cov_reference      float64 from the definition, on exactly the bytes the device is given, with the
                     number of Doppler bins kept and the error bound of every entry.
  spectra_reference  float32, the steps of the header literally: vectorised over rows and
                     directions (numpy rounds every float32 array operation on its own), Python loops
                     over a, b, k only.  Its bytes are what the device must write.
Also the two-source scenario, the peak rule its test uses, and the cases of the GPU parity tests.
Indices are 0-based except the gate, which is 1-based as in the library."""
import functools

import numpy as np

from tests.mti_reference import as_floats
from tests.sig_reference import kept_bins

U = 2.0 ** -24
F32 = np.float32
CAPON = 1


def tri(A, a, b):
    """Index of entry (a, b), a <= b, in the packed upper triangle."""
    return a * A - a * (a - 1) // 2 + (b - a)


def n_tri(A):
    return A * (A + 1) // 2


def gate_rows(nr, r_lo=0, r_hi=0):
    """0-based [g0, g1] inclusive."""
    return (0, nr - 1) if (r_lo, r_hi) == (0, 0) else (r_lo - 1, r_hi - 1)


def cov_reference(rds, dc_half=-1, r_lo=0, r_hi=0):
    """rds: A maps [F][nr][nd] (complex64, or float16 [..][2]).  Returns (cov float64 [F][nr][T][2],
    N, bound float64 [F][nr][T]): the exact-arithmetic sums of the stored values (fp16 storage: times
    (nr nd)^2), the number of Doppler bins kept, and (N + 8) 2^-24 sqrt(R_aa R_bb) per entry."""
    xs, halves = zip(*(as_floats(rd) for rd in rds))
    assert len(set(halves)) == 1
    A = len(xs)
    F, nr, nd = xs[0].shape[:3]
    keep = kept_bins(nd, dc_half)
    N = int(keep.sum())
    z = [x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64) for x in xs]
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    scale2 = (float(F32(nr) * F32(nd))) ** 2 if halves[0] else 1.0
    cov = np.zeros((F, nr, n_tri(A), 2))
    for a in range(A):
        for b in range(a, A):
            r = (z[a][:, g0:g1 + 1][..., keep] * np.conj(z[b][:, g0:g1 + 1][..., keep])).sum(axis=-1) * scale2
            cov[:, g0:g1 + 1, tri(A, a, b), 0] = r.real
            cov[:, g0:g1 + 1, tri(A, a, b), 1] = r.imag if b > a else 0.0
    bound = np.zeros((F, nr, n_tri(A)))
    for a in range(A):
        for b in range(a, A):
            bound[..., tri(A, a, b)] = (N + 8) * U * np.sqrt(cov[..., tri(A, a, a), 0] * cov[..., tri(A, b, b), 0])
    return cov, N, bound


def cov_loop(rds, dc_half=-1, r_lo=0, r_hi=0):
    """cov_reference's sums by a plain loop over frames, rows, bins and channel pairs (small inputs)."""
    xs, halves = zip(*(as_floats(rd) for rd in rds))
    A = len(xs)
    F, nr, nd = xs[0].shape[:3]
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    scale2 = (float(F32(nr) * F32(nd))) ** 2 if halves[0] else 1.0
    cov = np.zeros((F, nr, n_tri(A), 2))
    for f in range(F):
        for r in range(g0, g1 + 1):
            t = 0
            for a in range(A):
                for b in range(a, A):
                    s = 0j
                    for d in range(nd):
                        dist = abs(d - nd // 2)
                        if min(dist, nd - dist) <= dc_half:
                            continue
                        xa = complex(float(xs[a][f, r, d, 0]), float(xs[a][f, r, d, 1]))
                        xb = complex(float(xs[b][f, r, d, 0]), float(xs[b][f, r, d, 1]))
                        s += xa * xb.conjugate()
                    cov[f, r, t] = (s.real * scale2, s.imag * scale2 if b > a else 0.0)
                    t += 1
    return cov


def assert_cov_within_bound(got, rds, dc_half=-1, r_lo=0, r_hi=0, name=""):
    """The device's cov against cov_reference: every component within its bound, rows outside the
    gate and every diagonal im exactly +0 in bits.  Returns the largest share of the bound used."""
    got = np.asarray(got)
    ref, N, bound = cov_reference(rds, dc_half, r_lo, r_hi)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    nr, A = got.shape[1], len(rds)
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    bits = np.ascontiguousarray(got).view(np.uint32)
    assert not bits[:, :g0].any() and not bits[:, g1 + 1:].any(), f"{name}: rows outside the gate must be zero"
    for a in range(A):
        assert not bits[:, :, tri(A, a, a), 1].any(), f"{name}: a diagonal entry's im must be +0"
    err = np.abs(got.astype(np.float64) - ref).max(axis=-1)
    bad = err > bound
    share = float((err / np.maximum(bound, 1e-300))[bound > 0].max(initial=0.0))
    assert not bad.any(), f"{name}: {int(bad.sum())} entries off their bound, worst share {share:.3f}"
    return share


def weights_f32(w):
    """complex [K][A] -> float32 [K][A][2], the table the library reads."""
    w = np.asarray(w)
    if w.dtype != np.float32:
        w = np.ascontiguousarray(w.astype(np.complex64)).view(np.float32).reshape(w.shape + (2,))
    return np.ascontiguousarray(w)


def max_bits(ra):
    """The running maximum as the library raises it from 0: an integer maximum on the floats' bits."""
    m = np.ascontiguousarray(ra, np.float32).view(np.int32).max(initial=0)
    return np.array([max(int(m), 0)], np.int32).view(np.float32)[0]


def spectra_reference(cov, w, capon=False, load=0.0, r_lo=0, r_hi=0):
    """cov float32 [F][nr][T][2] (the device's bytes), w float32 [K][A][2].  Returns (ra float32
    [F][nr][K], ra_max float32): the header's steps in float32, every operation rounded on its own."""
    cov = np.ascontiguousarray(cov, np.float32)
    w = weights_f32(w)
    F, nr, T = cov.shape[:3]
    K, A = w.shape[:2]
    assert T == n_tri(A)
    g0, g1 = gate_rows(nr, r_lo, r_hi)
    C = cov.reshape(F * nr, T, 2)
    Rr = [C[:, t, 0][:, None] for t in range(T)]                 # [rows][1]
    Ri = [C[:, t, 1][:, None] for t in range(T)]
    for a in range(A):
        Ri[tri(A, a, a)] = np.zeros_like(Ri[0])                  # a diagonal entry is real: its im is not read
    wr = [w[:, a, 0][None, :] for a in range(A)]                 # [1][K]
    wi = [w[:, a, 1][None, :] for a in range(A)]
    rows = F * nr
    with np.errstate(all="ignore"):
        if not capon:
            acc = np.zeros((rows, K), F32)
            for a in range(A):
                for b in range(a, A):
                    cr = wr[a] * wr[b] + wi[a] * wi[b]
                    ci = wi[a] * wr[b] - wr[a] * wi[b]
                    t = cr * Rr[tri(A, a, b)] - ci * Ri[tri(A, a, b)]
                    acc = acc + t if a == b else acc + (t + t)
            ra = acc
            bad = np.zeros((rows, 1), bool)
        else:
            tr = np.zeros((rows, 1), F32)
            for a in range(A):
                tr = tr + Rr[tri(A, a, a)]
            delta = F32(load) * (tr / F32(A))
            Lr, Li = {}, {}
            bad = np.zeros((rows, 1), bool)
            for i in range(A):
                for j in range(i + 1):
                    if i == j:
                        sr, si = Rr[tri(A, i, i)] + delta, np.zeros((rows, 1), F32)
                    else:
                        sr, si = Rr[tri(A, j, i)], -Ri[tri(A, j, i)]
                    for k in range(j):
                        sr = sr - (Lr[i, k] * Lr[j, k] + Li[i, k] * Li[j, k])
                        si = si - (Li[i, k] * Lr[j, k] - Lr[i, k] * Li[j, k])
                    if i == j:
                        bad |= ~((sr > 0) & np.isfinite(sr))
                        Lr[i, i], Li[i, i] = np.sqrt(sr), np.zeros((rows, 1), F32)
                    else:
                        Lr[i, j], Li[i, j] = sr / Lr[j, j], si / Lr[j, j]
            yr, yi = {}, {}
            q = np.zeros((rows, K), F32)
            e = np.zeros((1, K), F32)
            for a in range(A):
                ur, ui = wr[a], -wi[a]
                sr, si = ur + np.zeros((rows, 1), F32), ui + np.zeros((rows, 1), F32)
                for b in range(a):
                    sr = sr - (Lr[a, b] * yr[b] - Li[a, b] * yi[b])
                    si = si - (Lr[a, b] * yi[b] + Li[a, b] * yr[b])
                yr[a], yi[a] = sr / Lr[a, a], si / Lr[a, a]
                q = q + (yr[a] * yr[a] + yi[a] * yi[a])
                e = e + (ur * ur + ui * ui)
            ra = (e * e) / q
            ra = np.where(q == 0, F32(0), ra)
        assert ra.dtype == np.float32
        ra = np.where(bad, F32(0), ra).astype(F32).reshape(F, nr, K)
    ra[:, :g0] = 0
    ra[:, g1 + 1:] = 0
    return ra, max_bits(ra)


def assert_same_bytes(got, ref, name=""):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != ref.view(np.uint32).reshape(-1))
        i = bad[0]
        raise AssertionError(f"{name}: {bad.size} of {got.size} values differ, the first at {i}: "
                             f"{got.reshape(-1)[i]!r} for {ref.reshape(-1)[i]!r}")


# ---- input pools --------------------------------------------------------------------------------------
def store(z, half):
    """complex [F][nr][nd] -> the stored form: complex64, or float16 [..][2] holding z / (nr nd)."""
    z = np.asarray(z)
    if not half:
        return np.ascontiguousarray(z.astype(np.complex64))
    nr, nd = z.shape[1:]
    v = np.stack([z.real, z.imag], axis=-1) / (nr * nd)
    return np.ascontiguousarray(v.astype(np.float16))


@functools.lru_cache(maxsize=None)
def pool(seed, A, F, nr, nd, half, dominant=False):
    """A maps [F][nr][nd] of the storage dtype: unit complex noise over a few binades with a phase
    step per channel that differs from row to row (so no entry of R is small by symmetry).  dominant:
    one cell 120 dB above the noise in the channel pair (0, A - 1).  Shared between tests: read only."""
    rng = np.random.default_rng(seed)
    base = (rng.standard_normal((F, nr, nd)) + 1j * rng.standard_normal((F, nr, nd))) * np.sqrt(0.5)
    step = rng.uniform(-np.pi, np.pi, (F, nr, 1))
    chans = []
    for a in range(A):
        own = (rng.standard_normal((F, nr, nd)) + 1j * rng.standard_normal((F, nr, nd))) * np.sqrt(0.5)
        z = (base * np.exp(1j * step * a) + own) * np.exp2(rng.integers(-2, 3, (F, nr, 1)))
        if dominant and a in (0, A - 1):
            z[F - 1, nr // 3, (nd // 2 + 1) % nd] = 1e6 * np.exp(1j * (0.3 + a))
        chans.append(z)
    out = [store(z, half) for z in chans]
    for c in out:
        c.setflags(write=False)
    return out


# ---- the two-source scenario ----------------------------------------------------------------------------
SCENE = dict(A=8, spacing=0.5, nr=16, nd=64, row=5, amp=30.0, bins=(20, 41), points=(32, 37), n_ang=65, dc_half=0,
             load=1e-3, frames=8)


def scene_sines():
    """The 65-point grid uniform in sin(theta) over [-1, 1]: point k is (k - 32) / 32, exact."""
    return ((np.arange(SCENE["n_ang"]) - 32) / 32.0).astype(F32)


@functools.lru_cache(maxsize=None)
def scene(seed=1, half=False):
    """A = 8 maps [8 frames][16][64]: unit complex noise everywhere; in row 5 of every frame two
    sources of amplitude 30 at Doppler bins 20 and 41, arriving from grid points 32 and 37
    (sin(theta) = 0 and 0.15625): channel a of a source carries the phase 2 pi spacing a sin(theta)."""
    S = SCENE
    rng = np.random.default_rng(seed)
    sines = scene_sines().astype(np.float64)
    chans = []
    ph = rng.uniform(-np.pi, np.pi, (S["frames"], 2))
    for a in range(S["A"]):
        z = (rng.standard_normal((S["frames"], S["nr"], S["nd"])) + 1j * rng.standard_normal((S["frames"], S["nr"], S["nd"]))) \
            * np.sqrt(0.5)
        for s, (d, k) in enumerate(zip(S["bins"], S["points"])):
            z[:, S["row"], d] += S["amp"] * np.exp(1j * (2 * np.pi * S["spacing"] * a * sines[k] + ph[:, s]))
        chans.append(store(z, half))
    for c in chans:
        c.setflags(write=False)
    return chans


def peaks(spec, share=0.25):
    """Indices of the local maxima of a 1-D spectrum that exceed `share` of its maximum."""
    s = np.asarray(spec, np.float64)
    left = np.concatenate([[-np.inf], s[:-1]])
    right = np.concatenate([s[1:], [-np.inf]])
    return [int(k) for k in np.flatnonzero((s > left) & (s >= right) & (s > share * s.max()))]


# ---- the cases of the GPU parity test: (nr, nd, F, A, half, dc_half, (r_lo, r_hi)) -----------------------
SHAPES = ((16, 4), (2048, 4), (16, 1024), (64, 64), (32, 128), (32, 256), (32, 16))
AS = (2, 3, 5, 8)


def parity_cases():
    """Every shape (either side of "a row fills one wave-load" for both dtypes, rows of several
    wave-loads, and lane groups of every width) with both storage forms and every A; F in 1..3,
    dc_half in {-1, 0, the largest allowed} and the gate in {all rows, one row, the first rows, the
    last rows} rotate so that every value meets every shape and dtype."""
    cases = []
    i = 0
    for nr, nd in SHAPES:
        for half in (False, True):
            for A in AS:
                dc = (-1, 0, nd // 2 - 1)[i % 3]
                gate = ((0, 0), (nr // 2, nr // 2), (1, 3), (nr - 4, nr))[(i // 3 + i) % 4]
                cases.append((nr, nd, 1 + i % 3, A, half, dc, gate))
                i += 1
    return cases


def case_id(c):
    nr, nd, F, A, half, dc, gate = c
    return f"{nr}x{nd}-F{F}-A{A}-{'c32h' if half else 'c64'}-dc{dc}-g{gate[0]}_{gate[1]}"


def case_seed(c):
    nr, nd, F, A, half, dc, gate = c
    return nr * 7 + nd * 3 + F * 101 + A * 11 + (500 if half else 0)
